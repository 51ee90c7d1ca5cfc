"""Gated batched point-to-plane registration (IcpBatch.estimate_point_to_plane*(..., max_correspondence_distance=r),
include/icp_mi355x.h section 19): every item's status, pose, indices, inner counts and inlier counts equal, bit for bit,
what a fresh Icp3d(dst_i) returns after compute_normals(k) from estimate_point_to_plane(src_i, init_i, max_iter,
max_correspondence_distance=r) -- whichever way the batch served it -- and the CPU statement of the gate (the tree oracle
chained on the kept points, tests/test_gpu_plane_parity.py: oracle_chain)."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from test_gpu_batch import random_item
from test_gpu_gated_plane import blob_scene, d2_of
from test_gpu_line_batch_gated import EDGE_PAIRS, outlier_places
from test_gpu_plane_batch import mixed_items
from test_gpu_plane_parity import Target, oracle_chain
from test_line_abi import pose_error
from test_p2plane import moved, room
from test_plane_batch_gated_abi import DZ_R, dz_case
from test_plane_reference import NORMALS_K, bits

pytestmark = pytest.mark.gpu

INF = float("inf")


def single(dst, src, init, max_iter, k, r):
    """(status, pose, indices, inner counts, inlier counts) of the single gated call on a fresh handle"""
    icp = None
    try:
        icp = I.Icp3d(dst)
        icp.compute_normals(k)
        T, idx, inner, inl = icp.estimate_point_to_plane(src, init, max_iter, return_info=True,
                                                         max_correspondence_distance=r)
        return _lib.OK, T.as_array(), idx, inner, inl
    except I.IcpError as e:
        return e.status, None, None, None, None
    finally:
        if icp is not None:
            icp.close()


def assert_items_match(srcs, dsts, inits, max_iter, k, r, got):
    """every item against its single call; returns the single calls' inlier counts (None for a failed item)"""
    Ts, idxs, inner, status, inliers = got
    assert len(Ts) == len(srcs) and inliers.shape == inner.shape == (len(srcs), max_iter)
    counts = []
    for i, (s, d, T0) in enumerate(zip(srcs, dsts, inits)):
        rc, pose, idx, inn, inl = single(d, s, T0, max_iter, k, r)
        counts.append(inl)
        assert status[i] == rc, (i, status[i], rc)
        if rc != _lib.OK:
            assert Ts[i] is None
            continue
        assert np.array_equal(inliers[i], inl), (i, inliers[i].tolist(), inl.tolist())
        assert np.array_equal(inner[i], inn), (i, inner[i].tolist(), inn.tolist())
        assert np.array_equal(idxs[i], idx), i
        assert np.array_equal(bits(Ts[i]), bits(pose)), i
    return counts


def assert_served_inside(counters, inside, outside=0):
    """finite coordinates and small rotations: none of the three hand-back reasons can occur, 0 expected; the cap only
    keeps a test from passing through the fallback"""
    served, one_by_one, _, refused = counters
    handed_back = one_by_one - outside
    assert refused == 0 and served + one_by_one == inside + outside and handed_back >= 0, counters
    assert 32 * handed_back <= inside, counters


# ------------------------------------------------------------------ 1. the compaction's and the fold tree's edges

def known_kept_item(rng, dst, n, kept, how):
    """n source points of which exactly `kept` lie within millimetres of a target; the others are 100 m away.  Two or
    three kept pairs leave rank-deficient normal equations, whose update is an accident of rounding: those items take
    the target points themselves and start at the identity (residuals 0, no update), so that the count stays `kept`."""
    src = dst[rng.integers(0, len(dst), n)] + (rng.normal(0.0, 3e-3, (n, 3)) if kept > 3 or kept < 2 else 0.0)
    out = outlier_places(n, n - kept, how)
    src[out] = np.array([100.0, 100.0, 100.0]) + rng.uniform(-1.0, 1.0, (len(out), 3))
    return np.ascontiguousarray(src)


def test_edges_of_the_compaction_and_of_the_fold_tree_over_the_kept_pairs():
    rng = np.random.default_rng(3200)
    dst = room(rng, 700)
    srcs, dsts, want = [], [], []
    for how in ("interleaved", "waves", "front"):
        for n, kept in EDGE_PAIRS:
            srcs.append(known_kept_item(rng, dst, n, kept, how))
            dsts.append(dst)
            want.append(kept)
    # the plan where a record of the line kernel's kind would overflow the grant: 1665 and 2048 targets, 1024 threads
    full, past = room(rng, 2048), room(rng, 1665)
    srcs += [known_kept_item(rng, full, 1024, 700, "interleaved"), known_kept_item(rng, past, 1024, 1000, "waves")]
    dsts += [full, past]
    want += [700, 1000]
    inside = len(srcs)
    big = room(rng, 2049)
    srcs += [known_kept_item(rng, dst, 1025, 900, "interleaved"), known_kept_item(rng, big, 300, 200, "interleaved")]
    dsts += [dst, big]  # n = 1025 and m = 2049: outside the limits, one by one
    want += [900, 200]
    inits = [I.Transform([1e-3, -2e-3, 1e-3]) if kept > 3 or kept < 2 else I.Transform() for kept in want]
    B = I.IcpBatch(3)
    got = B.estimate_point_to_plane(srcs, dsts, inits, 8, k=8, return_info=True, allow_failures=True,
                                    max_correspondence_distance=0.5)
    counters = B.plane_gated_counters()
    ungated = B.plane_counters()
    B.close()
    assert got[3].tolist() == [_lib.OK] * len(srcs)
    for i, kept in enumerate(want):
        assert got[4][i].tolist() == [kept] * 8, (i, len(srcs[i]), kept, got[4][i].tolist())
    assert_items_match(srcs, dsts, inits, 8, 8, 0.5, got)
    print("inner counts by kept:", [(len(s), k, got[2][i].tolist()) for i, (s, k) in enumerate(zip(srcs, want))][:16])
    assert counters == (inside, 2, 2, 0), counters  # every item within the limits in a launch, none handed back
    assert ungated == (0, 0, 0, 0)


# ------------------------------------------------------------------ 2. the dz term

def test_the_gate_measures_the_distance_in_three_dimensions():
    """sources exactly on the bound above their target (kept), one ulp past it, a metre above it with xy distance 0
    (both dropped), and on the bound along legs 0.3 / 0.4 (kept): tests/test_plane_batch_gated_abi.py: dz_case, whose
    count comes from d2_of in numpy.  All targets lie in the plane z = 0: no update, the count holds every iteration."""
    dst, src, want_kept, nearest = dz_case()
    d2 = d2_of(src, I.Transform(), dst[nearest])[3]
    assert 0 < want_kept < len(src) and want_kept == int(np.sum(d2 <= DZ_R * DZ_R))
    flat = d2_of(src, I.Transform(), dst[nearest] * np.array([1.0, 1.0, 0.0]) + src * np.array([0.0, 0.0, 1.0]))[3]
    assert int(np.sum(flat <= DZ_R * DZ_R)) > want_kept  # (a gate without the dz term would keep more)
    B = I.IcpBatch(3)
    got = B.estimate_point_to_plane([src], [dst], None, 4, k=8, return_info=True, max_correspondence_distance=DZ_R)
    assert B.plane_gated_counters() == (1, 0, 1, 0)
    B.close()
    Ts, idxs, inner, status, inl = got
    assert status[0] == _lib.OK and np.array_equal(idxs[0], nearest)
    assert inl[0].tolist() == [want_kept] * 4, inl[0].tolist()
    counts = assert_items_match([src], [dst], [I.Transform()], 4, 8, DZ_R, got)
    assert counts[0].tolist() == [want_kept] * 4


# ------------------------------------------------------------------ 3. the CPU statement

ROOM_M = (300, 700, 1100, 1600, 2048)
ROOM_N = (2, 3, 65, 513, 1024)
# the finite bound of each scene: between the scan's displacement under its pose (centimetres) and the displaced share's
# distance off its plane (decimetres); the oracle's run must show that it removes some pairs and keeps others
ROOM_R = {m: 0.1 for m in ROOM_M}


def room_scan(rng, dst, n):
    """n target points with millimetre noise, three in ten of them moved a few decimetres off the floor and off both
    walls, the whole seen from a small pose"""
    s = dst[rng.integers(0, len(dst), n)] + rng.normal(0.0, 1e-3, (n, 3))
    far = rng.permutation(n)[:(3 * n) // 10]
    s[far] += np.array([-0.3, 0.3, 0.3]) * rng.uniform(0.7, 1.3, (len(far), 1))
    return np.ascontiguousarray(moved(s, I.Transform([0.03, -0.02, 0.01]).inverse()))


@pytest.fixture(scope="module")
def rooms():
    O.set_threads(16)
    rng = np.random.default_rng(3300)
    made = {m: Target(3, room(rng, m)) for m in ROOM_M}
    scans = {(m, n): room_scan(rng, made[m].dst, n) for m in ROOM_M for n in ROOM_N}
    yield made, scans
    for t in made.values():
        t.icp.close()
    O.set_threads(1)


@pytest.mark.parametrize("bound", ["inf", "finite"])
def test_one_gated_batched_call_equals_the_tree_oracle_chained_on_the_kept_points(rooms, bound):
    made, scans = rooms
    by_r = {}  # (one call per bound: the scenes that share a finite bound share a call)
    for m in ROOM_M:
        by_r.setdefault(INF if bound == "inf" else ROOM_R[m], []).append(m)
    assert len(by_r) == 1
    for r, ms in by_r.items():
        what = [(m, n) for m in ms for n in ROOM_N]
        srcs, dsts = [scans[w] for w in what], [made[m].dst for m, _ in what]
        inits = [I.Transform() for _ in what]
        B = I.IcpBatch(3)
        Ts, idxs, inner, status, inl = B.estimate_point_to_plane(srcs, dsts, inits, 4, k=NORMALS_K, return_info=True,
                                                                 max_correspondence_distance=r)
        counters = B.plane_gated_counters()
        B.close()
        for i, (m, n) in enumerate(what):
            assert status[i] == _lib.OK
            oT, oidx, oinner, oinl = oracle_chain(made[m], srcs[i], inits[i], 4, r)
            where = (m, n, r)
            print(f"m={m} n={n} r={r}: inliers {oinl.tolist()}, inner {oinner.tolist()}")
            if r == INF:
                assert np.all(oinl == n), where
            elif n >= 65:
                assert 0 < oinl[0] < n, where  # the bound removes some pairs and keeps others
            assert np.array_equal(idxs[i], oidx), where
            assert np.array_equal(inner[i], oinner), (where, inner[i].tolist(), oinner.tolist())
            assert np.array_equal(inl[i], oinl), (where, inl[i].tolist(), oinl.tolist())
            assert np.array_equal(bits(Ts[i]), bits(oT)), (where, Ts[i].as_array(), oT.as_array())
        assert counters == (25, 0, 2, 0), counters


# ------------------------------------------------------------------ 4. an infinite bound

def test_an_infinite_bound_returns_the_bits_of_the_ungated_batch_call():
    rng = np.random.default_rng(3400)
    items = [random_item(rng, 3, n=n, m=m) for n, m in ((1, 1), (2, 3), (65, 64), (512, 2048), (513, 1665), (1024, 2048),
                                                         (1024, 1), (700, 900), (300, 1921), (1000, 1500))]
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(3)
    Ts, idxs, inner, status = B.estimate_point_to_plane(srcs, dsts, inits, 20, k=8, return_info=True)
    gTs, gidxs, ginner, gstatus, inl = B.estimate_point_to_plane(srcs, dsts, inits, 20, k=8, return_info=True,
                                                                 max_correspondence_distance=INF)
    gated, plain = B.plane_gated_counters(), B.plane_counters()
    B.close()
    assert_served_inside(gated, len(srcs))
    assert gated[2] == 2 and plain[:2] == gated[:2]
    assert np.array_equal(status, gstatus) and np.array_equal(inner, ginner)
    for i, s in enumerate(srcs):
        assert np.array_equal(bits(Ts[i]), bits(gTs[i])), i
        assert np.array_equal(idxs[i], gidxs[i]), i
        assert np.all(inl[i] == len(s)), (i, inl[i].tolist())  # (an iteration the fixed-point rule skips repeats one)


# ------------------------------------------------------------------ 5. a fixed point

def test_a_fixed_point_reports_the_counts_of_the_iterations_it_skips():
    rng = np.random.default_rng(3500)
    dst = room(rng, 900)
    sizes = [1, 2, 70, 513, 900]
    srcs = [np.ascontiguousarray(dst[rng.choice(900, n, replace=False)]) for n in sizes]
    ident = [I.Transform() for _ in srcs]
    B = I.IcpBatch(3)
    got = B.estimate_point_to_plane(srcs, [dst] * len(srcs), ident, 6, k=8, return_info=True,
                                    max_correspondence_distance=0.0)
    assert B.plane_gated_counters() == (len(srcs), 0, 2, 0)
    B.close()
    counts = assert_items_match(srcs, [dst] * len(srcs), ident, 6, 8, 0.0, got)
    assert not got[2].any()  # exact matches: residuals 0, no update
    for n, inl, mine in zip(sizes, counts, got[4]):
        assert inl.tolist() == mine.tolist() == [n] * 6  # (the single call runs all six)


# ------------------------------------------------------------------ 6. statuses

def test_statuses_and_bits_in_a_mixed_gated_batch():
    items = mixed_items()  # [1] a NaN source coordinate, [2] a NaN target (handed back), [3] n = 0, [4] m = 0, [5] m = 2,
    #                        [6] coplanar targets, [7] collinear targets, [8] every target three times
    s, d, T = random_item(np.random.default_rng(3600), 3, n=400, m=500)
    items.append((s + 500.0, d, T))  # all outliers
    srcs, dsts, inits = zip(*items)
    last = len(srcs) - 1
    B = I.IcpBatch(3)
    got = B.estimate_point_to_plane(srcs, dsts, inits, 20, k=8, return_info=True, allow_failures=True,
                                    max_correspondence_distance=0.75)
    assert_items_match(srcs, dsts, inits, 20, 8, 0.75, got)
    Ts, _, inner, status, inl = got
    print("statuses:", status.tolist(), "inliers of the item with a NaN source point:", inl[1].tolist())
    assert status[0] == _lib.OK and status[3] == _lib.OK and status[4] == _lib.EMPTY_DST
    assert status[5:].tolist() == [_lib.OK] * (len(srcs) - 5)
    if status[1] == _lib.OK:  # the NaN point's d2 is NaN: gated out
        assert inl[1].max() <= len(srcs[1]) - 1
    assert not inl[last].any() and not inner[last].any() and np.array_equal(bits(Ts[last]), bits(inits[last]))
    served, one_by_one = B.plane_gated_counters()[:2]
    assert served + one_by_one == len(srcs) and one_by_one >= 3  # (n = 0, m = 0 and the NaN target go one by one)
    assert 32 * (one_by_one - 3) <= served
    with pytest.raises(I.IcpError, match="item 1"):  # (of the items from [3] on: the one without targets)
        B.estimate_point_to_plane(srcs[3:], dsts[3:], inits[3:], 20, k=8, max_correspondence_distance=0.75)
    # a bound of zero: nothing but exact matches passes
    got_r0 = B.estimate_point_to_plane(srcs, dsts, inits, 20, k=8, return_info=True, allow_failures=True,
                                       max_correspondence_distance=0.0)
    assert_items_match(srcs, dsts, inits, 20, 8, 0.0, got_r0)
    # no outer iteration for the whole call: every item one by one, each as its single call
    before = B.plane_gated_counters()
    got0 = B.estimate_point_to_plane(srcs, dsts, inits, 0, k=8, return_info=True, allow_failures=True,
                                     max_correspondence_distance=0.75)
    assert_items_match(srcs, dsts, inits, 0, 8, 0.75, got0)
    assert got0[2].shape == got0[4].shape == (len(srcs), 0)
    after = B.plane_gated_counters()
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (0, len(srcs), 0)
    assert B.plane_counters() == (0, 0, 0, 0)
    B.close()


# ------------------------------------------------------------------ 7. hypotheses

def test_gated_hypotheses_share_one_range_and_each_equals_its_single_call():
    rng = np.random.default_rng(3700)
    dst = room(rng, 1500)
    src = room_scan(rng, dst, 650)
    inits = [I.Transform([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1)]) for _ in range(64)]
    B = I.IcpBatch(3)
    got = B.estimate_point_to_plane_packed(src, dst, [(0, len(src), 0, len(dst), T) for T in inits], 10, k=8,
                                           return_info=True, allow_failures=True, max_correspondence_distance=0.3)
    counters = B.plane_gated_counters()
    B.close()
    counts = assert_items_match([src] * 64, [dst] * 64, inits, 10, 8, 0.3, got)
    assert_served_inside(counters, 64)
    assert counters[2] == 1
    print("first counts:", sorted(int(c[0]) for c in counts if c is not None))


# ------------------------------------------------------------------ 8. the device entry, and the ungated call beside it

def test_device_entry_equals_host_entry_twice_and_leaves_the_ungated_call_alone():
    import torch

    rng = np.random.default_rng(3800)
    B = I.IcpBatch(3)
    total = 0
    for count in (24, 5, 40):  # grow, shrink, grow: the batch's buffers are reused and resized
        items = [random_item(rng, 3, n=int(rng.integers(1, 1025)), m=int(rng.integers(1, 800))) for _ in range(count)]
        total += count
        srcs, dsts, inits = zip(*items)
        src, dst = np.concatenate(srcs), np.concatenate(dsts)
        sf, df = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(d) for d in dsts])
        packed = [(sf[i], len(srcs[i]), df[i], len(dsts[i]), inits[i]) for i in range(count)]
        kw = dict(k=8, return_info=True)
        plain = B.estimate_point_to_plane_packed(src, dst, packed, 20, **kw)
        host = B.estimate_point_to_plane_packed(src, dst, packed, 20, max_correspondence_distance=0.6, **kw)
        again = B.estimate_point_to_plane_packed(src, dst, packed, 20, max_correspondence_distance=0.6, **kw)
        d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        ptrs = (d_src.data_ptr(), d_dst.data_ptr())
        dev = B.estimate_point_to_plane_packed(d_src, d_dst, packed, 20, max_correspondence_distance=0.6, **kw)
        assert (d_src.data_ptr(), d_dst.data_ptr()) == ptrs  # borrowed in place ...
        assert np.array_equal(d_src.cpu().numpy(), src) and np.array_equal(d_dst.cpu().numpy(), dst)  # ... and left alone
        after = B.estimate_point_to_plane_packed(src, dst, packed, 20, **kw)
        assert len(plain) == len(after) == 4 and len(host) == 5
        for a, b in ((host, again), (host, dev), (plain, after)):
            for i in range(count):
                assert np.array_equal(bits(a[0][i]), bits(b[0][i])), i
                assert np.array_equal(a[1][i], b[1][i]), i
            assert all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))
        assert host[4].min() < max(len(s) for s in srcs)  # (the bound removes something)
        if count == 5:
            assert_items_match(srcs, dsts, inits, 20, 8, 0.6, host)
    assert_served_inside(B.plane_gated_counters(), 3 * total)
    B.close()


# ------------------------------------------------------------------ 9. what the gate is for

def test_the_gate_brings_a_partly_overlapping_item_closer_to_the_true_pose():
    """tests/test_gpu_gated_plane.py's scene thinned to what a workgroup serves: 1024 points, 55 % of them a blob the
    room's 2048 targets do not hold.  Only the order is asserted, for the batch and for the single calls."""
    scenes = [blob_scene(seed, n=1024, m=2048) for seed in (5, 6, 7)]
    dsts, srcs, truth = zip(*scenes)
    B = I.IcpBatch(3)
    plain = B.estimate_point_to_plane(srcs, dsts, None, 10, k=10)
    gated, _, _, _, inl = B.estimate_point_to_plane(srcs, dsts, None, 10, k=10, return_info=True,
                                                    max_correspondence_distance=0.25)
    assert_served_inside(B.plane_gated_counters(), 3)
    B.close()
    for i in range(3):
        eg, ep = pose_error(gated[i], truth[i]), pose_error(plain[i], truth[i])
        icp = I.Icp3d(dsts[i])
        icp.compute_normals(10)
        sp = pose_error(icp.estimate_point_to_plane(srcs[i], I.Transform(), 10), truth[i])
        sg = pose_error(icp.estimate_point_to_plane(srcs[i], I.Transform(), 10, max_correspondence_distance=0.25), truth[i])
        icp.close()
        print(f"seed {5 + i}: pose error gated {eg:.3e} (single {sg:.3e}), ungated {ep:.3e} (single {sp:.3e}), "
              f"kept {inl[i].tolist()}")
        assert eg < ep, (i, eg, ep)
        assert sg < sp, (i, sg, sp)
