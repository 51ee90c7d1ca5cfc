"""Gated batched point-to-line registration (IcpBatch.estimate_point_to_line*(..., max_correspondence_distance=r),
include/icp_mi355x.h section 17): every item's status, pose, indices, inner counts and inlier counts equal, bit for bit,
what a fresh Icp2d(dst_i) returns after compute_line_normals(k) from estimate_point_to_line(src_i, init_i, max_iter,
max_correspondence_distance=r) -- whichever way the batch served it -- and the CPU statement of the gate (the tree oracle
chained on the kept points, tests/test_gpu_plane_parity.py: oracle_chain)."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from test_gpu_batch import random_item
from test_gpu_line_batch import mixed_items
from test_gpu_plane_parity import FAMILY, SCENES, Target, gate, oracle_chain
from test_line_abi import GOLDEN_K, TRUE_PARAM, load_golden, moved2, outline, outline_pair, pose_error
from test_plane_reference import NORMALS_K, bits

pytestmark = pytest.mark.gpu

INF = float("inf")


def single(dst, src, init, max_iter, k, r):
    """(status, pose, indices, inner counts, inlier counts) of the single gated call on a fresh handle"""
    icp = I.Icp2d(dst)
    try:
        icp.compute_line_normals(k)
        T, idx, inner, inl = icp.estimate_point_to_line(src, init, max_iter, return_info=True,
                                                        max_correspondence_distance=r)
        return _lib.OK, T.as_array(), idx, inner, inl
    except I.IcpError as e:
        return e.status, None, None, None, None
    finally:
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


# ------------------------------------------------------------------ 1. the compaction's and the fold tree's edges

EDGE_PAIRS = [(1, 0), (1, 1), (2, 1), (2, 2), (3, 0), (64, 63), (65, 64), (66, 65), (513, 511), (513, 512), (600, 513),
              (1024, 0), (1024, 1), (1024, 512), (1024, 1023), (1024, 1024)]


def outlier_places(n, count, how):
    """the positions of `count` outliers among n points: the first `count` of an order of preference"""
    every = np.arange(n)
    if how == "interleaved":  # every third point, then the others
        order = np.concatenate([every[0::3], every[1::3], every[2::3]])
    elif how == "waves":  # a whole first wave, a whole last wave, a whole middle wave, then the others
        waves = [every[w:w + 64] for w in range(0, n, 64)]
        first = [0, len(waves) - 1, len(waves) // 2]
        picked = list(dict.fromkeys(first)) + [w for w in range(len(waves)) if w not in first]
        order = np.concatenate([waves[w] for w in picked])
    else:  # all at the front
        order = every
    return np.sort(order[:count])


def known_kept_item(rng, dst, n, kept, how):
    """n source points of which exactly `kept` lie within millimetres of a target; the others are 100 m away.  Two or
    three kept pairs leave rank-deficient normal equations, whose update is an accident of rounding: those items take
    the target points themselves and start at the identity (residuals 0, no update), so that the count stays `kept`."""
    src = dst[rng.integers(0, len(dst), n)] + (rng.normal(0.0, 3e-3, (n, 2)) if kept > 3 or kept < 2 else 0.0)
    out = outlier_places(n, n - kept, how)
    src[out] = np.array([100.0, 100.0]) + rng.uniform(-1.0, 1.0, (len(out), 2))
    return np.ascontiguousarray(src)


def test_edges_of_the_compaction_and_of_the_fold_tree_over_the_kept_pairs():
    rng = np.random.default_rng(1900)
    dst = outline(rng, 700)
    srcs, dsts, want = [], [], []
    for how in ("interleaved", "waves", "front"):
        for n, kept in EDGE_PAIRS:
            srcs.append(known_kept_item(rng, dst, n, kept, how))
            dsts.append(dst)
            want.append(kept)
    inside = len(srcs)
    big = outline(rng, 2049)
    srcs += [known_kept_item(rng, dst, 1025, 900, "interleaved"), known_kept_item(rng, big, 300, 200, "interleaved")]
    dsts += [dst, big]  # n = 1025 and m = 2049: outside the limits, one by one
    want += [900, 200]
    inits = [I.Transform([1e-3, -2e-3, 1e-3]) if kept > 3 or kept < 2 else I.Transform() for kept in want]
    B = I.IcpBatch(2)
    got = B.estimate_point_to_line(srcs, dsts, inits, 8, k=8, return_info=True, allow_failures=True,
                                   max_correspondence_distance=0.5)
    counters = B.line_gated_counters()
    ungated = B.line_counters()
    B.close()
    assert got[3].tolist() == [_lib.OK] * len(srcs)
    for i, kept in enumerate(want):
        assert got[4][i].tolist() == [kept] * 8, (i, len(srcs[i]), kept, got[4][i].tolist())
    assert_items_match(srcs, dsts, inits, 8, 8, 0.5, got)
    print("inner counts by kept:", [(len(s), k, got[2][i].tolist()) for i, (s, k) in enumerate(zip(srcs, want))][:16])
    assert counters == (inside, 2, 2, 0), counters  # every item within the limits in a launch, none handed back
    assert ungated == (0, 0, 0, 0)


# ------------------------------------------------------------------ 2. the CPU statement

@pytest.fixture(scope="module")
def targets():
    O.set_threads(16)
    made = {}

    def get(scene):
        key = FAMILY[scene]
        if key not in made:
            made[key] = Target(2, SCENES[scene](2, 2)[0])
        return made[key]

    yield get
    for t in made.values():
        t.icp.close()
    O.set_threads(1)


@pytest.mark.parametrize("bound", ["inf", "finite"])
def test_one_gated_batched_call_equals_the_tree_oracle_chained_on_the_kept_points(targets, bound):
    sizes = [2, 3, 65, 513, 1024]
    by_r = {}  # (one call per bound: the scenes that share a finite bound share a call)
    for scene in SCENES:
        r = INF if bound == "inf" else gate(2, scene)
        by_r.setdefault(r, []).append(scene)
    for r, scenes in by_r.items():
        srcs, dsts, inits, what = [], [], [], []
        for scene in scenes:
            t = targets(scene)
            assert len(t.dst) <= 2048
            for n in sizes:
                _, src, init = SCENES[scene](2, n)
                srcs.append(src)
                dsts.append(t.dst)
                inits.append(init)
                what.append((scene, n))
        B = I.IcpBatch(2)
        Ts, idxs, inner, status, inl = B.estimate_point_to_line(srcs, dsts, inits, 4, k=NORMALS_K, return_info=True,
                                                                max_correspondence_distance=r)
        served, one_by_one, _, refused = B.line_gated_counters()
        B.close()
        print(f"r = {r}: served {served}, one by one {one_by_one}")
        assert served + one_by_one == len(srcs) and refused == 0
        for i, (scene, n) in enumerate(what):
            assert status[i] == _lib.OK
            oT, oidx, oinner, oinl = oracle_chain(targets(scene), srcs[i], inits[i], 4, r)
            where = (scene, n, r)
            print(f"{scene} n={n} r={r}: inliers {oinl.tolist()}, inner {oinner.tolist()}")
            if r == INF:
                assert np.all(oinl == n), where
            elif n >= 65:
                assert 0 < oinl[0] < n, where  # the bound removes some pairs and keeps others
            assert np.array_equal(idxs[i], oidx), where
            assert np.array_equal(inner[i], oinner), (where, inner[i].tolist(), oinner.tolist())
            assert np.array_equal(inl[i], oinl), (where, inl[i].tolist(), oinl.tolist())
            assert np.array_equal(bits(Ts[i]), bits(oT)), (where, Ts[i].as_array(), oT.as_array())


# ------------------------------------------------------------------ 3, 4. the golden scan pairs

def golden_pairs():
    scans = [load_golden(j) for j in range(1, 12)]
    return scans[:10] + [scans[0]], scans[1:11] + [scans[9]]  # 001 -> 002 ... 010 -> 011, and 001 -> 010


def test_an_infinite_bound_returns_the_bits_of_the_ungated_batch_call():
    srcs, dsts = golden_pairs()
    ident = [I.Transform() for _ in srcs]
    B = I.IcpBatch(2)
    Ts, idxs, inner, status = B.estimate_point_to_line(srcs, dsts, ident, 20, k=GOLDEN_K, return_info=True)
    gTs, gidxs, ginner, gstatus, inl = B.estimate_point_to_line(srcs, dsts, ident, 20, k=GOLDEN_K, return_info=True,
                                                                max_correspondence_distance=INF)
    assert B.line_gated_counters() == (len(srcs), 0, 1, 0) and B.line_counters()[:2] == (len(srcs), 0)
    B.close()
    assert np.array_equal(status, gstatus) and np.array_equal(inner, ginner)
    for i, s in enumerate(srcs):
        assert np.array_equal(bits(Ts[i]), bits(gTs[i])), i
        assert np.array_equal(idxs[i], gidxs[i]), i
        assert np.all(inl[i] == len(s)), (i, inl[i].tolist())  # (an iteration the fixed-point rule skips repeats one)


def test_golden_pairs_at_a_bound_that_bites_equal_their_single_calls():
    srcs, dsts = golden_pairs()
    ident = [I.Transform() for _ in srcs]
    for i in (0, 4, 10):  # one call per bound: the pair's median nearest-neighbour distance at the identity
        icp = I.Icp2d(dsts[i])
        icp.compute_line_normals(GOLDEN_K)
        _, idx, _ = icp.estimate_point_to_line(srcs[i], I.Transform(), 1, return_info=True)
        icp.close()
        e = srcs[i] - dsts[i][idx]
        r = float(np.sqrt(np.median(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])))  # the first gate's d2
        B = I.IcpBatch(2)
        got = B.estimate_point_to_line(srcs, dsts, ident, 20, k=GOLDEN_K, return_info=True, max_correspondence_distance=r)
        assert B.line_gated_counters()[:2] == (len(srcs), 0)  # no hand-back
        B.close()
        counts = assert_items_match(srcs, dsts, ident, 20, GOLDEN_K, r, got)
        print(f"r = {r:.5f} (pair {i}): inliers of the pair {counts[i].tolist()}")
        assert 0 < counts[i][0] < len(srcs[i]) and len(set(counts[i].tolist())) > 1, counts[i].tolist()


# ------------------------------------------------------------------ 5. a fixed point

def test_a_fixed_point_reports_the_counts_of_the_iterations_it_skips():
    rng = np.random.default_rng(2000)
    dst = outline(rng, 900)
    sizes = [1, 2, 70, 513, 900]
    srcs = [np.ascontiguousarray(dst[rng.choice(900, n, replace=False)]) for n in sizes]
    ident = [I.Transform() for _ in srcs]
    B = I.IcpBatch(2)
    got = B.estimate_point_to_line(srcs, [dst] * len(srcs), ident, 6, k=8, return_info=True,
                                   max_correspondence_distance=0.0)
    assert B.line_gated_counters()[:2] == (len(srcs), 0)
    B.close()
    counts = assert_items_match(srcs, [dst] * len(srcs), ident, 6, 8, 0.0, got)
    assert not got[2].any()  # exact matches: residuals 0, no update
    for n, inl in zip(sizes, counts):
        assert inl.tolist() == [n] * 6  # (the single call runs all six)


# ------------------------------------------------------------------ 6. statuses

def test_statuses_and_bits_in_a_mixed_gated_batch():
    items = mixed_items()  # [1] a NaN source point, [2] n = 0, [3] m = 0, [4] a single wall, [5] collinear targets
    s, d, T = random_item(np.random.default_rng(2100), 2, n=400, m=500)
    items.append((s + 500.0, d, T))  # all outliers
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(2)
    got = B.estimate_point_to_line(srcs, dsts, inits, 20, k=8, return_info=True, allow_failures=True,
                                   max_correspondence_distance=0.75)
    assert_items_match(srcs, dsts, inits, 20, 8, 0.75, got)
    Ts, _, inner, status, inl = got
    assert status.tolist() == [_lib.OK, _lib.OK, _lib.OK, _lib.EMPTY_DST, _lib.OK, _lib.OK, _lib.OK, _lib.OK]
    assert inl[1].max() <= len(srcs[1]) - 1  # the NaN point is gated out: not ICP_NAN_INPUT
    assert not inl[-1].any() and not inner[-1].any() and np.array_equal(bits(Ts[-1]), bits(inits[-1]))
    served, one_by_one = B.line_gated_counters()[:2]
    assert served + one_by_one == len(srcs) and one_by_one >= 2  # (n = 0 and m = 0 go one by one)
    with pytest.raises(I.IcpError, match="item 3"):
        B.estimate_point_to_line(srcs, dsts, inits, 20, k=8, max_correspondence_distance=0.75)
    # no outer iteration for the whole call: every item one by one, each as its single call
    before = B.line_gated_counters()
    got0 = B.estimate_point_to_line(srcs, dsts, inits, 0, k=8, return_info=True, allow_failures=True,
                                    max_correspondence_distance=0.75)
    assert_items_match(srcs, dsts, inits, 0, 8, 0.75, got0)
    after = B.line_gated_counters()
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (0, len(srcs), 0)
    B.close()


# ------------------------------------------------------------------ 7. hypotheses

def test_gated_hypotheses_share_one_range_and_each_equals_its_single_call():
    src, dst = load_golden(5), load_golden(6)
    rng = np.random.default_rng(8)
    inits = [I.Transform([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.4, 0.4)]) for _ in range(64)]
    B = I.IcpBatch(2)
    got = B.estimate_point_to_line_packed(src, dst, [(0, len(src), 0, len(dst), T) for T in inits], 20, k=GOLDEN_K,
                                          return_info=True, allow_failures=True, max_correspondence_distance=0.4)
    counts = assert_items_match([src] * 64, [dst] * 64, inits, 20, GOLDEN_K, 0.4, got)
    served, one_by_one, launches, refused = B.line_gated_counters()
    assert (served + one_by_one, launches, refused) == (64, 1, 0)
    B.close()
    print("first counts:", sorted(int(c[0]) for c in counts if c is not None))


# ------------------------------------------------------------------ 8. the device entry, and the ungated call beside it

def test_device_entry_equals_host_entry_twice_and_leaves_the_ungated_call_alone():
    import torch

    rng = np.random.default_rng(2200)
    B = I.IcpBatch(2)
    for count in (24, 5, 40):  # grow, shrink, grow: the batch's buffers are reused and resized
        items = [random_item(rng, 2, n=int(rng.integers(1, 1025)), m=int(rng.integers(1, 800))) for _ in range(count)]
        srcs, dsts, inits = zip(*items)
        src, dst = np.concatenate(srcs), np.concatenate(dsts)
        sf, df = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(d) for d in dsts])
        packed = [(sf[i], len(srcs[i]), df[i], len(dsts[i]), inits[i]) for i in range(count)]
        kw = dict(k=8, return_info=True)
        plain = B.estimate_point_to_line_packed(src, dst, packed, 20, **kw)
        host = B.estimate_point_to_line_packed(src, dst, packed, 20, max_correspondence_distance=0.6, **kw)
        again = B.estimate_point_to_line_packed(src, dst, packed, 20, max_correspondence_distance=0.6, **kw)
        dev = B.estimate_point_to_line_packed(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), packed, 20,
                                              max_correspondence_distance=0.6, **kw)
        after = B.estimate_point_to_line_packed(src, dst, packed, 20, **kw)
        assert len(plain) == len(after) == 4 and len(host) == 5
        for a, b in ((host, again), (host, dev), (plain, after)):
            for i in range(count):
                assert np.array_equal(bits(a[0][i]), bits(b[0][i])), i
                assert np.array_equal(a[1][i], b[1][i]), i
            assert all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))
        assert host[4].min() < max(len(s) for s in srcs)  # (the bound removes something)
        if count == 5:
            assert_items_match(srcs, dsts, inits, 20, 8, 0.6, host)
    B.close()


# ------------------------------------------------------------------ 9. what the gate is for

def test_the_gate_brings_a_partly_overlapping_scan_closer_to_the_true_pose():
    srcs, dsts, truth = [], [], []
    for seed in (11, 12, 13):
        dst, _, Tt = outline_pair(seed, 1500, 800)
        rng = np.random.default_rng(2300 + seed)
        scan = outline(np.random.default_rng(1000 + seed), 800)
        blob = rng.choice(800, 320, replace=False)  # 40 % of the scan: a blob in the open floor, 1 m from every wall
        scan[blob] = np.array([1.6, 0.0]) + rng.normal(0.0, 0.15, (320, 2))
        srcs.append(np.ascontiguousarray(moved2(scan, Tt.inverse())))
        dsts.append(dst)
        truth.append(Tt)
    assert tuple(truth[0].as_array()) == tuple(I.Transform(list(TRUE_PARAM)).as_array())
    B = I.IcpBatch(2)
    plain = B.estimate_point_to_line(srcs, dsts, None, 20, k=8)
    gated, _, _, _, inl = B.estimate_point_to_line(srcs, dsts, None, 20, k=8, return_info=True,
                                                   max_correspondence_distance=0.15)
    B.close()
    for i in range(3):
        eg, ep = pose_error(gated[i], truth[i]), pose_error(plain[i], truth[i])
        print(f"seed {11 + i}: pose error gated {eg:.3e}, ungated {ep:.3e}, kept {inl[i].tolist()}")
        assert eg < ep, (i, eg, ep)
