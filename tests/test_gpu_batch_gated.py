"""Gated batched point-to-point registration (IcpBatch.estimate*(..., max_correspondence_distance=r),
include/icp_mi355x.h section 21): every item's status, pose, indices, inner counts and inlier counts equal, bit for bit,
what a fresh Icp{2,3}d(dst_i) returns from estimate(src_i, init_i, max_iter, max_correspondence_distance=r) -- whichever
way the batch served it -- and the CPU statement of the gate (tests/test_gpu_gated.py: restate, with the oracle's
search)."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from test_gpu_batch import golden_scans, random_item
from test_gpu_gated import restate, searcher
from test_line_abi import outline

pytestmark = pytest.mark.gpu

INF = float("inf")


def bits(T):
    return np.asarray(T.as_array() if hasattr(T, "as_array") else T, dtype=np.float64).view(np.uint64)


def single(dim, dst, src, init, max_iter, r):
    """(status, pose, indices, inner counts, inlier counts) of the single gated call on a fresh handle"""
    icp = (I.Icp2d if dim == 2 else I.Icp3d)(dst)
    try:
        T, idx, inner, inl = icp.estimate(src, init, max_iter, return_info=True, max_correspondence_distance=r)
        return _lib.OK, T.as_array(), idx, inner, inl
    except I.IcpError as e:
        return e.status, None, None, None, None
    finally:
        icp.close()


def assert_items_match(dim, srcs, dsts, inits, max_iter, r, got):
    """every item against its single call; returns the single calls' inlier counts (None for a failed item)"""
    Ts, idxs, inner, status, inliers = got
    assert len(Ts) == len(srcs) and inliers.shape == inner.shape == (len(srcs), max_iter)
    counts = []
    for i, (s, d, T0) in enumerate(zip(srcs, dsts, inits)):
        rc, pose, idx, inn, inl = single(dim, d, s, T0, max_iter, r)
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


def room(rng, m, dim):
    """m samples of a room's outline; three dimensions: the walls between z = 0 and z = 1"""
    xy = outline(rng, m)
    return xy if dim == 2 else np.ascontiguousarray(np.column_stack([xy, rng.uniform(0.0, 1.0, m)]))


# ------------------------------------------------------------------ 1. counts known by construction

EDGE_PAIRS = [(1, 0), (1, 1), (2, 1), (2, 2), (3, 0), (64, 63), (65, 64), (66, 65), (512, 512), (513, 511), (513, 512),
              (600, 513), (768, 512), (768, 513), (769, 512), (769, 513), (1024, 0), (1024, 1), (1024, 512), (1024, 513),
              (1024, 1023), (1024, 1024)]


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
    """n source points of which exactly `kept` lie within millimetres of a target; the others are 100 m away, so a bound
    of 0.5 keeps exactly `kept` pairs in every iteration"""
    dim = dst.shape[1]
    src = dst[rng.integers(0, len(dst), n)] + rng.normal(0.0, 3e-3, (n, dim))
    out = outlier_places(n, n - kept, how)
    src[out] = 100.0 + rng.uniform(-1.0, 1.0, (len(out), dim))
    return np.ascontiguousarray(src)


@pytest.mark.parametrize("dim", [2, 3])
def test_counts_known_by_construction_across_every_workgroup_size_and_fold_tree(dim):
    rng = np.random.default_rng(2500 + dim)
    dst = room(rng, 700, dim)
    srcs, dsts, want = [], [], []
    for how in ("interleaved", "waves", "front"):
        for n, kept in EDGE_PAIRS:
            srcs.append(known_kept_item(rng, dst, n, kept, how))
            dsts.append(dst)
            want.append(kept)
    inside = len(srcs)
    big = room(rng, 2049, dim)
    srcs += [known_kept_item(rng, dst, 1025, 900, "interleaved"), known_kept_item(rng, big, 300, 200, "interleaved")]
    dsts += [dst, big]  # n = 1025 and m = 2049: outside the limits, one by one
    want += [900, 200]
    inits = [I.Transform([1e-3, -2e-3, 1e-3]) for _ in srcs]
    B = I.IcpBatch(dim)
    got = B.estimate(srcs, dsts, inits, 8, return_info=True, allow_failures=True, max_correspondence_distance=0.5)
    counters, ungated = B.gated_counters(), B.counters()
    B.close()
    assert got[3].tolist() == [_lib.OK] * len(srcs)
    for i, kept in enumerate(want):
        assert got[4][i].tolist() == [kept] * 8, (i, len(srcs[i]), kept, got[4][i].tolist())
    assert_items_match(dim, srcs, dsts, inits, 8, 0.5, got)
    print("inner counts by kept:", [(len(s), k, got[2][i].tolist()) for i, (s, k) in enumerate(zip(srcs, want))][:22])
    assert counters == (inside, 2, 3, 0), counters  # every item within the limits in a launch, none handed back
    assert ungated == (0, 0, 0, 0)


# ------------------------------------------------------------------ 2. the CPU statement

def noisy_scene(dim, n):
    """n re-observations of a room's outline with centimetres of noise, from a pose a few centimetres off; the bound
    (one sigma of the noise) keeps about a third of the pairs"""
    rng = np.random.default_rng(2600 + 10 * n + dim)
    dst = room(rng, 900, dim)
    src = dst[rng.integers(0, len(dst), n)] + rng.normal(0.0, 0.03, (n, dim))
    return np.ascontiguousarray(src), dst, I.Transform([0.01, -0.01, 0.004]), 0.03


def tie_scene(dim, n):
    """a run of equal residuals at the median (test_gpu_batch.py: equal_run_pair, the run 40 % of n at every n): targets
    on a grid of spacing 4 with coordinates in eighths, 40 % of the sources off their target by exactly (0.5, 0.25), 30 %
    by less in both coordinates, 30 % by more; the bound 0.56 (0.5^2 + 0.25^2 = 0.3125 < 0.56^2) keeps the run and the
    nearer 30 %, so the kept residuals' medians lie in the run"""
    assert dim == 2
    rng = np.random.default_rng(2700 + n)
    side = int(np.ceil(np.sqrt(n)))
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    dst = (np.stack([gx.ravel(), gy.ravel()], axis=1)[:n] * 4.0 + rng.integers(0, 8, size=(n, 2)) / 8.0).astype(np.float64)
    off = np.empty((n, 2))
    k = max(int(0.4 * n), 1)
    off[:k] = (0.5, 0.25)
    h = (n - k) // 2
    off[k:k + h] = (0.5, 0.25) - rng.integers(1, 32, size=(h, 2)) / 128.0
    off[k + h:] = (0.5, 0.25) + rng.integers(1, 64, size=(n - k - h, 2)) / 128.0
    order = rng.permutation(n)  # (the run is spread over the waves)
    return np.ascontiguousarray((dst + off)[order]), np.ascontiguousarray(dst), I.Transform(), 0.56


def blob_scene(dim, n, seed=0):
    """40 % of the scan replaced by a blob in the open floor that the target does not hold; the rest re-observes the
    room from the pose (0.25, -0.15, 0.04) away"""
    rng = np.random.default_rng(2800 + 10 * n + dim + 1000 * seed)
    dst = room(rng, 1500, dim)
    scan = room(rng, n, dim)
    blob = rng.choice(n, int(0.4 * n), replace=False)
    scan[blob, :2] = np.array([1.6, 0.0]) + rng.normal(0.0, 0.15, (len(blob), 2))
    true = O.transform_new(np.array([0.25, -0.15, 0.04]))
    src = scan.copy()
    src[:, :2] = O.transform_apply_many(O.transform_inverse(true), np.ascontiguousarray(scan[:, :2]))
    return np.ascontiguousarray(src), dst, I.Transform(), 0.5


STATEMENT_SCENES = [("noisy", 2, noisy_scene), ("noisy", 3, noisy_scene), ("ties", 2, tie_scene), ("blob", 2, blob_scene),
                    ("blob", 3, blob_scene)]
STATEMENT_SIZES = [2, 3, 65, 513, 769, 1024]
STATEMENT_ITERATIONS = 6


def oracle_pose(T):
    return O.Pose(*T.pose.as_tuple())


def restated(dim, dst, src, init, max_iter, r):
    """a batch item folds in the caller's order"""
    return restate(dim, dst, src, oracle_pose(init), max_iter, r, np.arange(len(src)), searcher(dst, True))


@pytest.mark.parametrize("bound", ["inf", "finite"])
@pytest.mark.parametrize("name,dim,scene", STATEMENT_SCENES, ids=[f"{s[0]}{s[1]}d" for s in STATEMENT_SCENES])
def test_one_gated_batched_call_equals_the_cpu_statement(name, dim, scene, bound):
    made = [scene(dim, n) for n in STATEMENT_SIZES]
    srcs, dsts, inits, rs = zip(*made)
    r = INF if bound == "inf" else rs[0]
    assert len(set(rs)) == 1
    B = I.IcpBatch(dim)
    Ts, idxs, inner, status, inl = B.estimate(srcs, dsts, inits, STATEMENT_ITERATIONS, return_info=True,
                                              max_correspondence_distance=r)
    served, one_by_one, _, refused = B.gated_counters()
    B.close()
    print(f"{name} {dim}-D r = {r}: served {served}, one by one {one_by_one}")
    assert served + one_by_one == len(srcs) and refused == 0
    if name != "ties":  # (a run of ties beyond the lists is handed back by the 512- and 768-thread workgroups)
        assert one_by_one == 0, (name, dim, r, served, one_by_one)  # the kernel itself stands against the statement
    for i, n in enumerate(STATEMENT_SIZES):
        oT, oidx, oinner, oinl = restated(dim, dsts[i], srcs[i], inits[i], STATEMENT_ITERATIONS, r)
        where = (name, dim, n, r)
        print(f"{name} {dim}-D n={n} r={r}: inliers {oinl.tolist()}, inner {oinner.tolist()}")
        if r == INF:
            assert np.all(oinl == n), where
        elif n >= 65:
            assert 0 < oinl[0] < n, where  # the bound removes some pairs and keeps others
        assert status[i] == _lib.OK, where
        assert np.array_equal(idxs[i], oidx), where
        assert np.array_equal(inner[i], oinner), (where, inner[i].tolist(), oinner.tolist())
        assert np.array_equal(inl[i], oinl), (where, inl[i].tolist(), oinl.tolist())
        assert np.array_equal(bits(Ts[i]), bits(oT)), (where, Ts[i].as_array(), oT.as_array())


# ------------------------------------------------------------------ 3, 4. the golden scan pairs

def golden_pairs():
    scans = golden_scans()[:11]
    return scans[:10] + [scans[0]], scans[1:11] + [scans[9]]  # 001 -> 002 ... 010 -> 011, and 001 -> 010


def test_an_infinite_bound_returns_the_bits_of_the_ungated_batch_call():
    srcs, dsts = golden_pairs()
    ident = [I.Transform() for _ in srcs]
    B = I.IcpBatch(2)
    Ts, idxs, inner, status = B.estimate(srcs, dsts, ident, 20, return_info=True)
    gTs, gidxs, ginner, gstatus, inl = B.estimate(srcs, dsts, ident, 20, return_info=True,
                                                  max_correspondence_distance=INF)
    gated, plain = B.gated_counters(), B.counters()
    B.close()
    assert gated[0] + gated[1] == len(srcs) and gated[3] == 0 and gated[:2] == plain[:2], (gated, plain)
    assert np.array_equal(status, gstatus) and np.array_equal(inner, ginner)
    for i, s in enumerate(srcs):
        assert np.array_equal(bits(Ts[i]), bits(gTs[i])), i
        assert np.array_equal(idxs[i], gidxs[i]), i
        assert np.all(inl[i] == len(s)), (i, inl[i].tolist())  # (an iteration the fixed-point rule skips repeats one)


def test_golden_pairs_at_a_bound_that_bites_equal_their_single_calls():
    srcs, dsts = golden_pairs()
    ident = [I.Transform() for _ in srcs]
    for i in range(len(srcs)):  # one call per bound: each pair's median nearest-neighbour distance at the identity
        icp = I.Icp2d(dsts[i])
        _, idx, _ = icp.estimate(srcs[i], I.Transform(), 1, return_info=True)
        icp.close()
        e = srcs[i] - dsts[i][idx]
        r = float(np.sqrt(np.median(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])))  # the first gate's d2
        B = I.IcpBatch(2)
        got = B.estimate(srcs, dsts, ident, 20, return_info=True, max_correspondence_distance=r)
        served, one_by_one, _, refused = B.gated_counters()
        B.close()
        assert served + one_by_one == len(srcs) and refused == 0
        counts = assert_items_match(2, srcs, dsts, ident, 20, r, got)
        print(f"r = {r:.5f} (pair {i}): served {served}, inliers of the pair {counts[i].tolist()}")
        assert 0 < counts[i][0] < len(srcs[i]) and len(set(counts[i].tolist())) > 1, counts[i].tolist()


# ------------------------------------------------------------------ 5. r = 0

@pytest.mark.parametrize("dim", [2, 3])
def test_a_zero_bound_on_exact_subsets_applies_no_update(dim):
    rng = np.random.default_rng(2900 + dim)
    dst = room(rng, 900, dim)
    sizes = [1, 2, 70, 513, 769, 900]
    srcs = [np.ascontiguousarray(dst[rng.choice(900, n, replace=False)]) for n in sizes]
    ident = [I.Transform() for _ in srcs]
    B = I.IcpBatch(dim)
    got = B.estimate(srcs, [dst] * len(srcs), ident, 6, return_info=True, max_correspondence_distance=0.0)
    served, one_by_one, _, refused = B.gated_counters()
    B.close()
    # (residuals that are all zero are one run of ties: a workgroup of 512 or 768 threads hands a run longer than its
    # lists back, and the item goes one by one)
    assert served + one_by_one == len(srcs) and served >= 4 and refused == 0, (served, one_by_one, refused)
    counts = assert_items_match(dim, srcs, [dst] * len(srcs), ident, 6, 0.0, got)
    assert not got[2].any()  # exact matches: residuals 0, no update
    for n, inl, row in zip(sizes, counts, got[4]):
        assert inl.tolist() == row.tolist() == [n] * 6


# ------------------------------------------------------------------ 6. the 3-D distance

def test_the_3d_gate_uses_the_3d_distance():
    """a third of the points differ from a target in z only: a gate on the xy distance would keep them"""
    rng = np.random.default_rng(3000)
    dst = room(rng, 1500, 3)
    srcs, z_only = [], []
    for n in (300, 700, 1000):
        src = dst[rng.choice(1500, n, replace=False)] + rng.normal(0.0, 2e-3, (n, 3))
        far = rng.choice(n, n // 3, replace=False)
        src[far] = dst[rng.integers(0, 1500, len(far))]
        src[far, 2] += 5.0  # exactly a target in xy, far in z
        srcs.append(np.ascontiguousarray(src))
        z_only.append(len(far))
    ident = [I.Transform([2e-3, -1e-3, 1e-3]) for _ in srcs]
    B = I.IcpBatch(3)
    got = B.estimate(srcs, [dst] * 3, ident, 5, return_info=True, max_correspondence_distance=0.5)
    assert B.gated_counters()[:2] == (3, 0)
    B.close()
    assert_items_match(3, srcs, [dst] * 3, ident, 5, 0.5, got)
    for i, s in enumerate(srcs):
        assert got[4][i].tolist() == [len(s) - z_only[i]] * 5, (i, got[4][i].tolist())
        oT, oidx, oinner, oinl = restated(3, dst, s, ident[i], 5, 0.5)
        assert np.array_equal(got[4][i], oinl) and np.array_equal(bits(got[0][i]), bits(oT)), i


# ------------------------------------------------------------------ 7. a mixed batch

def mixed_items(dim):
    rng = np.random.default_rng(3100 + dim)
    items = [random_item(rng, dim, n=300, m=400)]
    s, d, T = random_item(rng, dim, n=300, m=400)
    s[3, 1] = np.nan
    items.append((s, d, T))  # [1] a NaN source coordinate: dropped by the gate
    _, d, T = random_item(rng, dim, n=1, m=30)
    items.append((np.zeros((0, dim)), d, T))  # [2] n = 0
    s, _, T = random_item(rng, dim, n=40, m=10)
    items.append((s, np.zeros((0, dim)), T))  # [3] m = 0: ICP_EMPTY_DST
    x = np.linspace(-3, 3, 500)
    line = np.column_stack([x, 0.5 * x + 1.0] + ([0.25 * x] if dim == 3 else []))
    s = line[rng.integers(0, 500, 350)] + rng.normal(0.0, 5e-3, size=(350, dim))
    items.append((np.ascontiguousarray(s), np.ascontiguousarray(line), I.Transform([0.01, -0.01, 0.002])))  # [4] collinear
    items.append(random_item(rng, dim, n=900, m=1500))
    s, d, T = random_item(rng, dim, n=400, m=500)
    items.append((s + 500.0, d, T))  # [6] all outliers
    return items


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("r", [0.75, INF])
def test_statuses_and_bits_in_a_mixed_gated_batch(dim, r):
    srcs, dsts, inits = zip(*mixed_items(dim))
    B = I.IcpBatch(dim)
    got = B.estimate(srcs, dsts, inits, 20, return_info=True, allow_failures=True, max_correspondence_distance=r)
    assert_items_match(dim, srcs, dsts, inits, 20, r, got)
    Ts, _, inner, status, inl = got
    assert status.tolist() == [_lib.OK, _lib.OK, _lib.OK, _lib.EMPTY_DST, _lib.OK, _lib.OK, _lib.OK]
    assert inl[1].max() <= len(srcs[1]) - 1  # the NaN point is gated out: not ICP_NAN_INPUT
    if r == INF:
        assert inl[1].tolist() == [len(srcs[1]) - 1] * 20 and inl[6].tolist() == [len(srcs[6])] * 20
    else:
        assert not inl[6].any() and not inner[6].any() and np.array_equal(bits(Ts[6]), bits(inits[6]))
    served, one_by_one = B.gated_counters()[:2]
    assert served + one_by_one == len(srcs) and one_by_one >= 2  # (n = 0 and m = 0 go one by one)
    with pytest.raises(I.IcpError, match="item 3"):
        B.estimate(srcs, dsts, inits, 20, max_correspondence_distance=r)
    # no outer iteration for the whole call: every item one by one, each as its single call
    before = B.gated_counters()
    got0 = B.estimate(srcs, dsts, inits, 0, return_info=True, allow_failures=True, max_correspondence_distance=r)
    assert_items_match(dim, srcs, dsts, inits, 0, r, got0)
    after = B.gated_counters()
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (0, len(srcs), 0)
    B.close()


# ------------------------------------------------------------------ 8. hypotheses

def test_gated_hypotheses_share_one_range_and_each_equals_its_single_call():
    scans = golden_scans()
    src, dst = scans[4], scans[5]
    rng = np.random.default_rng(8)
    inits = [I.Transform([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.4, 0.4)]) for _ in range(64)]
    B = I.IcpBatch(2)
    got = B.estimate_packed(src, dst, [(0, len(src), 0, len(dst), T) for T in inits], 20, return_info=True,
                            allow_failures=True, max_correspondence_distance=0.4)
    counts = assert_items_match(2, [src] * 64, [dst] * 64, inits, 20, 0.4, got)
    served, one_by_one, launches, refused = B.gated_counters()
    assert (served + one_by_one, launches, refused) == (64, 1, 0)
    Ts, errs = B.estimate_hypotheses(src, dst, inits, 20, max_correspondence_distance=0.4)
    B.close()
    assert errs.shape == (64,) and np.all(np.isfinite(errs))
    for k in range(64):
        assert np.array_equal(bits(Ts[k]), bits(got[0][k])), k
    for k in range(0, 64, 9):
        assert errs[k] == I.huber_error(Ts[k], src, dst[got[1][k].astype(np.int64)])
    print("first counts:", sorted(int(c[0]) for c in counts if c is not None))


# ------------------------------------------------------------------ 9. the entries, and the ungated call beside them

@pytest.mark.parametrize("dim", [2, 3])
def test_device_entry_equals_host_entry_twice_and_leaves_the_ungated_call_alone(dim):
    import torch

    rng = np.random.default_rng(3200 + dim)
    B = I.IcpBatch(dim)
    for count in (24, 5, 40):  # grow, shrink, grow: the batch's buffers are reused and resized
        items = [random_item(rng, dim, n=int(rng.integers(1, 1025)), m=int(rng.integers(1, 800))) for _ in range(count)]
        srcs, dsts, inits = zip(*items)
        src, dst = np.concatenate(srcs), np.concatenate(dsts)
        sf, df = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(d) for d in dsts])
        packed = [(sf[i], len(srcs[i]), df[i], len(dsts[i]), inits[i]) for i in range(count)]
        plain = B.estimate_packed(src, dst, packed, 20, return_info=True)
        section8 = B.counters()
        host = B.estimate_packed(src, dst, packed, 20, return_info=True, max_correspondence_distance=0.6)
        again = B.estimate_packed(src, dst, packed, 20, return_info=True, max_correspondence_distance=0.6)
        dev = B.estimate_packed(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), packed, 20, return_info=True,
                                max_correspondence_distance=0.6)
        assert B.counters() == section8  # the gated calls leave section 8's counters alone
        after = B.estimate_packed(src, dst, packed, 20, return_info=True)
        assert len(plain) == len(after) == 4 and len(host) == 5
        for a, b in ((host, again), (host, dev), (plain, after)):
            for i in range(count):
                assert np.array_equal(bits(a[0][i]), bits(b[0][i])), i
                assert np.array_equal(a[1][i], b[1][i]), i
            assert all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))
        assert host[4].min() < max(len(s) for s in srcs)  # (the bound removes something)
        if count == 5:
            assert_items_match(dim, srcs, dsts, inits, 20, 0.6, host)
    B.close()


# ------------------------------------------------------------------ 10. what the gate is for

BLOB_SEEDS = (1, 2, 3)


def pose_error(T, true):
    return float(np.abs(np.asarray(T.as_array()) - np.asarray(true.as_array())).max())


def test_the_gate_brings_a_scan_with_a_blob_closer_to_the_true_pose():
    """blob_scene at n = 800 (320 points of the scan in a blob the target does not hold), bound 0.5, 20 iterations.  The
    restatement's errors against the true pose (the largest difference of a pose entry), gated / ungated:
    seed 1: 2.766e-03 / 1.015; seed 2: 3.222e-03 / 1.001; seed 3: 3.004e-03 / 1.024 (480 pairs kept in every iteration).
    The assertion is the ordering."""
    true = O.transform_new(np.array([0.25, -0.15, 0.04]))
    made = [blob_scene(2, 800, seed) for seed in BLOB_SEEDS]
    srcs, dsts, inits, rs = zip(*made)
    B = I.IcpBatch(2)
    plain = B.estimate(srcs, dsts, inits, 20)
    gated, _, _, _, inl = B.estimate(srcs, dsts, inits, 20, return_info=True, max_correspondence_distance=rs[0])
    assert B.gated_counters()[:2] == (3, 0)
    B.close()
    for i, seed in enumerate(BLOB_SEEDS):
        oT, _, _, oinl = restated(2, dsts[i], srcs[i], inits[i], 20, rs[i])
        assert np.array_equal(bits(gated[i]), bits(oT)) and np.array_equal(inl[i], oinl), seed
        eg, ep = pose_error(gated[i], true), pose_error(plain[i], true)
        print(f"seed {seed}: pose error gated {eg:.3e}, ungated {ep:.3e}, kept {inl[i].tolist()}")
        assert eg < ep, (seed, eg, ep)
