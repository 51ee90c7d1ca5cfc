"""Pose evaluation (Icp{2,3}d.evaluate, IcpBatch.evaluate: icp_evaluate* / icp_batch_evaluate* of include/icp_mi355x.h
section 9) against a numpy restatement of its definition, bit for bit: the correspondences come from the CPU oracle's
exact search, the per-point terms and the fold tree are restated here.  Also: the reference's left-fold error /
huber_error, statuses, host and device entries, state neutrality, map handles, and every batch item against its single
call."""
import os

import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib, synth
from icp_rust_amd.scans import load_scan2d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCANS = os.path.join(ROOT, "tests", "golden", "scans2d")
K = 1.345  # ICP_HUBER_K


def fold(v):
    """the fold of section 9: n == 0 -> +0.0, n == 1 -> v[0], else groups of 256 padded with +0.0, tree inside each"""
    v = np.asarray(v, dtype=np.float64).ravel()
    if v.size == 0:
        return np.float64(0.0)
    if v.size == 1:
        return v[0]
    while v.size > 1:
        g = np.concatenate([v, np.zeros((-v.size) % 256)]).reshape(-1, 256)
        s = 128
        while s >= 1:
            g = g[:, :s] + g[:, s:2 * s]
            s //= 2
        v = g[:, 0]
    return v[0]


def transformed(src, T):
    """q = transform_xy(T, p) for every point, no FMA (numpy forms each product and sum on its own)"""
    p = T.pose
    q = np.array(src, dtype=np.float64, copy=True)
    px, py = src[:, 0], src[:, 1]
    q[:, 0] = (p.r00 * px + p.r01 * py) + p.tx
    q[:, 1] = (p.r10 * px + p.r11 * py) + p.ty
    return q


def restate(dim, dst, src, T, r, idx):
    """(status, inliers, float fields in Quality.as_array order) by the definition"""
    n = len(src)
    if n == 0:
        return _lib.OK, 0, np.zeros(14)
    q = transformed(src, T)
    b = dst[idx.astype(np.int64)]
    ex, ey = q[:, 0] - b[:, 0], q[:, 1] - b[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        e2 = ex * ex + ey * ey
        if np.isnan(e2).any():
            return _lib.NAN_INPUT, 0, np.zeros(14)
        d2 = e2.copy()
        if dim == 3:
            dz = q[:, 2] - b[:, 2]
            d2 = d2 + dz * dz
        h = np.where(e2 <= K * K, e2, 2.0 * K * np.sqrt(e2) - K * K)
        inl = d2 <= r * r
        z = np.zeros(n)
        sd2, sx = fold(np.where(inl, d2, z)), fold(np.where(inl, q[:, 0], z))
        sy, srr = fold(np.where(inl, q[:, 1], z)), fold(np.where(inl, q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1], z))
        cnt = int(inl.sum())
        c = float(cnt)
        rmse = np.sqrt(sd2 / cnt) if cnt else 0.0
    return _lib.OK, cnt, np.array([cnt / n, rmse, sd2, fold(e2), fold(h), c, 0.0, -sy, 0.0, c, sx, -sy, sx, srr])


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))


def assert_restated(dim, dst, src, T, r, got, gidx, oidx, where):
    assert np.array_equal(gidx, oidx), (where, np.nonzero(gidx != oidx)[0][:10])
    rc, cnt, want = restate(dim, dst, src, T, r, oidx)
    assert rc == _lib.OK, where
    assert got.n == len(src) and got.inliers == cnt, (where, got.n, got.inliers, cnt)
    assert same_bits(got.as_array(), want), (where, got.as_array(), want)


def oracle_idx(dst, q, brute=False):
    if brute:
        rc, idx = O.nn_brute(dst, q)
    else:
        rc, idx = O.KdTree(dst).search(q)
    assert rc == O.OK
    return idx


def cloud(rng, dim, n, m):
    """targets with duplicates (ties), sources: a third exact copies of targets (d2 == 0 at identity), the rest noisy"""
    dst = rng.uniform(-20.0, 20.0, size=(m, dim))
    dst[7] = dst[3]
    dst[m // 2] = dst[m // 3]
    src = dst[rng.integers(0, m, size=n)].copy()
    k = n // 3
    src[k:] += rng.normal(0.0, 0.05, size=(n - k, dim))
    return src, dst


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65_537, 300_000])
def test_evaluate_equals_the_restated_definition(dim, n):
    rng = np.random.default_rng(10 * n + dim)
    m = 3000 if n < 65_537 else 40_000
    src, dst = cloud(rng, dim, n, m)
    icp = (I.Icp2d if dim == 2 else I.Icp3d)(dst)
    for T in (I.Transform(), I.Transform([rng.normal(0.0, 0.3), rng.normal(0.0, 0.3), rng.normal(0.0, 0.05)])):
        q = transformed(src, T)
        oidx = oracle_idx(dst, q)
        b = dst[oidx.astype(np.int64)]
        d2 = ((q[:, 0] - b[:, 0]) ** 2 + (q[:, 1] - b[:, 1]) ** 2) + (((q[:, 2] - b[:, 2]) ** 2) if dim == 3 else 0.0)
        for r in (0.0, float(np.sqrt(np.median(d2))), float("inf")):
            got, gidx = icp.evaluate(src, T, r, return_indices=True)
            assert_restated(dim, dst, src, T, r, got, gidx, oidx, (dim, n, r))
        # the reference's error / huber_error (left folds) on the same pairs
        oT = O.Pose(*T.pose.as_tuple())
        a2, b2 = np.ascontiguousarray(src[:, :2]), np.ascontiguousarray(b[:, :2])
        for mine, ref in ((got.error, O.error(oT, a2, b2)), (got.huber_error, O.huber_error(oT, a2, b2))):
            assert abs(mine - ref) <= 1e-12 * abs(ref), (mine, ref)
    icp.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_nan_targets_and_far_queries(dim):
    """NaN targets are never matched (the handle then searches by brute force), queries at 1e20 / 1e30 keep their exact
    neighbour -- the settings the estimator's tests use"""
    rng = np.random.default_rng(40 + dim)
    src, dst = cloud(rng, dim, 5000, 3000)
    dst[17] = np.nan
    dst[1000, dim - 1] = np.nan
    far = rng.choice(len(src), size=8, replace=False)
    src[far[:4]] = rng.normal(size=(4, dim)) * 1e20
    src[far[4:]] = rng.normal(size=(4, dim)) * 1e30
    icp = (I.Icp2d if dim == 2 else I.Icp3d)(dst)
    T = I.Transform([0.2, -0.1, 0.03])
    oidx = oracle_idx(dst, transformed(src, T), brute=True)
    for r in (0.0, 0.3, float("inf")):
        got, gidx = icp.evaluate(src, T, r, return_indices=True)
        assert_restated(dim, dst, src, T, r, got, gidx, oidx, r)


def test_far_queries_on_the_grid_engine():
    """test_gpu_parity's far queries beyond the f32 screen, 70 000 of them against 30 000 targets (grid engine)"""
    rng = np.random.default_rng(31)
    m, n = 30_000, 70_000
    dst = rng.normal(size=(m, 3)) * 5
    src = dst[rng.integers(0, m, size=n)] + rng.normal(size=(n, 3)) * 0.05
    far = rng.choice(n, size=12, replace=False)
    src[far[:6]] = rng.normal(size=(6, 3)) * 1e20
    src[far[6:]] = rng.normal(size=(6, 3)) * 1e30
    icp = I.Icp3d(dst)
    assert I.lib().icp_get_nn_mode(icp._h) == I.NN_GRID
    T = I.Transform()
    O.set_threads(16)
    try:
        oidx = oracle_idx(dst, transformed(src, T), brute=True)
    finally:
        O.set_threads(1)
    for r in (0.1, float("inf")):
        got, gidx = icp.evaluate(src, T, r, return_indices=True)
        assert_restated(3, dst, src, T, r, got, gidx, oidx, r)


def test_million_point_pair_equals_the_restatement():
    src, dst = synth.synthetic_pair(1_000_000, 1_000_000)  # bench.py's pair
    icp = I.Icp3d(dst)
    T = I.Transform(list(synth.TRUTH_PARAM))
    got, gidx = icp.evaluate(src, T, 0.05, return_indices=True)
    O.set_threads(16)
    try:
        oidx = oracle_idx(dst, transformed(src, T))
    finally:
        O.set_threads(1)
    assert_restated(3, dst, src, T, 0.05, got, gidx, oidx, "1M")


def test_statuses_of_the_edge_cases():
    rng = np.random.default_rng(3)
    src, dst = cloud(rng, 2, 100, 200)
    icp = I.Icp2d(dst)
    T = I.Transform([0.1, 0.0, 0.01])
    q = icp.evaluate(np.zeros((0, 2)), T, 1.0)  # n == 0: OK, zeros
    assert q.n == 0 and q.inliers == 0 and same_bits(q.as_array(), np.zeros(14))
    empty = I.Icp2d(np.zeros((0, 2)))
    assert empty.evaluate(np.zeros((0, 2)), T).n == 0  # (n == 0 comes first)
    with pytest.raises(I.IcpError) as e:
        empty.evaluate(src, T)
    assert e.value.status == _lib.EMPTY_DST
    bad = src.copy()
    bad[3, 1] = np.nan
    with pytest.raises(I.IcpError) as e:
        icp.evaluate(bad, T)
    assert e.value.status == _lib.NAN_INPUT
    for r in (-1.0, float("nan")):
        with pytest.raises(I.IcpError) as e:
            icp.evaluate(src, T, r)
        assert e.value.status == _lib.BAD_ARGUMENT
    assert icp.evaluate(src, T, 1.0).n == 100  # (the handle is usable after each of them)


def test_device_entry_equals_host_entry():
    import torch

    rng = np.random.default_rng(8)
    for dim, n, m in ((2, 700, 650), (3, 100_000, 80_000)):
        src, dst = cloud(rng, dim, n, m)
        icp = (I.Icp2d if dim == 2 else I.Icp3d)(dst)
        T = I.Transform([0.05, -0.02, 0.01])
        h, hi = icp.evaluate(src, T, 0.04, return_indices=True)
        d, di = icp.evaluate(torch.from_numpy(src).cuda(), T, 0.04, return_indices=True)
        assert np.array_equal(hi, di) and h.inliers == d.inliers and same_bits(h.as_array(), d.as_array())
        icp.close()


@pytest.mark.parametrize("n,m", [(600, 650), (100_000, 80_000)])
def test_evaluate_leaves_the_registration_state_alone(n, m):
    """estimate -> evaluate -> estimate on one handle == estimate -> estimate on a twin (pose, indices, inner counts)"""
    src, dst = synth.synthetic_pair(n, m)
    a, b = I.Icp3d(dst), I.Icp3d(dst)
    Ta, ia, na = a.estimate(src, I.Transform(), 5, return_info=True)
    Tb, ib, nb = b.estimate(src, I.Transform(), 5, return_info=True)
    assert np.array_equal(Ta.as_array(), Tb.as_array()) and np.array_equal(ia, ib)
    a.evaluate(src, Ta, 0.1)
    a.evaluate(src, I.Transform([0.4, -0.3, 0.05]), float("inf"), return_indices=True)
    Ta, ia, na = a.estimate(src, Ta, 5, return_info=True)
    Tb, ib, nb = b.estimate(src, Tb, 5, return_info=True)
    assert np.array_equal(Ta.as_array(), Tb.as_array()) and np.array_equal(ia, ib) and np.array_equal(na, nb)


def test_map_handle_after_append_and_both_engines():
    src, dst = synth.synthetic_pair(30_000, 40_000)
    more = synth.synthetic_pair(20_000, 1, seed=synth.SEED + 5)[0]
    icp = I.Icp3d(dst)
    icp.append(more, I.Transform([0.1, 0.2, 0.03]))
    full = icp.read_targets()
    fresh = I.Icp3d(full)
    brute, grid = I.Icp3d(full, nn_mode=I.NN_BRUTE), I.Icp3d(full, nn_mode=I.NN_GRID)
    T = I.Transform([0.3, -0.2, 0.015])
    oidx = oracle_idx(full, transformed(src, T))
    for r in (0.0, 0.05, float("inf")):
        want, widx = fresh.evaluate(src, T, r, return_indices=True)
        assert_restated(3, full, src, T, r, want, widx, oidx, r)
        for h in (icp, brute, grid):
            got, gidx = h.evaluate(src, T, r, return_indices=True)
            assert np.array_equal(gidx, widx) and got.inliers == want.inliers
            assert same_bits(got.as_array(), want.as_array())


# ---- the batch ---------------------------------------------------------------------------------------------------

def single(dim, dst, src, T, r):
    icp = (I.Icp2d if dim == 2 else I.Icp3d)(dst)
    try:
        return _lib.OK, icp.evaluate(src, T, r)
    except I.IcpError as e:
        return e.status, None
    finally:
        icp.close()


def assert_items_match(dim, srcs, dsts, Ts, r, got):
    qs, status = got
    for i, (s, d, T) in enumerate(zip(srcs, dsts, Ts)):
        rc, q = single(dim, d, s, T, r)
        assert status[i] == rc, (i, status[i], rc)
        if rc != _lib.OK:
            assert qs[i] is None
            continue
        assert (qs[i].n, qs[i].inliers) == (q.n, q.inliers), i
        assert same_bits(qs[i].as_array(), q.as_array()), (i, qs[i].as_array(), q.as_array())


def random_item(rng, dim, n=None, m=None):
    n = int(rng.integers(1, 1025)) if n is None else n
    m = int(rng.integers(1, 2049)) if m is None else m
    dst = rng.uniform(-20.0, 20.0, size=(m, dim))
    src = dst[rng.integers(0, m, size=n)] + rng.normal(0.0, 0.05, size=(n, dim))
    T = I.Transform([rng.normal(0.0, 0.05), rng.normal(0.0, 0.05), rng.normal(0.0, 0.01)])
    return src, dst, T


@pytest.mark.parametrize("dim", [2, 3])
def test_random_batch_items_equal_their_single_calls(dim):
    rng = np.random.default_rng(200 + dim)
    fixed_n = [1, 2, 255, 256, 257, 511, 512, 513, 1000, 1024]
    items = [random_item(rng, dim, n=fixed_n[k] if k < len(fixed_n) else None,
                         m=2048 if k == 3 else (1 if k == 4 else None)) for k in range(120)]
    srcs, dsts, Ts = zip(*items)
    B = I.IcpBatch(dim)
    for r in (0.05, float("inf")):
        got = B.evaluate(srcs, dsts, Ts, r, allow_failures=True, return_status=True)
        assert_items_match(dim, srcs, dsts, Ts, r, got)
    assert B.evaluate_counters() == (240, 0, 2)


def golden_scans():
    return [load_scan2d(os.path.join(SCANS, f"{k:03d}.txt")) for k in range(1, 41)]


def test_golden_scan_pairs_at_their_estimated_poses():
    scans = golden_scans()
    srcs, dsts = scans[:-1], scans[1:]
    B = I.IcpBatch(2)
    Ts = B.estimate(srcs, dsts, None, 20)
    got = B.evaluate(srcs, dsts, Ts, 0.2, allow_failures=True, return_status=True)
    assert_items_match(2, srcs, dsts, Ts, 0.2, got)
    assert B.evaluate_counters() == (len(srcs), 0, 1)


def test_hypotheses_share_one_range_and_each_equals_its_single_call():
    scans = golden_scans()
    src, dst = scans[4], scans[5]
    rng = np.random.default_rng(7)
    Ts = [I.Transform([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.4, 0.4)]) for _ in range(256)]
    B = I.IcpBatch(2)
    got = B.evaluate_packed(src, dst, [(0, len(src), 0, len(dst), T) for T in Ts], 0.3, allow_failures=True,
                            return_status=True)
    assert_items_match(2, [src] * 256, [dst] * 256, Ts, 0.3, got)
    assert B.evaluate_counters() == (256, 0, 1)


def test_mixed_batch_of_edge_items_keeps_every_single_call_status_and_bits():
    rng = np.random.default_rng(5)
    items, kernel = [], []

    def add(item, in_kernel):
        items.append(item)
        kernel.append(in_kernel)

    add(random_item(rng, 2), True)
    add(random_item(rng, 2, n=1500, m=300), False)  # beyond one workgroup: n
    add(random_item(rng, 2, n=300, m=3000), False)  # ... m
    s, d, T = random_item(rng, 2, n=300, m=400)
    d[17] = np.nan
    add((s, d, T), True)  # a NaN target: never matched
    s, d, T = random_item(rng, 2, n=300, m=400)
    s[3, 1] = np.nan
    add((s, d, T), True)  # a NaN source: ICP_NAN_INPUT
    s, d, T = random_item(rng, 2, n=50, m=10)
    d[:] = np.nan
    add((s, d, T), True)  # no finite target: index 0, a NaN residual
    s, _, T = random_item(rng, 2, n=40, m=10)
    add((s, np.zeros((0, 2)), T), False)  # m = 0: ICP_EMPTY_DST
    _, d, T = random_item(rng, 2, n=1, m=30)
    add((np.zeros((0, 2)), d, T), False)  # n = 0: OK, zeros
    add(random_item(rng, 2, n=1, m=30), True)
    s, d, T = random_item(rng, 2, n=600, m=700)
    s[10] = 1e30
    add((s, d, T), True)  # a far query
    add(random_item(rng, 2), True)
    srcs, dsts, Ts = zip(*items)
    B = I.IcpBatch(2)
    got = B.evaluate(srcs, dsts, Ts, 0.1, allow_failures=True, return_status=True)
    assert_items_match(2, srcs, dsts, Ts, 0.1, got)
    status = got[1]
    assert status[4] == _lib.NAN_INPUT and status[5] == _lib.NAN_INPUT and status[6] == _lib.EMPTY_DST
    assert status[7] == _lib.OK and got[0][7].n == 0
    served, one_by_one, launches = B.evaluate_counters()
    assert (served, one_by_one, launches) == (sum(kernel), len(kernel) - sum(kernel), 1)
    with pytest.raises(I.IcpError, match="item 4"):
        B.evaluate(srcs, dsts, Ts, 0.1)


def test_batch_device_entry_equals_host_entry_and_two_calls_are_identical():
    import torch

    rng = np.random.default_rng(11)
    B = I.IcpBatch(3)
    for count in (40, 7, 90):  # grow, shrink, grow: the batch's buffers are reused and resized
        items = [random_item(rng, 3) for _ in range(count)]
        srcs, dsts, Ts = zip(*items)
        src, dst = np.concatenate(srcs), np.concatenate(dsts)
        sf, df = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(d) for d in dsts])
        packed = [(sf[i], len(srcs[i]), df[i], len(dsts[i]), Ts[i]) for i in range(count)]
        host = B.evaluate_packed(src, dst, packed, 0.08, return_status=True)
        again = B.evaluate_packed(src, dst, packed, 0.08, return_status=True)
        dev = B.evaluate_packed(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), packed, 0.08,
                                return_status=True)
        for other in (again, dev):
            assert np.array_equal(host[1], other[1])
            for a, b in zip(host[0], other[0]):
                assert a.inliers == b.inliers and same_bits(a.as_array(), b.as_array())
        if count == 7:
            assert_items_match(3, srcs, dsts, Ts, 0.08, host)
