"""Point-to-line pose quality (Icp2d.evaluate_point_to_line, IcpBatch.evaluate_point_to_line*: include/icp_mi355x.h
section 16) against a numpy restatement of its definition, bit for bit: the correspondences are checked against the CPU
oracle's exact search first, the per-point terms and the fold tree are restated (tests/test_line_quality_abi.py) on the
handle's own targets and line normals.  Also: the fields it shares with Icp2d.evaluate, the information matrix against
an independent float64 sum of J J^T, statuses, host and device entries, state neutrality, map handles (append, crop), a
corridor whose axis the line residual cannot see next to a room it can -- and the batch, every item against the single
call on a fresh handle, whichever way the batch served it."""
import ctypes as C

import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from test_gpu_batch import random_item
from test_line_abi import GOLDEN_K, lift, load_golden, moved2, outline
from test_line_quality_abi import (INF, NFLOATS, SCENE_K, closed_room, corridor, restate, scene_scan, terms)

pytestmark = pytest.mark.gpu

M_LINE, N_LINE = 2048, 1024  # the largest item a workgroup serves
POSE = [0.12, -0.07, 0.04]


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.set_threads(16)
    yield
    O.set_threads(1)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))


def oracle_idx(dst, src, T):
    rc, idx = O.KdTree(lift(dst)).search(lift(moved2(src, T)))
    assert rc == O.OK
    return idx


def assert_restated(dst, nrm, src, T, r, got, gidx, oidx, where):
    assert np.array_equal(gidx, oidx), (where, np.nonzero(gidx != oidx)[0][:10])
    rc, cnt, want = restate(dst, nrm, src, T, r, oidx)
    assert rc == _lib.OK, where
    print(where, "inliers", got.inliers, "of", got.n, "line_rmse", got.line_rmse, "eig", got.translation_eig)
    assert got.n == len(src) and got.inliers == cnt, (where, got.n, got.inliers, cnt)
    assert same_bits(got.as_array(), want), (where, got.as_array(), want)


def scan_of(rng, dst, n, T, sigma=0.02):
    """n samples of the targets with noise, in the frame the pose T maps into the targets' frame"""
    world = dst[rng.integers(0, len(dst), n)] + rng.normal(size=(n, 2)) * sigma
    return np.ascontiguousarray(moved2(np.ascontiguousarray(world), T.inverse()))


def half_bound(dst, nrm, src, T, idx):
    """a finite bound that keeps about half the points"""
    return float(np.sqrt(np.median(terms(dst, nrm, src, T, idx)[0])))


@pytest.fixture(scope="module")
def small():
    """m = 5 000 on an outline, line normals from 8 neighbours; the targets and normals the handle holds"""
    dst = outline(np.random.default_rng(21), 5000)
    icp = I.Icp2d(dst)
    icp.compute_line_normals(8)
    yield icp, dst, icp.read_line_normals()
    icp.close()


@pytest.fixture(scope="module")
def big():
    """m = 20 000 on the grid engine: source clouds of 16 384 points and more take its sorted snapshot"""
    dst = outline(np.random.default_rng(22), 20_000)
    icp = I.Icp2d(dst, nn_mode=I.NN_GRID)
    icp.compute_line_normals(8)
    yield icp, dst, icp.read_line_normals()
    icp.close()


def both_entries(icp, src, T, r):
    import torch

    yield "host", icp.evaluate_point_to_line(src, T, r, return_indices=True)
    yield "device", icp.evaluate_point_to_line(torch.from_numpy(src).cuda(), T, r, return_indices=True)


# ------------------------------------------------------------------ the definition, bit for bit

@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65_537])
def test_equals_the_restated_definition(small, n):
    icp, dst, nrm = small
    assert np.array_equal(icp.read_targets(), dst)
    rng = np.random.default_rng(100 + n)
    T = I.Transform(POSE)
    src = scan_of(rng, dst, n, T)
    oidx = oracle_idx(dst, src, T)
    for r in (0.0, half_bound(dst, nrm, src, T, oidx), INF):
        for entry, (got, gidx) in both_entries(icp, src, T, r):
            assert_restated(dst, nrm, src, T, r, got, gidx, oidx, (entry, n, r))
        if r == INF:
            assert got.inliers == n
        elif r > 0.0 and n >= 255:
            assert 0.4 * n <= got.inliers <= 0.6 * n, (n, got.inliers)
        # what it shares with the point-to-point evaluation at the same pose and bound: the same bits
        pp = icp.evaluate(src, T, r)
        assert pp.inliers == got.inliers
        assert same_bits([pp.inlier_sum_d2, pp.inlier_rmse], [got.inlier_sum_d2, got.inlier_rmse]), (n, r)
    # without the indices: the same result
    assert same_bits(icp.evaluate_point_to_line(src, T, INF).as_array(), got.as_array())


def test_equals_the_restated_definition_where_the_search_sorts_the_queries(big):
    icp, dst, nrm = big
    rng = np.random.default_rng(300)
    T = I.Transform(POSE)
    src = scan_of(rng, dst, 20_000, T)
    oidx = oracle_idx(dst, src, T)
    r = half_bound(dst, nrm, src, T, oidx)
    for entry, (got, gidx) in both_entries(icp, src, T, r):
        assert_restated(dst, nrm, src, T, r, got, gidx, oidx, (entry, len(src), r))
    pp = icp.evaluate(src, T, r)
    assert pp.inliers == got.inliers
    assert same_bits([pp.inlier_sum_d2, pp.inlier_rmse], [got.inlier_sum_d2, got.inlier_rmse])


@pytest.mark.parametrize("n", [257, 65_537])
def test_information_is_the_unweighted_sum_of_j_jt(small, n):
    """the independent check: with r = +inf every pair counts, and the matrix is sum J J^T for J = (nx, ny, c), summed
    here by a matrix product in float64.  Bound: 1e-12 relative, each entry against the sum of the magnitudes of its own
    terms (the scale a sum's rounding error is relative to).  A tree and a blocked sum of n terms each stay within about
    log2(n) * 2^-53 of that scale: below 1e-14 here."""
    icp, dst, nrm = small
    rng = np.random.default_rng(400 + n)
    T = I.Transform(POSE)
    src = scan_of(rng, dst, n, T)
    got, idx = icp.evaluate_point_to_line(src, T, INF, return_indices=True)
    q = moved2(src, T)
    nj = nrm[idx.astype(np.int64)]
    J = np.stack([nj[:, 0], nj[:, 1], nj[:, 1] * q[:, 0] - nj[:, 0] * q[:, 1]], axis=1)
    want = J.T @ J
    scale = np.abs(J).T @ np.abs(J)
    print("n", n, "relative error of the information matrix", (np.abs(got.information - want) / scale).max())
    assert np.all(np.abs(got.information - want) <= 1e-12 * scale), (got.information, want)
    assert np.array_equal(got.information, got.information.T)
    # ... and the line error is the sum of the squared residuals of the same pairs
    rp = np.einsum("ij,ij->i", nj, q - dst[idx.astype(np.int64)])
    assert abs(got.error - np.sum(rp * rp)) <= 1e-12 * np.sum(rp * rp)
    assert abs(got.line_rmse - np.sqrt(np.mean(rp * rp))) <= 1e-12 * got.line_rmse


# ------------------------------------------------------------------ statuses on a real handle

def raw_call(icp, src, T, r):
    q = _lib.LineQualityStruct()
    C.memset(C.byref(q), 0x5a, C.sizeof(q))
    rc = I.lib().icp_evaluate_point_to_line(icp._h, C.c_void_p(src.ctypes.data if len(src) else None), len(src),
                                            C.byref(T.pose), r, C.byref(q), None)
    return rc, q


def n_and_zeros(q, n):
    raw = bytes(q)
    return q.n == n and raw[8:] == bytes(len(raw) - 8)


def test_statuses_on_a_real_handle():
    import torch

    rng = np.random.default_rng(50)
    dst = outline(rng, 3000)
    T = I.Transform(POSE)
    src = scan_of(rng, dst, 500, T)
    icp = I.Icp2d(dst)
    with pytest.raises(I.IcpError) as e:  # line normals first
        icp.evaluate_point_to_line(src, T, 0.5)
    assert e.value.status == _lib.BAD_ARGUMENT
    rc, q = raw_call(icp, src, T, 0.5)
    assert rc == _lib.BAD_ARGUMENT and n_and_zeros(q, 500)
    icp.compute_line_normals(8)
    assert icp.evaluate_point_to_line(src, T, 0.5).inliers > 0
    icp.append(outline(rng, 400))
    for s in (src, torch.from_numpy(src).cuda()):  # the appended targets have no normal yet
        with pytest.raises(I.IcpError) as e:
            icp.evaluate_point_to_line(s, T, 0.5)
        assert e.value.status == _lib.BAD_ARGUMENT
    icp.update_line_normals(8)
    assert icp.evaluate_point_to_line(src, T, 0.5).n == 500
    # n == 0: ICP_OK and zeros
    for s in (np.zeros((0, 2)), torch.zeros((0, 2), dtype=torch.float64, device="cuda")):
        z, zidx = icp.evaluate_point_to_line(s, T, 0.5, return_indices=True)
        assert z.n == 0 and z.inliers == 0 and not z.as_array().any() and len(zidx) == 0
    # a NaN source coordinate: ICP_NAN_INPUT at any bound (p2 is formed for every point), *out holds n and zeros
    for col in (0, 1):
        bad = src.copy()
        bad[123, col] = np.nan
        for r in (0.5, INF):
            for s in (bad, torch.from_numpy(bad).cuda()):
                with pytest.raises(I.IcpError) as e:
                    icp.evaluate_point_to_line(s, T, r)
                assert e.value.status == _lib.NAN_INPUT
            rc, q = raw_call(icp, bad, T, r)
            assert rc == _lib.NAN_INPUT and n_and_zeros(q, 500)
    assert icp.evaluate_point_to_line(src, T, 0.5).inliers > 0
    icp.close()
    # a 3-D handle: refused by the library too (the Python layer refuses it before)
    d3 = np.ascontiguousarray(rng.random((100, 3)))
    icp3 = I.Icp3d(d3)
    icp3.compute_normals(8)
    q = _lib.LineQualityStruct()
    rc = I.lib().icp_evaluate_point_to_line(icp3._h, C.c_void_p(d3.ctypes.data), 50, C.byref(T.pose), 0.5, C.byref(q), None)
    assert rc == _lib.BAD_ARGUMENT and n_and_zeros(q, 50)
    icp3.close()


# ------------------------------------------------------------------ state and map contract

def bits(T):
    return np.asarray(T.as_array(), dtype=np.float64).view(np.uint64)


def test_an_estimate_after_an_evaluation_returns_the_bits_it_returns_without_one_on_golden_scans():
    import torch

    src, dst = load_golden(1), load_golden(2)
    alone = I.Icp2d(dst)
    alone.compute_line_normals(GOLDEN_K)
    T0, idx0, inner0 = alone.estimate_point_to_line(src, I.Transform(), 20, return_info=True)
    alone.close()
    icp = I.Icp2d(dst)
    icp.compute_line_normals(GOLDEN_K)
    for s in (src, torch.from_numpy(src).cuda()):
        assert icp.evaluate_point_to_line(s, T0, 100.0).inliers > 0  # (the golden scans are in millimetres)
        T, idx, inner = icp.estimate_point_to_line(src, I.Transform(), 20, return_info=True)
        assert np.array_equal(bits(T), bits(T0)), (T.as_array(), T0.as_array())
        assert np.array_equal(idx, idx0) and np.array_equal(inner, inner0)
    assert inner0.sum() > 0
    icp.close()


def test_an_estimate_after_an_evaluation_returns_the_same_bits_at_20k_points(big):
    import torch

    icp, dst, nrm = big
    rng = np.random.default_rng(61)
    Tt = I.Transform([0.05, -0.04, 0.02])
    src = scan_of(rng, dst, 20_000, Tt, sigma=2e-3)
    d_src = torch.from_numpy(src).cuda()
    T0, idx0, inner0 = icp.estimate_point_to_line(d_src, I.Transform(), 3, return_info=True)
    for s in (d_src, src):
        assert icp.evaluate_point_to_line(s, Tt, 0.1).inliers > 0
        T, idx, inner = icp.estimate_point_to_line(d_src, I.Transform(), 3, return_info=True)
        assert np.array_equal(bits(T), bits(T0)), (T.as_array(), T0.as_array())
        assert np.array_equal(idx, idx0) and np.array_equal(inner, inner0)
    # ... and the point-to-point estimate, whose snapshot the evaluation takes and drops
    P0 = icp.estimate(d_src, I.Transform(), 3)
    icp.evaluate_point_to_line(d_src, Tt, 0.1)
    assert np.array_equal(bits(icp.estimate(d_src, I.Transform(), 3)), bits(P0))
    assert inner0.sum() > 0


def test_after_an_append_and_after_a_crop_it_scores_the_cloud_the_handle_holds():
    rng = np.random.default_rng(70)
    dst = outline(rng, 4000)
    T = I.Transform(POSE)
    icp = I.Icp2d(dst)
    icp.compute_line_normals(8)
    icp.append(outline(rng, 1500))
    icp.update_line_normals(8)
    src = scan_of(rng, dst, 3000, T)
    for step in ("append", "crop"):
        if step == "crop":
            removed = icp.crop(T.t, 2.5)
            assert 0 < removed < 5500
        cur, nrm = icp.read_targets(), icp.read_line_normals()
        assert len(cur) == icp.target_count == len(nrm)
        oidx = oracle_idx(cur, src, T)
        for r in (0.05, INF):
            for entry, (got, gidx) in both_entries(icp, src, T, r):
                assert_restated(cur, nrm, src, T, r, got, gidx, oidx, (step, entry, r))
    icp.close()


# ------------------------------------------------------------------ what it is for

def test_a_corridor_is_not_observed_along_its_axis_and_the_point_to_point_matrix_cannot_tell():
    dst = corridor()
    icp = I.Icp2d(dst)
    icp.compute_line_normals(SCENE_K)
    src, T = scene_scan(dst)
    q = icp.evaluate_point_to_line(src, T, 0.5)
    lmin, lmax = q.translation_eig
    w = q.weak_direction()
    print("corridor: inliers", q.inliers, "of", q.n, "lmin", lmin, "lmax", lmax, "ratio", lmin / lmax, "weak", w)
    assert q.inliers == q.n == len(src)
    assert lmax > 0.0 and lmin / lmax <= 1e-6
    assert abs(w[0]) >= 0.999
    pp = icp.evaluate(src, T, 0.5)
    assert pp.information[0][0] == pp.information[1][1] == float(q.inliers)
    icp.close()


def test_a_room_is_observed_in_both_directions():
    dst = closed_room()
    icp = I.Icp2d(dst)
    icp.compute_line_normals(SCENE_K)
    src, T = scene_scan(dst)
    q = icp.evaluate_point_to_line(src, T, 0.5)
    lmin, lmax = q.translation_eig
    print("room: inliers", q.inliers, "of", q.n, "lmin", lmin, "lmax", lmax, "ratio", lmin / lmax)
    assert q.inliers == q.n == len(src)
    assert lmin / lmax >= 1e-2
    icp.close()


# ------------------------------------------------------------------ the batch against the single call

def single(dst, src, T, k, r):
    """(status, inliers, float fields) of the single call on a fresh handle"""
    icp = None
    try:
        icp = I.Icp2d(dst)
        icp.compute_line_normals(k)
        q = icp.evaluate_point_to_line(src, T, r)
        return _lib.OK, q.inliers, q.as_array()
    except I.IcpError as e:
        return e.status, None, None
    finally:
        if icp is not None:
            icp.close()


def assert_items_match(srcs, dsts, Ts, k, r, got):
    qs, status = got
    assert len(qs) == len(srcs)
    for i, (s, d, T) in enumerate(zip(srcs, dsts, Ts)):
        rc, inl, arr = single(d, s, T, k, r)
        assert status[i] == rc, (i, status[i], rc)
        if rc != _lib.OK:
            assert qs[i] is None
            continue
        assert qs[i].n == len(s) and qs[i].inliers == inl, (i, qs[i].inliers, inl)
        assert np.array_equal(qs[i].as_array(), arr), (i, qs[i].as_array(), arr)


def fits(n, m):
    return 1 <= n <= N_LINE and 1 <= m <= M_LINE


def test_edges_of_the_fold_tree_and_of_the_limits():
    ns = [1, 2, 3, 255, 256, 257, 512, 513, 1023, 1024, 1025]
    ms = [1, 2, 3, 5, 63, 64, 65, 668, 2047, 2048, 2049]
    # every n with an m and every m with an n, then more crossings of the edges of both: 40 items
    shapes = [(n, ms[(3 * i + 5) % len(ms)]) for i, n in enumerate(ns)]
    shapes += [(ns[(5 * i + 4) % len(ns)], m) for i, m in enumerate(ms)]
    shapes += [(1024, 2048), (1025, 2049), (1, 1), (512, 2048), (513, 2047), (1023, 65), (256, 64), (257, 5), (2, 3),
               (3, 2), (255, 1), (1024, 668), (513, 668), (1024, 1), (1025, 64), (512, 2049), (257, 2048), (1, 2048)]
    assert len(shapes) == 40
    assert {n for n, _ in shapes} == set(ns) and {m for _, m in shapes} == set(ms)
    rng = np.random.default_rng(2500)
    items = [random_item(rng, 2, n=n, m=m) for n, m in shapes]
    srcs, dsts, Ts = zip(*items)
    B = I.IcpBatch(2)
    got = B.evaluate_point_to_line(srcs, dsts, Ts, k=8, max_correspondence_distance=0.5, allow_failures=True,
                                   return_status=True)
    assert_items_match(srcs, dsts, Ts, 8, 0.5, got)
    assert all(st == _lib.OK for st in got[1])
    served, one_by_one, launches, refused = B.line_quality_counters()
    inside = sum(fits(n, m) for n, m in shapes)
    print(f"inside the limits {inside}, served {served}, one by one {one_by_one}")
    assert refused == 0 and launches == 1
    assert served == inside                     # none of those inside was handed back
    assert one_by_one == len(shapes) - inside   # those outside went one by one
    assert B.evaluate_counters() == (0, 0, 0) and B.line_counters() == (0, 0, 0, 0)  # (the other calls' are their own)
    B.close()


@pytest.mark.parametrize("k", [3, 16])
def test_neighbourhood_size_at_its_ends_and_clamped_and_too_few_targets(k):
    rng = np.random.default_rng(2600 + k)
    items = [random_item(rng, 2, n=200, m=5), random_item(rng, 2, n=700, m=5), random_item(rng, 2, n=200, m=300),
             random_item(rng, 2, n=700, m=300), random_item(rng, 2, n=40, m=2), random_item(rng, 2, n=300, m=1)]
    srcs, dsts, Ts = zip(*items)  # (m = 5 with k = 16: k > m, clamped; m < 3: zero normals, a valid result)
    B = I.IcpBatch(2)
    got = B.evaluate_point_to_line(srcs, dsts, Ts, k=k, allow_failures=True, return_status=True)
    assert_items_match(srcs, dsts, Ts, k, INF, got)
    assert B.line_quality_counters()[:2] == (6, 0)
    for i in (4, 5):
        q = got[0][i]
        assert got[1][i] == _lib.OK and q.inliers == q.n and not q.information.any() and q.error == 0.0
        assert q.inlier_sum_d2 > 0.0
    B.close()


@pytest.mark.parametrize("r", [0.0, 0.3, INF])
def test_bounds(r):
    rng = np.random.default_rng(2700)
    items = [random_item(rng, 2, n=n, m=m) for n, m in ((300, 400), (1000, 1500), (2, 700))]
    srcs, dsts, Ts = zip(*items)
    B = I.IcpBatch(2)
    got = B.evaluate_point_to_line(srcs, dsts, Ts, k=8, max_correspondence_distance=r, return_status=True)
    assert_items_match(srcs, dsts, Ts, 8, r, got)
    if r == 0.0:
        assert all(q.inliers == 0 and q.line_rmse == 0.0 and q.error > 0.0 for q in got[0])
    if r == INF:
        assert all(q.inliers == q.n for q in got[0])
    B.close()


def test_golden_scan_pairs():
    scans = [load_golden(j) for j in range(1, 12)]
    srcs, dsts = scans[:10], scans[1:11]  # 001 -> 002 ... 010 -> 011
    ident = [I.Transform() for _ in srcs]
    B = I.IcpBatch(2)
    Ts = B.estimate_point_to_line(srcs, dsts, ident, 20, k=GOLDEN_K)
    r = 100.0  # (the golden scans are in millimetres)
    got = B.evaluate_point_to_line(srcs, dsts, Ts, k=GOLDEN_K, max_correspondence_distance=r, return_status=True)
    assert_items_match(srcs, dsts, Ts, GOLDEN_K, r, got)
    assert B.line_quality_counters() == (10, 0, 1, 0)  # no hand-back
    assert all(0 < q.inliers <= q.n for q in got[0])
    print("line_rmse:", [round(q.line_rmse, 5) for q in got[0]], "fitness:", [round(q.fitness, 3) for q in got[0]])
    B.close()


def test_hypotheses_share_one_range_and_each_equals_its_single_call():
    src, dst = load_golden(5), load_golden(6)
    rng = np.random.default_rng(7)
    Ts = [I.Transform([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.4, 0.4)]) for _ in range(64)]
    B = I.IcpBatch(2)
    got = B.evaluate_point_to_line_packed(src, dst, [(0, len(src), 0, len(dst), T) for T in Ts], k=GOLDEN_K,
                                          max_correspondence_distance=100.0, return_status=True)
    assert_items_match([src] * 64, [dst] * 64, Ts, GOLDEN_K, 100.0, got)
    assert B.line_quality_counters() == (64, 0, 1, 0)
    B.close()


def mixed_items():
    rng = np.random.default_rng(2800)
    items = [random_item(rng, 2, n=300, m=400)]
    s, d, T = random_item(rng, 2, n=300, m=400)
    s[3, 1] = np.nan
    items.append((s, d, T))  # a NaN source coordinate: ICP_NAN_INPUT, decided by the workgroup
    _, d, T = random_item(rng, 2, n=1, m=30)
    items.append((np.zeros((0, 2)), d, T))  # n = 0: ICP_OK and zeros
    s, _, T = random_item(rng, 2, n=40, m=10)
    items.append((s, np.zeros((0, 2)), T))  # m = 0: ICP_EMPTY_DST
    s, d, T = random_item(rng, 2, n=300, m=400)
    d[17, 0] = np.nan
    items.append((s, d, T))  # a NaN target: handed back, the single call's verdict stands (compared below)
    line = np.ascontiguousarray(np.stack([np.linspace(-3, 3, 500), 0.5 * np.linspace(-3, 3, 500) + 1.0], axis=1))
    s = line[rng.integers(0, 500, 350)] + rng.normal(0.0, 5e-3, size=(350, 2))
    items.append((np.ascontiguousarray(s), line, I.Transform([0.01, -0.01, 0.002])))  # collinear targets
    items.append(random_item(rng, 2, n=900, m=1500))
    return items


def test_statuses_and_bits_in_a_mixed_batch():
    srcs, dsts, Ts = zip(*mixed_items())
    B = I.IcpBatch(2)
    got = B.evaluate_point_to_line(srcs, dsts, Ts, k=8, max_correspondence_distance=0.5, allow_failures=True,
                                   return_status=True)
    assert_items_match(srcs, dsts, Ts, 8, 0.5, got)
    status = got[1].tolist()
    assert status[:4] == [_lib.OK, _lib.NAN_INPUT, _lib.OK, _lib.EMPTY_DST] and status[5:] == [_lib.OK, _lib.OK]
    assert got[0][2].n == 0 and not got[0][2].as_array().any()
    served, one_by_one, launches, refused = B.line_quality_counters()
    assert (served, one_by_one, launches, refused) == (4, 3, 1, 0)  # n = 0, m = 0 and the handed-back item one by one
    q = got[0][5]  # collinear targets: one normal direction, the translation block has rank one
    assert q.translation_eig[0] <= 1e-9 * q.translation_eig[1]
    with pytest.raises(I.IcpError, match="item 1"):
        B.evaluate_point_to_line(srcs, dsts, Ts, k=8, max_correspondence_distance=0.5)
    B.close()


def test_device_entry_equals_host_entry_twice_and_buffers_are_reused():
    import torch

    rng = np.random.default_rng(2900)
    B = I.IcpBatch(2)
    for count in (24, 5, 40):  # grow, shrink, grow: the batch's buffers are reused and resized
        items = [random_item(rng, 2, n=int(rng.integers(1, 1025)), m=int(rng.integers(1, 800))) for _ in range(count)]
        srcs, dsts, Ts = zip(*items)
        src, dst = np.concatenate(srcs), np.concatenate(dsts)
        sf, df = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(d) for d in dsts])
        packed = [(sf[i], len(srcs[i]), df[i], len(dsts[i]), Ts[i]) for i in range(count)]
        host = B.evaluate_point_to_line_packed(src, dst, packed, 8, 0.5, return_status=True)
        again = B.evaluate_point_to_line_packed(src, dst, packed, 8, 0.5, return_status=True)
        dev = B.evaluate_point_to_line_packed(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), packed, 8, 0.5,
                                              return_status=True)
        for other in (again, dev):
            for i in range(count):
                assert host[0][i].inliers == other[0][i].inliers, i
                assert np.array_equal(host[0][i].as_array(), other[0][i].as_array()), i
            assert np.array_equal(host[1], other[1])
        if count == 5:
            assert_items_match(srcs, dsts, Ts, 8, 0.5, host)
    B.close()


def test_batched_items_equal_the_restated_definition_directly():
    """not through the single call: the oracle's indices, the device's normals, the numpy restatement"""
    dst = outline(np.random.default_rng(3000), 1500)
    icp = I.Icp2d(dst)
    icp.compute_line_normals(8)
    nrm = icp.read_line_normals()
    icp.close()
    rng = np.random.default_rng(3001)
    T = I.Transform(POSE)
    srcs = [scan_of(rng, dst, n, T) for n in (2, 257, 1024)]
    B = I.IcpBatch(2)
    qs = B.evaluate_point_to_line(srcs, [dst] * 3, T, k=8, max_correspondence_distance=0.03)
    assert B.line_quality_counters()[:2] == (3, 0)
    B.close()
    for s, q in zip(srcs, qs):
        rc, cnt, want = restate(dst, nrm, s, T, 0.03, oracle_idx(dst, s, T))
        assert rc == _lib.OK and q.n == len(s) and q.inliers == cnt, (len(s), q.inliers, cnt)
        assert len(want) == NFLOATS and same_bits(q.as_array(), want), (len(s), q.as_array(), want)
        if len(s) > 2:
            assert 0 < cnt < len(s)
