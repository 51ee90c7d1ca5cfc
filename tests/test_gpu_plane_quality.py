"""Point-to-plane pose quality (Icp3d.evaluate_point_to_plane: icp_evaluate_point_to_plane[_device] of
include/icp_mi355x.h section 13) against a numpy restatement of its definition, bit for bit: the correspondences are
checked against the CPU oracle's exact search first, the per-point terms and the fold tree are restated here on the
handle's own targets and normals.  Also: the fields it shares with Icp3d.evaluate, the information matrix against an
independent float64 sum of J J^T, statuses, host and device entries, state neutrality, map handles (append, crop), and
what it is for: a corridor whose axis the plane residual cannot see, next to a room it can."""
import ctypes as C

import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from test_p2plane import moved, room

pytestmark = pytest.mark.gpu

INF = float("inf")
K = 1.345  # ICP_HUBER_K
NFLOATS = 18  # PlaneQuality.as_array()


def fold(v):
    """the fold of section 9: n == 1 -> v[0], else groups of 256 padded with +0.0, g[i] += g[i + s], s = 128 .. 1"""
    v = np.asarray(v, dtype=np.float64).ravel()
    if v.size == 0:
        return np.float64(0.0)
    while v.size > 1:
        g = np.concatenate([v, np.zeros((-v.size) % 256)]).reshape(-1, 256)
        s = 128
        while s >= 1:
            g = g[:, :s] + g[:, s:2 * s]
            s //= 2
        v = g[:, 0]
    return v[0]


def terms(dst, nrm, src, T, idx):
    """section 13's per-point values, every operation rounded on its own (numpy forms each product and sum separately)"""
    r00, r10, r01, r11, tx, ty = T.pose.as_tuple()
    px, py, pz = src[:, 0], src[:, 1], src[:, 2]
    qx = (r00 * px + r01 * py) + tx
    qy = (r10 * px + r11 * py) + ty
    j = idx.astype(np.int64)
    b, nj = dst[j], nrm[j]
    nx, ny, nz = nj[:, 0], nj[:, 1], nj[:, 2]
    ex, ey, dz = qx - b[:, 0], qy - b[:, 1], pz - b[:, 2]
    d2 = (ex * ex + ey * ey) + dz * dz
    rp = (nx * ex + ny * ey) + nz * dz
    c = (nx * (-qy)) + (ny * qx)
    return d2, rp * rp, nx, ny, c


def restate(dst, nrm, src, T, r, idx):
    """(status, inliers, the float fields in PlaneQuality.as_array order) by the definition"""
    n = len(src)
    if n == 0:
        return _lib.OK, 0, np.zeros(NFLOATS)
    with np.errstate(invalid="ignore", over="ignore"):
        d2, p2, nx, ny, c = terms(dst, nrm, src, T, idx)
        if np.isnan(p2).any():
            return _lib.NAN_INPUT, 0, np.zeros(NFLOATS)
        inl = d2 <= r * r
        z = np.zeros(n)
        h = np.where(p2 <= K * K, p2, 2.0 * K * np.sqrt(p2) - K * K)
        sd2, sp2 = fold(np.where(inl, d2, z)), fold(np.where(inl, p2, z))
        ixx, ixy, iyy = fold(np.where(inl, nx * nx, z)), fold(np.where(inl, nx * ny, z)), fold(np.where(inl, ny * ny, z))
        ixt, iyt, itt = fold(np.where(inl, nx * c, z)), fold(np.where(inl, ny * c, z)), fold(np.where(inl, c * c, z))
        cnt = int(inl.sum())
        rmse = np.sqrt(sd2 / cnt) if cnt else 0.0
        prmse = np.sqrt(sp2 / cnt) if cnt else 0.0
        hh = (ixx + iyy) * 0.5
        gg = (ixx - iyy) * 0.5
        ss = np.sqrt(gg * gg + ixy * ixy)
    return _lib.OK, cnt, np.array([cnt / n, rmse, sd2, prmse, sp2, fold(p2), fold(h), ixx, ixy, ixt, ixy, iyy, iyt, ixt,
                                   iyt, itt, hh - ss, hh + ss])


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))


def assert_restated(dst, nrm, src, T, r, got, gidx, oidx, where):
    assert np.array_equal(gidx, oidx), (where, np.nonzero(gidx != oidx)[0][:10])
    rc, cnt, want = restate(dst, nrm, src, T, r, oidx)
    assert rc == _lib.OK, where
    print(where, "inliers", got.inliers, "of", got.n, "plane_rmse", got.plane_rmse, "eig", got.translation_eig)
    assert got.n == len(src) and got.inliers == cnt, (where, got.n, got.inliers, cnt)
    assert same_bits(got.as_array(), want), (where, got.as_array(), want)


def oracle_idx(dst, src, T):
    rc, idx = O.KdTree(dst).search(moved(src, T))
    assert rc == O.OK
    return idx


def scan_of(rng, dst, n, T, sigma=0.02):
    """n samples of the targets with noise, in the frame the pose T maps into the targets' frame"""
    world = dst[rng.integers(0, len(dst), n)] + rng.normal(size=(n, 3)) * sigma
    return np.ascontiguousarray(moved(world, T.inverse()))


def half_bound(dst, nrm, src, T, idx):
    """a finite bound that keeps about half the points"""
    return float(np.sqrt(np.median(terms(dst, nrm, src, T, idx)[0])))


POSE = [0.12, -0.07, 0.04]


@pytest.fixture(scope="module")
def small():
    """m = 5 000 on a room-like cloud, normals from 8 neighbours; the targets and normals the handle holds"""
    rng = np.random.default_rng(21)
    dst = room(rng, 5000)
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    yield icp, dst, icp.read_normals()
    icp.close()


@pytest.fixture(scope="module")
def big():
    """m = 80 000: source clouds of 16 384 points and more take the grid engine's sorted snapshot"""
    rng = np.random.default_rng(22)
    dst = room(rng, 80_000)
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    yield icp, dst, icp.read_normals()
    icp.close()


def both_entries(icp, src, T, r):
    import torch

    yield "host", icp.evaluate_point_to_plane(src, T, r, return_indices=True)
    yield "device", icp.evaluate_point_to_plane(torch.from_numpy(src).cuda(), T, r, return_indices=True)


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
    assert same_bits(icp.evaluate_point_to_plane(src, T, INF).as_array(), got.as_array())


def test_equals_the_restated_definition_where_the_search_takes_a_snapshot(big):
    icp, dst, nrm = big
    rng = np.random.default_rng(300)
    T = I.Transform(POSE)
    src = scan_of(rng, dst, 300_000, T)
    oidx = oracle_idx(dst, src, T)
    r = half_bound(dst, nrm, src, T, oidx)
    for entry, (got, gidx) in both_entries(icp, src, T, r):
        assert_restated(dst, nrm, src, T, r, got, gidx, oidx, (entry, len(src), r))
    pp = icp.evaluate(src, T, r)
    assert pp.inliers == got.inliers
    assert same_bits([pp.inlier_sum_d2, pp.inlier_rmse], [got.inlier_sum_d2, got.inlier_rmse])


@pytest.mark.parametrize("n", [257, 65_537])
def test_information_is_the_unweighted_sum_of_j_jt(small, n):
    """the independent check: with r = +inf every pair counts, and the matrix is sum J J^T for J = (nx, ny, c) of
    k_p2pl_accumulate at the identity inner pose, summed here by a matrix product in float64.  Bound: 1e-12 relative,
    each entry against the sum of the magnitudes of its own terms (the scale a sum's rounding error is relative to:
    an entry whose terms cancel has no smaller error than one whose terms do not).  A tree and a blocked sum of n
    terms each stay within about log2(n) * 2^-53 of that scale: below 1e-14 here."""
    icp, dst, nrm = small
    rng = np.random.default_rng(400 + n)
    T = I.Transform(POSE)
    src = scan_of(rng, dst, n, T)
    got, idx = icp.evaluate_point_to_plane(src, T, INF, return_indices=True)
    q = moved(src, T)
    nj = nrm[idx.astype(np.int64)]
    J = np.stack([nj[:, 0], nj[:, 1], nj[:, 1] * q[:, 0] - nj[:, 0] * q[:, 1]], axis=1)
    want = J.T @ J
    scale = np.abs(J).T @ np.abs(J)
    err = np.abs(got.information - want) / scale
    print("n", n, "relative error of the information matrix", err.max())
    assert np.all(np.abs(got.information - want) <= 1e-12 * scale), (got.information, want)
    assert np.array_equal(got.information, got.information.T)
    # ... and the plane error is the sum of the squared residuals of the same pairs
    b = dst[idx.astype(np.int64)]
    rp = np.einsum("ij,ij->i", nj, np.stack([q[:, 0] - b[:, 0], q[:, 1] - b[:, 1], src[:, 2] - b[:, 2]], axis=1))
    assert abs(got.error - np.sum(rp * rp)) <= 1e-12 * np.sum(rp * rp)
    assert abs(got.plane_rmse - np.sqrt(np.mean(rp * rp))) <= 1e-12 * got.plane_rmse


# ------------------------------------------------------------------ statuses on a real handle

def raw_call(icp, src, T, r):
    q = _lib.PlaneQualityStruct()
    C.memset(C.byref(q), 0x5a, C.sizeof(q))
    rc = I.lib().icp_evaluate_point_to_plane(icp._h, C.c_void_p(src.ctypes.data if len(src) else None), len(src),
                                             C.byref(T.pose), r, C.byref(q), None)
    return rc, q


def n_and_zeros(q, n):
    raw = bytes(q)
    return q.n == n and raw[8:] == bytes(len(raw) - 8)


def test_statuses_on_a_real_handle():
    import torch

    rng = np.random.default_rng(50)
    dst = room(rng, 3000)
    T = I.Transform(POSE)
    src = scan_of(rng, dst, 500, T)
    icp = I.Icp3d(dst)
    with pytest.raises(I.IcpError) as e:  # normals first
        icp.evaluate_point_to_plane(src, T, 0.5)
    assert e.value.status == _lib.BAD_ARGUMENT
    rc, q = raw_call(icp, src, T, 0.5)
    assert rc == _lib.BAD_ARGUMENT and n_and_zeros(q, 500)
    icp.compute_normals(8)
    ok = icp.evaluate_point_to_plane(src, T, 0.5)
    assert ok.inliers > 0
    icp.append(room(rng, 400) + np.array([0.0, 0.0, 0.001]))
    for s in (src, torch.from_numpy(src).cuda()):  # the appended targets have no normal yet
        with pytest.raises(I.IcpError) as e:
            icp.evaluate_point_to_plane(s, T, 0.5)
        assert e.value.status == _lib.BAD_ARGUMENT
    icp.update_normals(8)
    assert icp.evaluate_point_to_plane(src, T, 0.5).n == 500
    # n == 0: ICP_OK and zeros
    for s in (np.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.float64, device="cuda")):
        z, zidx = icp.evaluate_point_to_plane(s, T, 0.5, return_indices=True)
        assert z.n == 0 and z.inliers == 0 and not z.as_array().any() and len(zidx) == 0
    # a NaN source point: ICP_NAN_INPUT at any bound (p2 is formed for every point), *out holds n and zeros
    for col in (0, 2):
        bad = src.copy()
        bad[123, col] = np.nan
        for r in (0.5, INF):
            for s in (bad, torch.from_numpy(bad).cuda()):
                with pytest.raises(I.IcpError) as e:
                    icp.evaluate_point_to_plane(s, T, r)
                assert e.value.status == _lib.NAN_INPUT
            rc, q = raw_call(icp, bad, T, r)
            assert rc == _lib.NAN_INPUT and n_and_zeros(q, 500)
    after = icp.evaluate_point_to_plane(src, T, 0.5)
    assert after.inliers > 0
    icp.close()


# ------------------------------------------------------------------ state and map contract

def bits(T):
    return np.asarray(T.as_array(), dtype=np.float64).view(np.uint64)


def test_an_estimate_after_an_evaluation_returns_the_bits_it_returns_without_one():
    import torch

    rng = np.random.default_rng(60)
    dst = room(rng, 650)
    Tt = I.Transform([0.05, -0.04, 0.02])
    src = scan_of(rng, dst, 600, Tt, sigma=2e-3)
    alone = I.Icp3d(dst)
    alone.compute_normals(8)
    T0, idx0, inner0 = alone.estimate_point_to_plane(src, I.Transform(), 5, return_info=True)
    alone.close()
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    for s in (src, torch.from_numpy(src).cuda()):
        q = icp.evaluate_point_to_plane(s, Tt, 0.1)
        assert q.inliers > 0
        T, idx, inner = icp.estimate_point_to_plane(src, I.Transform(), 5, return_info=True)
        assert np.array_equal(bits(T), bits(T0)), (T.as_array(), T0.as_array())
        assert np.array_equal(idx, idx0) and np.array_equal(inner, inner0)
    assert inner0.sum() > 0
    icp.close()


def test_an_estimate_after_an_evaluation_returns_the_same_bits_at_100k_points(big):
    import torch

    icp, dst, nrm = big
    rng = np.random.default_rng(61)
    Tt = I.Transform([0.05, -0.04, 0.02])
    src = scan_of(rng, dst, 100_000, Tt, sigma=2e-3)
    d_src = torch.from_numpy(src).cuda()
    T0, idx0, inner0 = icp.estimate_point_to_plane(d_src, I.Transform(), 3, return_info=True)
    for s in (d_src, src):
        q = icp.evaluate_point_to_plane(s, Tt, 0.1)
        assert q.inliers > 0
        T, idx, inner = icp.estimate_point_to_plane(d_src, I.Transform(), 3, return_info=True)
        assert np.array_equal(bits(T), bits(T0)), (T.as_array(), T0.as_array())
        assert np.array_equal(idx, idx0) and np.array_equal(inner, inner0)
    # ... and the point-to-point estimate, whose snapshot the evaluation takes and drops
    P0 = icp.estimate(d_src, I.Transform(), 3)
    icp.evaluate_point_to_plane(d_src, Tt, 0.1)
    assert np.array_equal(bits(icp.estimate(d_src, I.Transform(), 3)), bits(P0))
    assert inner0.sum() > 0


def test_after_an_append_and_after_a_crop_it_scores_the_cloud_the_handle_holds():
    rng = np.random.default_rng(70)
    dst = room(rng, 4000)
    T = I.Transform(POSE)
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    icp.append(room(rng, 1500) + np.array([0.0, 0.0, 0.003]))
    icp.update_normals(8)
    src = scan_of(rng, dst, 3000, T)
    for step in ("append", "crop"):
        if step == "crop":
            removed = icp.crop(T.t, 2.5)
            assert 0 < removed < 5500
        cur, nrm = icp.read_targets(), icp.read_normals()
        assert len(cur) == icp.target_count == len(nrm)
        oidx = oracle_idx(cur, src, T)
        for r in (0.05, INF):
            for entry, (got, gidx) in both_entries(icp, src, T, r):
                assert_restated(cur, nrm, src, T, r, got, gidx, oidx, (step, entry, r))
    icp.close()


# ------------------------------------------------------------------ what it is for

def wall_y(y):
    x, z = np.meshgrid(np.linspace(-10.0, 10.0, 201), np.linspace(0.0, 2.0, 21), indexing="ij")
    return np.stack([x.ravel(), np.full(x.size, y), z.ravel()], axis=1)


def wall_x(x):
    y, z = np.meshgrid(np.linspace(-2.0, 2.0, 41), np.linspace(0.0, 2.0, 21), indexing="ij")
    return np.stack([np.full(y.size, x), y.ravel(), z.ravel()], axis=1)


def corridor():
    """two walls y = +-2, x in [-10, 10], z in [0, 2], on a 0.1 grid"""
    return np.ascontiguousarray(np.concatenate([wall_y(-2.0), wall_y(2.0)]))


def closed_room():
    """the corridor plus the end walls x = +-10, y in [-2, 2]"""
    return np.ascontiguousarray(np.concatenate([corridor(), wall_x(-10.0), wall_x(10.0)]))


SCENE_POSE = [0.03, -0.02, 0.01]


def scene_scan(dst):
    """every third target moved by the inverse of a small pose: evaluated at that pose it lies on the map"""
    T = I.Transform(SCENE_POSE)
    return np.ascontiguousarray(moved(dst[::3], T.inverse())), T


def test_a_corridor_is_not_observed_along_its_axis_and_the_point_to_point_matrix_cannot_tell():
    """Exact planar walls y = const give normals (0, +-1, 0) with an in-plane component at rounding level, so the
    translation block is diag(~0, inliers): lmin / lmax <= 1e-6 and the weak direction is the x axis.  On the CPU (the
    oracle's normals, the restatement above) the ratio is 0.0 exactly."""
    dst = corridor()
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    src, T = scene_scan(dst)
    q = icp.evaluate_point_to_plane(src, T, 0.5)
    lmin, lmax = q.translation_eig
    w = q.weak_direction()
    print("corridor: inliers", q.inliers, "of", q.n, "lmin", lmin, "lmax", lmax, "ratio", lmin / lmax, "weak", w)
    assert q.inliers == q.n == len(src)
    assert lmax > 0.0 and lmin / lmax <= 1e-6
    assert abs(w[0]) >= 0.999
    assert q.plane_rmse <= 1e-9  # the scan lies on the map at that pose
    pp = icp.evaluate(src, T, 0.5)
    assert pp.information[0][0] == pp.information[1][1] == float(q.inliers)
    icp.close()


def test_a_room_is_observed_in_both_directions():
    """The end walls x = +-10 carry normals (+-1, 0, 0): lmin / lmax is about their share of the points (0.17 of the
    targets; 0.2036 on the CPU with the oracle's normals and the restatement above, the normals of the corner columns
    lean towards the diagonal), far above 1e-2."""
    dst = closed_room()
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    src, T = scene_scan(dst)
    q = icp.evaluate_point_to_plane(src, T, 0.5)
    lmin, lmax = q.translation_eig
    print("room: inliers", q.inliers, "of", q.n, "lmin", lmin, "lmax", lmax, "ratio", lmin / lmax)
    assert q.inliers == q.n == len(src)
    assert lmin / lmax >= 1e-2
    icp.close()
