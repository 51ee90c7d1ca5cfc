"""The owner phase of the shared warm walk (nn_grid.hip: warm_wave): every lane's tile of rows is evaluated only as
far as its WAVE needs it (1, 2 or 4 entries along y and along z), and a round's rows are picked in straight-line
code, the next tile of a box behind a wave-uniform branch.  Every mask shape and that branch, against the
brute-force engine on the same clouds: the index array, the pose bytes and the inner counts of estimate() for
k = 1 (the seeded search), 2 (the warm search) and 3 (the run-ahead warm search).

warm_wave serves source clouds beyond 65 536 points only, and there the grid engine folds its sums in the order of
its cell-sorted snapshot while the sweep keeps the caller's order.  The sweep is therefore handed the cloud in the
fold order of the grid call (icp_last_fold_order, as parity_util.oracle_in_device_order hands it to the oracle) and
its indices go back through the permutation: same points, same poses, same fold -- same bits.

A NaN coordinate in the source makes estimate() report ICP_NAN_INPUT whatever the engine, so the NaN query is checked
through the search itself (prepare_source_device + correspond_device: seeded, then warm from the previous matches).

What a cloud is meant to provoke is asserted on the host first, from the grid's documented geometry (cell size: two
targets per cell, four times finer along x) and the waves of the fold order: 64 consecutive points of it.
"""
import functools

import numpy as np
import pytest

import icp_rust_amd as I
from blind_clouds import _geometry
from parity_util import apply_pose

pytestmark = pytest.mark.gpu

N_SRC = 66_003  # > 65 536 (the shared walk), and not a multiple of 64: the last wave has 45 lanes past the end
T0 = (0.02, -0.015, 0.004)
HUGE = 1e20     # a finite query beyond the f32 geometry: its box is the whole grid (`wide`)


def _rows(q, r, geo, d):
    """cells along axis d that the box of radius r around q spans (1 for an axis the cloud does not have)"""
    lo, h, n = geo
    if d >= q.shape[1]:
        return np.ones(len(q), dtype=np.int64)
    c0 = np.clip(np.floor((q[:, d] - r - lo[d]) / h[d]), 0, n[d] - 1)
    c1 = np.clip(np.floor((q[:, d] + r - lo[d]) / h[d]), 0, n[d] - 1)
    return (c1 - c0 + 1).astype(np.int64)


def _near(rng, dst, count, noise):
    return dst[rng.integers(0, len(dst), size=count)] + rng.normal(size=(count, dst.shape[1])) * noise


def _sheet(dim):
    """a dense planar sheet, queries a fraction of a cell from their targets: boxes of 1 x 1 and 2 x 1 rows"""
    rng = np.random.default_rng(800 + dim)
    dst = np.zeros((4000, dim))
    dst[:, :2] = rng.uniform(0, 20, size=(4000, 2))
    src = _near(rng, dst, N_SRC, 0.02)
    src[12345, 0] = HUGE
    return dst, src


def _uniform():
    """two densities in one box and queries drawn independently of the targets: the previous match is about a cell
    away (3 x 3, 4 x 4 rows; more in the sparse half), queries in the first and the last cell of y and z, and a few
    hundred outside the box on every side"""
    rng = np.random.default_rng(811)
    dst = np.concatenate([rng.uniform(0, 1, size=(3600, 3)) * [8, 8, 4], rng.uniform(0, 1, size=(400, 3)) * [8, 8, 4] + [0, 0, 4]])
    src = rng.uniform(0, 8, size=(N_SRC, 3))
    out = rng.choice(N_SRC, size=600, replace=False)
    src[out] = (src[out] - 4.0) * 1.15 + 4.0
    src[out[:300], 1:] = np.where(src[out[:300], 1:] < 4.0, -0.3, 8.3)
    src[777, 1] = -HUGE
    return dst, src


def _far(dim, thin):
    """three tight clusters in an otherwise empty box (its corners are targets); most queries sit on a target, three
    hundred lie 3 - 5.5 cells from their cluster along x -- in the cluster's own rows, so the fold order puts them next
    to the cluster's queries -- with boxes beyond one tile of 4 x 4 rows in y, in z or in both (`thin`: the axis that
    has too few cells for that)"""
    rng = np.random.default_rng(820 + 10 * dim + (thin or 0))
    size = np.full(dim, 16.0)
    if thin is not None:
        size[thin] = 1.2
    corners = np.stack(np.meshgrid(*[[0.0, 1.0]] * dim, indexing="ij"), axis=-1).reshape(-1, dim) * size
    centres = np.array([[7.6, 0.35, 0.55], [8.0, 0.5, 0.4], [8.4, 0.62, 0.6]])[:, :dim] * np.where(np.arange(dim) == 0, 1.0, size)
    hh = _geometry(np.concatenate([corners, np.repeat(centres, 1300, axis=0)]))[1][1]  # (to the percent: the clusters are small)
    dst = np.concatenate([corners] + [c + rng.normal(size=(1300, dim)) * 0.3 * hh for c in centres])
    hh = _geometry(dst)[1][1]
    src = _near(rng, dst[len(corners):], N_SRC, 0.01 * hh)
    far = rng.choice(N_SRC, size=300, replace=False)
    off = rng.normal(size=(300, dim)) * 0.1 * hh
    off[:, 0] = rng.uniform(3.0, 5.5, size=300) * hh * rng.choice([-1.0, 1.0], size=300)
    src[far] = centres[rng.integers(0, 3, size=300)] + off
    if dim == 3 and thin is None:
        src[4242, 2] = HUGE
    return dst, src


CLOUDS = {
    "sheet3": lambda: _sheet(3),
    "sheet2": lambda: _sheet(2),
    "uniform3": _uniform,
    "far3_y": lambda: _far(3, 2),
    "far3_z": lambda: _far(3, 1),
    "far3_yz": lambda: _far(3, None),
    "far2": lambda: _far(2, None),
}


@functools.lru_cache(maxsize=None)
def _cloud(name):
    dst, src = CLOUDS[name]()
    dst, src = np.ascontiguousarray(dst), np.ascontiguousarray(src)
    dst.setflags(write=False)
    src.setflags(write=False)
    return dst, src


def _handle(dst, mode):
    icp = (I.Icp3d if dst.shape[1] == 3 else I.Icp2d)(dst, nn_mode=mode)
    assert I.lib().icp_get_nn_mode(icp._h) == mode
    return icp


def _exact_nn(dst, q):
    """argmin of the contract's f64 distance (dx^2 + dy^2) + dz^2, lowest index on ties (np.argmin: the first minimum;
    a NaN query has only NaN distances and gets index 0)"""
    out = np.empty(len(q), dtype=np.uint32)
    for i in range(0, len(q), 500):
        d = q[i:i + 500, None, :] - dst[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        if dst.shape[1] == 3:
            d2 = d2 + d[..., 2] * d[..., 2]
        out[i:i + 500] = np.argmin(d2, axis=1)
    return out


def _moved(T, src):
    q = src.copy()
    q[:, :2] = apply_pose(T, src)
    return q


def _waves(perm, *cols):
    """per-lane values in fold order, one row per full wave"""
    w = len(perm) // 64
    return [c[perm[:64 * w]].reshape(w, 64) for c in cols]


def _check_shapes(name, dst, src, perm, idx1):
    """the boxes the warm search of k = 2 starts from (the match of k = 1, the query a pose step further), by wave"""
    geo = _geometry(dst)
    q = _moved(I.Transform(np.array(T0)), src)
    ok = np.all(np.abs(q) < 1e18, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(((q - dst[idx1]) ** 2).sum(1))
        ry, rz = _rows(q, r, geo, 1), _rows(q, r, geo, 2)
    ry[~ok], rz[~ok] = 1, 1
    wy, wz = _waves(perm, ry, rz)
    my, mz = wy.max(1), wz.max(1)
    small = ((wy == 1) & (wz == 1)).sum(1)
    if name.startswith("sheet"):
        assert ry.max() == 2 and rz.max() == 1 and (my == 1).any() and (my == 2).any()
    elif name == "uniform3":
        assert ((my == 3) & (mz <= 4)).any() and ((my == 4) & (mz == 4)).any() and ((my <= 2) & (mz <= 2)).any()
        assert (my > 4).any() and (mz > 4).any()
        lo, h, n = geo
        for d in (1, 2):  # queries in the first and the last cell, and beyond them
            c = np.floor((q[ok, d] - lo[d]) / h[d])
            assert (c == 0).any() and (c == n[d] - 1).any() and (c < 0).any() and (c > n[d] - 1).any()
    else:
        assert geo[2][1] > 8 or name == "far3_z"
        want_y, want_z = name != "far3_z", name in ("far3_z", "far3_yz")
        assert (geo[2][1] <= 4) == (not want_y) and (dst.shape[1] == 2 or (geo[2][2] <= 4) == (not want_z))
        beyond = ((my > 4) == want_y) & ((mz > 4) == want_z)
        assert (beyond & (small >= 8)).any(), (my.max(), mz.max())  # ... beside lanes whose box is one row
    assert len(src) % 64 != 0


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_estimate_on_the_shared_walk_equals_the_brute_force_engine(name):
    dst, src = _cloud(name)
    grid, brute = _handle(dst, I.NN_GRID), _handle(dst, I.NN_BRUTE)
    start = I.Transform(np.array(T0))
    for k in (1, 2, 3):
        T, idx, inner = grid.estimate(src, start, k, return_info=True)
        perm = grid.last_fold_order(len(src))
        assert np.array_equal(np.sort(perm), np.arange(len(src)))
        bT, bidx_s, binner = brute.estimate(np.ascontiguousarray(src[perm]), start, k, return_info=True)
        bidx = np.empty_like(bidx_s)
        bidx[perm] = bidx_s
        if k == 1:  # the reference itself, on a sample: the search of k = 1 runs at the initial pose
            some = np.random.default_rng(5).choice(len(src), size=2000, replace=False)
            assert np.array_equal(bidx[some], _exact_nn(dst, _moved(start, src)[some]))
            _check_shapes(name, dst, src, perm, bidx)
        assert np.array_equal(idx, bidx), (k, np.nonzero(idx != bidx)[0][:10])
        assert np.array_equal(inner, binner), (k, inner, binner)
        assert T.as_array().tobytes() == bT.as_array().tobytes(), (k, T.as_array(), bT.as_array())


@pytest.mark.parametrize("name", ["uniform3", "sheet2", "far3_yz"])
def test_a_nan_query_beside_a_huge_one_through_the_seeded_and_the_warm_search(name):
    import torch

    dst, src = _cloud(name)
    src = src.copy()
    src[31_000, 1] = np.nan
    assert (np.abs(src) == HUGE).any()
    grid, brute = _handle(dst, I.NN_GRID), _handle(dst, I.NN_BRUTE)
    d_q = torch.from_numpy(src).cuda()
    idx = torch.empty(len(src), dtype=torch.int32, device="cuda")
    a = torch.empty((len(src), 2), dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    some = np.random.default_rng(6).choice(len(src), size=2000, replace=False)
    some[:2] = 31_000, int(np.nonzero((np.abs(src) == HUGE).any(1))[0][0])
    poses = [I.Transform(np.array(T0)), I.Transform(np.array([0.05, -0.03, 0.006])), I.Transform(np.array([0.06, -0.02, 0.005]))]
    grid.prepare_source_device(d_q, poses[0])
    for T in poses:  # the first: seeds + the walk; the others: the walk from the previous matches
        got = []
        for icp in (grid, brute):
            icp.correspond_device(d_q, T, a, b, idx)
            icp.synchronize()
            got.append(idx.cpu().numpy().view(np.uint32).copy())
        with np.errstate(invalid="ignore", over="ignore"):
            assert np.array_equal(got[1][some], _exact_nn(dst, _moved(T, src)[some]))
        assert got[1][31_000] == 0
        assert np.array_equal(got[0], got[1]), np.nonzero(got[0] != got[1])[0][:10]
