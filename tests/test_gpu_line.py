"""Point-to-line registration for 2-D handles on the GPU (Icp2d.compute_line_normals / update_line_normals /
read_line_normals / estimate_point_to_line: include/icp_mi355x.h section 14).  An extension without a reference
counterpart: the checkers are the numpy restatement of the normal definition (tests/test_line_abi.py) and the CPU
statement of the estimator, the oracle's point-to-plane estimate fed lifted clouds [x, y, 0] and normals [nx, ny, 0].
  * the normals against the restatement, at the sizes where the kernel takes another path;
  * the estimate against the CPU statement fed the device's normals: indices and inner counts equal, pose within 1e-9;
  * properties: closer than point-to-point on independent samples, no update on a single wall;
  * the gate: +inf equals the ungated call bit for bit, nothing within 0, a finite bound against the chained restatement
    of tests/test_gpu_gated_plane.py, at the compaction's tile edges;
  * append and crop: normals go stale / are carried along as section 7's are."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from parity_util import oracle_plane_in_device_order
from test_gpu_gated_plane import chain
from test_line_abi import (GOLDEN_K, SEEDS, lift, line_normals_numpy, load_golden, moved2, oracle_point_to_line, outline,
                           outline_pair, pose_error)

pytestmark = pytest.mark.gpu

INF = float("inf")
TILE_EDGES = [1023, 1024, 1025, 2500]  # the compaction's tile is 1 024 points


def bits(T):
    return np.asarray(T.as_array(), dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.set_threads(16)
    yield
    O.set_threads(1)


# ------------------------------------------------------------------ normals

def cluttered(seed, m):
    """three quarters outline, one quarter scattered over the room: the scattered targets are sparse against the grid's
    cells (sized for the whole cloud), so their neighbourhoods need several rings"""
    rng = np.random.default_rng(seed)
    k = m // 4
    scatter = np.stack([rng.uniform(-3, 3, k), rng.uniform(-2, 2, k)], axis=1)
    return np.ascontiguousarray(rng.permutation(np.concatenate([outline(rng, m - k), scatter])))


def collinear(m):
    """m points with exactly the same x: e_x == 0 for every neighbour, a[0][1] == 0, no rotation"""
    rng = np.random.default_rng(4)
    return np.ascontiguousarray(np.stack([np.full(m, 3.0), rng.uniform(-3, 3, m)], axis=1))


NORMAL_CASES = {
    "2-k3": (lambda: outline(np.random.default_rng(2), 2), 3, None),
    "3-k3": (lambda: outline(np.random.default_rng(3), 3), 3, None),
    "300-k3": (lambda: outline(np.random.default_rng(300), 300), 3, None),
    "5000-k10": (lambda: outline(np.random.default_rng(5000), 5000), 10, None),
    "20000-k16-grid": (lambda: cluttered(20000, 20000), 16, I.NN_GRID),
    "golden-k8": (lambda: load_golden(2), 8, None),
    "collinear-1000": (lambda: collinear(1000), 8, None),
}


@pytest.mark.parametrize("case", list(NORMAL_CASES))
def test_device_line_normals_equal_the_restatement(case):
    make, k, mode = NORMAL_CASES[case]
    dst = make()
    m = len(dst)
    icp = I.Icp2d(dst, nn_mode=mode) if mode is not None else I.Icp2d(dst)
    icp.compute_line_normals(k)
    got = icp.read_line_normals()
    icp.close()
    assert got.shape == (m, 2)
    rows = np.arange(m) if m <= 6000 else np.sort(np.random.default_rng(1).choice(m, 500, replace=False))
    want = line_normals_numpy(dst, k, rows)
    err = float(np.max(np.abs(got[rows] - want)))
    length = np.hypot(got[:, 0], got[:, 1])
    zero = (got[:, 0] == 0.0) & (got[:, 1] == 0.0)
    print(f"{case}: m={m} k={k} max |diff| {err:.3g}, zero rows {int(zero.sum())}")
    assert np.all(zero | (np.abs(length - 1.0) < 1e-12))
    # same neighbours (exact k-NN by (d^2, index)), same operation sequence: equal to rounding
    assert err < 1e-9
    if case == "2-k3":
        assert np.all(zero)  # fewer than 3 neighbours
    else:
        assert not zero.any()
    if case == "collinear-1000":
        assert np.array_equal(got, np.tile([1.0, 0.0], (m, 1)))
    if case == "golden-k8":
        assert m == 668


def test_reading_a_range_of_normals_and_what_a_handle_refuses():
    dst = outline(np.random.default_rng(12), 700)
    icp = I.Icp2d(dst)
    for call in (lambda: icp.read_line_normals(), lambda: icp.estimate_point_to_line(dst[:50], I.Transform(), 1),
                 lambda: icp.estimate_point_to_line(dst[:50], I.Transform(), 1, max_correspondence_distance=1.0)):
        with pytest.raises(I.IcpError) as e:  # normals first
            call()
        assert e.value.status == _lib.BAD_ARGUMENT
    with pytest.raises(I.IcpError):  # the plane entries keep refusing a 2-D handle
        icp.compute_normals(8)
    icp.compute_line_normals(6)
    whole = icp.read_line_normals()
    assert np.array_equal(icp.read_line_normals(123, 77), whole[123:200])
    assert icp.read_line_normals(700, 0).shape == (0, 2)
    with pytest.raises(I.IcpError):
        icp.read_line_normals(650, 51)
    # a 3-D handle is refused by the library as well as by the Python layer
    cube = I.Icp3d(np.random.default_rng(0).random((64, 3)))
    assert I.lib().icp_compute_target_line_normals(cube._h, 8) == _lib.BAD_ARGUMENT
    assert I.lib().icp_update_target_line_normals(cube._h, 8) == _lib.BAD_ARGUMENT
    # too few source points: no update; an empty target cloud: only when a search would run
    T0 = I.Transform([0.1, 0.2, 0.05])
    T, idx, inner = icp.estimate_point_to_line(dst[:1], T0, 3, return_info=True)
    assert np.array_equal(bits(T), bits(T0)) and inner.tolist() == [0, 0, 0]
    assert np.array_equal(bits(icp.estimate_point_to_line(np.zeros((0, 2)), T0, 3)), bits(T0))
    bad = dst[:40].copy()
    bad[7, 0] = np.nan
    with pytest.raises(I.IcpError) as e:
        icp.estimate_point_to_line(bad, I.Transform(), 2)
    assert e.value.status == _lib.NAN_INPUT
    icp.close()
    cube.close()
    empty = I.Icp2d(np.zeros((0, 2)))
    with pytest.raises(I.IcpError) as e:
        empty.estimate_point_to_line(dst[:5], T0, 1)
    assert e.value.status == _lib.EMPTY_DST
    assert np.array_equal(bits(empty.estimate_point_to_line(dst[:5], T0, 0)), bits(T0))
    empty.close()


# ------------------------------------------------------------------ the estimate against the CPU statement

def golden_pair(k):
    return load_golden(k), load_golden(1), GOLDEN_K, 20


def outline_case():
    dst, src, _ = outline_pair(*SEEDS[0])
    return dst, src, 10, 6


@pytest.mark.parametrize("case", ["golden-001-002", "golden-001-010", "outline-3000x1500"])
def test_device_point_to_line_equals_the_cpu_statement(case):
    import torch

    dst, src, k, iters = {"golden-001-002": lambda: golden_pair(2), "golden-001-010": lambda: golden_pair(10),
                          "outline-3000x1500": outline_case}[case]()
    icp = I.Icp2d(dst)
    icp.compute_line_normals(k)
    T, idx, inner = icp.estimate_point_to_line(src, I.Transform(), iters, return_info=True)
    normals = icp.read_line_normals()
    rc, oT, oidx, oinner = oracle_point_to_line(dst, normals, src, I.Transform(), iters)
    assert rc == O.OK
    err = float(np.max(np.abs(T.as_array() - oT.as_array())))
    print(f"{case}: inner {inner.tolist()}, CPU statement {oinner.tolist()}, pose difference {err:.3g}")
    assert np.array_equal(idx, oidx)      # the handle's exact 2-D nearest neighbour either way
    assert np.array_equal(inner, oinner)  # (the CPU statement: [8, 5, 3, 0, ...] and [8, 5, 4, 1, 0, ...] on the golden pairs)
    assert inner.sum() > 0
    assert err < 1e-9                     # tree sums vs left folds
    # ... and the same statement with its sums folded in the device's tree: equal to the bit
    trc, tT, tidx, tinner = oracle_plane_in_device_order(icp, lift(dst), lift(normals), lift(src), I.Transform(), iters)
    assert trc == O.OK and np.array_equal(idx, tidx) and np.array_equal(inner, tinner)
    assert np.array_equal(bits(T), bits(tT)), (T.as_array(), tT.as_array())
    # device-resident source: same bits as the host-buffer call
    T2, idx2, inner2 = icp.estimate_point_to_line(torch.from_numpy(src).cuda(), I.Transform(), iters, return_info=True)
    assert np.array_equal(bits(T), bits(T2)) and np.array_equal(idx, idx2) and np.array_equal(inner, inner2)
    assert np.array_equal(bits(icp.estimate_point_to_line(src, I.Transform(), iters)), bits(T))  # (without the info)
    icp.close()


# ------------------------------------------------------------------ properties

@pytest.mark.parametrize("seed,m,n", SEEDS)
def test_point_to_line_on_independent_samples_is_closer_than_point_to_point(seed, m, n):
    """scan and target are INDEPENDENT samples of the same walls: nearest-neighbour pairs differ by up to the sample
    spacing ALONG the walls; the line residual does not see that, the point residual does.  Bound: 2e-3, the noise
    scale (the CPU statement gives 2.8e-4 to 8.3e-4 here: tests/test_line_abi.py)."""
    dst, src, Tt = outline_pair(seed, m, n)
    icp = I.Icp2d(dst)
    icp.compute_line_normals(10)
    ep = pose_error(icp.estimate_point_to_line(src, I.Transform(), 6), Tt)
    eq = pose_error(icp.estimate(src, I.Transform(), 6), Tt)
    icp.close()
    print(f"seed {seed}: point-to-line {ep:.3g}, point-to-point {eq:.3g}")
    assert ep < 2e-3 and ep < eq, (ep, eq)


def test_a_single_wall_gives_no_update():
    """every normal is (1, 0): y and theta are unobserved, the normal equations are exactly singular and -- as the
    reference's inverse3x3 does (src/linalg.rs:12-14) -- no update is produced at all"""
    rng = np.random.default_rng(9)
    wall = np.ascontiguousarray(np.stack([np.full(4000, 3.0), rng.uniform(-3, 3, 4000)], axis=1))
    src = wall[rng.integers(0, 4000, 1200)].copy()
    src[:, 0] += rng.normal(-0.02, 2e-3, len(src))
    icp = I.Icp2d(wall)
    icp.compute_line_normals(8)
    T, _, inner = icp.estimate_point_to_line(src, I.Transform(), 3, return_info=True)
    icp.close()
    assert inner.tolist() == [0, 0, 0]
    assert np.array_equal(T.as_array(), I.Transform().as_array())


# ------------------------------------------------------------------ the gate

def blob_scene(seed, n, m=3000, share=0.4):
    """an outline of m targets; the scan: n points, `share` of them a Gaussian blob (sigma 0.25) at (1.6, 0.3) that the
    target does not hold (the nearest wall is 1.4 away), the rest independent outline samples; true pose
    (0.10, -0.08, 0.03)"""
    rng = np.random.default_rng(seed)
    dst = outline(rng, m)
    k = int(n * share)
    world = np.concatenate([np.array([1.6, 0.3]) + rng.normal(size=(k, 2)) * 0.25, outline(rng, n - k)])
    Tt = I.Transform([0.10, -0.08, 0.03])
    return dst, np.ascontiguousarray(moved2(rng.permutation(world), Tt.inverse())), Tt


@pytest.fixture(scope="module")
def gate_handle():
    dst, _, _ = blob_scene(5, 16)
    icp = I.Icp2d(dst)
    icp.compute_line_normals(10)
    yield icp, dst, icp.read_line_normals()
    icp.close()


@pytest.mark.parametrize("n", TILE_EDGES)
def test_an_infinite_bound_returns_the_bits_of_the_ungated_call(gate_handle, n):
    import torch

    icp, _, _ = gate_handle
    _, src, _ = blob_scene(5, n)
    T0, idx0, inner0 = icp.estimate_point_to_line(src, I.Transform(), 4, return_info=True)
    for s in (src, torch.from_numpy(src).cuda()):
        T, idx, inner, inl = icp.estimate_point_to_line(s, I.Transform(), 4, return_info=True,
                                                        max_correspondence_distance=INF)
        assert np.array_equal(bits(T), bits(T0)), (n, T.as_array(), T0.as_array())
        assert np.array_equal(idx, idx0) and np.array_equal(inner, inner0), (n, inner, inner0)
        assert np.array_equal(inl, np.full(4, n)), (n, inl)
        T1 = icp.estimate_point_to_line(s, I.Transform(), 4, max_correspondence_distance=INF)  # (without the info)
        assert np.array_equal(bits(T1), bits(T0))
    assert inner0.sum() > 0


def test_a_zero_bound_on_disjoint_clouds_keeps_nothing_and_leaves_the_pose_alone(gate_handle):
    icp, dst, _ = gate_handle
    init = I.Transform([0.01, 0.02, 0.005])
    far = np.ascontiguousarray(dst[:1500] + np.array([50.0, 0.0]))
    for r in (0.0, 0.25):
        T, _, inner, inl = icp.estimate_point_to_line(far, init, 3, return_info=True, max_correspondence_distance=r)
        assert np.array_equal(bits(T), bits(init)) and inner.tolist() == [0, 0, 0] and inl.tolist() == [0, 0, 0]


class _Lifted:
    """what tests/test_gpu_gated_plane.py's chain() asks of a handle, answered by a 2-D handle for lifted clouds"""

    def __init__(self, icp):
        self.icp = icp

    def read_targets(self):
        return lift(self.icp.read_targets())

    def evaluate(self, src3, T, r, return_indices=False):
        return self.icp.evaluate(np.ascontiguousarray(src3[:, :2]), T, r, return_indices=return_indices)


@pytest.mark.parametrize("n", TILE_EDGES)
def test_a_finite_bound_tracks_the_chained_cpu_statement(gate_handle, n):
    """the definition one outer iteration at a time (chain(): the kept points of iteration k are those whose match under
    T_k lies within r; the step is the CPU statement's single iteration on them), on lifted clouds: d2 gets + 0 * 0"""
    icp, dst, normals = gate_handle
    _, src, Tt = blob_scene(5, n)
    T, _, inner, inl = icp.estimate_point_to_line(src, I.Transform(), 10, return_info=True,
                                                  max_correspondence_distance=0.25)
    tree, normals3 = O.KdTree(lift(dst)), lift(normals)

    def step(kept3, Tk):
        rc, oT, _, oinner = O.p2pl_estimate(tree, normals3, kept3, O.Pose(*Tk.pose.as_tuple()), 1)
        assert rc == O.OK
        return I.Transform.from_pose(oT), oinner[0]

    oT, oinner, oinl = chain(_Lifted(icp), lift(src), 10, 0.25, step)
    err = float(np.max(np.abs(T.as_array() - oT.as_array())))
    print(f"n={n}: inliers {inl.tolist()}, inner {inner.tolist()}, against the CPU statement {err:.3g}")
    assert np.array_equal(inl, oinl), (inl, oinl)
    assert np.array_equal(inner, oinner), (inner, oinner)
    assert err < 1e-9

    def tree_step(kept3, Tk):  # the same step with its sums in the tree of reduce_geometry(kept): equal to the bit
        rc, tT, _, tinner = oracle_plane_in_device_order(icp, tree, normals3, kept3, Tk, 1)
        assert rc == O.OK
        return I.Transform.from_pose(tT), tinner[0]

    tT, tinner, tinl = chain(_Lifted(icp), lift(src), 10, 0.25, tree_step)
    assert np.array_equal(inl, tinl) and np.array_equal(inner, tinner), (inner, tinner)
    assert np.array_equal(bits(T), bits(tT)), (T.as_array(), tT.as_array())
    assert np.all(inl < n) and np.all(inl > 0) and inner.sum() > 0  # the gate removes the blob, not the walls
    print(f"n={n}: pose error gated {pose_error(T, Tt):.3g}, ungated "
          f"{pose_error(icp.estimate_point_to_line(src, I.Transform(), 10), Tt):.3g}")


# ------------------------------------------------------------------ a map that grows and lets go

def test_after_an_append_the_normals_are_stale_until_the_update_and_the_older_rows_are_kept():
    dst = outline(np.random.default_rng(21), 2500)
    extra = outline(np.random.default_rng(22), 700)
    src = dst[::5].copy()
    icp = I.Icp2d(dst)
    icp.compute_line_normals(8)
    before = icp.read_line_normals()
    icp.append(extra)
    for kw in ({}, {"max_correspondence_distance": 0.5}):
        with pytest.raises(I.IcpError) as e:  # the appended targets have no normal yet
            icp.estimate_point_to_line(src, I.Transform(), 1, **kw)
        assert e.value.status == _lib.BAD_ARGUMENT
    with pytest.raises(I.IcpError):
        icp.read_line_normals()
    with pytest.raises(I.IcpError) as e:  # one neighbourhood size per cloud
        icp.update_line_normals(10)
    assert e.value.status == _lib.BAD_ARGUMENT
    icp.update_line_normals(8)
    got = icp.read_line_normals()
    assert got.shape == (3200, 2)
    assert np.array_equal(got[:2500].view(np.uint64), before.view(np.uint64))  # kept, bit for bit
    # the appended rows: from their neighbours in the cloud as it is now
    want = line_normals_numpy(np.concatenate([dst, extra]), 8, np.arange(2500, 3200))
    assert np.max(np.abs(got[2500:] - want)) < 1e-9
    T, idx, inner = icp.estimate_point_to_line(src, I.Transform([0.01, 0.0, 0.002]), 2, return_info=True)  # usable again
    assert inner.sum() > 0 and idx.max() < 3200
    icp.close()


def test_a_crop_carries_the_normals_of_the_kept_targets_along():
    dst = outline(np.random.default_rng(31), 4000)
    icp = I.Icp2d(dst)
    icp.compute_line_normals(8)
    old = icp.read_line_normals()
    removed, new_index = icp.crop([1.0, 0.0], 2.2, return_index=True)
    kept = new_index != 0xffffffff
    assert 0 < removed < 4000 and removed == int((~kept).sum())
    got = icp.read_line_normals()
    want = np.zeros((int(kept.sum()), 2))
    want[new_index[kept]] = old[kept]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))  # the old rows at new_index, bit for bit
    # the estimate works without recomputing, and is the CPU statement on the kept cloud with the carried normals
    kept_dst = icp.read_targets()
    assert np.array_equal(kept_dst, dst[kept])
    Tt = I.Transform([0.02, -0.015, 0.008])
    src = np.ascontiguousarray(moved2(kept_dst[::3], Tt.inverse()))
    T, idx, inner = icp.estimate_point_to_line(src, I.Transform(), 4, return_info=True)
    rc, oT, oidx, oinner = oracle_point_to_line(kept_dst, got, src, I.Transform(), 4)
    assert rc == O.OK and np.array_equal(idx, oidx) and np.array_equal(inner, oinner)
    assert np.max(np.abs(T.as_array() - oT.as_array())) < 1e-9
    # an append after the crop: only the appended targets get a normal from the update
    icp.append(outline(np.random.default_rng(32), 300))
    icp.update_line_normals(8)
    again = icp.read_line_normals()
    assert np.array_equal(again[:len(got)].view(np.uint64), got.view(np.uint64))
    icp.close()
