"""The k nearest targets "by (d^2, index)" behind every normal (include/icp_mi355x.h sections 7 and 14), where the
continuous random clouds of the other suites never go: exact ties at the k-th place, candidates outside the visited
block at the distance of the current k-th, coincident targets, clouds far from the origin, clipped k.  Three device
searches choose those neighbours -- k_target_normals (3-D grid), k_line_normals (2-D grid) and the one-workgroup sweep
normals_of_sorted_targets<DIM> behind the batch kernels -- and none returns its lists: the observable is the normal,
so the clouds (tests/tie_clouds.py: lattices, every d^2 exact) make the normal depend on which tied candidates got in.

The CPU tests prove that on the inputs themselves: most rows tie at the k-th place, the covariances are well
conditioned, and the wrong rule "ties by highest index" moves most normals by more than 1e-3 -- a million times the
1e-9 the device tests allow against the CPU statements (O.p2pl_normals, line_normals_numpy), on ALL rows."""
import time

import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
import tie_clouds as TC
from icp_rust_amd import _lib
from test_line_abi import line_normals_numpy, moved2
from test_line_quality_abi import nearest, restate

gpu = pytest.mark.gpu
TOL = 1e-9  # of test_device_normals_equal_the_cpu_statement and test_device_line_normals_equal_the_restatement
BATCH_K = (3, 8, 16)
BATCH_CASES = [(name, k) for name in TC.LINE_CLOUDS for k in BATCH_K]
BATCH_ROWS = 300
BATCH_POSE = [0.02, -0.015, 0.01]
BATCH_ITER = 4


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


def ids(cases):
    return [f"{name}-k{k}" for name, k in cases]


# ------------------------------------------------------------------ 1. the inputs themselves (CPU)

def test_every_squared_distance_of_every_cloud_is_exact():
    """d^2 as the kernels form it from the float64 coordinates has the bits of the integer d^2 of the lattice
    coordinates times spacing^2 (a power of two): no rounding anywhere, so equal distances are equal doubles"""
    names = list(dict.fromkeys(name for name, _ in TC.PLANE_CASES + TC.LINE_CASES))
    clouds = [TC.cloud(name) for name in names]
    clouds += [TC.tiny(name) for name in dict.fromkeys(name for name, _ in TINY)]
    assert {name for name, _ in TINY} == set(TC.TINY_NAMES)
    for c in clouds:
        assert np.array_equal(c.pts * 2.0 ** c.shift, c.lattice.astype(np.float64)), c  # the coordinates themselves
        got = TC.d2_float(c)
        want = TC.d2_integer(c).astype(np.float64) * c.spacing ** 2
        assert TC.d2_integer(c).max() < 2 ** 53, c
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), c
    assert np.abs(TC.cloud("slab+x31").pts[:, 0]).min() >= 2.0 ** 31
    assert TC.cloud("strip200x3+split").pts[:, 0].min() == -float(TC.SPLIT_AT)


@pytest.mark.parametrize("name,k", TC.PLANE_CASES + TC.LINE_CASES, ids=ids(TC.PLANE_CASES + TC.LINE_CASES))
def test_the_tie_rule_decides_the_normals_of_these_clouds(name, k):
    """(a) at least 0.6 of the rows tie exactly at the k-th place; (b) no row's covariance is ill conditioned (the
    duplicated slab: at most 5 %); (c) "ties by highest index" moves at least half of the normals by more than 1e-3"""
    c = TC.cloud(name)
    tie, ill, moved = TC.tie_share(c, k), TC.ill_conditioned(c, k), TC.moved_share(c, k)
    print(f"{name} k={k} m={c.m}: tie at k {tie:.3f}, ill-conditioned rows {int(ill.sum())}, wrong rule moves {moved:.3f}")
    assert tie >= 0.6
    assert ill.mean() <= TC.ILL_CAP.get(name, 0.0), int(ill.sum())
    assert moved >= 0.5
    n = TC.reference(c, k)
    assert np.max(np.abs(np.linalg.norm(n, axis=1) - 1.0)) < 1e-12  # every row has a normal


def test_the_cpu_statements_know_the_tie_rule():
    """the rule itself on a few points by hand: of targets equally far, the lower indices are the neighbours"""
    # row 0 at the origin; rows 1 and 2 at distance 1 along x; rows 3 and 4 at the same distance along y and z (3-D) or
    # +-y (2-D).  k = 3: {0, 1, 2}, a line along x.  Under the wrong rule: {0, 4, 3}, a line across it.
    p3 = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 1], [9, 9, 9]], dtype=np.float64)
    n = O.p2pl_normals(p3, 3)[0]
    assert n[0] == 0.0 and abs(np.hypot(n[1], n[2]) - 1.0) < 1e-12
    p2 = np.array([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1], [9, 9]], dtype=np.float64)
    assert np.array_equal(line_normals_numpy(p2, 3)[0], [0.0, 1.0])
    assert np.array_equal(line_normals_numpy(np.ascontiguousarray(p2[::-1]), 3)[::-1][0], [1.0, 0.0])


def batch_pair(name):
    """(targets, source, pose, bound, initial pose) of the batch comparisons: BATCH_ROWS rows of the cloud seen from
    the small pose BATCH_POSE, evaluated 0.3 / -0.2 lattice spacings off it -- every match is the row's own lattice
    point, off its line by a known amount, and no match is a tie between DIFFERENT points.  The estimate starts at
    least 4 / 3 mm off, so that on the fine lattice of the split cloud too its first update is above the threshold
    under which the inner loop stops"""
    c = TC.cloud(name)
    rows = np.random.default_rng(TC.SEED + 1).choice(c.m, BATCH_ROWS, replace=False)
    T = I.Transform(BATCH_POSE)
    src = np.ascontiguousarray(moved2(np.ascontiguousarray(c.pts[rows]), T.inverse()))
    Te = I.Transform([0.3 * c.spacing, -0.2 * c.spacing, 0.0]) * T
    Ti = I.Transform([max(0.3 * c.spacing, 0.004), -max(0.2 * c.spacing, 0.003), 0.0]) * T
    return c, src, Te, c.spacing, Ti


BLIND = [(b + v, k) for v in ("", "+far", "+x31") for b, k in (("strip300x2", 8), ("strip300x2", 16))] + [("stripdup", 3)]


@pytest.mark.parametrize("name,k", BATCH_CASES, ids=ids(BATCH_CASES))
def test_the_quality_restatement_sees_a_wrong_neighbour_set_on_the_batch_pairs(name, k):
    """the bit-for-bit comparison of part 4 is only worth what a wrong set changes, so on EVERY pair of part 4: where
    any row ties at the k-th place, the numpy LineQuality of the pair with the wrong rule's normals differs in its bits
    from the one with the right normals.  The pairs of BLIND have no tie at the k-th place -- the two rows of
    strip300x2 with k = 8 or 16, and stripdup with k = 3, whose three neighbours are the point's own copies: there the
    wrong rule gives the same normals and the same bits, and the device comparison of those pairs exercises the sweep,
    its worst-slot update and the rank pack, but not the tie rule.  Which pairs are blind is pinned here."""
    c, src, Te, r, _ = batch_pair(name)
    idx = nearest(c.pts, moved2(src, Te))
    rc, cnt, right = restate(c.pts, TC.reference(c, k), src, Te, r, idx)
    rc2, cnt2, wrong = restate(c.pts, TC.wrong_rule(c, k), src, Te, r, idx)
    assert rc == rc2 == _lib.OK and cnt == cnt2 == BATCH_ROWS
    differ = right.view(np.uint64) != wrong.view(np.uint64)
    tie = TC.tie_share(c, k)
    print(f"{name} k={k}: tie at k {tie:.3f}, {int(differ.sum())} of {len(right)} fields differ, "
          f"line_rmse {right[3]:.6g} vs {wrong[3]:.6g}")
    assert (tie == 0.0) == ((name, k) in BLIND)
    if tie > 0.0:
        assert differ[3] and differ[7:16].any()  # the line RMSE and the information matrix
    else:
        assert np.array_equal(TC.reference(c, k).view(np.uint64), TC.wrong_rule(c, k).view(np.uint64))
        assert not differ.any()


# ------------------------------------------------------------------ 2. the grid kernels against the CPU statement

def device_normals(c, k):
    """(normals, seconds) from a fresh handle: three columns from a 3-D cloud, two from a 2-D one"""
    t0 = time.perf_counter()
    icp = I.Icp3d(c.pts) if c.dim == 3 else I.Icp2d(c.pts)
    try:
        if c.dim == 3:
            icp.compute_normals(k)
            got = icp.read_normals()
        else:
            icp.compute_line_normals(k)
            got = icp.read_line_normals()
        return got, time.perf_counter() - t0
    finally:
        icp.close()


def assert_normals(c, k, got, want):
    assert got.shape == want.shape
    diff = float(np.max(np.abs(got - want))) if got.size else 0.0
    bad = np.nonzero(np.max(np.abs(got - want), axis=1) >= TOL)[0]
    print(f"{c.name} k={k} m={c.m}: max |device - CPU statement| {diff:.3g}, rows off {len(bad)}")
    assert len(bad) == 0 and diff < TOL, (c.name, k, diff, bad[:10], got[bad[:3]], want[bad[:3]])


@gpu
@pytest.mark.parametrize("name,k", TC.PLANE_CASES + TC.LINE_CASES, ids=ids(TC.PLANE_CASES + TC.LINE_CASES))
def test_grid_normals_equal_the_cpu_statement_at_ties(name, k):
    """plain (the lattice's faces and corners lie in the grid's first and last cells: the clamped-edge branches of
    `cover`), far from the origin, so far that the cover test can pass for no ring ("+x31": every lane ends at the
    whole grid), split into two distant halves at a fine spacing (the elongated grid with capped x cells), coincident
    targets -- all rows, 1e-9"""
    c = TC.cloud(name)
    got, dt = device_normals(c, k)
    if name.endswith("+x31"):
        print(f"{name} k={k}: create + normals + read took {dt * 1e3:.1f} ms")
    assert_normals(c, k, got, TC.reference(c, k))


@gpu
@pytest.mark.parametrize("name", ["slabdup", "stripdup"])
def test_coincident_targets_with_k_3_take_column_zero(name):
    """each point three times and k = 3: every neighbour is the point itself, the covariance is zero, no rotation, and
    the tie of the diagonals takes column 0 -- exactly"""
    c = TC.cloud(name)
    got, _ = device_normals(c, 3)
    want = np.tile([1.0, 0.0, 0.0][:c.dim], (c.m, 1))
    assert np.array_equal(TC.reference(c, 3), want)
    assert np.array_equal(got[:, :c.dim], want) and not got[:, c.dim:].any()


TINY = [("one3", 3), ("two3", 16), ("three3", 16), ("five3", 16), ("cube", 4), ("cube", 5), ("cube", 7), ("cube", 8),
        ("one2", 3), ("two2", 16), ("three2", 16), ("five2", 16), ("square", 3), ("square", 4)]


def test_the_small_clouds_have_the_normals_their_shapes_say():
    """CPU: m < 3 gives zeros; three points in the plane z = 0 give (0, 0, 1); the cube with all 8 or the square with
    all 4 has a covariance that is a multiple of the identity -- no rotation, column 0"""
    for name, k in TINY:
        c = TC.tiny(name)
        n = TC.reference(c, k)
        assert n.shape == (c.m, c.dim)
        if c.m < 3:
            assert not n.any(), name
        elif name not in ("cube", "square"):  # (k clipped to m: a generic handful of points, well conditioned)
            assert not TC.ill_conditioned(c, k).any(), name
    assert np.array_equal(TC.reference(TC.tiny("three3"), 16), np.tile([0.0, 0.0, 1.0], (3, 1)))
    assert np.array_equal(TC.reference(TC.tiny("cube"), 8), np.tile([1.0, 0.0, 0.0], (8, 1)))
    assert np.array_equal(TC.reference(TC.tiny("square"), 4), np.tile([1.0, 0.0], (4, 1)))
    # the cube with k = 4: the corner and its three edge neighbours, the normal along the corner's diagonal
    assert np.max(np.abs(np.abs(TC.reference(TC.tiny("cube"), 4)) - 1.0 / np.sqrt(3.0))) < 1e-12
    # ... and 5 or 7 of 8 take some of the three face diagonals, all at d^2 = 2: by index
    assert TC.tie_share(TC.tiny("cube"), 5) == 1.0 and TC.tie_share(TC.tiny("cube"), 4) == 0.0


@gpu
@pytest.mark.parametrize("name,k", TINY, ids=ids(TINY))
def test_small_clouds_and_clipped_k(name, k):
    c = TC.tiny(name)
    got, _ = device_normals(c, k)
    if c.dim == 2:
        assert got.shape == (c.m, 2)
    assert_normals(c, k, got[:, :c.dim], TC.reference(c, k))
    if c.m < 3:
        assert not got.any()


# ------------------------------------------------------------------ 3. the update path at ties

@gpu
@pytest.mark.parametrize("name,k,share,extended", [("slab", 7, 2, False), ("slab", 7, 4, True), ("slab", 16, 4, True),
                                                   ("strip200x3", 8, 2, False), ("strip200x3", 8, 4, True),
                                                   ("lat40x30", 10, 4, True)])
def test_normals_of_appended_lattice_rows_and_the_older_ones_kept(name, k, share, extended):
    """a handle on the first rows of the permuted lattice, the rest appended: it lies inside the bounding box.  Half
    and half doubles the cloud, past the factor of 1.5 up to which an append keeps the grid, so the grid is rebuilt;
    three quarters and a quarter extends it (append_counters says which).  Rows below `first` keep their bits, the
    others equal the CPU statement on the whole cloud."""
    c = TC.cloud(name)
    first = c.m - c.m // share
    head, tail = np.ascontiguousarray(c.pts[:first]), np.ascontiguousarray(c.pts[first:])
    assert np.array_equal(head.min(axis=0), c.pts.min(axis=0)) and np.array_equal(head.max(axis=0), c.pts.max(axis=0))
    icp = I.Icp3d(head) if c.dim == 3 else I.Icp2d(head)
    compute, update, read = ((icp.compute_normals, icp.update_normals, icp.read_normals) if c.dim == 3 else
                             (icp.compute_line_normals, icp.update_line_normals, icp.read_line_normals))
    compute(k)
    before = read()
    icp.append(tail)
    assert icp.append_counters() == ((1, 0) if extended else (0, 1))
    update(k)
    got = read()
    icp.close()
    assert np.array_equal(got[:first].view(np.uint64), before.view(np.uint64))
    if c.dim == 3:
        O.set_threads(16)
        try:
            want = O.p2pl_normals_update(c.pts, first, k, before)[first:]
        finally:
            O.set_threads(1)
    else:
        want = line_normals_numpy(c.pts, k, rows=range(first, c.m))
    diff = float(np.max(np.abs(got[first:] - want)))
    print(f"{name} k={k} first={first} of {c.m}, extended={extended}: max |device - CPU statement| {diff:.3g}")
    assert diff < TOL
    # the appended rows see the whole cloud: their normals are the full statement's
    assert np.max(np.abs(want - TC.reference(c, k)[first:])) == 0.0


# ------------------------------------------------------------------ 4. the one-workgroup sweep against the grid kernel

def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@gpu
@pytest.mark.parametrize("name,k", BATCH_CASES, ids=ids(BATCH_CASES))
def test_batch_items_equal_the_single_calls_at_ties(name, k):
    """the sweep over the x-sorted targets (unordered k-best with a tracked worst, ranks packed 4 bits x 16: k = 16
    fills them) against the grid kernel: the quality of a pose and a short estimate, served by the batch LAUNCH, equal
    the single calls on a fresh handle bit for bit.  (The pairs of BLIND have no tie at the k-th place: they hold the
    sweep, the worst-slot update and the pack to the grid kernel, not the tie rule.  The quality is taken a fraction of
    a lattice spacing off the pose the source was moved by, and the estimate starts off it too: at that pose itself
    every residual is zero and neither result would depend on the normals -- see batch_pair.)"""
    c, src, Te, r, Ti = batch_pair(name)
    icp = I.Icp2d(c.pts)
    icp.compute_line_normals(k)
    q1 = icp.evaluate_point_to_line(src, Te, r)
    T1, idx1, inner1 = icp.estimate_point_to_line(src, Ti, BATCH_ITER, return_info=True)
    icp.close()
    B = I.IcpBatch(2)
    qs, status = B.evaluate_point_to_line([src], [c.pts], [Te], k=k, max_correspondence_distance=r, return_status=True)
    assert B.line_quality_counters() == (1, 0, 1, 0)  # by the batch kernel, not one by one through the grid kernel
    Ts, idxs, inner, st = B.estimate_point_to_line([src], [c.pts], [Ti], BATCH_ITER, k=k, return_info=True)
    assert B.line_counters() == (1, 0, 1, 0)
    B.close()
    assert status[0] == _lib.OK and st[0] == _lib.OK
    print(f"{name} k={k}: inliers {q1.inliers} of {q1.n}, line_rmse {q1.line_rmse:.6g}, inner counts {inner1.tolist()}")
    assert q1.n == qs[0].n == BATCH_ROWS and q1.inliers == qs[0].inliers == BATCH_ROWS
    assert same_bits(qs[0].as_array(), q1.as_array()), (qs[0].as_array(), q1.as_array())
    assert same_bits(Ts[0].as_array(), T1.as_array()), (Ts[0].as_array(), T1.as_array())
    assert np.array_equal(idxs[0], idx1) and np.array_equal(inner[0], inner1)
