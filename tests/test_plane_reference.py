"""The CPU statement of the scalar-residual estimators (point-to-plane, and point-to-line on lifted clouds) in both
of its fold orders -- orc_p2pl_update / orc_p2pl_estimate with sum_mode 0 (left folds) and 1 (the device's tree) --
against three things that are not the oracle:
  * a long-double witness of one update written from the definition at the top of icp_rust_amd/csrc/p2plane.hip
    (parity_util.reference_plane_update), within the rounding bound below;
  * a hand-written 64-lane butterfly in numpy, to the bit;
  * (the bits the left fold returned before the update was factored out of orc_p2pl_estimate are held as constants in
    tests/test_p2plane.py and tests/test_line_abi.py).
tests/test_gpu_plane_parity.py then holds the device to the bits of the tree order; the scenes it runs are built here.

The bound.  The witness shares the f64 residuals and sigma (exact order statistics of them) with the code under test,
so what differs is the rounding of each term and of the sums.  A term of the device's sums is
    (wg * J[a]) * J[b]   or   (wg * J[a]) * r,   wg = drho(r * r) * (1. / sigma),   J[2] = nx * b0 + ny * b1
(k_p2pl_accumulate; at the identity inner pose J[0] = nx * 1 + ny * 0 and J[1], b0 = -p_y, b1 = p_x are exact).  Its
roundings: r * r, sqrt, k / sqrt, 1. / sigma and their product -- 5 for wg; the two products and the sum of J[2],
relative to |nx p_y| + |ny p_x| -- 2 for each of the two J factors that can be J[2], 4; the term's own two products
-- 2.  c = 11.  Folded to a depth of D additions the sum is off by at most (D + 11) u times the sum of its terms'
magnitudes (u = 2^-53, first order), and a relative perturbation eps of every term moves delta by at most eps times
the Skeel condition number the witness computes with those magnitudes:
    max |delta - delta_ref| <= cond * (D + 11) * u * max |delta_ref|.
D is n for the left fold and test_wgn_reference.fold_depth_tree(n) for the tree.  One pair of n dropped moves delta
by about 1 / n of itself: seven orders of magnitude above the tree's bound at n = 131 073."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from parity_util import plane_residuals_identity, reference_plane_update
from test_gpu_gated_plane import blob_scene as blob_scene_3d
from test_gpu_line import blob_scene as blob_scene_2d
from test_line_abi import TRUE_PARAM, lift, line_normals_numpy, moved2, outline
from test_p2plane import moved, room
from test_wgn_reference import U, fold_depth_tree, rel_err

C_TERM = 11  # roundings in one term, counted in the module docstring
M_ROOM = 3000   # targets of the 3-D scenes
M_LINE = 1800   # targets of the 2-D scenes (a batch workgroup serves up to 2 048)
NORMALS_K = 8
D_TIE = 0.125   # the distance off the wall that the tied run sits at


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.set_threads(16)
    yield
    O.set_threads(1)


def bits(a):
    a = a.as_array() if hasattr(a, "as_array") else a
    return np.asarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ the scenes (shared with test_gpu_plane_parity.py)
# Every builder returns (dst, src, init Transform): `dim` = 3 for the plane call on a room, 2 for the line call on the
# room's outline.  Targets depend on (dim, scene) only, so one handle serves every size of a scene.

def lifted(dim, a):
    return a if dim == 3 else lift(a)


def noisy_targets(dim):
    rng = np.random.default_rng(40 + dim)
    return room(rng, M_ROOM) if dim == 3 else outline(rng, M_LINE)


def noisy_scene(dim, n):
    """today's room / outline scan: n target points drawn with replacement, 1e-3 noise, moved by the inverse of a small
    true pose, so that the inner loops run several updates"""
    dst = noisy_targets(dim)
    rng = np.random.default_rng(1000 * dim + n)
    src = dst[rng.integers(0, len(dst), n)] + rng.normal(0.0, 1e-3, (n, dim))
    Tt = I.Transform([0.05, -0.04, 0.015] if dim == 3 else list(TRUE_PARAM))
    src = moved(src, Tt.inverse()) if dim == 3 else moved2(src, Tt.inverse())
    return dst, np.ascontiguousarray(src), I.Transform()


def wall_targets(dim):
    """exact walls.  3-D: 600 lattice points (multiples of 1/64) on each of the planes z = 0, x = 3, y = -3; the walls'
    z-values are offset by 1/128 so that no wall point lies on the floor.  2-D: the lines x = 3 and y = -2 of the
    outline, the coordinate along the line a multiple of 1/1024.  No point twice."""
    rng = np.random.default_rng(60 + dim)
    if dim == 3:
        k = M_ROOM // 5
        fl = rng.choice(384 * 384, k, replace=False)
        w1 = rng.choice(384 * 128, k, replace=False)
        w2 = rng.choice(384 * 128, k, replace=False)
        floor = np.stack([(fl % 384) / 64.0 - 3.0, (fl // 384) / 64.0 - 3.0, np.zeros(k)], axis=1)
        wall1 = np.stack([np.full(k, 3.0), (w1 % 384) / 64.0 - 3.0, (w1 // 384) / 64.0 + 1.0 / 128], axis=1)
        wall2 = np.stack([(w2 % 384) / 64.0 - 3.0, np.full(k, -3.0), (w2 // 384) / 64.0 + 1.0 / 128], axis=1)
        return np.ascontiguousarray(np.concatenate([floor, wall1, wall2]))
    k = M_LINE * 2 // 5
    a = rng.choice(4096, k, replace=False)
    b = rng.choice(6144, M_LINE - k, replace=False)
    return np.ascontiguousarray(np.concatenate([np.stack([np.full(k, 3.0), a / 1024.0 - 2.0], axis=1),
                                                np.stack([b / 1024.0 - 3.0, np.full(M_LINE - k, -2.0)], axis=1)]))


_WALLS = {}


def walls(dim):
    """(targets, the CPU statement of their normals, a kd-tree of the lifted targets).  The scenes are built from the
    CPU normals, so that they are the same scenes wherever they are built; the estimators under test are fed the
    device's own normals."""
    if dim not in _WALLS:
        dst = wall_targets(dim)
        normals = O.p2pl_normals(dst, NORMALS_K) if dim == 3 else line_normals_numpy(dst, NORMALS_K)
        _WALLS[dim] = (dst, normals, O.KdTree(lifted(dim, dst)))
    return _WALLS[dim]


def wall_scene(dim, n, tied):
    """n sources off the exact walls: each is target + normal * d for a target whose normal is exactly an axis, d
    dyadic -- `tied` of them at d = 1/8 exactly, the rest at 1/8 + k/512, k in [-31, 31] -- in a shuffled order.  Every
    coordinate is a dyadic rational of few bits, so at the identity pose the residuals are exact; a source whose
    nearest target does not give it the residual d (next to a corner: a target of the other wall, or one whose
    neighbourhood spans both) is drawn again."""
    dst, normals, tree = walls(dim)
    axis = np.flatnonzero((np.abs(normals) == 1.0).any(axis=1))
    rng = np.random.default_rng(2000 * dim + 7 * n + tied)
    j = axis[rng.integers(0, len(axis), n)]
    d = D_TIE + rng.integers(-31, 32, n) / 512.0
    d[:tied] = D_TIE
    d = d[rng.permutation(n)]
    for _ in range(50):
        src = np.ascontiguousarray(dst[j] + normals[j] * d[:, None])
        rc, idx = tree.search(lifted(dim, src))
        assert rc == O.OK
        bad = plane_residuals_identity(lifted(dim, src), idx, tree.dst, lifted(dim, normals)) != d
        if not bad.any():
            return dst, src, I.Transform()
        j[bad] = axis[rng.integers(0, len(axis), int(bad.sum()))]
    raise AssertionError("the walls have too few targets away from the corners")


def ties_scene(dim, n):
    """two fifths of the residuals sit at exactly 1/8: the median lies inside a run of equal values, sigma > 0"""
    return wall_scene(dim, n, (2 * n) // 5)


def sigma0_scene(dim, n):
    """more than half of the residuals sit at exactly 1/8: the MAD is 0, no term is accumulated, the solve is
    singular, no update is applied -- while the Huber error is still summed"""
    return wall_scene(dim, n, (3 * n) // 5 + 1)


def heavy_scene(dim, n):
    """a scan that is half a blob the target does not hold (tests/test_gpu_gated_plane.py, tests/test_gpu_line.py).  The
    2-D blob lies 1.4 from the nearest wall: residuals on both sides of the Huber threshold.  The 3-D blob lies 0.8
    from the floor and both walls: large residuals, but none above 1.345 -- far_scene is there for that."""
    if dim == 3:
        dst, src, _ = blob_scene_3d(5, n=n, m=M_ROOM)
    else:
        dst, src, _ = blob_scene_2d(5, n, m=M_LINE)
    return dst, src, I.Transform()


def far_scene(dim, n):
    """the noisy scene's targets; half of the scan is a Gaussian blob (sigma 0.3) 2.2 above the floor and 2.5 from both
    walls (2-D: sigma 0.2, 1.5 from the nearest walls), the rest target points with 1e-3 noise; true pose
    (0.10, -0.08, 0.03).  About half of the |r| lie above 1.345: both branches of rho and drho carry weight."""
    dst = noisy_targets(dim)
    rng = np.random.default_rng(3000 * dim + n)
    k = n // 2
    centre, spread = (np.array([0.5, -0.5, 2.2]), 0.3) if dim == 3 else (np.array([1.5, 0.0]), 0.2)
    world = np.concatenate([centre + rng.normal(size=(k, dim)) * spread,
                            dst[rng.integers(0, len(dst), n - k)] + rng.normal(size=(n - k, dim)) * 1e-3])
    Tt = I.Transform([0.10, -0.08, 0.03])
    world = rng.permutation(world)
    src = moved(world, Tt.inverse()) if dim == 3 else moved2(world, Tt.inverse())
    return dst, np.ascontiguousarray(src), I.Transform()


SCENES = {"noisy": noisy_scene, "ties": ties_scene, "sigma0": sigma0_scene, "heavy": heavy_scene, "far": far_scene}


def cpu_normals(dim, dst):
    return O.p2pl_normals(dst, NORMALS_K) if dim == 3 else lift(line_normals_numpy(dst, NORMALS_K))


def pairs_at_identity(dim, scene, n):
    """(st, idx, dst3, normals3) of the scene's first evaluation, with the CPU statements of the normals"""
    dst, src, init = SCENES[scene](dim, n)
    assert np.array_equal(init.as_array(), I.Transform().as_array())
    dst3, st = lifted(dim, dst), lifted(dim, src)
    rc, idx = O.KdTree(dst3).search(st)
    assert rc == O.OK
    return st, idx, dst3, cpu_normals(dim, dst)


# ------------------------------------------------------------------ the scenes are what they say

@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [2, 3, 65, 513, 1000])
def test_wall_scenes_have_exact_residuals_a_tied_median_and_a_zero_mad(dim, n):
    for scene in ("ties", "sigma0"):
        st, idx, dst3, normals = pairs_at_identity(dim, scene, n)
        r = plane_residuals_identity(st, idx, dst3, normals)
        tied = int((r == D_TIE).sum())
        exact = np.all(r * 1024.0 == np.round(r * 1024.0))  # multiples of 1/1024: nothing was rounded
        want = (2 * n) // 5 if scene == "ties" else (3 * n) // 5 + 1
        print(f"dim {dim} {scene} n={n}: {tied} residuals at 1/8 (wanted {want}), exact {exact}")
        assert exact and tied >= want  # (k = 0 puts a few more there)
        for mode in (0, 1):
            rc, sigma, delta, err = O.p2pl_update(O.transform_identity(), st, idx, dst3, normals, mode, 1, 512)
            assert np.isfinite(err) and err > 0.0
            if scene == "sigma0":
                assert (rc, sigma) == (O.NONE, 0.0)
            elif n >= 65:
                assert rc == O.OK and sigma > 0.0 and np.median(r) == D_TIE and np.all(np.isfinite(delta))
        dst, src, init = SCENES[scene](dim, n)
        rc, T, _, inner = O.p2pl_estimate(O.KdTree(dst3), normals, lifted(dim, src), O.transform_identity(), 3)
        assert rc == O.OK
        if scene == "sigma0":
            assert inner.tolist() == [0, 0, 0] and np.array_equal(bits(T), bits(O.transform_identity()))
        elif n >= 65:
            assert inner.sum() > 0


@pytest.mark.parametrize("dim,scene", [(3, "far"), (2, "far"), (2, "heavy"), (3, "heavy")])
def test_which_scenes_have_residuals_on_both_sides_of_the_huber_threshold(dim, scene):
    st, idx, dst3, normals = pairs_at_identity(dim, scene, 1025)
    r = np.abs(plane_residuals_identity(st, idx, dst3, normals))
    above = int((r > 1.345).sum())
    print(f"dim {dim} {scene}: {above} of {len(r)} |r| above 1.345, largest {r.max():.3f}")
    if (dim, scene) == (3, "heavy"):
        assert above == 0 and r.max() > 0.5  # (what far_scene is for)
    else:
        assert 100 <= above <= len(r) - 100


# ------------------------------------------------------------------ both fold orders against the long-double witness

def test_both_fold_orders_meet_the_bound_of_the_longdouble_update_and_a_dropped_pair_does_not():
    n = 131_073  # odd, and the first size at which a thread of the tree folds a second pair
    st, idx, dst3, normals = pairs_at_identity(3, "noisy", n)
    want, sigma, want_err, cond = reference_plane_update(st, idx, dst3, normals, skeel=True)
    print(f"n={n}: Skeel condition number {cond:.3f}, sigma {sigma:.3e}")
    # the premise of the bound (the witness reports 2.54 on this scene: the scan is a frame's motion away from the map,
    # J^T r does not cancel)
    assert 1.0 <= cond < 4.0, cond
    blocks, threads = I.reduce_geometry(n)
    assert (blocks, threads) == (256, 512) and n > blocks * threads
    depth = {0: n, 1: fold_depth_tree(n)}
    assert depth[1] == 2 + 6 + 7 + 1 + 6 + 7
    T = O.transform_identity()
    bound = {}
    for mode in (0, 1):
        rc, osigma, delta, err = O.p2pl_update(T, st, idx, dst3, normals, mode, blocks, threads)
        assert rc == O.OK and osigma == sigma  # the order statistics: exact on both sides
        bound[mode] = cond * (depth[mode] + C_TERM) * U
        e = rel_err(delta, want)
        # the Huber error: r * r, and above the threshold sqrt, the product with 2 k, k * k and the difference, each
        # at most twice rho -- 8 roundings
        ee = float(abs(np.longdouble(err) - want_err) / want_err)
        print(f"sum_mode {mode}: delta off by {e:.3g} (bound {bound[mode]:.3g}), Huber error by {ee:.3g}")
        assert e <= bound[mode], (mode, e, bound[mode])
        assert ee <= (depth[mode] + 8) * U, (mode, ee)
    assert bound[1] < 2e-14 and bound[0] < 1e-10  # (at the cap of cond: 4 * 40 u, 4 * 131 084 u)
    # ... and the witness sees a dropped pair (what the bound is for)
    keep = np.ones(n, dtype=bool)
    keep[n // 2] = False
    rc, _, short, _ = O.p2pl_update(T, np.ascontiguousarray(st[keep]), idx[keep], dst3, normals, 1, blocks, threads)
    assert rc == O.OK and rel_err(short, want) > 100 * bound[1], (rel_err(short, want), bound[1])


# ------------------------------------------------------------------ the tree against a hand-written butterfly

def butterfly(v):
    """one wave of tree_block_reduce on the rows of v (64 x k): v[l] += v[l + off], off = 32 .. 1"""
    v = v.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[:off] = v[:off] + v[off:2 * off]
    return v[0]


@pytest.mark.parametrize("scene", ["noisy", "far", "ties"])
@pytest.mark.parametrize("n", [2, 3, 37, 64])
def test_one_wave_of_the_tree_equals_a_butterfly_in_numpy(scene, n):
    """blocks = 1, threads = 64, n <= 64: every lane holds one pair's terms, the wave folds them, the second stage adds
    zeros.  The terms are k_p2pl_accumulate's expressions in numpy f64 (each operation rounded on its own) at an inner
    pose that is not the identity; the solve is the oracle's inverse3x3 (tests/test_oracle_kat.py) and -inv * jtr."""
    st, idx, dst3, normals = pairs_at_identity(3, scene, 64)
    st, idx = np.ascontiguousarray(st[:n]), idx[:n]
    Ti = O.transform_new(np.array([0.01, -0.02, 0.005]))
    q, nq = dst3[idx], normals[idx]
    ax, ay = st[:, 0], st[:, 1]
    rx = ((Ti.r00 * ax + Ti.r01 * ay) + Ti.tx) - q[:, 0]
    ry = ((Ti.r10 * ax + Ti.r11 * ay) + Ti.ty) - q[:, 1]
    r = (nq[:, 0] * rx + nq[:, 1] * ry) + nq[:, 2] * (st[:, 2] - q[:, 2])
    rc, sigma = O.standard_deviation(r)
    assert rc == O.OK and sigma > 0.0
    e = r * r
    k2 = 1.345 * 1.345
    with np.errstate(divide="ignore"):
        drho = np.where(e <= k2, 1.0, 1.345 / np.sqrt(e))
    rho = np.where(e <= k2, e, 2.0 * 1.345 * np.sqrt(e) - k2)
    b0 = Ti.r00 * -ay + Ti.r01 * ax
    b1 = Ti.r10 * -ay + Ti.r11 * ax
    J = [nq[:, 0] * Ti.r00 + nq[:, 1] * Ti.r10, nq[:, 0] * Ti.r01 + nq[:, 1] * Ti.r11, nq[:, 0] * b0 + nq[:, 1] * b1]
    wg = drho * (1.0 / sigma)
    lanes = np.zeros((64, 13))
    for a in range(3):
        lanes[:n, 9 + a] = (wg * J[a]) * r
        for b in range(3):
            lanes[:n, 3 * a + b] = (wg * J[a]) * J[b]
    lanes[:n, 12] = rho
    tot = butterfly(lanes)
    solvable, inv = O.inverse3x3(tot[:9].reshape(3, 3))
    rc, osigma, delta, err = O.p2pl_update(Ti, st, idx, dst3, normals, 1, 1, 64)
    assert osigma == sigma and np.array_equal(bits(np.array([err])), bits(tot[12:13]))
    if solvable != O.OK:  # (two pairs, or three of which one lies on the floor: J^T J has no full rank)
        assert n <= 3 and rc == O.NONE
        return
    want = np.array([((-inv[i, 0]) * tot[9] + (-inv[i, 1]) * tot[10]) + (-inv[i, 2]) * tot[11] for i in range(3)])
    assert rc == O.OK and np.array_equal(bits(delta), bits(want)), (delta, want)
    # the left fold adds the same terms in another order: equal to rounding, and at n = 2 (one addition) to the bit
    rc, _, left, lerr = O.p2pl_update(Ti, st, idx, dst3, normals, 0, 0, 0)
    assert rc == O.OK and np.max(np.abs(left - delta)) <= 1e-12 * np.max(np.abs(delta))
    if n == 2:
        assert np.array_equal(bits(left), bits(delta)) and lerr == err


def test_a_nan_source_point_is_a_nan_status_in_either_fold_order():
    dst, src, _ = noisy_scene(3, 65)
    src[17, 1] = np.nan
    tree, normals = O.KdTree(dst), O.p2pl_normals(dst, NORMALS_K)
    for mode in (0, 1):
        rc, _, _, _ = O.p2pl_estimate(tree, normals, src, O.transform_identity(), 2, mode, 1, 512)
        assert rc == O.NAN
