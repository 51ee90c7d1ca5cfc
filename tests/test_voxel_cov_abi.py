"""CPU-side checks of voxel covariances (icp_voxel_covariances[_device]: include/icp_mi355x.h section 26): declared,
exported and bound; ABI version still 8; the numpy restatement of the rule (covariances_of, the arbiter of
tests/test_gpu_voxel_cov.py, built on section 25's centroids_of and fold) against a dict-based loop and against exact
rational arithmetic, on clouds far from the origin where the one-pass E[xx] - mm fails the same bound; the c <= ddof,
lone-point, overflow and NaN cases; every argument error rejected before the device is touched; the Python refusals; the
kernels' register and scratch use (hipcc cross-compiles without a GPU)."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib
from test_crop_abi import HIPCC, ROOT, _usage, declared
from test_voxel_abi import BAD_SIZES, boundary_input, special_input
from test_voxel_mean_abi import GONE, _fold_rows, centroids_by_dict, centroids_of, fold

NEW = ("icp_voxel_covariances", "icp_voxel_covariances_device")
PAIRS = {2: ((0, 0), (0, 1), (1, 1)), 3: ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}  # xx, xy, yy / xx .. zz


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


# ------------------------------------------------------------------------ the rule, restated ----
def moments_of(p, v):
    """the sums of section 26 before their division: (S, mean, count, first_index, voxel_of), S[r, ab] = fold of the
    products (x[i, a] - mean[r, a]) * (x[i, b] - mean[r, b]) over voxel r's members in ascending index.  Everything but
    S is centroids_of's.  Voxels of up to 256 members are one group of the tree each (folded many rows at a time);
    larger ones go through fold."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    n, dim = p.shape
    mean, count, first, voxel_of = centroids_of(p, v)
    S = np.zeros((len(first), len(PAIRS[dim])))
    if len(first) == 0:
        return S, mean, count, first, voxel_of
    members = np.flatnonzero(voxel_of != GONE)
    order = members[np.argsort(voxel_of[members], kind="stable")]  # by (voxel, index)
    start = np.concatenate([[0], np.cumsum(count.astype(np.int64))])
    with np.errstate(over="ignore", invalid="ignore"):
        one = np.flatnonzero(count == 1)  # the fold of one value is the value
        d = p[order[start[one]]] - mean[one]
        for k, (a, b) in enumerate(PAIRS[dim]):
            S[one, k] = d[:, a] * d[:, b]
        group = np.flatnonzero((count >= 2) & (count <= 256))
        for lo in range(0, len(group), 4096):
            g = group[lo:lo + 4096]
            col = np.arange(256)[None, :]
            inside = col < count[g][:, None]
            src = order[np.minimum(start[g][:, None] + col, len(order) - 1)]
            d = [p[src, a] - mean[g, a][:, None] for a in range(dim)]
            for k, (a, b) in enumerate(PAIRS[dim]):
                S[g, k] = _fold_rows(np.where(inside, d[a] * d[b], 0.0))
        for r in np.flatnonzero(count > 256):
            idx = order[start[r]:start[r + 1]]
            d = p[idx] - mean[r]
            for k, (a, b) in enumerate(PAIRS[dim]):
                S[r, k] = fold(d[:, a] * d[:, b])
    return S, mean, count, first, voxel_of


def divided(S, count, ddof):
    """cov = S / (c - ddof), +0.0 in every entry of a voxel with c <= ddof"""
    c = count.astype(np.int64) - ddof
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return np.where((c > 0)[:, None], S / np.maximum(c, 1).astype(np.float64)[:, None], 0.0)


def covariances_of(p, v, ddof):
    """the rule of section 26 in numpy: (cov, mean, count, first_index, voxel_of), cov packed (xx, xy, yy / xx, xy, xz,
    yy, yz, zz)"""
    S, mean, count, first, voxel_of = moments_of(p, v)
    return divided(S, count, ddof), mean, count, first, voxel_of


def covariances_by_dict(p, v, ddof):
    """the same rule as a plain loop over the members of every cell: centroids_by_dict's voxels and means, then per pair
    of axes the fold of the products of the deviations, divided once"""
    p = np.asarray(p, dtype=np.float64)
    mean, count, first, voxel_of = centroids_by_dict(p, v)
    pairs = PAIRS[p.shape[1]]
    cov = np.zeros((len(count), len(pairs)))
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(len(count)):
            idx = np.flatnonzero(voxel_of == r)
            if len(idx) <= ddof:
                continue
            for k, (a, b) in enumerate(pairs):
                prod = [(p[i, a] - mean[r, a]) * (p[i, b] - mean[r, b]) for i in idx]
                cov[r, k] = fold(prod) / np.float64(len(idx) - ddof)
    return cov, mean, count, first, voxel_of


def same_bits_but_nans(a, b):
    """equal byte for byte, except that a NaN matches any NaN (host and device differ in the default NaN's sign bit)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def test_the_restatement_agrees_with_the_dict_loop():
    rng = np.random.default_rng(3)
    for dim in (2, 3):
        crowded = rng.uniform(0.0, 1.0, (900, dim)) * np.where(rng.random((900, 1)) < 0.7, 0.2, 3.0)  # voxels above 256
        for p, v in ((rng.normal(size=(2000, dim)) * 2.0, 0.5), (boundary_input(dim), 0.1), (special_input(dim), 0.1),
                     (special_input(dim), 1e-3), (special_input(dim), 1e300), (rng.integers(-3, 3, (500, dim)) * 0.25, 0.25),
                     (crowded, 0.25)):
            for ddof in (0, 1):
                got, want = covariances_of(p, v, ddof), covariances_by_dict(p, v, ddof)
                assert same_bits_but_nans(got[0], want[0]), (dim, v, ddof)
                assert got[1].tobytes() == want[1].tobytes()
                for g, w in zip(got[2:], want[2:]):
                    assert np.array_equal(g, w), (dim, v)
                assert got[0].shape == (len(want[2]), len(PAIRS[dim])) and 0 < len(want[2]) < len(p)
        assert covariances_of(crowded, 0.25, 1)[2].max() > 256


def _levels(c):
    levels = 0
    while c > 1:
        levels, c = levels + 1, -(-c // 256)
    return levels


def test_the_restatement_is_as_accurate_as_its_tree_allows_and_one_pass_is_not():
    """against exact rational arithmetic on the deviations from the rule's own mean (so the mean's error does not
    enter).  The bound is derived: a product d_a d_b carries three roundings (the two subtractions and the
    multiplication), then passes 8 additions per level of the tree (s = 128 .. 1) over L = ceil(log256 c) levels, and
    the division adds one more, each with a relative error of at most u = 2^-53:
      |cov - exact| <= ((1 + u)^(8 L + 4) - 1) sum|d_a d_b| / (c - ddof) <= (8 L + 4) u 1.01 sum|d_a d_b| / (c - ddof)
    with d exact here.  The clouds lie about 1e6 from the origin in voxels of 0.1: there the one-pass statement
    fold(x_a x_b) / c - m_a m_b, rescaled by c / (c - ddof), has lost every digit, and is asserted to miss the bound."""
    rng = np.random.default_rng(12)
    u = 2.0 ** -53
    v = 0.1
    at3 = np.array([[1e6, -1e6, 2e6]])
    clouds = [(rng.normal(size=(3000, 3)) * 0.12 + at3, 12),                  # many voxels of a few members
              (rng.uniform(0.005, 0.095, (2500, 3)) + at3, 2),                # one voxel, two levels
              (rng.uniform(0.005, 0.095, (65_700, 2)) + at3[:, :2], 1)]       # one voxel, three levels
    K = 1 << 200  # every coordinate and mean here is an integer multiple of 1 / K

    def scaled(x):
        num, den = float(x).as_integer_ratio()
        assert K % den == 0
        return num * (K // den)

    seen = set()
    for p, most in clouds:
        dim = p.shape[1]
        S, mean, count, first, voxel_of = moments_of(p, v)
        misses = 0
        for r in np.argsort(count, kind="stable")[::-1][:most]:
            idx = np.flatnonzero(voxel_of == r)
            c = len(idx)
            assert c == count[r] and c > 1
            seen.add(_levels(c))
            d = [[scaled(p[i, a]) - scaled(mean[r, a]) for i in idx] for a in range(dim)]  # exact, in units of 1 / K
            for k, (a, b) in enumerate(PAIRS[dim]):
                prods = [x * y for x, y in zip(d[a], d[b])]
                total, size = Fraction(sum(prods), K * K), Fraction(sum(abs(t) for t in prods), K * K)
                for ddof in (0, 1):
                    exact = total / (c - ddof)
                    bound = (8 * _levels(c) + 4) * Fraction(u) * Fraction(101, 100) * size / (c - ddof)
                    got = divided(S[r:r + 1], count[r:r + 1], ddof)[0, k]
                    assert abs(Fraction(float(got)) - exact) <= bound, (c, ddof, k, got, float(exact), float(bound))
                    assert a != b or got >= 0.0
                    with np.errstate(over="ignore"):
                        one_pass = (fold(p[idx, a] * p[idx, b]) / np.float64(c) - mean[r, a] * mean[r, b]) * c / (c - ddof)
                    misses += abs(Fraction(float(one_pass)) - exact) > bound
        assert misses > 0, "the one-pass formula is expected to fail this bound at this offset"
    assert {1, 2, 3} <= seen  # voxels of one, two and three levels of the tree


def test_a_lone_point_and_a_voxel_of_no_more_than_ddof_members_give_positive_zeros():
    p = np.array([[-0.0, 0.25, -7.5], [5.0, 5.0, 5.0], [5.25, 5.5, 5.75]])
    for dim in (2, 3):
        for ddof in (0, 1):
            cov, mean, count, _, _ = covariances_of(p[:, :dim], 1.0, ddof)
            assert np.array_equal(count, [1, 2])
            assert not cov[0].any() and not np.signbit(cov[0]).any()  # +0.0 in every entry, for either ddof
            want = np.array([0.125 ** 2, 0.125 * 0.25, 0.125 * 0.375, 0.25 ** 2, 0.25 * 0.375, 0.375 ** 2])
            keep = [k for k, (a, b) in enumerate(PAIRS[3]) if a < dim and b < dim]
            assert np.array_equal(cov[1], 2.0 * want[keep] / (2 - ddof))  # (exact: powers of two throughout)
            assert np.signbit(mean[0, 0])  # the lone point's bytes, as section 25 has them


def test_overflowing_products_give_infinities_and_nans_only_off_the_diagonal():
    big = 2e200
    p = np.array([[0.0, 0.0, 1.0], [big, big, 1.0], [big, 0.0, 1.0], [0.0, big, 1.0]])
    for dim in (2, 3):
        for ddof in (0, 1):
            cov, mean, count, _, _ = covariances_of(p[:, :dim], 1e300, ddof)
            assert np.array_equal(count, [4]) and mean[0, 0] == 1e200
            packed = dict(zip(PAIRS[dim], cov[0]))
            assert packed[(0, 0)] == np.inf and packed[(1, 1)] == np.inf  # sums of squares: never a NaN
            assert np.isnan(packed[(0, 1)])  # +inf, +inf, -inf, -inf
            if dim == 3:
                assert packed[(0, 2)] == 0.0 and packed[(2, 2)] == 0.0
            got, want = covariances_of(p[:, :dim], 1e300, ddof), covariances_by_dict(p[:, :dim], 1e300, ddof)
            assert same_bits_but_nans(got[0], want[0])
    # a mean that overflowed: infinite deviations on that axis, a diagonal of +inf
    q = np.full((3, 2), 0.5)
    q[:, 0], q[:, 1] = [1e308, 1e308, 1e308], [0.25, 0.5, 0.75]
    cov, mean, _, _, _ = covariances_of(q, 1e300, 1)
    assert mean[0, 0] == np.inf and cov[0, 0] == np.inf and cov[0, 2] == 0.0625
    assert np.isnan(cov[0, 1])  # -inf * -0.25, -inf * 0.0, -inf * 0.25
    for dim in (2, 3):  # the inputs of section 22's tests: a diagonal entry is never negative and never a NaN
        for p, v in ((special_input(dim), 0.1), (special_input(dim), 1e300), (boundary_input(dim), 0.1)):
            cov = covariances_of(p, v, 0)[0]
            diag = [k for k, (a, b) in enumerate(PAIRS[dim]) if a == b]
            assert (cov[:, diag] >= 0.0).all()


# ----------------------------------------------------------------------------------- the ABI ----
def test_covariance_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in public and s not in debug, s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8
    makefile = open(os.path.join(ROOT, "icp_rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bvoxel_cov\.hip\b", makefile, flags=re.M)
    assert re.search(r"^HDRS\s*:=.*\bvoxel_fold_device\.hpp\b", makefile, flags=re.M)
    assert callable(I.voxel_covariances)


def _covariances(entry, dim, pts, n, v, ddof, voxels, outs=(None, None, None, None, None), device=-1):
    f = getattr(I.lib(), entry)
    p = C.c_void_p(pts.ctypes.data) if pts is not None else None
    k = C.byref(voxels) if voxels is not None else None
    o = [C.c_void_p(a.ctypes.data) if a is not None else None for a in outs]
    if entry == "icp_voxel_covariances":
        return f(dim, p, n, v, ddof, o[0], o[1], o[2], o[3], o[4], k, device)
    return f(dim, p, n, v, ddof, o[0], o[1], o[2], o[3], o[4], k, device, None)


@pytest.mark.parametrize("entry", NEW)
def test_covariance_argument_errors_are_rejected_before_the_device_is_used(entry):
    pts = np.zeros((4, 3))
    voxels = C.c_size_t(7)
    cov, mean = np.full((4, 6), 9.0), np.full((4, 3), 9.0)
    words = [np.full(4, 9, dtype=np.uint32) for _ in range(3)]
    outs = (cov, mean, *words)  # (host arrays: a refused call must not write them, and never reads them as device memory)
    for dim in (1, 4, 0, -2):
        assert _covariances(entry, dim, pts, 4, 0.5, 1, voxels, outs) == _lib.BAD_ARGUMENT, dim
    for v in BAD_SIZES + (float("-inf"), 2e-308):
        assert _covariances(entry, 3, pts, 4, v, 1, voxels, outs) == _lib.BAD_ARGUMENT, v
    for ddof in (-1, 2, 3, 1 << 16):
        assert _covariances(entry, 3, pts, 4, 0.5, ddof, voxels, outs) == _lib.BAD_ARGUMENT, ddof
    assert _covariances(entry, 3, pts, 4, 0.5, 1, None, outs) == _lib.BAD_ARGUMENT
    assert _covariances(entry, 3, None, 4, 0.5, 1, voxels, outs) == _lib.BAD_ARGUMENT
    assert _covariances(entry, 3, pts, 4, 0.5, 1, voxels, (None,) + outs[1:]) == _lib.BAD_ARGUMENT  # cov is required
    assert _covariances(entry, 3, pts, 4, 0.5, 1, voxels) == _lib.BAD_ARGUMENT
    assert _covariances(entry, 3, pts, 0, 0.5, 1, voxels) == _lib.BAD_ARGUMENT  # ... for n == 0 as well
    assert _covariances(entry, 3, pts, 0xFFFFFFFF, 0.5, 1, voxels, outs) == _lib.BAD_ARGUMENT
    # more than 2^27 points: the limit of the sort underneath, whatever else is asked for (cov always needs the sort)
    for asked in (outs, (cov, None, None, None, None), (cov, None, None, words[1], words[2])):
        assert _covariances(entry, 3, pts, (1 << 27) + 1, 0.5, 0, voxels, asked) == _lib.BAD_ARGUMENT
    assert _covariances(entry, 3, pts, 4, 0.5, 1, voxels, outs, device=-2) == _lib.BAD_ARGUMENT
    assert voxels.value == 7 and np.all(cov == 9.0) and np.all(mean == 9.0) and all(np.all(w == 9) for w in words)
    if I.lib().icp_device_count() == 0:
        # valid arguments reach the device check only now; DBL_MIN and DBL_MAX are valid sizes, and so is n == 0
        for dim, v, n, ddof in ((2, 0.5, 4, 0), (3, 2.2250738585072014e-308, 4, 1), (3, 1.7976931348623157e308, 4, 0),
                                (3, 0.5, 0, 1)):
            assert _covariances(entry, dim, pts, n, v, ddof, voxels, outs) == _lib.NO_DEVICE, (dim, v, n)
        assert _covariances(entry, 3, pts, 1 << 27, 0.5, 1, voxels, (cov, None, None, None, None)) == _lib.NO_DEVICE
        assert voxels.value == 0 and np.all(cov == 9.0)  # (a valid call: *voxels is cleared; no output without a device)


def test_python_refuses_a_bad_size_shape_or_ddof_before_any_device_use():
    for v in BAD_SIZES + (-1e-9,):
        with pytest.raises(ValueError):
            I.voxel_covariances(np.zeros((4, 3)), v)
    for shape in ((4,), (4, 1), (4, 4), (2, 2, 3)):
        with pytest.raises(ValueError):
            I.voxel_covariances(np.zeros(shape), 0.5, return_counts=True)
    for ddof in (-1, 2, 0.5, None, True, "1"):
        with pytest.raises(ValueError):
            I.voxel_covariances(np.zeros((4, 3)), 0.5, ddof=ddof)


def test_python_refuses_device_tensors_the_kernels_would_misread():
    class FakeTensor:
        is_cuda = True

        def __init__(self, shape, dtype="torch.float64", contiguous=True):
            self.shape, self.dtype, self._c = shape, dtype, contiguous

        def data_ptr(self):
            raise AssertionError("a refused tensor is never read")

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._c

    pytest.importorskip("torch")
    for t in (FakeTensor((8, 3), dtype="torch.float32"), FakeTensor((8, 3), contiguous=False), FakeTensor((8, 4)),
              FakeTensor((8,))):
        with pytest.raises(ValueError):
            I.voxel_covariances(t, 0.5)
    with pytest.raises(ValueError):
        I.voxel_covariances(FakeTensor((8, 3)), float("nan"))
    with pytest.raises(ValueError):
        I.voxel_covariances(FakeTensor((8, 3)), 0.5, ddof=2)


def test_the_mirroring_is_a_copy_of_the_packed_values():
    from icp_rust_amd.api import _mirrored

    for dim in (2, 3):
        packed = np.arange(1.0, 1.0 + 2 * len(PAIRS[dim])).reshape(2, -1)
        packed[1, 1] = np.nan
        full = _mirrored(packed, dim, np)
        assert full.shape == (2, dim, dim) and full.flags.c_contiguous
        for k, (a, b) in enumerate(PAIRS[dim]):
            assert full[:, a, b].tobytes() == packed[:, k].tobytes() == full[:, b, a].tobytes()


# ------------------------------------------------------------------------- kernel resources ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_covariance_kernels_do_not_spill_and_leave_room_for_four_waves_per_simd():
    """no scratch and at most 128 VGPRs (512 per lane of a SIMD: four waves) in every kernel of voxel_cov.hip -- the
    bound tests/test_voxel_mean_abi.py puts on the centroid kernels; the names stay clear of the budgeted search /
    evaluation kernels (tests/test_registers.py)"""
    from test_registers import BUDGET

    regs = _usage("voxel_cov.hip")
    kernels = [k for k in regs if not k.endswith("#scratch")]
    for frag in ("k_vc_foldILi2E", "k_vc_foldILi3E", "k_vc_itemsILi2E", "k_vc_itemsILi3E", "k_vc_topILi2E", "k_vc_topILi3E"):
        assert len([k for k in kernels if frag in k]) == 1, (frag, kernels)
    assert len(kernels) == 6, kernels
    for k in kernels:
        assert regs.get(k + "#scratch", 0) == 0, (k, regs.get(k + "#scratch"))
        assert regs[k] <= 128, (k, regs[k])
        assert not any(frag in k for frag in BUDGET), k
