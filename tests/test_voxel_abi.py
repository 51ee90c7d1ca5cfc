"""CPU-side checks of voxel thinning (icp_voxel_downsample[_device], icp_thin_targets, icp_multi_thin_targets,
icp_grid_thin_counters: include/icp_mi355x.h section 22): declared, exported and bound; ABI version still 8; every
argument error rejected before the device is touched; valid arguments answer ICP_NO_DEVICE on a host without one; the
Python refusals; run_scan_to_map thins right after the append and only when asked; the numpy restatement of the rule
against a dict-based loop; the kernels' register and scratch use (hipcc cross-compiles without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib
from test_crop_abi import HIPCC, ROOT, _Handle, _usage, declared

NEW = ("icp_voxel_downsample", "icp_voxel_downsample_device", "icp_thin_targets", "icp_multi_thin_targets",
       "icp_grid_thin_counters")
BAD_SIZES = (float("nan"), 0.0, -1.0, 5e-324, float("inf"))


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


# ------------------------------------------------------------------------ the rule, restated ----
def kept_index_of(p, v):
    """the rule of section 22 in numpy (the arbiter of every test of the feature): the lowest index of every voxel,
    ascending; a point with a NaN or infinite coordinate is in no voxel"""
    p = np.asarray(p, dtype=np.float64)
    if len(p) == 0:
        return np.zeros(0, dtype=np.int64)
    ok = np.isfinite(p).all(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.floor(p / np.float64(v)) + 0.0
    _, first = np.unique(c[ok], axis=0, return_index=True)
    return np.sort(np.flatnonzero(ok)[first])


def keep_mask(p, v):
    mask = np.zeros(len(p), dtype=bool)
    mask[kept_index_of(p, v)] = True
    return mask


def kept_index_by_dict(p, v):
    """the same rule as a plain loop: a dict from the tuple of cell coordinates to the first index seen (-0.0 and 0.0
    are equal as dict keys, as they are as doubles)"""
    seen, out = {}, []
    for i, row in enumerate(np.asarray(p, dtype=np.float64)):
        if not np.isfinite(row).all():
            continue
        with np.errstate(over="ignore"):
            cell = tuple(float(np.floor(x / np.float64(v))) for x in row)
        if cell not in seen:
            seen[cell] = i
            out.append(i)
    return np.array(out, dtype=np.int64)


def boundary_input(dim):
    """k * 0.1 for k in [-1000, 1000): at v = 0.1 the quotient's floor differs from k, and from the floor of the product
    with 1 / v, for many of them (neighbours then share a voxel); the other coordinates are constant"""
    k = np.arange(-1000, 1000)
    p = np.zeros((2000, dim))
    p[:, 0] = k * 0.1
    p[:, 1:] = 0.05
    return p


def special_input(dim):
    """+-0.0, subnormals, NaN and infinite rows, 1e308, repeated cells on both sides of zero"""
    x = np.array([0.0, -0.0, -1e-320, 1e-320, 0.05, -0.05, np.nan, np.inf, -np.inf, 1e308, -1e308, 1e308, 0.1, 0.1,
                  0.30000000000000004, 0.3, -0.0, 0.0, 7.0, 7.0999])
    p = np.zeros((len(x), dim))
    p[:, 0] = x
    p[:, dim - 1] = np.roll(x, 7) if dim > 1 else x
    return p


def test_the_restatement_agrees_with_the_dict_loop():
    rng = np.random.default_rng(3)
    for dim in (2, 3):
        for p, v in ((rng.normal(size=(3000, dim)) * 2.0, 0.5), (boundary_input(dim), 0.1), (special_input(dim), 0.1),
                     (special_input(dim), 1e-3), (special_input(dim), 1e300), (rng.integers(-3, 3, (500, dim)) * 0.25, 0.25)):
            want = kept_index_by_dict(p, v)
            assert np.array_equal(kept_index_of(p, v), want), (dim, v)
            assert 0 < len(want) < len(p)


def test_the_boundary_input_tells_a_division_from_a_product_with_the_reciprocal():
    k = np.arange(-1000, 1000)
    x, v = k * 0.1, np.float64(0.1)
    assert np.count_nonzero(np.floor(x / v) != k) == 149
    assert np.count_nonzero(np.floor(x / v) != np.floor(x * (1.0 / v))) == 195
    by_product = np.unique(np.floor(boundary_input(2) * (1.0 / v)), axis=0, return_index=True)[1]
    assert not np.array_equal(np.sort(by_product), kept_index_of(boundary_input(2), 0.1))


# ----------------------------------------------------------------------------------- the ABI ----
def test_voxel_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    for s in NEW[:4]:
        assert s in public, s
    assert "icp_grid_thin_counters" in debug and "icp_grid_thin_counters" not in public
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    makefile = open(os.path.join(ROOT, "icp_rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bvoxel\.hip\b", makefile, flags=re.M)
    for cls in (I.Icp2d, I.Icp3d):
        assert callable(cls.thin) and callable(cls.thin_counters)
    assert callable(I.IcpMulti.thin) and callable(I.voxel_downsample)


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def _downsample(entry, dim, pts, n, v, kept):
    f = getattr(I.lib(), entry)
    p = C.c_void_p(pts.ctypes.data) if pts is not None else None
    k = C.byref(kept) if kept is not None else None
    return f(dim, p, n, v, None, None, k, -1) if entry == "icp_voxel_downsample" else f(dim, p, n, v, None, None, k, -1, None)


@pytest.mark.parametrize("entry", ["icp_voxel_downsample", "icp_voxel_downsample_device"])
def test_downsample_argument_errors_are_rejected_before_the_device_is_used(entry):
    pts = np.zeros((4, 3))
    kept = C.c_size_t(7)
    for dim in (1, 4, 0, -2):
        assert _downsample(entry, dim, pts, 4, 0.5, kept) == _lib.BAD_ARGUMENT, dim
    for v in BAD_SIZES + (float("-inf"), 2e-308):
        assert _downsample(entry, 3, pts, 4, v, kept) == _lib.BAD_ARGUMENT, v
    assert _downsample(entry, 3, pts, 4, 0.5, None) == _lib.BAD_ARGUMENT
    assert _downsample(entry, 3, None, 4, 0.5, kept) == _lib.BAD_ARGUMENT
    assert _downsample(entry, 3, pts, 0xFFFFFFFF, 0.5, kept) == _lib.BAD_ARGUMENT  # (n above 2^32 - 2: decided on n alone)
    assert kept.value == 7  # a refused call writes nothing
    if I.lib().icp_device_count() == 0:
        # valid arguments reach the device check only now; DBL_MIN and DBL_MAX are valid sizes, and so is n == 0
        for dim, v, n in ((2, 0.5, 4), (3, 2.2250738585072014e-308, 4), (3, 1.7976931348623157e308, 4), (3, 0.5, 0)):
            assert _downsample(entry, dim, pts, n, v, kept) == _lib.NO_DEVICE, (dim, v, n)


@pytest.mark.parametrize("entry", ["icp_thin_targets", "icp_multi_thin_targets"])
def test_thin_argument_errors_are_rejected_before_the_device_is_used(entry):
    f = getattr(I.lib(), entry)
    removed = C.c_size_t(7)
    multi = entry == "icp_multi_thin_targets"

    def call(h, v):
        return f(h, v, C.byref(removed)) if multi else f(h, v, None, C.byref(removed))

    H = _Handle()
    try:
        for v in BAD_SIZES + (float("-inf"), -1e-300, 2e-308):
            assert call(H.h, v) == _lib.BAD_ARGUMENT, v
        assert call(None, 0.5) == _lib.BAD_ARGUMENT
        assert removed.value == 7
        if not H.real and not multi:
            for v in (0.5, 2.2250738585072014e-308, 1.7976931348623157e308):
                assert call(H.h, v) == _lib.NO_DEVICE, v
    finally:
        H.close()


def test_counters_refuse_null():
    out = (C.c_uint64 * 2)()
    assert I.lib().icp_grid_thin_counters(None, out) == _lib.BAD_ARGUMENT


def test_python_refuses_a_bad_voxel_size_before_any_handle_is_reached():
    for cls in (I.Icp2d, I.Icp3d):
        icp = object.__new__(cls)  # (no handle is reached: the size is checked first)
        icp._h = C.c_void_p()
        for v in BAD_SIZES + (-1e-9,):
            with pytest.raises(ValueError):
                icp.thin(v)
    multi = object.__new__(I.IcpMulti)
    multi._h = C.c_void_p()
    for v in BAD_SIZES:
        with pytest.raises(ValueError):
            multi.thin(v)
        with pytest.raises(ValueError):
            I.voxel_downsample(np.zeros((4, 3)), v)
    for shape in ((4,), (4, 1), (4, 4), (2, 2, 3)):
        with pytest.raises(ValueError):
            I.voxel_downsample(np.zeros(shape), 0.5)


def test_python_refuses_device_tensors_the_kernels_would_misread():
    """what _dev_points refuses, on tensors that only claim to live on a GPU (no device is needed to refuse them)"""

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
            I.voxel_downsample(t, 0.5)


# ------------------------------------------------------------------------------- the harness ----
def test_scan_to_map_thins_right_after_the_append_and_only_when_asked(monkeypatch):
    from icp_rust_amd import harness, synth

    log = []

    class Fake:
        def __init__(self, dst):
            log.append(("create", len(dst)))

        def estimate(self, src, T, max_iter, **kw):
            log.append(("estimate", len(src)))
            return I.Transform([0.25, -0.5, 0.01])

        def estimate_point_to_plane(self, src, T, max_iter):
            return self.estimate(src, T, max_iter)

        def compute_normals(self, k):
            log.append(("compute_normals", k))

        def update_normals(self, k):
            log.append(("update_normals", k))

        def append(self, pts, T):
            log.append(("append", len(pts)))

        def crop(self, center, radius):
            log.append(("crop", radius))

        def thin(self, v):
            log.append(("thin", v))

    class NoThin(Fake):
        thin = None  # (a factory without a usable thin method keeps working when no size is given)

    def fail(*a, **k):
        raise AssertionError("voxel_downsample is called only with scan_voxel")

    packets = synth.synthetic_scan3d_packets(4 * synth.PACKETS_PER_FRAME)
    monkeypatch.setattr(harness, "voxel_downsample", fail)
    harness.run_scan_to_map(packets, icp_factory=NoThin, max_iter=2, map_radius=3.0)
    assert [e[0] for e in log] == ["create"] + ["estimate", "append", "crop"] * 3
    full = [e[1] for e in log if e[0] in ("create", "append")]
    del log[:]
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, point_to_plane=8, map_radius=3.0, map_voxel=0.125)
    assert [e[0] for e in log] == ["create", "compute_normals"] + ["estimate", "append", "thin", "update_normals", "crop"] * 3
    assert [e[1] for e in log if e[0] == "thin"] == [0.125] * 3
    del log[:]
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, map_voxel=0.5)
    assert [e[0] for e in log] == ["create"] + ["estimate", "append", "thin"] * 3
    del log[:]
    # scan_voxel: every frame, frame 0 included, goes through voxel_downsample before anything else sees it
    seen = []

    def thinned(scan, v):
        seen.append((len(scan), v))
        return scan[kept_index_of(scan, v)]

    monkeypatch.setattr(harness, "voxel_downsample", thinned)
    harness.run_scan_to_map(packets, icp_factory=NoThin, max_iter=2, scan_voxel=0.25)
    assert [e[0] for e in log] == ["create"] + ["estimate", "append"] * 3
    assert seen == [(n, 0.25) for n in full]
    sizes = [e[1] for e in log]
    assert sizes[0] < full[0] and sizes[1] == sizes[2] < full[1]  # the estimate and the append see the thinned scan


# ------------------------------------------------------------------------- kernel resources ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_voxel_kernels_do_not_spill_and_leave_room_for_four_waves_per_simd():
    """no scratch and at most 128 VGPRs (512 per lane of a SIMD: four waves) in every kernel of voxel.hip; the names stay
    clear of the budgeted search / evaluation kernels (tests/test_registers.py)"""
    from test_registers import BUDGET

    regs = _usage("voxel.hip")
    kernels = [k for k in regs if not k.endswith("#scratch")]
    for frag in ("k_voxel_insertILi2E", "k_voxel_insertILi3E", "k_voxel_markILi2E", "k_voxel_markILi3E",
                 "k_voxel_placeILi2E", "k_voxel_placeILi3E", "k_compact_chunks"):
        assert len([k for k in kernels if frag in k]) == 1, (frag, kernels)
    for k in kernels:
        assert regs.get(k + "#scratch", 0) == 0, (k, regs.get(k + "#scratch"))
        assert regs[k] <= 128, (k, regs[k])
        assert not any(frag in k for frag in BUDGET), k
