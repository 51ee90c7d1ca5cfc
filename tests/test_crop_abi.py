"""CPU-side checks of the sliding-window map (icp_crop_targets, icp_multi_crop_targets, icp_grid_crop_counters:
include/icp_mi355x.h section 11): declared, exported and bound; ABI version still 8; every argument error rejected
before the device is touched; valid arguments answer ICP_NO_DEVICE on a host without one; run_scan_to_map crops once
per frame, after the append, and only when asked; the crop kernels' register and scratch use (hipcc cross-compiles
without a GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("icp_crop_targets", "icp_multi_crop_targets", "icp_grid_crop_counters")
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


def declared(*names):
    out = set()
    for name in names:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        out |= set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", text))
    return out


def test_crop_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    assert "icp_crop_targets" in public and "icp_multi_crop_targets" in public
    assert "icp_grid_crop_counters" in debug and "icp_grid_crop_counters" not in public
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    assert "crop.hip" in open(os.path.join(ROOT, "icp_rust_amd", "csrc", "Makefile")).read()
    for cls in (I.Icp2d, I.Icp3d):
        assert callable(cls.crop) and callable(cls.crop_counters)
    assert callable(I.IcpMulti.crop)


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


class _Handle:
    """A real handle where there is a device; on a host without one no handle can exist (icp_create answers
    ICP_NO_DEVICE), so the entries are given a block of zeroed memory in its place: they must decide on their
    arguments, and then on the device, before they read a handle."""

    def __init__(self):
        self.h = C.c_void_p()
        self.real = I.lib().icp_device_count() > 0
        if self.real:
            dst = np.zeros((4, 2))
            assert I.lib().icp_create(C.byref(self.h), 2, C.c_void_p(dst.ctypes.data), 4, -1) == _lib.OK
        else:
            self.block = (C.c_char * 65536)()
            self.h = C.c_void_p(C.addressof(self.block))

    def close(self):
        if self.real:
            I.lib().icp_destroy(self.h)


def _xy(x, y):
    a = np.array([x, y], dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


@pytest.mark.parametrize("entry", ["icp_crop_targets", "icp_multi_crop_targets"])
def test_argument_errors_are_rejected_before_the_device_is_used(entry):
    f = getattr(I.lib(), entry)
    removed = C.c_size_t(7)
    multi = entry == "icp_multi_crop_targets"

    def call(h, c, r):
        return f(h, c, r, C.byref(removed)) if multi else f(h, c, r, None, C.byref(removed))

    H = _Handle()
    try:
        keep, c = _xy(1.0, -2.0)
        nan = float("nan")
        for r in (nan, -1.0, float("-inf"), -1e-300):
            assert call(H.h, c, r) == _lib.BAD_ARGUMENT, r
        for x, y in ((nan, 0.0), (0.0, nan), (nan, nan)):
            keep2, c2 = _xy(x, y)
            assert call(H.h, c2, 1.0) == _lib.BAD_ARGUMENT, (x, y)
        assert call(None, c, 1.0) == _lib.BAD_ARGUMENT
        assert call(H.h, None, 1.0) == _lib.BAD_ARGUMENT
        if not H.real and not multi:  # valid arguments reach the device check only now; 0 and +inf are valid radii
            for r in (0.0, 1.0, float("inf")):
                assert call(H.h, c, r) == _lib.NO_DEVICE, r
    finally:
        H.close()


def test_counters_refuse_null():
    out = (C.c_uint64 * 2)()
    assert I.lib().icp_grid_crop_counters(None, out) == _lib.BAD_ARGUMENT


def test_python_crop_refuses_a_negative_or_nan_radius_and_a_nan_centre():
    icp = object.__new__(I.Icp2d)  # (no handle is reached: the arguments are checked first)
    icp._h = C.c_void_p()
    for r in (-1, -1e-9, float("nan"), float("-inf")):
        with pytest.raises(ValueError):
            icp.crop([0.0, 0.0], r)
    with pytest.raises(ValueError):
        icp.crop([float("nan"), 0.0], 1.0)
    with pytest.raises(ValueError):
        icp.crop([0.0, 0.0, 0.0], 1.0)


def test_scan_to_map_crops_once_per_frame_after_the_append_and_only_when_asked():
    from icp_rust_amd import harness, synth

    log = []

    class Fake:
        def __init__(self, dst):
            pass

        def estimate(self, src, T, max_iter, **kw):
            log.append(("estimate",))
            return I.Transform([0.25 * (1 + len([e for e in log if e[0] == "estimate"])), -0.5, 0.01])

        def estimate_point_to_plane(self, src, T, max_iter):
            return self.estimate(src, T, max_iter)

        def compute_normals(self, k):
            log.append(("compute_normals", k))

        def update_normals(self, k):
            log.append(("update_normals", k))

        def append(self, pts, T):
            log.append(("append", T.t.copy()))

        def crop(self, center, radius):
            log.append(("crop", np.array(center, dtype=np.float64), radius))

    class NoCrop(Fake):
        crop = None  # (a factory without a usable crop method keeps working when no radius is given)

    packets = synth.synthetic_scan3d_packets(4 * synth.PACKETS_PER_FRAME)
    harness.run_scan_to_map(packets, icp_factory=NoCrop, max_iter=2)
    assert [e[0] for e in log] == ["estimate", "append"] * 3
    del log[:]
    Ts, _, _ = harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, map_radius=12.5)
    assert [e[0] for e in log] == ["estimate", "append", "crop"] * 3
    crops = [e for e in log if e[0] == "crop"]
    for T, (_, centre, radius) in zip(Ts, crops):
        assert np.array_equal(centre, T.t) and radius == 12.5
    del log[:]
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, point_to_plane=8, map_radius=3.0)
    assert [e[0] for e in log] == ["compute_normals"] + ["estimate", "append", "update_normals", "crop"] * 3
    with pytest.raises(ValueError):  # (the existing refusal stays)
        harness.run_scan_to_map(packets, icp_factory=Fake, point_to_plane=8, max_correspondence_distance=1.0,
                                map_radius=3.0)


def _usage(src):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "icp_rust_amd", "csrc", src),
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    regs, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs: (\d+)", line)
        if m and name:
            regs[name] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            regs[name + "#scratch"] = int(m.group(1))
    return regs


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_crop_kernels_do_not_spill_and_leave_room_for_four_waves_per_simd():
    """no scratch and at most 128 VGPRs (512 per lane of a SIMD: four waves) in every kernel of crop.hip; the names stay
    clear of the budgeted search / evaluation kernels (tests/test_registers.py)"""
    from test_registers import BUDGET

    regs = _usage("crop.hip")
    kernels = [k for k in regs if not k.endswith("#scratch")]
    for frag in ("k_crop_markILi2E", "k_crop_markILi3E", "k_compact_chunks", "k_crop_placeILi2E", "k_crop_placeILi3E",
                 "k_crop_rec_mark", "k_crop_rec_place", "k_crop_starts"):
        assert len([k for k in kernels if frag in k]) == 1, (frag, kernels)
    assert len(kernels) == 8, kernels
    for k in kernels:
        assert regs.get(k + "#scratch", 0) == 0, (k, regs.get(k + "#scratch"))
        assert regs[k] <= 128, (k, regs[k])
        assert not any(frag in k for frag in BUDGET), k
