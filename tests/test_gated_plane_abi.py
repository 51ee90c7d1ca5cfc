"""CPU-side checks of the gated point-to-plane registration (icp_estimate_point_to_plane_gated*,
icp_gate_plane_pairs_device, icp_multi_estimate_point_to_plane_gated: include/icp_mi355x.h section 12): declared,
exported and bound; ABI version still 8; every argument error rejected before the device is touched and before the
handle is read; valid arguments answer ICP_NO_DEVICE on a host without one; the gate kernels' register and scratch use
(hipcc cross-compiles without a GPU); the Python keyword refuses a negative bound."""
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
ESTIMATES = ("icp_estimate_point_to_plane_gated", "icp_estimate_point_to_plane_gated_device",
             "icp_multi_estimate_point_to_plane_gated")
NEW = ESTIMATES + ("icp_gate_plane_pairs_device",)
TOO_MANY = 0xffffffff  # n >= 2^32 - 1


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", text))


def test_gated_plane_symbols_are_declared_exported_and_bound():
    public = declared("icp_mi355x.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in public and s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    srcs = open(os.path.join(ROOT, "icp_rust_amd", "csrc", "Makefile")).read()
    assert "gate_plane.hip" in srcs.split("SRCS")[1].split("\n")[0]
    assert "p2plane_device.hpp" in srcs.split("HDRS")[1].split("\n")[0]


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def _identity():
    T = _lib.Pose()
    I.lib().icp_transform_identity(C.byref(T))
    return T


class _Handle:
    """A real 3-D handle with current normals where there is a device; on a host without one no handle can exist
    (icp_create answers ICP_NO_DEVICE), so the entries are given a block of zeroed memory in its place: they must decide
    on their arguments, and then on the device, before they read a handle."""

    def __init__(self, stand_in=False):
        self.h = C.c_void_p()
        self.real = I.lib().icp_device_count() > 0 and not stand_in
        if self.real:
            rng = np.random.default_rng(0)
            dst = np.ascontiguousarray(rng.random((64, 3)))
            assert I.lib().icp_create(C.byref(self.h), 3, C.c_void_p(dst.ctypes.data), 64, -1) == _lib.OK
            assert I.lib().icp_compute_target_normals(self.h, 8) == _lib.OK
        else:
            self.block = (C.c_char * 65536)()
            self.h = C.c_void_p(C.addressof(self.block))

    def close(self):
        if self.real:
            I.lib().icp_destroy(self.h)


@pytest.mark.parametrize("entry", ESTIMATES)
def test_estimate_argument_errors_are_rejected_before_the_device_is_used(entry):
    f = getattr(I.lib(), entry)
    multi = entry.startswith("icp_multi")
    src = np.zeros((4, 3))
    sp = C.c_void_p(src.ctypes.data)
    T, out = _identity(), _lib.Pose()
    H = _Handle(stand_in=multi)  # (an icp_handle is no icp_multi: the multi entry always gets the block, which it never reads)
    no_device = I.lib().icp_device_count() <= 0
    try:
        for r in (float("nan"), -1.0, float("-inf"), -1e-300):
            assert f(H.h, sp, 4, C.byref(T), 3, r, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT, r
        assert f(None, sp, 4, C.byref(T), 3, 1.0, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT
        assert f(H.h, sp, 4, None, 3, 1.0, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT
        assert f(H.h, sp, 4, C.byref(T), 3, 1.0, None, None, None, None) == _lib.BAD_ARGUMENT
        assert f(H.h, None, 4, C.byref(T), 3, 1.0, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT
        assert f(H.h, sp, TOO_MANY, C.byref(T), 3, 1.0, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT
        if no_device:  # valid arguments reach the device check only now; 0 and +inf are valid bounds
            for r in (0.0, 1.0, float("inf")):
                assert f(H.h, sp, 4, C.byref(T), 3, r, C.byref(out), None, None, None) == _lib.NO_DEVICE, r
    finally:
        H.close()


def test_stage_call_argument_errors_are_rejected_before_the_device_is_used():
    f = I.lib().icp_gate_plane_pairs_device
    T = _identity()
    kept = C.c_size_t(7)
    p = C.c_void_p(np.zeros(64).ctypes.data)  # (never dereferenced: every call below is refused)
    H = _Handle()
    try:
        for r in (float("nan"), -1.0, float("-inf")):
            assert f(H.h, p, 4, C.byref(T), p, r, p, None, C.byref(kept)) == _lib.BAD_ARGUMENT, r
        assert f(None, p, 4, C.byref(T), p, 1.0, p, None, C.byref(kept)) == _lib.BAD_ARGUMENT
        assert f(H.h, p, 4, None, p, 1.0, p, None, C.byref(kept)) == _lib.BAD_ARGUMENT
        assert f(H.h, p, 4, C.byref(T), p, 1.0, p, None, None) == _lib.BAD_ARGUMENT
        assert f(H.h, p, TOO_MANY, C.byref(T), p, 1.0, p, None, C.byref(kept)) == _lib.BAD_ARGUMENT
        for bad in range(3):  # src, idx, pairs
            args = [p, p, p]
            args[bad] = None
            assert f(H.h, args[0], 4, C.byref(T), args[1], 1.0, args[2], None, C.byref(kept)) == _lib.BAD_ARGUMENT
        assert f(H.h, None, 0, C.byref(T), None, 0.0, None, None, C.byref(kept)) == _lib.OK and kept.value == 0
        if not H.real:
            for r in (0.0, 1.0, float("inf")):
                assert f(H.h, p, 4, C.byref(T), p, r, p, None, C.byref(kept)) == _lib.NO_DEVICE, r
    finally:
        H.close()


@pytest.mark.parametrize("cls", [I.Icp3d, I.IcpMulti])
def test_python_keyword_refuses_a_negative_or_nan_bound(cls):
    icp = object.__new__(cls)  # (no handle is reached: the bound is checked first)
    icp._h = C.c_void_p()
    for r in (-1, -1e-9, float("nan"), float("-inf")):
        with pytest.raises(ValueError):
            icp.estimate_point_to_plane(np.zeros((4, 3)), I.Transform(), 3, max_correspondence_distance=r)
        with pytest.raises(ValueError):
            icp.estimate_point_to_plane(np.zeros((4, 3)), I.Transform(), 3, return_info=True,
                                        max_correspondence_distance=r)


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


# (VGPRs, scratch bytes per lane) of the 3-D kernels as the build reported them while each had a body of its own, before
# csrc/normal_single_device.hpp and gate_plane.hip's normal_gate_stage put one body behind them and their 2-D twins
PLANE_KERNELS_BEFORE_SHARING = {
    "gate_plane.hip": {"k_plgate_stage": (78, 0), "k_plgate_place": (30, 0)},
    "p2plane.hip": {"k_target_normals": (72, 0), "k_p2pl_gather": (24, 0)},
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_plane_gate_kernels_do_not_spill_and_leave_room_for_four_waves_per_simd():
    """no scratch and at most 128 VGPRs (512 per lane of a SIMD: four waves) in every kernel of gate_plane.hip -- the
    stage kernels of both dimensions, the chunk sums, the one place kernel; the names stay clear of the budgeted search /
    evaluation kernels (tests/test_registers.py) and of the fragments tests/test_gated_abi.py counts gate.hip's kernels
    by; the 3-D kernels, here and in p2plane.hip, need no more than before they shared a body with their 2-D twins"""
    from test_registers import BUDGET

    regs = _usage("gate_plane.hip")
    kernels = [k for k in regs if not k.endswith("#scratch")]
    for frag in ("k_plgate_stage", "k_lngate_stage", "k_compact_chunks", "k_plgate_place"):
        assert len([k for k in kernels if frag in k]) == 1, (frag, kernels)
    assert len(kernels) == 4, kernels
    for k in kernels:
        assert regs.get(k + "#scratch", 0) == 0, (k, regs.get(k + "#scratch"))
        assert regs[k] <= 128, (k, regs[k])
        assert not any(frag in k for frag in BUDGET), k
        assert not any(frag in k for frag in ("k_gate_stage", "k_gate_chunks", "k_gate_place")), k
    for src, table in PLANE_KERNELS_BEFORE_SHARING.items():
        regs = _usage(src) if src != "gate_plane.hip" else regs
        for frag, (vgprs, scratch) in table.items():
            names = [k for k in regs if frag in k and not k.endswith("#scratch")]
            assert len(names) == 1, (frag, names)
            assert regs[names[0]] <= vgprs, f"{names[0]}: {regs[names[0]]} VGPRs > {vgprs}"
            assert regs.get(names[0] + "#scratch", 0) <= scratch, f"{names[0]}: scratch"
