"""CPU-side checks of the batch call (icp_batch_*, include/icp_mi355x.h section 8): declared, exported and bound; ABI
version 8 in the header and the library; every argument error rejected before the device is touched; and the batch
kernel's register budget at the three workgroup sizes (hipcc cross-compiles without a GPU)."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("icp_batch_create", "icp_batch_destroy", "icp_batch_estimate", "icp_batch_estimate_device")


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", text))


def test_batch_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in public and s in _lib.SIGNATURES and hasattr(L, s), s
    assert "icp_batch_counters" in debug and "icp_batch_counters" not in public
    assert "icp_batch_counters" in _lib.SIGNATURES and hasattr(L, "icp_batch_counters")
    assert C.sizeof(_lib.BatchItem) == 4 * 8 + 6 * 8


def test_abi_version_is_8_in_header_and_library():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def _batch(dim=2):
    b = C.c_void_p()
    assert I.lib().icp_batch_create(C.byref(b), dim, -1) == _lib.OK  # (no device use: works without a GPU)
    return b


def _call(b, src, dst, items, max_iter=20, out=True, status=True, entry="icp_batch_estimate", count=None):
    count = len(items) if count is None else count
    arr = (_lib.BatchItem * max(len(items), 1))()
    for i, (f, n, g, m) in enumerate(items):
        arr[i].src_first, arr[i].n, arr[i].dst_first, arr[i].m = f, n, g, m
        I.lib().icp_transform_identity(C.byref(arr[i].init))
    o = (_lib.Pose * max(count, 1))() if out else None
    st = np.zeros(max(count, 1), dtype=np.int32)
    sp = C.c_void_p(src.ctypes.data) if src is not None else None
    dp = C.c_void_p(dst.ctypes.data) if dst is not None else None
    return getattr(I.lib(), entry)(b, sp, 0 if src is None else len(src), dp, 0 if dst is None else len(dst),
                                   arr if items else None, count, max_iter, o,
                                   C.c_void_p(st.ctypes.data) if status else None, None, None)


def test_bad_dim_is_refused():
    b = C.c_void_p()
    for dim in (0, 1, 4, -2):
        assert I.lib().icp_batch_create(C.byref(b), dim, -1) == _lib.BAD_ARGUMENT
    assert I.lib().icp_batch_create(None, 2, -1) == _lib.BAD_ARGUMENT


@pytest.mark.parametrize("entry", ["icp_batch_estimate", "icp_batch_estimate_device"])
def test_argument_errors_are_rejected_before_the_device_is_used(entry):
    src, dst = np.zeros((10, 2)), np.zeros((20, 2))
    b = _batch()
    try:
        bad = [
            [(0, 11, 0, 20)],                     # source range past the array
            [(5, 6, 0, 20)],
            [(0, 10, 1, 20)],                     # target range past the array
            [(0, 10, 21, 0)],                     # (an empty range that starts past the end)
            [(0, 10, 0, 20), (2**63, 2**63, 0, 1)],  # (first + n overflows)
        ]
        for items in bad:
            assert _call(b, src, dst, items, entry=entry) == _lib.BAD_ARGUMENT, items
        good = [(0, 10, 0, 20), (3, 7, 0, 0), (10, 0, 20, 0)]
        assert _call(b, src, dst, good, out=False, entry=entry) == _lib.BAD_ARGUMENT
        assert _call(b, src, dst, good, status=False, entry=entry) == _lib.BAD_ARGUMENT
        assert _call(b, src, dst, [], count=3, entry=entry) == _lib.BAD_ARGUMENT  # items NULL, count > 0
        assert getattr(I.lib(), entry)(None, None, 0, None, 0, None, 0, 20, None, None, None, None) == _lib.BAD_ARGUMENT
        # count == 0 is a successful no-op whatever the other pointers are
        assert _call(b, None, None, [], count=0, out=False, status=False, entry=entry) == _lib.OK
        if I.lib().icp_device_count() == 0:  # valid arguments reach the device check only now
            assert _call(b, src, dst, good, entry=entry) == _lib.NO_DEVICE
    finally:
        I.lib().icp_batch_destroy(b)


def test_python_batch_refuses_mismatched_lists():
    B = I.IcpBatch(2)
    with pytest.raises(ValueError):
        B.estimate([np.zeros((3, 2))], [], None, 20)
    with pytest.raises(ValueError):
        B.estimate([np.zeros((3, 2))], [np.zeros((3, 2))], [I.Transform(), I.Transform()], 20)
    with pytest.raises(ValueError):
        I.IcpBatch(4)
    assert B.estimate([], [], [], 20) == []


def _usage(src):
    import subprocess

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
def test_batch_kernel_register_and_spill_budget():
    """the batch kernel runs the single kernel's body behind a box prologue: no spill at 512 and 768 threads, and at 1024
    no more than the single kernel may (tests/test_registers.py: 96 bytes per lane for 2-D; the 3-D body spills a little
    more already in the single kernel)"""
    regs = _usage("gn_fast.hip")
    for dim, caps in ((2, {512: 0, 768: 0, 1024: 96}), (3, {512: 0, 768: 0, 1024: 112})):
        for b, cap in caps.items():
            names = [k for k in regs if "k_tiny_estimate_batchILi%dELj%dE" % (dim, b) in k and not k.endswith("#scratch")]
            assert len(names) == 1, names
            assert regs.get(names[0] + "#scratch", 0) <= cap, (names[0], regs.get(names[0] + "#scratch"))
            assert regs[names[0]] <= 512 // (b // 256), names[0]  # (a workgroup must fit a CU at all)
        # the single kernel is still there, once per size, under its own name
        for b in (512, 768, 1024):
            assert len([k for k in regs if "k_tiny_estimateILi%dELj%dE" % (dim, b) in k and not k.endswith("#scratch")]) == 1
