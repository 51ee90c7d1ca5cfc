"""CPU-side checks of pose evaluation (icp_quality, icp_evaluate*, icp_batch_evaluate*: include/icp_mi355x.h section 9):
declared, exported and bound; ABI version still 8; the struct's layout as a C compiler sees it equals the ctypes one;
every argument error rejected before the device is touched; and the new kernels' register and scratch use (hipcc
cross-compiles without a GPU)."""
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
NEW = ("icp_evaluate", "icp_evaluate_device", "icp_batch_evaluate", "icp_batch_evaluate_device")
FIELDS = ("n", "inliers", "fitness", "inlier_rmse", "inlier_sum_d2", "error", "huber_error", "information")


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", text))


def test_quality_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in public and s in _lib.SIGNATURES and hasattr(L, s), s
    c = "icp_batch_evaluate_counters"
    assert c in debug and c not in public and c in _lib.SIGNATURES and hasattr(L, c)
    assert I.Quality is I.api.Quality


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not found")
def test_quality_struct_layout_matches_the_header(tmp_path):
    """size and offsets of icp_quality as a C99 compiler lays it out (-pedantic -Werror) against the ctypes struct"""
    src = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "icp_mi355x.h"', "int main(void) {",
             '  printf("size %u\\n", (unsigned)sizeof(icp_quality));']
    lines += ['  printf("%s %%u\\n", (unsigned)offsetof(icp_quality, %s));' % (f, f) for f in FIELDS]
    lines += ["  return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=120)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True,
                                                       timeout=60).stdout.splitlines())
    S = _lib.QualityStruct
    assert int(got["size"]) == C.sizeof(S) == 2 * 8 + 5 * 8 + 9 * 8
    for f in FIELDS:
        assert int(got[f]) == getattr(S, f).offset, f


def _batch(dim=2):
    b = C.c_void_p()
    assert I.lib().icp_batch_create(C.byref(b), dim, -1) == _lib.OK  # (no device use: works without a GPU)
    return b


def _call(b, src, dst, items, r=1.0, out=True, status=True, entry="icp_batch_evaluate", count=None):
    count = len(items) if count is None else count
    arr = (_lib.BatchItem * max(len(items), 1))()
    for i, (f, n, g, m) in enumerate(items):
        arr[i].src_first, arr[i].n, arr[i].dst_first, arr[i].m = f, n, g, m
        I.lib().icp_transform_identity(C.byref(arr[i].init))
    o = (_lib.QualityStruct * max(count, 1))() if out else None
    st = np.zeros(max(count, 1), dtype=np.int32)
    sp = C.c_void_p(src.ctypes.data) if src is not None else None
    dp = C.c_void_p(dst.ctypes.data) if dst is not None else None
    return getattr(I.lib(), entry)(b, sp, 0 if src is None else len(src), dp, 0 if dst is None else len(dst),
                                   arr if items else None, count, r, o, C.c_void_p(st.ctypes.data) if status else None)


@pytest.mark.parametrize("entry", ["icp_batch_evaluate", "icp_batch_evaluate_device"])
def test_batch_argument_errors_are_rejected_before_the_device_is_used(entry):
    src, dst = np.zeros((10, 2)), np.zeros((20, 2))
    b = _batch()
    try:
        good = [(0, 10, 0, 20), (3, 7, 0, 0), (10, 0, 20, 0)]
        for items in ([(0, 11, 0, 20)], [(5, 6, 0, 20)], [(0, 10, 1, 20)], [(0, 10, 21, 0)],
                      [(0, 10, 0, 20), (2**63, 2**63, 0, 1)]):  # ranges outside their arrays
            assert _call(b, src, dst, items, entry=entry) == _lib.BAD_ARGUMENT, items
        for r in (float("nan"), -1.0, -1e-300, float("-inf")):  # a NaN or negative distance bound
            assert _call(b, src, dst, good, r=r, entry=entry) == _lib.BAD_ARGUMENT, r
            assert _call(b, None, None, [], r=r, count=0, out=False, status=False, entry=entry) == _lib.BAD_ARGUMENT, r
        assert _call(b, src, dst, good, out=False, entry=entry) == _lib.BAD_ARGUMENT  # NULL out
        assert _call(b, src, dst, good, status=False, entry=entry) == _lib.BAD_ARGUMENT  # NULL status
        assert _call(b, src, dst, [], count=3, entry=entry) == _lib.BAD_ARGUMENT  # items NULL, count > 0
        assert _call(b, None, None, [(0, 1, 0, 1)], entry=entry) == _lib.BAD_ARGUMENT  # arrays NULL, ranges past them
        assert getattr(I.lib(), entry)(None, None, 0, None, 0, None, 0, 1.0, None, None) == _lib.BAD_ARGUMENT
        # count == 0 is a successful no-op whatever the other pointers are; r = 0 and +inf are valid bounds
        for r in (0.0, float("inf")):
            assert _call(b, None, None, [], r=r, count=0, out=False, status=False, entry=entry) == _lib.OK
        if I.lib().icp_device_count() == 0:  # valid arguments reach the device check only now
            for r in (0.0, 1.0, float("inf")):
                assert _call(b, src, dst, good, r=r, entry=entry) == _lib.NO_DEVICE
    finally:
        I.lib().icp_batch_destroy(b)


def test_bad_dim_is_refused_by_the_batch():
    b = C.c_void_p()
    for dim in (0, 1, 4, -2):
        assert I.lib().icp_batch_create(C.byref(b), dim, -1) == _lib.BAD_ARGUMENT


@pytest.mark.parametrize("entry", ["icp_evaluate", "icp_evaluate_device"])
def test_single_entry_rejects_null_handle_and_out(entry):
    src = np.zeros((4, 2))
    T = _lib.Pose()
    I.lib().icp_transform_identity(C.byref(T))
    q = _lib.QualityStruct()
    f = getattr(I.lib(), entry)
    sp = C.c_void_p(src.ctypes.data)
    assert f(None, sp, 4, C.byref(T), 1.0, C.byref(q), None) == _lib.BAD_ARGUMENT
    assert f(None, sp, 4, C.byref(T), 1.0, None, None) == _lib.BAD_ARGUMENT
    assert f(None, sp, 4, None, 1.0, C.byref(q), None) == _lib.BAD_ARGUMENT
    assert f(None, sp, 4, C.byref(T), float("nan"), C.byref(q), None) == _lib.BAD_ARGUMENT


def test_batch_counters_start_at_zero_and_need_a_batch():
    b = _batch(3)
    try:
        out = (C.c_uint64 * 3)(7, 7, 7)
        assert I.lib().icp_batch_evaluate_counters(b, out) == _lib.OK and list(out) == [0, 0, 0]
        assert I.lib().icp_batch_evaluate_counters(None, out) == _lib.BAD_ARGUMENT
    finally:
        I.lib().icp_batch_destroy(b)


def test_python_batch_evaluate_refuses_mismatched_lists():
    B = I.IcpBatch(2)
    with pytest.raises(ValueError):
        B.evaluate([np.zeros((3, 2))], [], None, 1.0)
    with pytest.raises(ValueError):
        B.evaluate([np.zeros((3, 2))], [np.zeros((3, 2))], [I.Transform(), I.Transform()], 1.0)
    assert B.evaluate([], [], [], 1.0) == []


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
def test_quality_kernels_do_not_spill_and_fit_a_cu():
    """no scratch in any k_quality_* kernel, and a workgroup's registers fit a CU (512 per lane of a SIMD, the
    batch kernel's 1024 threads = four waves per SIMD); the names stay clear of the budgeted search / evaluation
    kernels (tests/test_registers.py)"""
    from test_registers import BUDGET

    regs = _usage("quality.hip")
    threads = {"k_quality_termsILi2E": 256, "k_quality_termsILi3E": 256, "k_fold_levelILi6E": 256,
               "k_quality_batchILi2E": 1024, "k_quality_batchILi3E": 1024}
    for frag, b in threads.items():
        names = [k for k in regs if frag in k and not k.endswith("#scratch")]
        assert len(names) == 1, (frag, names)
        assert regs.get(names[0] + "#scratch", 0) == 0, (names[0], regs.get(names[0] + "#scratch"))
        assert regs[names[0]] <= 512 // (b // 256), (names[0], regs[names[0]])
    for k in regs:
        if "k_quality" in k:
            assert not any(frag in k for frag in BUDGET), k
