"""CPU-side checks of the batched point-to-plane registration (icp_batch_estimate_point_to_plane*, include/icp_mi355x.h
section 18): declared, exported and bound, the counters and the LDS plan's accessor in the debug header; ABI version still
8; every argument error -- a 2-D batch, k outside [3, 16], a range outside the packed arrays, null outputs -- rejected
before the device is touched, count == 0 a successful no-op; the Python layer's refusals and return shapes (with a library
that is not the real one); the LDS plan at its corners (DESIGN.md section 9m derives the figures); and the kernel's
cross-compile for gfx950 with its register and scratch budget."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib
from icp_rust_amd import api as api_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "icp_rust_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ("icp_batch_estimate_point_to_plane", "icp_batch_estimate_point_to_plane_device")
DEBUG = ("icp_batch_plane_counters", "icp_debug_plane_batch_plan")
GRANT = 160 * 1024 - 256  # the dynamic LDS a one-workgroup kernel asks for (163 584 bytes)


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", text))


def test_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in public and s in _lib.SIGNATURES and hasattr(L, s), s
    for s in DEBUG:
        assert s in debug and s not in public and s in _lib.SIGNATURES and hasattr(L, s), s
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "p2plane_batch.hip" in mk and "pair_loop_device.hpp" in mk
    for name in ("estimate_point_to_plane", "estimate_point_to_plane_packed", "plane_counters"):
        assert callable(getattr(I.IcpBatch, name)), name


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def _batch(dim=3):
    b = C.c_void_p()
    assert I.lib().icp_batch_create(C.byref(b), dim, -1) == _lib.OK  # (no device use: works without a GPU)
    return b


def _call(b, src, dst, items, k=8, max_iter=20, out=True, status=True, entry=NEW[0], count=None):
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
                                   arr if items else None, count, k, max_iter, o,
                                   C.c_void_p(st.ctypes.data) if status else None, None, None)


@pytest.mark.parametrize("entry", NEW)
def test_argument_errors_are_rejected_before_the_device_is_used(entry):
    src, dst = np.zeros((10, 3)), np.zeros((20, 3))
    good = [(0, 10, 0, 20), (3, 7, 0, 0), (10, 0, 20, 0)]
    b, b2 = _batch(), _batch(2)
    try:
        assert _call(b2, np.zeros((10, 2)), np.zeros((20, 2)), good, entry=entry) == _lib.BAD_ARGUMENT  # a 2-D batch
        assert _call(b2, None, None, [], count=0, entry=entry) == _lib.BAD_ARGUMENT
        for k in (2, 17, 0, -1):
            assert _call(b, src, dst, good, k=k, entry=entry) == _lib.BAD_ARGUMENT, k
        bad = [
            [(0, 11, 0, 20)],                     # source range past the array
            [(5, 6, 0, 20)],
            [(0, 10, 1, 20)],                     # target range past the array
            [(0, 10, 21, 0)],                     # (an empty range that starts past the end)
            [(0, 10, 0, 20), (2**63, 2**63, 0, 1)],  # (first + n overflows)
        ]
        for items in bad:
            assert _call(b, src, dst, items, entry=entry) == _lib.BAD_ARGUMENT, items
        assert _call(b, src, dst, good, out=False, entry=entry) == _lib.BAD_ARGUMENT
        assert _call(b, src, dst, good, status=False, entry=entry) == _lib.BAD_ARGUMENT
        assert _call(b, src, dst, [], count=3, entry=entry) == _lib.BAD_ARGUMENT  # items NULL, count > 0
        assert getattr(I.lib(), entry)(None, None, 0, None, 0, None, 0, 8, 20, None, None, None, None) == _lib.BAD_ARGUMENT
        # null clouds with points claimed
        arr = (_lib.BatchItem * 1)()
        o, st = (_lib.Pose * 1)(), np.zeros(1, dtype=np.int32)
        assert getattr(I.lib(), entry)(b, None, 10, C.c_void_p(dst.ctypes.data), 20, arr, 1, 8, 20, o,
                                       C.c_void_p(st.ctypes.data), None, None) == _lib.BAD_ARGUMENT
        assert getattr(I.lib(), entry)(b, C.c_void_p(src.ctypes.data), 10, None, 20, arr, 1, 8, 20, o,
                                       C.c_void_p(st.ctypes.data), None, None) == _lib.BAD_ARGUMENT
        # count == 0 is a successful no-op whatever the other pointers are, for k = 3 and k = 16 too
        for k in (3, 8, 16):
            assert _call(b, None, None, [], k=k, count=0, out=False, status=False, entry=entry) == _lib.OK
        if I.lib().icp_device_count() == 0:  # valid arguments reach the device check only now
            assert _call(b, src, dst, good, entry=entry) == _lib.NO_DEVICE
            assert _call(b, src, dst, good, k=3, entry=entry) == _lib.NO_DEVICE
            assert _call(b, src, dst, good, k=16, entry=entry) == _lib.NO_DEVICE
        out = (C.c_uint64 * 4)(9, 9, 9, 9)
        assert I.lib().icp_batch_plane_counters(b, out) == _lib.OK and list(out) == [0, 0, 0, 0]
        assert I.lib().icp_batch_plane_counters(None, out) == _lib.BAD_ARGUMENT
        assert I.lib().icp_batch_plane_counters(b, None) == _lib.BAD_ARGUMENT
    finally:
        I.lib().icp_batch_destroy(b)
        I.lib().icp_batch_destroy(b2)


def test_python_layer_refuses_before_the_library_is_reached():
    B2 = object.__new__(I.IcpBatch)  # (no batch object is reached: the dimension is checked first)
    B2.DIM, B2._b, B2._device = 2, None, None
    with pytest.raises(ValueError):
        B2.estimate_point_to_plane([np.zeros((3, 2))], [np.zeros((3, 2))], None, 20)
    with pytest.raises(ValueError):
        B2.estimate_point_to_plane_packed(np.zeros((3, 2)), np.zeros((3, 2)), [], 20)
    B = I.IcpBatch(3)
    with pytest.raises(ValueError):
        B.estimate_point_to_plane([np.zeros((3, 3))], [], None, 20)
    with pytest.raises(ValueError):
        B.estimate_point_to_plane([np.zeros((3, 3))], [np.zeros((3, 3))], [I.Transform(), I.Transform()], 20)
    for k in (2, 17):
        with pytest.raises(ValueError):
            B.estimate_point_to_plane([np.zeros((3, 3))], [np.zeros((3, 3))], None, 20, k=k)
    assert B.estimate_point_to_plane([], [], [], 20) == []
    assert B.plane_counters() == (0, 0, 0, 0)
    assert B.counters() == (0, 0, 0, 0) and B.line_counters() == (0, 0, 0, 0)
    B.close()


class _FakeLib:
    """Stands in for the library: records the host entry's arguments, answers item i with the pose (i, 0, 0), indices
    i, i, ..., inner counts i + 1 and the statuses handed to it."""

    def __init__(self, statuses):
        self.statuses, self.calls, self.real = statuses, [], I.lib()

    def __getattr__(self, name):  # (the host-only pose algebra stays the library's)
        return getattr(self.real, name)

    def icp_batch_estimate_point_to_plane(self, b, src, src_points, dst, dst_points, arr, count, k, max_iter, out, status,
                                          idx, inner):
        self.calls.append((src_points, dst_points, count, k, max_iter))
        st = np.ctypeslib.as_array(C.cast(status, C.POINTER(C.c_int32)), shape=(count,))
        st[:] = self.statuses[:count]
        ii = np.ctypeslib.as_array(C.cast(inner, C.POINTER(C.c_uint32)), shape=(count * max_iter,))
        at = 0
        for i in range(count):
            out[i].r00, out[i].r10, out[i].r01, out[i].r11, out[i].tx, out[i].ty = 1.0, 0.0, 0.0, 1.0, float(i), 0.0
            ii[i * max_iter:(i + 1) * max_iter] = i + 1
            n = int(arr[i].n)
            if idx is not None and n:
                np.ctypeslib.as_array(C.cast(idx, C.POINTER(C.c_uint32)), shape=(at + n,))[at:] = i
            at += n
        return _lib.OK


def test_python_return_shapes_with_a_fake_library(monkeypatch):
    fake = _FakeLib([_lib.OK, _lib.NAN_INPUT, _lib.OK])
    monkeypatch.setattr(api_module, "lib", lambda: fake)
    B = object.__new__(I.IcpBatch)
    B.DIM, B._b, B._device = 3, C.c_void_p(), None
    srcs = [np.zeros((4, 3)), np.ones((2, 3)), np.zeros((0, 3))]
    dsts = [np.zeros((5, 3)), np.ones((6, 3)), np.ones((3, 3))]
    Ts, idxs, inner, status = B.estimate_point_to_plane(srcs, dsts, None, 7, k=5, return_info=True, allow_failures=True)
    assert fake.calls == [(6, 14, 3, 5, 7)]
    assert [T is None for T in Ts] == [False, True, False] and Ts[2].as_array()[4] == 2.0
    assert [len(x) for x in idxs] == [4, 2, 0] and idxs[1].tolist() == [1, 1]
    assert inner.shape == (3, 7) and inner[:, 0].tolist() == [1, 2, 3] and status.tolist() == [0, _lib.NAN_INPUT, 0]
    with pytest.raises(I.IcpError, match="item 1"):
        B.estimate_point_to_plane(srcs, dsts, None, 7)
    fake.statuses = [_lib.OK] * 3
    Ts = B.estimate_point_to_plane_packed(np.zeros((4, 3)), np.zeros((9, 3)), [(0, 4, 0, 9, I.Transform())] * 3, 2)
    assert len(Ts) == 3 and all(isinstance(T, I.Transform) for T in Ts)
    assert fake.calls[-1] == (4, 9, 3, 10, 2)  # (k defaults to 10)
    B._b = None  # (nothing to destroy)


def _plan(threads, m):
    out = (C.c_uint32 * 4)()
    assert I.lib().icp_debug_plane_batch_plan(threads, m, out) == _lib.OK
    return tuple(out)  # lists per round, shared bytes, fixed bytes, dynamic LDS


def test_lds_plan_at_its_corners():
    """the figures DESIGN.md section 9m derives: with mp = m rounded up to 64, fixed = 24 mp (x | y | z) +
    16 (mp + 4) (screen records) + 24 mp (normals) + 16 x 13 x 8 (wave sums) + 128 (totals) + 256 (control block); the
    shared region holds in turn the sort keys (8 B x next power of two of m), the lists (192 B each, a multiple of 64 of
    them) and the three sort buffers (8 B x threads each)"""
    # m = 2048: 133 184 fixed, 30 400 left, 128 lists -> sixteen rounds; the 24 576 B of sort buffers fit in what is left
    for threads in (512, 1024):
        lists, shared, fixed, lds = _plan(threads, 2048)
        assert fixed == 133184 and GRANT - fixed == 30400
        assert lists == 128 and -(-2048 // lists) == 16
        assert shared == max(128 * 192, 2048 * 8, 3 * threads * 8) == 24576 and shared <= GRANT - fixed
        assert lds == fixed + shared == 157760 <= GRANT
    # m = 1024: 67 648 fixed, 448 lists -> three rounds
    for threads in (512, 1024):
        lists, shared, fixed, lds = _plan(threads, 1024)
        assert fixed == 67648 and lists == 448 and -(-1024 // lists) == 3
        assert shared == 448 * 192 and lds == fixed + shared <= GRANT
    # m = 1: one wave of lists; the sort buffers decide the shared region
    for threads in (512, 1024):
        lists, shared, fixed, lds = _plan(threads, 1)
        assert fixed == 24 * 64 + 16 * 68 + 24 * 64 + 16 * 13 * 8 + 128 + 256 == 6208
        assert lists == 64 and shared == max(64 * 192, 3 * threads * 8) and lds == fixed + shared
    # every m: whole waves of lists, no more than threads or targets (rounded up), and never more LDS than the grant
    for threads in (512, 1024):
        for m in range(1, 2049):
            lists, shared, fixed, lds = _plan(threads, m)
            mp = (m + 63) // 64 * 64
            assert lists % 64 == 0 and 64 <= lists <= min(threads, mp), (threads, m)
            assert shared >= lists * 192 and shared >= 3 * threads * 8 and lds == fixed + shared <= GRANT, (threads, m)
    out = (C.c_uint32 * 4)()
    for threads, m in ((256, 8), (512, 0), (512, 2049), (768, 8)):
        assert I.lib().icp_debug_plane_batch_plan(threads, m, out) == _lib.BAD_ARGUMENT
    assert I.lib().icp_debug_plane_batch_plan(512, 8, None) == _lib.BAD_ARGUMENT


def _usage(src):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(CSRC, src), "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    use, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            use[name] = {}
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                use[name][key] = int(m.group(1))
    return use


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_batch_kernel_cross_compiles_within_its_budget():
    """one instantiation per workgroup size; no scratch at 512 threads, at 1024 (128 registers per thread) no more than
    the point kernel may (tests/test_registers.py: 96 bytes per lane); no static LDS on top of the dynamic plan"""
    use = _usage("p2plane_batch.hip")
    for b, cap in ((512, 0), (1024, 96)):
        names = [k for k in use if "k_plane_estimate_batchILj%dE" % b in k]
        assert len(names) == 1, names
        u = use[names[0]]
        assert u["scratch"] <= cap, (names[0], u)
        assert u["vgpr"] <= 512 // (b // 256), (names[0], u)  # (a workgroup must fit a CU at all)
        assert u["lds"] == 0, (names[0], u)
