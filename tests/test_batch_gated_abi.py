"""CPU-side checks of the gated batched point-to-point registration (icp_batch_estimate_gated*, include/icp_mi355x.h
section 21): declared, exported and bound, the counters in the debug header; ABI version still 8; every argument error
-- a bound that is negative or NaN, a range outside the packed arrays, null outputs -- rejected before the device is
touched, count == 0 a successful no-op; the Python layer's refusals and return shapes (with a library that is not the
real one), None still reaching the ungated symbols; and the kernels' cross-compile for gfx950 with their register and
scratch budget (the LDS plan is asserted at compile time)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib
from icp_rust_amd import api as api_module
from test_line_batch_abi import CSRC, HIPCC, _batch, _usage, declared

NEW = ("icp_batch_estimate_gated", "icp_batch_estimate_gated_device")
COUNTERS = "icp_batch_gated_counters"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


def test_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in public and s in _lib.SIGNATURES and hasattr(L, s), s
    assert COUNTERS in debug and COUNTERS not in public
    assert COUNTERS in _lib.SIGNATURES and hasattr(L, COUNTERS)
    assert callable(I.IcpBatch.gated_counters)
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def _call(b, src, dst, items, max_iter=20, max_dist=0.5, out=True, status=True, entry=NEW[0], count=None):
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
                                   arr if items else None, count, max_iter, max_dist, o,
                                   C.c_void_p(st.ctypes.data) if status else None, None, None, None)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("entry", NEW)
def test_argument_errors_are_rejected_before_the_device_is_used(entry, dim):
    src, dst = np.zeros((10, dim)), np.zeros((20, dim))
    good = [(0, 10, 0, 20), (3, 7, 0, 0), (10, 0, 20, 0)]
    b = _batch(dim)
    try:
        for r in (-1.0, float("nan"), -0.5, float("-inf")):
            assert _call(b, src, dst, good, max_dist=r, entry=entry) == _lib.BAD_ARGUMENT, r
            assert _call(b, None, None, [], count=0, max_dist=r, entry=entry) == _lib.BAD_ARGUMENT, r
        # an item range past the arrays, an empty range that starts past the end, first + n overflowing
        for items in ([(0, 11, 0, 20)], [(5, 6, 0, 20)], [(0, 10, 1, 20)], [(0, 10, 21, 0)],
                      [(0, 10, 0, 20), (2**63, 2**63, 0, 1)]):
            assert _call(b, src, dst, items, entry=entry) == _lib.BAD_ARGUMENT, items
        assert _call(b, src, dst, good, out=False, entry=entry) == _lib.BAD_ARGUMENT
        assert _call(b, src, dst, good, status=False, entry=entry) == _lib.BAD_ARGUMENT
        assert _call(b, src, dst, [], count=3, entry=entry) == _lib.BAD_ARGUMENT  # items NULL, count > 0
        assert getattr(I.lib(), entry)(None, None, 0, None, 0, None, 0, 20, 0.5, None, None, None, None,
                                       None) == _lib.BAD_ARGUMENT
        # count == 0 is a successful no-op whatever the other pointers are, for the bounds 0 and +inf too
        for r in (0.0, 0.5, float("inf")):
            assert _call(b, None, None, [], count=0, max_dist=r, out=False, status=False, entry=entry) == _lib.OK
        if I.lib().icp_device_count() == 0:  # valid arguments reach the device check only now
            for r in (0.0, 0.5, float("inf")):
                assert _call(b, src, dst, good, max_dist=r, entry=entry) == _lib.NO_DEVICE
        out = (C.c_uint64 * 4)(9, 9, 9, 9)
        assert getattr(I.lib(), COUNTERS)(b, out) == _lib.OK and list(out) == [0, 0, 0, 0]
        assert getattr(I.lib(), COUNTERS)(None, out) == _lib.BAD_ARGUMENT
        assert getattr(I.lib(), COUNTERS)(b, None) == _lib.BAD_ARGUMENT
    finally:
        I.lib().icp_batch_destroy(b)


class _FakeLib:
    """Stands in for the library: records which entry was called with what, answers item i with the pose (i, 0, 0),
    indices i, i, ..., inner counts i + 1, inlier counts 10 + i and the statuses handed to it."""

    def __init__(self, statuses):
        self.statuses, self.calls, self.real = statuses, [], I.lib()

    def __getattr__(self, name):  # (the host-only pose algebra stays the library's)
        return getattr(self.real, name)

    def _answer(self, name, src_points, dst_points, arr, count, max_iter, max_dist, out, status, idx, inner, inl):
        self.calls.append((name, src_points, dst_points, count, max_iter, max_dist))
        st = np.ctypeslib.as_array(C.cast(status, C.POINTER(C.c_int32)), shape=(count,))
        st[:] = self.statuses[:count]
        ii = np.ctypeslib.as_array(C.cast(inner, C.POINTER(C.c_uint32)), shape=(count * max_iter,))
        ll = np.ctypeslib.as_array(C.cast(inl, C.POINTER(C.c_uint32)), shape=(count * max_iter,)) if inl else None
        at = 0
        for i in range(count):
            out[i].r00, out[i].r10, out[i].r01, out[i].r11, out[i].tx, out[i].ty = 1.0, 0.0, 0.0, 1.0, float(i), 0.0
            ii[i * max_iter:(i + 1) * max_iter] = i + 1
            if ll is not None:
                ll[i * max_iter:(i + 1) * max_iter] = 10 + i
            n = int(arr[i].n)
            if idx is not None and n:
                np.ctypeslib.as_array(C.cast(idx, C.POINTER(C.c_uint32)), shape=(at + n,))[at:] = i
            at += n
        return _lib.OK

    def icp_batch_estimate(self, b, src, src_points, dst, dst_points, arr, count, max_iter, out, status, idx, inner):
        return self._answer("ungated", src_points, dst_points, arr, count, max_iter, None, out, status, idx, inner, None)

    def icp_batch_estimate_gated(self, b, src, src_points, dst, dst_points, arr, count, max_iter, max_dist, out, status,
                                 idx, inner, inl):
        return self._answer("gated", src_points, dst_points, arr, count, max_iter, max_dist, out, status, idx, inner, inl)


def _fake_batch(monkeypatch, statuses, dim=2):
    fake = _FakeLib(statuses)
    monkeypatch.setattr(api_module, "lib", lambda: fake)
    B = object.__new__(I.IcpBatch)
    B.DIM, B._b, B._device = dim, C.c_void_p(), None
    return fake, B


@pytest.mark.parametrize("dim", [2, 3])
def test_python_layer_refuses_a_bad_bound_before_the_library_is_reached(monkeypatch, dim):
    fake, B = _fake_batch(monkeypatch, [_lib.OK], dim)
    z = np.zeros((3, dim))
    for r in (-1.0, float("nan"), -1e-300, float("-inf")):
        with pytest.raises(ValueError):
            B.estimate([z], [z], None, 20, max_correspondence_distance=r)
        with pytest.raises(ValueError):
            B.estimate_packed(z, z, [(0, 3, 0, 3, I.Transform())], 20, max_correspondence_distance=r)
        with pytest.raises(ValueError):
            B.estimate_hypotheses(z, z, [I.Transform()], 20, max_correspondence_distance=r)
    assert fake.calls == []
    B._b = None  # (nothing to destroy)


def test_python_return_shapes_with_a_fake_library(monkeypatch):
    fake, B = _fake_batch(monkeypatch, [_lib.OK, _lib.NAN_INPUT, _lib.OK])
    srcs = [np.zeros((4, 2)), np.ones((2, 2)), np.zeros((0, 2))]
    dsts = [np.zeros((5, 2)), np.ones((6, 2)), np.ones((3, 2))]
    # None: the ungated symbol, the four-tuple unchanged
    got = B.estimate(srcs, dsts, None, 7, return_info=True, allow_failures=True, max_correspondence_distance=None)
    assert fake.calls == [("ungated", 6, 14, 3, 7, None)] and len(got) == 4
    assert got[2].shape == (3, 7) and got[3].tolist() == [0, _lib.NAN_INPUT, 0]
    assert len(B.estimate(srcs, dsts, None, 7, return_info=True, allow_failures=True)) == 4
    assert fake.calls[-1][0] == "ungated"
    # a bound: the gated symbol, the inlier counts behind the four
    for r in (0.25, 0.0, float("inf"), 1):
        Ts, idxs, inner, status, inl = B.estimate(srcs, dsts, None, 7, return_info=True, allow_failures=True,
                                                  max_correspondence_distance=r)
        assert fake.calls[-1] == ("gated", 6, 14, 3, 7, float(r))
        assert [T is None for T in Ts] == [False, True, False] and Ts[2].as_array()[4] == 2.0
        assert [len(x) for x in idxs] == [4, 2, 0] and idxs[1].tolist() == [1, 1]
        assert inner.shape == (3, 7) and inner[:, 0].tolist() == [1, 2, 3] and status.tolist() == [0, _lib.NAN_INPUT, 0]
        assert inl.shape == (3, 7) and inl.dtype == np.uint32 and inl[:, 6].tolist() == [10, 11, 12]
    with pytest.raises(I.IcpError, match="item 1"):
        B.estimate(srcs, dsts, None, 7, max_correspondence_distance=0.25)
    fake.statuses = [_lib.OK] * 3
    packed = (np.zeros((4, 2)), np.zeros((9, 2)), [(0, 4, 0, 9, I.Transform())] * 3, 2)
    Ts = B.estimate_packed(*packed, max_correspondence_distance=0.5)
    assert len(Ts) == 3 and all(isinstance(T, I.Transform) for T in Ts)
    assert fake.calls[-1] == ("gated", 4, 9, 3, 2, 0.5)
    assert len(B.estimate_packed(*packed, return_info=True)) == 4 and fake.calls[-1] == ("ungated", 4, 9, 3, 2, None)
    # the hypotheses: scored alike with and without the bound, through the symbol the bound selects (the score itself
    # needs a device: here it is the pose's translation and the first index)
    monkeypatch.setattr(api_module, "huber_error", lambda T, a, b: float(T.as_array()[4]) + float(b[0, 0]))
    inits = [I.Transform(), I.Transform([0.1, 0.0, 0.0])]
    Ts, errs = B.estimate_hypotheses(np.ones((4, 2)), np.zeros((9, 2)), inits, 2)
    assert fake.calls[-1] == ("ungated", 4, 9, 2, 2, None) and len(Ts) == 2 and errs.shape == (2,)
    gTs, gerrs = B.estimate_hypotheses(np.ones((4, 2)), np.zeros((9, 2)), inits, 2, max_correspondence_distance=0.5)
    assert fake.calls[-1] == ("gated", 4, 9, 2, 2, 0.5) and len(gTs) == 2 and np.array_equal(errs, gerrs)
    assert B.estimate([], [], [], 20, max_correspondence_distance=0.5) == []
    B._b = None  # (nothing to destroy)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gated_batch_kernels_cross_compile_within_their_budget():
    """one instantiation per dimension and workgroup size, under the kernel's own name; no spill at 512 and 768 threads,
    at 1024 (128 registers to a lane) no more than 96 bytes per lane, the cap of the one-workgroup kernels at that size
    (tests/test_registers.py); no static LDS on top of the dynamic plan.  Measured: 137 / 135 / 128 registers and 0 / 0 /
    60 bytes in two dimensions, 142 / 140 / 128 and 0 / 0 / 68 in three.  The ungated kernels of
    the same translation unit are held to theirs in tests/test_registers.py and tests/test_batch_abi.py."""
    assert "gn_fast.hip" in open(os.path.join(CSRC, "Makefile")).read()
    use = _usage("gn_fast.hip")
    for dim in (2, 3):
        for b, vgpr, scratch in ((512, 256, 0), (768, 168, 0), (1024, 128, 96)):
            names = [k for k in use if "k_tiny_estimate_gated_batchILi%dELj%dE" % (dim, b) in k]
            assert len(names) == 1, names
            u = use[names[0]]
            print(names[0], u)
            assert u["vgpr"] <= vgpr, (names[0], u)  # (512 registers per lane of a SIMD, b / 256 waves on it)
            assert u["scratch"] <= scratch, (names[0], u)
            assert u["lds"] == 0, (names[0], u)
    assert len([k for k in use if "k_tiny_estimate_gated_batch" in k]) == 6
