"""CPU-side checks of the gated batched point-to-plane registration (icp_batch_estimate_point_to_plane_gated*,
include/icp_mi355x.h section 19): declared, exported and bound, the counters and the LDS plan's accessor in the debug
header; ABI version still 8; every argument error -- a 2-D batch, k outside [3, 16], a bound that is negative or NaN, a
range outside the packed arrays, null outputs, count x max_iter words that cannot be addressed -- rejected before the
device is touched, count == 0 a successful no-op; the Python layer's refusals and return shapes (with a library that is
not the real one), None still reaching the ungated symbol; the LDS plan at its corners and its invariants at every m
(DESIGN.md section 9n derives the figures), the ungated plan unchanged; the numpy statement of the gate's d2 at the
bound, which tests/test_gpu_plane_batch_gated.py builds its `dz` case on; and the kernels' cross-compile for gfx950 with
their register and scratch budget."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib
from icp_rust_amd import api as api_module
from test_plane_batch_abi import CSRC, GRANT, HIPCC, _batch, _usage, declared

NEW = ("icp_batch_estimate_point_to_plane_gated", "icp_batch_estimate_point_to_plane_gated_device")
COUNTERS = "icp_batch_plane_gated_counters"
PLAN = "icp_debug_plane_gated_batch_plan"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


def test_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in public and s in _lib.SIGNATURES and hasattr(L, s), s
    for s in (COUNTERS, PLAN):
        assert s in debug and s not in public and s in _lib.SIGNATURES and hasattr(L, s), s
    assert callable(I.IcpBatch.plane_gated_counters)
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def _call(b, src, dst, items, k=8, max_iter=20, max_dist=0.5, out=True, status=True, entry=NEW[0], count=None,
          inner=None, inliers=None):
    count = len(items) if count is None else count
    arr = (_lib.BatchItem * max(len(items), 1))()
    for i, (f, n, g, m) in enumerate(items):
        arr[i].src_first, arr[i].n, arr[i].dst_first, arr[i].m = f, n, g, m
        I.lib().icp_transform_identity(C.byref(arr[i].init))
    o = (_lib.Pose * max(min(count, 64), 1))() if out else None
    st = np.zeros(max(min(count, 64), 1), dtype=np.int32)
    sp = C.c_void_p(src.ctypes.data) if src is not None else None
    dp = C.c_void_p(dst.ctypes.data) if dst is not None else None
    return getattr(I.lib(), entry)(b, sp, 0 if src is None else len(src), dp, 0 if dst is None else len(dst),
                                   arr if items else None, count, k, max_iter, max_dist, o,
                                   C.c_void_p(st.ctypes.data) if status else None, None, inner, inliers)


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
        for r in (-1.0, float("nan"), -0.5, float("-inf")):
            assert _call(b, src, dst, good, max_dist=r, entry=entry) == _lib.BAD_ARGUMENT, r
            assert _call(b, None, None, [], count=0, max_dist=r, entry=entry) == _lib.BAD_ARGUMENT, r
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
        assert getattr(I.lib(), entry)(None, None, 0, None, 0, None, 0, 8, 20, 0.5, None, None, None, None,
                                       None) == _lib.BAD_ARGUMENT
        # count x max_iter words that no size_t addresses, with only the inlier counts asked for (and only the inner
        # counts): refused before an item is read -- the items given are good ones
        word = np.zeros(1, dtype=np.uint32)
        wp = C.c_void_p(word.ctypes.data)
        huge_iter = 2**62
        for kw in (dict(inliers=wp), dict(inner=wp), dict(inner=wp, inliers=wp)):
            assert _call(b, src, dst, good, max_iter=huge_iter, entry=entry, **kw) == _lib.BAD_ARGUMENT, kw
        # count == 0 is a successful no-op whatever the other pointers are, for the bounds 0 and +inf too
        for r in (0.0, 0.5, float("inf")):
            for k in (3, 8, 16):
                assert _call(b, None, None, [], k=k, count=0, max_dist=r, out=False, status=False, entry=entry) == _lib.OK
        if I.lib().icp_device_count() == 0:  # valid arguments reach the device check only now
            for r in (0.0, 0.5, float("inf")):
                assert _call(b, src, dst, good, max_dist=r, entry=entry) == _lib.NO_DEVICE
            assert _call(b, src, dst, good, k=3, entry=entry) == _lib.NO_DEVICE
            assert _call(b, src, dst, good, k=16, entry=entry) == _lib.NO_DEVICE
        out = (C.c_uint64 * 4)(9, 9, 9, 9)
        assert getattr(I.lib(), COUNTERS)(b, out) == _lib.OK and list(out) == [0, 0, 0, 0]
        assert getattr(I.lib(), COUNTERS)(None, out) == _lib.BAD_ARGUMENT
        assert getattr(I.lib(), COUNTERS)(b, None) == _lib.BAD_ARGUMENT
        assert I.lib().icp_batch_plane_counters(b, out) == _lib.OK and list(out) == [0, 0, 0, 0]
    finally:
        I.lib().icp_batch_destroy(b)
        I.lib().icp_batch_destroy(b2)


class _FakeLib:
    """Stands in for the library: records which entry was called with what, answers item i with the pose (i, 0, 0),
    indices i, i, ..., inner counts i + 1, inlier counts 10 + i and the statuses handed to it."""

    def __init__(self, statuses):
        self.statuses, self.calls, self.real = statuses, [], I.lib()

    def __getattr__(self, name):  # (the host-only pose algebra stays the library's)
        return getattr(self.real, name)

    def _answer(self, name, src_points, dst_points, arr, count, k, max_iter, max_dist, out, status, idx, inner, inl):
        self.calls.append((name, src_points, dst_points, count, k, max_iter, max_dist))
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

    def icp_batch_estimate_point_to_plane(self, b, src, src_points, dst, dst_points, arr, count, k, max_iter, out, status,
                                          idx, inner):
        return self._answer("ungated", src_points, dst_points, arr, count, k, max_iter, None, out, status, idx, inner,
                            None)

    def icp_batch_estimate_point_to_plane_gated(self, b, src, src_points, dst, dst_points, arr, count, k, max_iter,
                                                max_dist, out, status, idx, inner, inl):
        return self._answer("gated", src_points, dst_points, arr, count, k, max_iter, max_dist, out, status, idx, inner,
                            inl)


def test_python_layer_refuses_a_bad_bound_before_the_library_is_reached(monkeypatch):
    fake = _FakeLib([_lib.OK])
    monkeypatch.setattr(api_module, "lib", lambda: fake)
    B = object.__new__(I.IcpBatch)
    B.DIM, B._b, B._device = 3, C.c_void_p(), None
    one = ([np.zeros((3, 3))], [np.zeros((3, 3))], None, 20)
    for r in (-1.0, float("nan"), -1e-300, float("-inf")):
        with pytest.raises(ValueError, match="max_correspondence_distance must be >= 0"):
            B.estimate_point_to_plane(*one, max_correspondence_distance=r)
        with pytest.raises(ValueError, match="max_correspondence_distance must be >= 0"):
            B.estimate_point_to_plane_packed(np.zeros((3, 3)), np.zeros((3, 3)), [(0, 3, 0, 3, I.Transform())], 20,
                                             max_correspondence_distance=r)
    for k in (2, 17):
        with pytest.raises(ValueError):
            B.estimate_point_to_plane(*one, k=k, max_correspondence_distance=0.5)
    assert fake.calls == []
    B2 = object.__new__(I.IcpBatch)  # (the dimension is checked first)
    B2.DIM, B2._b, B2._device = 2, None, None
    with pytest.raises(ValueError):
        B2.estimate_point_to_plane([np.zeros((3, 2))], [np.zeros((3, 2))], None, 20, max_correspondence_distance=0.5)
    with pytest.raises(ValueError):
        B2.estimate_point_to_plane_packed(np.zeros((3, 2)), np.zeros((3, 2)), [], 20, max_correspondence_distance=0.5)
    assert fake.calls == []
    B._b = None  # (nothing to destroy)


def test_python_return_shapes_with_a_fake_library(monkeypatch):
    fake = _FakeLib([_lib.OK, _lib.NAN_INPUT, _lib.OK])
    monkeypatch.setattr(api_module, "lib", lambda: fake)
    B = object.__new__(I.IcpBatch)
    B.DIM, B._b, B._device = 3, C.c_void_p(), None
    srcs = [np.zeros((4, 3)), np.ones((2, 3)), np.zeros((0, 3))]
    dsts = [np.zeros((5, 3)), np.ones((6, 3)), np.ones((3, 3))]
    # None: the ungated symbol, the four-tuple unchanged
    got = B.estimate_point_to_plane(srcs, dsts, None, 7, k=5, return_info=True, allow_failures=True,
                                    max_correspondence_distance=None)
    assert fake.calls == [("ungated", 6, 14, 3, 5, 7, None)] and len(got) == 4
    assert got[2].shape == (3, 7) and got[3].tolist() == [0, _lib.NAN_INPUT, 0]
    assert len(B.estimate_point_to_plane(srcs, dsts, None, 7, k=5, return_info=True, allow_failures=True)) == 4
    assert fake.calls[-1][0] == "ungated"
    # a bound: the gated symbol, the inlier counts behind the four
    for r in (0.25, 0.0, float("inf"), 1):
        Ts, idxs, inner, status, inl = B.estimate_point_to_plane(srcs, dsts, None, 7, k=5, return_info=True,
                                                                 allow_failures=True, max_correspondence_distance=r)
        assert fake.calls[-1] == ("gated", 6, 14, 3, 5, 7, float(r))
        assert [T is None for T in Ts] == [False, True, False] and Ts[2].as_array()[4] == 2.0
        assert [len(x) for x in idxs] == [4, 2, 0] and idxs[1].tolist() == [1, 1]
        assert inner.shape == (3, 7) and inner[:, 0].tolist() == [1, 2, 3] and status.tolist() == [0, _lib.NAN_INPUT, 0]
        assert inl.shape == (3, 7) and inl.dtype == np.uint32 and inl[:, 6].tolist() == [10, 11, 12]
    with pytest.raises(I.IcpError, match="item 1"):
        B.estimate_point_to_plane(srcs, dsts, None, 7, max_correspondence_distance=0.25)
    fake.statuses = [_lib.OK] * 3
    Ts = B.estimate_point_to_plane_packed(np.zeros((4, 3)), np.zeros((9, 3)), [(0, 4, 0, 9, I.Transform())] * 3, 2,
                                          max_correspondence_distance=0.5)
    assert len(Ts) == 3 and all(isinstance(T, I.Transform) for T in Ts)
    assert fake.calls[-1] == ("gated", 4, 9, 3, 10, 2, 0.5)  # (k defaults to 10)
    assert B.estimate_point_to_plane([], [], [], 20, max_correspondence_distance=0.5) == []
    B._b = None  # (nothing to destroy)


def _plan(threads, m, name=PLAN):
    out = (C.c_uint32 * 4)()
    assert getattr(I.lib(), name)(threads, m, out) == _lib.OK
    return tuple(out)  # lists per round, shared bytes, fixed bytes, dynamic LDS


def test_lds_plan_at_its_corners_and_at_every_m():
    """the figures DESIGN.md section 9n derives: fixed = 64 mp + 2112 with mp = m rounded up to 64; behind the three
    sort buffers (3 x 8 B x threads) the gate keeps ONE 4-byte word per thread and 16 wave counts, 4 B x threads + 64;
    the record of the line kernel's gate -- the moved point's x, y, the point's z and the position, 28 B a pair -- would
    overflow the grant from m = 1665 on"""
    gate = {512: 4 * 512 + 64, 1024: 4 * 1024 + 64}
    line_style = 28 * 1024 + 64
    assert gate == {512: 2112, 1024: 4160} and line_style == 28736
    # m = 2048: 30 400 bytes beside the fixed part; sort buffers + gate words = 28 736 at 1024 threads
    for threads in (512, 1024):
        lists, shared, fixed, lds = _plan(threads, 2048)
        assert fixed == 133184 and GRANT - fixed == 30400 and lists == 128
        assert shared == max(128 * 192, 3 * threads * 8 + gate[threads]) and lds == fixed + shared <= GRANT
    assert _plan(1024, 2048)[1] == 24576 + 4160 == 28736 <= 30400 and _plan(1024, 2048)[3] == 161920
    assert _plan(512, 2048)[3] == 157760
    assert 24576 + line_style == 53312 > 30400  # what does not carry over from the line kernel
    # m = 1664 and 1665: the last m the line-style record would fit at, and the first it would not
    for m, fixed_want in ((1664, 108608), (1665, 112704)):
        for threads in (512, 1024):
            lists, shared, fixed, lds = _plan(threads, m)
            assert fixed == fixed_want == 64 * ((m + 63) // 64 * 64) + 2112 and lists == 256
            assert shared == 256 * 192 and lds == fixed + shared <= GRANT
    assert 108608 + 24576 + line_style == 161920 <= GRANT < 112704 + 24576 + line_style
    # m = 1024: the gate's words lie where the lists were
    for threads in (512, 1024):
        assert _plan(threads, 1024) == (448, 448 * 192, 67648, 67648 + 448 * 192)
    # m = 1: the sort buffers and the gate's words decide the shared region
    assert _plan(512, 1) == (64, 12288 + 2112, 6208, 6208 + 14400)
    assert _plan(1024, 1) == (64, 24576 + 4160, 6208, 6208 + 28736)
    # every m: within the grant, room for the sort buffers and the gate's words, the rounds of the normals those of the
    # ungated plan -- whose own figures are what they were
    for threads in (512, 1024):
        for m in range(1, 2049):
            lists, shared, fixed, lds = _plan(threads, m)
            ulists, ushared, ufixed, ulds = _plan(threads, m, "icp_debug_plane_batch_plan")
            mp = (m + 63) // 64 * 64
            keys = max(64, 1 << (m - 1).bit_length())
            fit = (GRANT - ufixed) // 192 // 64 * 64
            assert ufixed == 64 * mp + 2112 and ulists == min(mp, threads, fit), (threads, m)
            assert ushared == max(ulists * 192, keys * 8, 3 * threads * 8) and ulds == ufixed + ushared, (threads, m)
            assert lists == ulists and 64 <= lists <= threads and lists % 64 == 0 and fixed == ufixed, (threads, m)
            assert shared == max(ushared, 3 * threads * 8 + gate[threads]), (threads, m)
            assert lds == fixed + shared <= GRANT, (threads, m)
    assert _plan(1024, 2048, "icp_debug_plane_batch_plan") == (128, 24576, 133184, 157760)
    out = (C.c_uint32 * 4)()
    for threads, m in ((256, 8), (512, 0), (512, 2049), (768, 8)):
        assert getattr(I.lib(), PLAN)(threads, m, out) == _lib.BAD_ARGUMENT
    assert getattr(I.lib(), PLAN)(512, 8, None) == _lib.BAD_ARGUMENT


DZ_R = 0.5


def dz_case():
    """The scene of the gate's `dz` term (tests/test_gpu_plane_batch_gated.py runs it): a floor patch of 16 x 16 targets
    at z = 0 with dyadic coordinates (x whole numbers, y whole numbers plus multiples of 2^-10), and 176 sources, each
    over one target: 40 exactly DZ_R above (d2 == r^2: kept), 40 nextafter(DZ_R, 1) above (dropped), 40 one metre above
    (xy distance 0, dropped), 16 displaced 0.3 in x and 0.4 in z over the targets with x = 0 (d2 rounds to exactly r^2:
    kept), 40 a quarter above (kept).  Returns (dst, src, kept count by d2_of, the target each source sits over)."""
    from test_gpu_gated_plane import d2_of

    rng = np.random.default_rng(3100)
    i, j = np.meshgrid(np.arange(-8, 8), np.arange(-8, 8), indexing="ij")
    y = j + ((j * 37) % 64) / 1024.0
    dst = np.ascontiguousarray(np.stack([i.ravel().astype(np.float64), y.ravel(), np.zeros(256)], axis=1))
    over, off = [], []
    for dz in (DZ_R, np.nextafter(DZ_R, 1.0), 1.0, 0.25):
        over.append(rng.integers(0, 256, 40))
        off.append(np.tile([0.0, 0.0, dz], (40, 1)))
    over.append(np.flatnonzero(dst[:, 0] == 0.0))
    off.append(np.tile([0.3, 0.0, 0.4], (16, 1)))
    over, off = np.concatenate(over), np.concatenate(off)
    order = rng.permutation(len(over))
    nearest = over[order]
    src = np.ascontiguousarray(dst[nearest] + off[order])
    d2 = d2_of(src, I.Transform(), dst[nearest])[3]
    return dst, src, int(np.sum(d2 <= DZ_R * DZ_R)), nearest


def test_the_gate_at_the_bound_in_numpy():
    """what tests/test_gpu_plane_batch_gated.py's `dz` case rests on, without a GPU: its sources' d2 (section 12's
    expression, every operation rounded on its own) against r^2 = 0.25 -- exactly on the bound, one ulp past it, far
    above with xy distance 0, and legs 0.3 / 0.4 whose squares round to a sum of exactly 0.25"""
    dst, src, want_kept, nearest = dz_case()
    assert want_kept == 40 + 16 + 40 and len(src) == 176
    assert DZ_R * DZ_R == 0.25
    assert (0.3 * 0.3 + 0.0) + 0.4 * 0.4 == 0.25  # (the legs the case uses: else other dyadic ones would be needed)
    assert np.all(dst * 1024 == np.round(dst * 1024)) and len(dst) <= 2048 and len(src) <= 1024
    # every source's nearest target by 3-D distance (exhaustive, f64) is the one it was built over, and no other is as near
    d = src[:, None, :] - dst[None, :, :]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    assert np.array_equal(np.argmin(d2, axis=1), nearest)
    best = d2[np.arange(len(src)), nearest]
    d2[np.arange(len(src)), nearest] = np.inf
    assert np.all(d2.min(axis=1) > best)
    from test_gpu_gated_plane import d2_of

    got = d2_of(src, I.Transform(), dst[nearest])[3]
    assert np.array_equal(got, best)
    kinds = {k: int(np.sum(got == v)) for k, v in (("on", 0.25), ("above", 1.0))}
    assert kinds["on"] > 0 and kinds["above"] > 0
    assert int(np.sum(got <= 0.25)) == want_kept and 0 < want_kept < len(src)
    assert int(np.sum((got > 0.25) & (got < 0.2500001))) > 0  # the one-ulp-past sources are there, and dropped


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_gated_batch_kernels_cross_compile_within_their_budget():
    """one instantiation per workgroup size, under the kernel's own name; no spill at 512 threads (256 registers to a
    lane), at 1024 (128 registers) no more than the point kernel may (tests/test_registers.py: 96 bytes per lane); no
    static LDS on top of the dynamic plan.  The ungated kernels: the budget of tests/test_plane_batch_abi.py."""
    assert "p2plane_batch.hip" in open(os.path.join(CSRC, "Makefile")).read()
    use = _usage("p2plane_batch.hip")
    for b, vgpr, scratch in ((512, 256, 0), (1024, 128, 96)):
        names = [k for k in use if "k_plane_estimate_gated_batchILj%dE" % b in k]
        assert len(names) == 1, names
        u = use[names[0]]
        print(names[0], u)
        assert u["vgpr"] <= vgpr, (names[0], u)
        assert u["scratch"] <= scratch, (names[0], u)
        assert u["lds"] == 0, (names[0], u)
    assert len([k for k in use if "k_plane_estimate_gated_batch" in k]) == 2
    for b, cap in ((512, 0), (1024, 96)):  # the ungated kernels, still one each and within their own test's budget
        names = [k for k in use if "k_plane_estimate_batchILj%dE" % b in k]
        assert len(names) == 1, names
        u = use[names[0]]
        assert u["scratch"] <= cap and u["vgpr"] <= 512 // (b // 256) and u["lds"] == 0, (names[0], u)
