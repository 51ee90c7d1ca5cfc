"""CPU-side checks of the point-to-plane pose quality (icp_evaluate_point_to_plane[_device], icp_plane_quality:
include/icp_mi355x.h section 13): declared, exported and bound; ABI version still 8; every argument error rejected
before the device is touched; valid arguments answer ICP_NO_DEVICE on a host without one; the Python layer (PlaneQuality,
Icp2d's refusal); run_scan_to_map scores each frame between its estimate and its append, and only when asked; the two
kernels' register and scratch use (hipcc cross-compiles without a GPU)."""
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
ENTRIES = ("icp_evaluate_point_to_plane", "icp_evaluate_point_to_plane_device")
TOO_MANY = 0xffffffff  # n >= 2^32 - 1 is refused


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", text))


def test_symbols_are_declared_exported_and_bound():
    public = declared("icp_mi355x.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in ENTRIES:
        assert s in public, s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    assert "quality_plane.hip" in open(os.path.join(ROOT, "icp_rust_amd", "csrc", "Makefile")).read()
    assert callable(I.Icp3d.evaluate_point_to_plane)
    assert I.PlaneQuality is not None


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def test_struct_layout_matches_the_header():
    """two u64, seven doubles, nine of the matrix, two eigenvalues: 160 bytes, in the header's order"""
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    body = re.search(r"typedef struct icp_plane_quality \{(.*?)\} icp_plane_quality;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n) for stmt in body.split(";") if stmt.strip()
             for n in re.split(r",\s*", stmt.strip().split(None, 1)[1])]
    assert names == [f[0] for f in _lib.PlaneQualityStruct._fields_], names
    assert C.sizeof(_lib.PlaneQualityStruct) == 8 * (2 + 7 + 9 + 2)


def _identity():
    T = _lib.Pose()
    I.lib().icp_transform_identity(C.byref(T))
    return T


class _Handle:
    """A real 3-D handle with current normals where there is a device; on a host without one no handle can exist
    (icp_create answers ICP_NO_DEVICE), so the entries are given a block of zeroed memory in its place: they must decide
    on their arguments, and then on the device, before they read a handle."""

    def __init__(self):
        self.h = C.c_void_p()
        self.real = I.lib().icp_device_count() > 0
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


def _dirty():
    q = _lib.PlaneQualityStruct()
    C.memset(C.byref(q), 0x5a, C.sizeof(q))
    return q


def _is_n_and_zeros(q, n):
    raw = bytes(q)
    return q.n == n and raw[8:] == bytes(len(raw) - 8)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_rejected_before_the_device_is_used(entry):
    f = getattr(I.lib(), entry)
    src = np.zeros((4, 3))
    sp = C.c_void_p(src.ctypes.data)
    T = _identity()
    H = _Handle()
    try:
        for r in (float("nan"), -1.0, float("-inf"), -1e-300):
            out = _dirty()
            assert f(H.h, sp, 4, C.byref(T), r, C.byref(out), None) == _lib.BAD_ARGUMENT, r
            assert _is_n_and_zeros(out, 4), r  # anything but ICP_OK: n and zeros
        out = _dirty()
        assert f(None, sp, 4, C.byref(T), 1.0, C.byref(out), None) == _lib.BAD_ARGUMENT
        assert f(H.h, sp, 4, None, 1.0, C.byref(out), None) == _lib.BAD_ARGUMENT
        assert f(H.h, sp, 4, C.byref(T), 1.0, None, None) == _lib.BAD_ARGUMENT
        assert f(H.h, None, 4, C.byref(T), 1.0, C.byref(out), None) == _lib.BAD_ARGUMENT
        assert f(H.h, sp, TOO_MANY, C.byref(T), 1.0, C.byref(out), None) == _lib.BAD_ARGUMENT
        # n == 0: ICP_OK and zeros, whatever the handle is and without a source
        out = _dirty()
        assert f(H.h, None, 0, C.byref(T), 0.0, C.byref(out), None) == _lib.OK
        assert _is_n_and_zeros(out, 0)
        if not H.real:  # valid arguments reach the device check only now; 0 and +inf are valid bounds
            for r in (0.0, 1.0, float("inf")):
                out = _dirty()
                assert f(H.h, sp, 4, C.byref(T), r, C.byref(out), None) == _lib.NO_DEVICE, r
                assert _is_n_and_zeros(out, 4), r
    finally:
        H.close()


def test_python_layer_refuses_a_2d_handle_before_any_call_and_wraps_the_struct():
    icp = object.__new__(I.Icp2d)  # (no handle is reached: the dimension is checked first)
    icp._h = C.c_void_p()
    with pytest.raises(ValueError):
        icp.evaluate_point_to_plane(np.zeros((3, 2)), I.Transform())
    with pytest.raises(ValueError):
        icp.evaluate_point_to_plane(np.zeros((3, 3)), I.Transform(), 1.0, return_indices=True)
    q = _lib.PlaneQualityStruct()
    q.n, q.inliers = 7, 5
    q.fitness, q.inlier_rmse, q.inlier_sum_d2, q.plane_rmse, q.plane_sum_r2, q.error, q.huber_error = 1, 2, 3, 4, 5, 6, 7
    for k, v in enumerate([4.0, 0.0, 10.0, 0.0, 1.0, 11.0, 10.0, 11.0, 12.0]):
        q.information[k] = v
    q.translation_eig[0], q.translation_eig[1] = 1.0, 4.0
    Q = I.PlaneQuality(q)
    assert Q.n == 7 and Q.inliers == 5 and Q.information.shape == (3, 3) and Q.information[1, 2] == 11.0
    assert Q.as_array().tolist() == [1, 2, 3, 4, 5, 6, 7, 4, 0, 10, 0, 1, 11, 10, 11, 12, 1, 4]
    w = Q.weak_direction()  # the block is diag(4, 1): least observed along y
    assert abs(abs(w[1]) - 1.0) < 1e-15 and abs(w[0]) < 1e-15
    assert "plane_rmse" in repr(Q)


def test_scan_to_map_scores_each_frame_between_its_estimate_and_its_append_and_only_when_asked():
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

        def evaluate(self, src, T, r):
            log.append(("evaluate", len(src), T.as_array().copy(), r))
            return "q%d" % len(log)

        def evaluate_point_to_plane(self, src, T, r):
            log.append(("evaluate_point_to_plane", len(src), T.as_array().copy(), r))
            return "pq%d" % len(log)

        def compute_normals(self, k):
            log.append(("compute_normals", k))

        def update_normals(self, k):
            log.append(("update_normals", k))

        def append(self, pts, T):
            log.append(("append", T.as_array().copy()))

        def crop(self, center, radius):
            log.append(("crop",))

    class NoEvaluate(Fake):
        evaluate = None  # (a factory without the evaluations keeps working when no list is given)
        evaluate_point_to_plane = None

    packets = synth.synthetic_scan3d_packets(4 * synth.PACKETS_PER_FRAME)
    # the defaults call neither, with either residual, and return what they returned
    Ts0, path0, _ = harness.run_scan_to_map(packets, icp_factory=NoEvaluate, max_iter=2)
    assert [e[0] for e in log] == ["estimate", "append"] * 3
    del log[:]
    harness.run_scan_to_map(packets, icp_factory=NoEvaluate, max_iter=2, point_to_plane=8, quality_distance=0.5)
    assert [e[0] for e in log] == ["compute_normals"] + ["estimate", "append", "update_normals"] * 3
    del log[:]
    # point-to-plane: estimate -> evaluate_point_to_plane -> append -> update_normals, once per frame
    got = []
    Ts, path, _ = harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, point_to_plane=8, qualities=got,
                                          quality_distance=0.5)
    assert [e[0] for e in log] == ["compute_normals"] + ["estimate", "evaluate_point_to_plane", "append",
                                                         "update_normals"] * 3
    evs = [e for e in log if e[0] == "evaluate_point_to_plane"]
    assert got == ["pq3", "pq7", "pq11"]
    for T, e in zip(Ts, evs):
        assert np.array_equal(e[2], T.as_array()) and e[3] == 0.5 and e[1] > 0
    assert np.array_equal(path, path0) and all(np.array_equal(a.as_array(), b.as_array()) for a, b in zip(Ts, Ts0))
    del log[:]
    # point-to-point: evaluate, with +inf when no distance is given; the crop stays last
    got = []
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, qualities=got, map_radius=5.0)
    assert [e[0] for e in log] == ["estimate", "evaluate", "append", "crop"] * 3
    assert all(e[3] == float("inf") for e in log if e[0] == "evaluate") and len(got) == 3
    del log[:]
    with pytest.raises(ValueError):  # (the existing refusal stays)
        harness.run_scan_to_map(packets, icp_factory=Fake, point_to_plane=8, max_correspondence_distance=1.0,
                                qualities=[])


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
def test_plane_quality_kernels_do_not_spill_and_leave_room_for_four_waves_per_simd():
    """exactly the two kernels of quality_plane.hip; no scratch and at most 128 VGPRs (512 per lane of a SIMD: four
    waves) in both; the names stay clear of the budgeted search / evaluation kernels (tests/test_registers.py)"""
    from test_registers import BUDGET

    regs = _usage("quality_plane.hip")
    kernels = [k for k in regs if not k.endswith("#scratch")]
    for frag in ("k_plane_quality_terms", "k_fold_levelILi10E"):
        assert len([k for k in kernels if frag in k]) == 1, (frag, kernels)
    assert len(kernels) == 2, kernels
    for k in kernels:
        assert regs.get(k + "#scratch", 0) == 0, (k, regs.get(k + "#scratch"))
        assert regs[k] <= 128, (k, regs[k])
        assert not any(frag in k for frag in BUDGET), k
