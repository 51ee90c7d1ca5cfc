"""CPU-side checks of the point-to-line pose quality, single and batched (icp_evaluate_point_to_line[_device],
icp_batch_evaluate_point_to_line[_device], icp_line_quality: include/icp_mi355x.h section 16): declared, exported and
bound, the counters in the debug header; ABI version still 8; the struct's layout; every argument error rejected before
the device is touched; the Python layer (LineQuality, Icp3d's and a 3-D batch's refusal, a bad bound, a bad k);
run_scan2d scores each frame after its estimate, with the right scorer, and only when asked; a numpy restatement of the
definition (imported by tests/test_gpu_line_quality.py) on a corridor, a room and independent samples of an outline; the
two kernels' register and scratch use (hipcc cross-compiles without a GPU)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib
from test_line_abi import GOLDEN, SEEDS, line_normals_numpy, load_golden, moved2, outline_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "icp_rust_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SINGLE = ("icp_evaluate_point_to_line", "icp_evaluate_point_to_line_device")
BATCH = ("icp_batch_evaluate_point_to_line", "icp_batch_evaluate_point_to_line_device")
COUNTERS = "icp_batch_line_quality_counters"
TOO_MANY = 0xffffffff  # n >= 2^32 - 1 is refused
INF = float("inf")
K = 1.345  # ICP_HUBER_K
NFLOATS = 18  # LineQuality.as_array()
SCENE_POSE = [0.03, -0.02, 0.01]
SCENE_K = 8


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


# ------------------------------------------------------------------ shared with tests/test_gpu_line_quality.py

def fold(v):
    """the fold of section 9: n == 1 -> v[0], else groups of 256 padded with +0.0, g[i] += g[i + s], s = 128 .. 1"""
    v = np.asarray(v, dtype=np.float64).ravel()
    if v.size == 0:
        return np.float64(0.0)
    while v.size > 1:
        g = np.concatenate([v, np.zeros((-v.size) % 256)]).reshape(-1, 256)
        s = 128
        while s >= 1:
            g = g[:, :s] + g[:, s:2 * s]
            s //= 2
        v = g[:, 0]
    return v[0]


def nearest(dst, q):
    """exact 2-D nearest neighbours by brute force: d2 = dx dx + dy dy, ties to the lowest index"""
    out = np.empty(len(q), dtype=np.int64)
    for lo in range(0, len(q), 1024):
        dx = q[lo:lo + 1024, 0][:, None] - dst[None, :, 0]
        dy = q[lo:lo + 1024, 1][:, None] - dst[None, :, 1]
        out[lo:lo + 1024] = np.argmin(dx * dx + dy * dy, axis=1)
    return out


def terms(dst, nrm, src, T, idx):
    """section 16's per-point values, every operation rounded on its own (numpy forms each product and sum separately)"""
    q = moved2(np.ascontiguousarray(src, dtype=np.float64), T)
    qx, qy = q[:, 0], q[:, 1]
    j = np.asarray(idx).astype(np.int64)
    b, nj = dst[j], nrm[j]
    nx, ny = nj[:, 0], nj[:, 1]
    ex, ey = qx - b[:, 0], qy - b[:, 1]
    d2 = ex * ex + ey * ey
    rp = nx * ex + ny * ey
    c = (nx * (-qy)) + (ny * qx)
    return d2, rp * rp, nx, ny, c


def restate(dst, nrm, src, T, r, idx):
    """(status, inliers, the float fields in LineQuality.as_array order) by the definition"""
    n = len(src)
    if n == 0:
        return _lib.OK, 0, np.zeros(NFLOATS)
    with np.errstate(invalid="ignore", over="ignore"):
        d2, p2, nx, ny, c = terms(dst, nrm, src, T, idx)
        if np.isnan(p2).any():
            return _lib.NAN_INPUT, 0, np.zeros(NFLOATS)
        inl = d2 <= r * r
        z = np.zeros(n)
        h = np.where(p2 <= K * K, p2, 2.0 * K * np.sqrt(p2) - K * K)
        sd2, sp2 = fold(np.where(inl, d2, z)), fold(np.where(inl, p2, z))
        ixx, ixy, iyy = fold(np.where(inl, nx * nx, z)), fold(np.where(inl, nx * ny, z)), fold(np.where(inl, ny * ny, z))
        ixt, iyt, itt = fold(np.where(inl, nx * c, z)), fold(np.where(inl, ny * c, z)), fold(np.where(inl, c * c, z))
        cnt = int(inl.sum())
        rmse = np.sqrt(sd2 / cnt) if cnt else 0.0
        lrmse = np.sqrt(sp2 / cnt) if cnt else 0.0
        hh = (ixx + iyy) * 0.5
        gg = (ixx - iyy) * 0.5
        ss = np.sqrt(gg * gg + ixy * ixy)
    return _lib.OK, cnt, np.array([cnt / n, rmse, sd2, lrmse, sp2, fold(p2), fold(h), ixx, ixy, ixt, ixy, iyy, iyt, ixt,
                                   iyt, itt, hh - ss, hh + ss])


def wall_y(y):
    return np.stack([np.round(np.arange(-100, 101) * 0.1, 10), np.full(201, y)], axis=1)


def wall_x(x):
    return np.stack([np.full(39, x), np.round(np.arange(-19, 20) * 0.1, 10)], axis=1)


def corridor():
    """two walls y = +-2, x = -10 ... 10, on a 0.1 grid"""
    return np.ascontiguousarray(np.concatenate([wall_y(-2.0), wall_y(2.0)]))


def closed_room():
    """the corridor plus the end walls x = +-10, y = -1.9 ... 1.9"""
    return np.ascontiguousarray(np.concatenate([corridor(), wall_x(-10.0), wall_x(10.0)]))


def scene_scan(dst):
    """every third target moved by the inverse of a small pose: evaluated at that pose it lies on the map"""
    T = I.Transform(SCENE_POSE)
    return np.ascontiguousarray(moved2(np.ascontiguousarray(dst[::3]), T.inverse())), T


def weak_direction(f):
    """of the float fields in as_array order: the eigenvector of lmin of the translation block"""
    info = np.asarray(f[7:16]).reshape(3, 3)
    return np.linalg.eigh(info[:2, :2])[1][:, 0]


# ------------------------------------------------------------------ the boundary

def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", text))


def test_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in SINGLE + BATCH:
        assert s in public, s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    assert COUNTERS in debug and COUNTERS not in public
    assert COUNTERS in _lib.SIGNATURES and hasattr(L, COUNTERS)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "quality_line.hip" in mk and "p2line_device.hpp" in mk
    assert callable(I.Icp2d.evaluate_point_to_line) and I.LineQuality is not None
    for name in ("evaluate_point_to_line", "evaluate_point_to_line_packed", "line_quality_counters"):
        assert callable(getattr(I.IcpBatch, name)), name


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def test_struct_layout_matches_the_header():
    """two u64, seven doubles, nine of the matrix, two eigenvalues: 160 bytes, in the header's order"""
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    body = re.search(r"typedef struct icp_line_quality \{(.*?)\} icp_line_quality;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n) for stmt in body.split(";") if stmt.strip()
             for n in re.split(r",\s*", stmt.strip().split(None, 1)[1])]
    assert names == ["n", "inliers", "fitness", "inlier_rmse", "inlier_sum_d2", "line_rmse", "line_sum_r2", "error",
                     "huber_error", "information", "translation_eig"]
    assert names == [f[0] for f in _lib.LineQualityStruct._fields_], names
    assert C.sizeof(_lib.LineQualityStruct) == 160


def _identity():
    T = _lib.Pose()
    I.lib().icp_transform_identity(C.byref(T))
    return T


class _Handle:
    """A real 2-D handle with current line normals where there is a device; on a host without one no handle can exist
    (icp_create answers ICP_NO_DEVICE), so the entries are given a block of zeroed memory in its place: they must decide
    on their arguments, and then on the device, before they read a handle."""

    def __init__(self):
        self.h = C.c_void_p()
        self.real = I.lib().icp_device_count() > 0
        if self.real:
            dst = np.ascontiguousarray(np.random.default_rng(0).random((64, 2)))
            assert I.lib().icp_create(C.byref(self.h), 2, C.c_void_p(dst.ctypes.data), 64, -1) == _lib.OK
            assert I.lib().icp_compute_target_line_normals(self.h, 8) == _lib.OK
        else:
            self.block = (C.c_char * 65536)()
            self.h = C.c_void_p(C.addressof(self.block))

    def close(self):
        if self.real:
            I.lib().icp_destroy(self.h)


def _dirty():
    q = _lib.LineQualityStruct()
    C.memset(C.byref(q), 0x5a, C.sizeof(q))
    return q


def _is_n_and_zeros(q, n):
    raw = bytes(q)
    return q.n == n and raw[8:] == bytes(len(raw) - 8)


@pytest.mark.parametrize("entry", SINGLE)
def test_argument_errors_are_rejected_before_the_device_is_used(entry):
    f = getattr(I.lib(), entry)
    src = np.zeros((4, 2))
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
            for r in (0.0, 1.0, INF):
                out = _dirty()
                assert f(H.h, sp, 4, C.byref(T), r, C.byref(out), None) == _lib.NO_DEVICE, r
                assert _is_n_and_zeros(out, 4), r
    finally:
        H.close()


def _batch(dim=2):
    b = C.c_void_p()
    assert I.lib().icp_batch_create(C.byref(b), dim, -1) == _lib.OK  # (no device use: works without a GPU)
    return b


def _call(b, src, dst, items, k=8, r=1.0, out=True, status=True, entry=BATCH[0], count=None):
    count = len(items) if count is None else count
    arr = (_lib.BatchItem * max(len(items), 1))()
    for i, (f, n, g, m) in enumerate(items):
        arr[i].src_first, arr[i].n, arr[i].dst_first, arr[i].m = f, n, g, m
        I.lib().icp_transform_identity(C.byref(arr[i].init))
    o = (_lib.LineQualityStruct * max(count, 1))() if out else None
    st = np.zeros(max(count, 1), dtype=np.int32)
    sp = C.c_void_p(src.ctypes.data) if src is not None else None
    dp = C.c_void_p(dst.ctypes.data) if dst is not None else None
    return getattr(I.lib(), entry)(b, sp, 0 if src is None else len(src), dp, 0 if dst is None else len(dst),
                                   arr if items else None, count, k, r, o,
                                   C.c_void_p(st.ctypes.data) if status else None)


@pytest.mark.parametrize("entry", BATCH)
def test_batch_argument_errors_are_rejected_before_the_device_is_used(entry):
    src, dst = np.zeros((10, 2)), np.zeros((20, 2))
    good = [(0, 10, 0, 20), (3, 7, 0, 0), (10, 0, 20, 0)]
    b, b3 = _batch(), _batch(3)
    try:
        assert _call(b3, np.zeros((10, 3)), np.zeros((20, 3)), good, entry=entry) == _lib.BAD_ARGUMENT  # a 3-D batch
        assert _call(b3, None, None, [], count=0, entry=entry) == _lib.BAD_ARGUMENT
        for k in (2, 17, 0, -1):
            assert _call(b, src, dst, good, k=k, entry=entry) == _lib.BAD_ARGUMENT, k
        for r in (float("nan"), -1.0, float("-inf"), -1e-300):
            assert _call(b, src, dst, good, r=r, entry=entry) == _lib.BAD_ARGUMENT, r
            assert _call(b, None, None, [], r=r, count=0, entry=entry) == _lib.BAD_ARGUMENT, r
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
        assert getattr(I.lib(), entry)(None, None, 0, None, 0, None, 0, 8, 1.0, None, None) == _lib.BAD_ARGUMENT
        # count == 0 is a successful no-op whatever the other pointers are, at the ends of k and of the bound too
        for k in (3, 8, 16):
            for r in (0.0, 1.0, INF):
                assert _call(b, None, None, [], k=k, r=r, count=0, out=False, status=False, entry=entry) == _lib.OK
        if I.lib().icp_device_count() == 0:  # valid arguments reach the device check only now
            for k, r in ((8, 1.0), (3, 0.0), (16, INF)):
                assert _call(b, src, dst, good, k=k, r=r, entry=entry) == _lib.NO_DEVICE, (k, r)
        out = (C.c_uint64 * 4)(9, 9, 9, 9)
        assert getattr(I.lib(), COUNTERS)(b, out) == _lib.OK and list(out) == [0, 0, 0, 0]
        assert getattr(I.lib(), COUNTERS)(None, out) == _lib.BAD_ARGUMENT
        assert getattr(I.lib(), COUNTERS)(b, None) == _lib.BAD_ARGUMENT
    finally:
        I.lib().icp_batch_destroy(b)
        I.lib().icp_batch_destroy(b3)


# ------------------------------------------------------------------ the Python layer

def test_python_layer_refuses_before_the_library_is_reached_and_wraps_the_struct():
    icp3 = object.__new__(I.Icp3d)  # (no handle is reached: the dimension is checked first)
    icp3._h = C.c_void_p()
    with pytest.raises(ValueError):
        icp3.evaluate_point_to_line(np.zeros((3, 3)), I.Transform())
    with pytest.raises(ValueError):
        icp3.evaluate_point_to_line(np.zeros((3, 2)), I.Transform(), 1.0, return_indices=True)
    B3 = object.__new__(I.IcpBatch)  # (no batch object is reached either)
    B3.DIM, B3._b, B3._device = 3, None, None
    with pytest.raises(ValueError):
        B3.evaluate_point_to_line([np.zeros((3, 3))], [np.zeros((3, 3))], None)
    with pytest.raises(ValueError):
        B3.evaluate_point_to_line_packed(np.zeros((3, 3)), np.zeros((3, 3)), [])
    B = object.__new__(I.IcpBatch)
    B.DIM, B._b, B._device = 2, None, None
    one = ([np.zeros((3, 2))], [np.zeros((3, 2))], None)
    for k in (2, 17):
        with pytest.raises(ValueError):
            B.evaluate_point_to_line(*one, k=k)
    for r in (-1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError):
            B.evaluate_point_to_line(*one, max_correspondence_distance=r)
        with pytest.raises(ValueError):
            B.evaluate_point_to_line_packed(np.zeros((3, 2)), np.zeros((3, 2)), [(0, 3, 0, 3, I.Transform())], 8, r)
    with pytest.raises(ValueError):
        B.evaluate_point_to_line([np.zeros((3, 2))], [], None)
    with pytest.raises(ValueError):
        B.evaluate_point_to_line([np.zeros((3, 2))], [np.zeros((3, 2))], [I.Transform(), I.Transform()])
    real = I.IcpBatch(2)
    assert real.evaluate_point_to_line([], [], []) == []
    assert real.line_quality_counters() == (0, 0, 0, 0)
    real.close()
    q = _lib.LineQualityStruct()
    q.n, q.inliers = 7, 5
    q.fitness, q.inlier_rmse, q.inlier_sum_d2, q.line_rmse, q.line_sum_r2, q.error, q.huber_error = 1, 2, 3, 4, 5, 6, 7
    for k, v in enumerate([4.0, 0.0, 10.0, 0.0, 1.0, 11.0, 10.0, 11.0, 12.0]):
        q.information[k] = v
    q.translation_eig[0], q.translation_eig[1] = 1.0, 4.0
    Q = I.LineQuality(q)
    assert Q.n == 7 and Q.inliers == 5 and Q.information.shape == (3, 3) and Q.information[1, 2] == 11.0
    assert Q.as_array().tolist() == [1, 2, 3, 4, 5, 6, 7, 4, 0, 10, 0, 1, 11, 10, 11, 12, 1, 4]
    w = Q.weak_direction()  # the block is diag(4, 1): least observed along y
    assert abs(abs(w[1]) - 1.0) < 1e-15 and abs(w[0]) < 1e-15
    assert "line_rmse" in repr(Q)


def test_scan2d_scores_each_frame_after_its_estimate_with_the_right_scorer_and_only_when_asked():
    from icp_rust_amd import harness

    log = []

    class Fake:
        def __init__(self, dst):
            log.append(("new", len(dst)))

        def estimate(self, src, T, max_iter):
            log.append(("estimate", max_iter))
            return I.Transform([0.1, 0.0, 0.0]) * T

        def compute_line_normals(self, k):
            log.append(("compute_line_normals", k))

        def estimate_point_to_line(self, src, T, max_iter):
            log.append(("estimate_point_to_line", max_iter))
            return I.Transform([0.1, 0.0, 0.0]) * T

        def evaluate(self, src, T, r):
            log.append(("evaluate", len(src), T.as_array().copy(), r))
            return "q%d" % len(log)

        def evaluate_point_to_line(self, src, T, r):
            log.append(("evaluate_point_to_line", len(src), T.as_array().copy(), r))
            return "lq%d" % len(log)

    class NoEvaluate(Fake):
        evaluate = None  # (a factory without the evaluations keeps working when no list is given)
        evaluate_point_to_line = None

    n1 = len(load_golden(1))
    # the defaults call neither, with either residual, and return what they returned
    Ts0, inv0, path0 = harness.run_scan2d(GOLDEN, max_iter=3, icp_factory=NoEvaluate, max_frames=3)
    assert [e[0] for e in log] == ["new", "estimate"] * 3
    del log[:]
    harness.run_scan2d(GOLDEN, max_iter=3, icp_factory=NoEvaluate, max_frames=3, point_to_line=7, quality_distance=0.5)
    assert [e[0] for e in log] == ["new", "compute_line_normals", "estimate_point_to_line"] * 3
    del log[:]
    # point-to-line: new -> normals -> estimate -> evaluate_point_to_line at the estimated pose, once per frame
    got = []
    Ts, inv, path = harness.run_scan2d(GOLDEN, max_iter=3, icp_factory=Fake, max_frames=3, point_to_line=7, qualities=got,
                                       quality_distance=0.5)
    assert [e[0] for e in log] == ["new", "compute_line_normals", "estimate_point_to_line", "evaluate_point_to_line"] * 3
    evs = [e for e in log if e[0] == "evaluate_point_to_line"]
    assert got == ["lq4", "lq8", "lq12"]
    for T, e in zip(Ts, evs):
        assert np.array_equal(e[2], T.as_array()) and e[3] == 0.5 and e[1] == n1
    assert np.array_equal(path, path0) and all(np.array_equal(a.as_array(), b.as_array()) for a, b in zip(Ts, Ts0))
    del log[:]
    # point-to-point: evaluate, with +inf when no distance is given
    got = []
    harness.run_scan2d(GOLDEN, max_iter=3, icp_factory=Fake, max_frames=2, qualities=got)
    assert [e[0] for e in log] == ["new", "estimate", "evaluate"] * 2
    assert all(e[3] == INF for e in log if e[0] == "evaluate") and got == ["q3", "q6"]


# ------------------------------------------------------------------ the definition, restated, and what it is for

def scene_fields(dst):
    nrm = line_normals_numpy(dst, SCENE_K)
    src, T = scene_scan(dst)
    rc, cnt, f = restate(dst, nrm, src, T, 0.5, nearest(dst, moved2(src, T)))
    assert rc == _lib.OK
    return nrm, len(src), cnt, f


def test_a_corridor_is_not_observed_along_its_axis():
    """walls y = const: a[0][1] == 0 and a[1][1] == 0 exactly, so every normal is (0, 1) to the bit, the translation
    block is diag(0, inliers): lmin = 0.0 exactly, lmax = 134, and the weak direction is the x axis"""
    nrm, n, cnt, f = scene_fields(corridor())
    assert np.array_equal(nrm, np.tile([0.0, 1.0], (len(nrm), 1)))
    lmin, lmax = f[16], f[17]
    w = weak_direction(f)
    print("corridor: inliers", cnt, "of", n, "lmin", lmin, "lmax", lmax, "weak", w, "line_rmse", f[3])
    assert cnt == n == 134 and lmin == 0.0 and lmax == 134.0
    assert lmin / lmax <= 1e-6
    assert abs(w[0]) >= 0.999


def test_a_room_is_observed_in_both_directions():
    """the end walls x = +-10 carry normals (1, 0): lmin / lmax = 27.04 / 132.96 = 0.2034, far above 1e-2"""
    nrm, n, cnt, f = scene_fields(closed_room())
    lmin, lmax = f[16], f[17]
    print("room: inliers", cnt, "of", n, "lmin", lmin, "lmax", lmax, "ratio", lmin / lmax)
    assert cnt == n
    assert lmin / lmax >= 1e-2
    assert abs(lmin / lmax - 0.2034) < 5e-4  # (the figure this bar was set from)


@pytest.mark.parametrize("seed,m,n", SEEDS)
def test_line_rmse_is_the_sensor_noise_where_point_rmse_is_the_sample_spacing(seed, m, n):
    """independent samples of the same walls (2 mm noise) at the true pose: the line RMSE is the noise, the point RMSE
    moves with the sampling density (measured ratios: 0.42, 0.30, 0.58)"""
    dst, src, Tt = outline_pair(seed, m, n)
    nrm = line_normals_numpy(dst, SCENE_K)
    rc, cnt, f = restate(dst, nrm, src, Tt, INF, nearest(dst, moved2(src, Tt)))
    assert rc == _lib.OK and cnt == n
    point_rmse, line_rmse = f[1], f[3]
    print(f"seed {seed}: line_rmse {line_rmse:.3g}, point rmse {point_rmse:.3g}, ratio {line_rmse / point_rmse:.3g}")
    assert line_rmse < 0.6 * point_rmse
    assert line_rmse <= 3e-3


def test_restated_fold_and_terms_on_values_known_by_hand():
    """n == 1 keeps the one value (a -0.0 stays); 257 ones are 256 + 1 in the second level; a non-inlier adds zeros"""
    assert np.signbit(fold([-0.0])) and fold(np.ones(257)) == 257.0 and fold([]) == 0.0
    dst = np.array([[0.0, 0.0], [4.0, 0.0]])
    nrm = np.array([[0.0, 1.0], [1.0, 0.0]])
    src = np.array([[0.5, 0.25], [3.0, 2.0]])
    rc, cnt, f = restate(dst, nrm, src, I.Transform(), 1.0, [0, 1])
    # point 0: d2 = 0.3125 (inlier), rp = 0.25, c = 0.5; point 1: d2 = 5 (not an inlier), rp = -1, c = -2
    assert rc == _lib.OK and cnt == 1
    assert f.tolist() == [0.5, np.sqrt(0.3125), 0.3125, 0.25, 0.0625, 1.0625, 1.0625, 0.0, 0.0, 0.0, 0.0, 1.0, 0.5, 0.0,
                          0.5, 0.25, 0.0, 1.0]
    bad = src.copy()
    bad[1, 0] = np.nan
    assert restate(dst, nrm, bad, I.Transform(), 1.0, [0, 1])[0] == _lib.NAN_INPUT


# ------------------------------------------------------------------ the kernels' resources

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
def test_line_quality_kernels_cross_compile_within_their_budgets():
    """exactly the three kernels of quality_line.hip.  k_line_quality_terms and the fold level: no scratch, at most 128
    VGPRs.  k_line_quality_batch (1024 threads: 128 registers per thread at most): at most 96 bytes per lane of scratch,
    the cap the other 1024-thread kernels are held to (it compiles to 0), and no static LDS on top of the dynamic plan.
    The names stay clear of the budgeted search / evaluation kernels (tests/test_registers.py)."""
    from test_registers import BUDGET

    use = _usage("quality_line.hip")
    for frag in ("k_line_quality_terms", "k_line_quality_batch", "k_fold_levelILi10E"):
        assert len([k for k in use if frag in k]) == 1, (frag, list(use))
    assert len(use) == 3, list(use)
    for k, u in use.items():
        print(k, u)
        assert not any(frag in k for frag in BUDGET), k
        assert u["vgpr"] <= 128, (k, u)
        if "k_line_quality_batch" in k:
            assert u["scratch"] <= 96 and u["lds"] == 0, (k, u)
        else:
            assert u["scratch"] == 0, (k, u)
