"""CPU-side checks of the point-to-line registration for 2-D handles (include/icp_mi355x.h section 14): the five families
of entries are declared, exported and bound; ABI version still 8; argument errors are rejected before the device is
touched; the Python layer (Icp3d's refusal, the bound of a gated call); run_scan2d calls the new methods only when asked;
a numpy restatement of the line-normal definition (imported by tests/test_gpu_line.py); the CPU statement of the
estimator -- the oracle's point-to-plane estimate fed lifted clouds [x, y, 0] and normals [nx, ny, 0] -- on a room
outline and on a single wall; the new kernels' register and scratch use."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NORMALS = ("icp_compute_target_line_normals", "icp_update_target_line_normals", "icp_read_target_line_normals")
UNGATED = ("icp_estimate_point_to_line", "icp_estimate_point_to_line_device")
GATED = ("icp_estimate_point_to_line_gated", "icp_estimate_point_to_line_gated_device")
TOO_MANY = 0xffffffff  # n >= 2^32 - 1 is refused
GOLDEN = os.path.join(ROOT, "tests", "golden", "scans2d")
TRUE_PARAM = (0.03, -0.02, 0.01)  # the pose the synthetic scans are moved by
GOLDEN_K = 8  # the neighbourhood size the golden scans are registered with
SEEDS = ((5, 3000, 1500), (6, 2000, 700), (7, 6000, 2500))  # seed, targets, scan points


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


# ------------------------------------------------------------------ shared with tests/test_gpu_line.py

def lift(a):
    """[x, y] -> [x, y, 0]: the oracle's 3-D statement sees a 2-D cloud in the plane z = 0"""
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([a, np.zeros((len(a), 1))], axis=1))


def moved2(p, T):
    """Transform::transform on every row, each operation rounded on its own"""
    r00, r10, r01, r11, tx, ty = T.pose.as_tuple()
    q = np.empty_like(p)
    q[:, 0] = (r00 * p[:, 0] + r01 * p[:, 1]) + tx
    q[:, 1] = (r10 * p[:, 0] + r11 * p[:, 1]) + ty
    return q


def outline(rng, m, noise=2e-3):
    """m samples of the outline of a room: the walls of [-3, 3] x [-2, 2] and a partition from (0, -2) to (0, 0.5), drawn
    uniformly along their length, moved off the wall by N(0, noise).  Two draws with different generators share no
    point: independent samples of the same walls."""
    segs = np.array([[-3, -2, 3, -2], [3, -2, 3, 2], [3, 2, -3, 2], [-3, 2, -3, -2], [0, -2, 0, 0.5]], dtype=np.float64)
    d = segs[:, 2:] - segs[:, :2]
    length = np.hypot(d[:, 0], d[:, 1])
    which = rng.choice(len(segs), size=m, p=length / length.sum())
    t = rng.random(m)
    off = rng.normal(0.0, noise, m)
    nrm = np.stack([-d[:, 1], d[:, 0]], axis=1) / length[:, None]
    return np.ascontiguousarray(segs[which, :2] + t[:, None] * d[which] + off[:, None] * nrm[which])


def outline_pair(seed, m, n):
    """(targets, scan moved by the inverse of the true pose, true pose)"""
    dst = outline(np.random.default_rng(seed), m)
    scan = outline(np.random.default_rng(1000 + seed), n)
    Tt = I.Transform(list(TRUE_PARAM))
    return dst, np.ascontiguousarray(moved2(scan, Tt.inverse())), Tt


def line_normals_numpy(dst, k, rows=None):
    """The definition of include/icp_mi355x.h section 14 in numpy, every operation rounded on its own and in the
    documented order, for the targets `rows` (default: all).  Brute-force neighbours, ordered by (d2, index)."""
    dst = np.ascontiguousarray(dst, dtype=np.float64)
    m = len(dst)
    rows = np.arange(m) if rows is None else np.asarray(rows)
    out = np.zeros((len(rows), 2))
    kk = min(int(k), m)
    if kk < 3:
        return out
    for lo in range(0, len(rows), 512):
        r = rows[lo:lo + 512]
        dx = dst[r, 0][:, None] - dst[None, :, 0]
        dy = dst[r, 1][:, None] - dst[None, :, 1]
        d2 = dx * dx + dy * dy
        nb = np.argsort(d2, axis=1, kind="stable")[:, :kk]  # (stable: equal d2 in index order)
        p = dst[nb]  # (rows, kk, 2)
        mean = np.zeros((len(r), 2))
        for j in range(kk):
            mean = mean + p[:, j]
        mean = mean / float(kk)
        a = np.zeros((len(r), 2, 2))
        for j in range(kk):
            e = p[:, j] - mean
            for s in range(2):
                for t in range(2):
                    a[:, s, t] = a[:, s, t] + e[:, s] * e[:, t]
        v = np.zeros((len(r), 2, 2))
        v[:, 0, 0] = v[:, 1, 1] = 1.0
        rot = a[:, 0, 1] != 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            theta = (a[:, 1, 1] - a[:, 0, 0]) / (2.0 * a[:, 0, 1])
            t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        ar, vr = a.copy(), v.copy()
        for q in range(2):  # A <- A J
            a0, a1 = ar[:, q, 0].copy(), ar[:, q, 1].copy()
            ar[:, q, 0] = c * a0 - s * a1
            ar[:, q, 1] = s * a0 + c * a1
        for q in range(2):  # A <- J^T A
            a0, a1 = ar[:, 0, q].copy(), ar[:, 1, q].copy()
            ar[:, 0, q] = c * a0 - s * a1
            ar[:, 1, q] = s * a0 + c * a1
        for q in range(2):
            v0, v1 = vr[:, q, 0].copy(), vr[:, q, 1].copy()
            vr[:, q, 0] = c * v0 - s * v1
            vr[:, q, 1] = s * v0 + c * v1
        a = np.where(rot[:, None, None], ar, a)
        v = np.where(rot[:, None, None], vr, v)
        col = np.where(a[:, 1, 1] < a[:, 0, 0], 1, 0)
        n0 = v[np.arange(len(r)), 0, col]
        n1 = v[np.arange(len(r)), 1, col]
        length = np.sqrt(n0 * n0 + n1 * n1)
        ok = length > 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            n0, n1 = n0 / length, n1 / length
        lead = np.where(n1 != 0.0, n1, n0)
        flip = lead < 0.0
        n0, n1 = np.where(flip, -n0, n0), np.where(flip, -n1, n1)
        out[lo:lo + 512, 0] = np.where(ok, n0, 0.0)
        out[lo:lo + 512, 1] = np.where(ok, n1, 0.0)
    return out


def oracle_point_to_line(dst, normals, src, init, max_iter):
    """the CPU statement of the estimator: (rc, pose, indices, inner counts)"""
    return O.p2pl_estimate(O.KdTree(lift(dst)), lift(normals), lift(src), O.Pose(*init.pose.as_tuple()), max_iter)


def pose_error(T, Tt):
    return float(np.max(np.abs(np.asarray(T.as_array()) - np.asarray(Tt.as_array()))))


def load_golden(k):
    from icp_rust_amd.scans import load_scan2d

    return np.ascontiguousarray(load_scan2d(os.path.join(GOLDEN, f"{k:03d}.txt")))


# ------------------------------------------------------------------ the boundary

def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(icp_[a-z0-9_]+)\s*\(", text))


def test_symbols_are_declared_exported_and_bound():
    public = declared("icp_mi355x.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in NORMALS + UNGATED + GATED:
        assert s in public, s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    mk = open(os.path.join(ROOT, "icp_rust_amd", "csrc", "Makefile")).read()
    assert "p2plane.hip" in mk and "gate_plane.hip" in mk and "api_normal.hip" in mk
    for name in ("compute_line_normals", "update_line_normals", "read_line_normals", "estimate_point_to_line"):
        assert callable(getattr(I.Icp2d, name)), name


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


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


def test_argument_errors_are_rejected_before_the_device_is_used():
    L = I.lib()
    src = np.zeros((4, 2))
    sp = C.c_void_p(src.ctypes.data)
    T, out = _identity(), _lib.Pose()
    H = _Handle()
    try:
        for name in NORMALS[:2]:
            f = getattr(L, name)
            assert f(None, 8) == _lib.BAD_ARGUMENT
            for k in (2, 17, 0, -1):
                assert f(H.h, k) == _lib.BAD_ARGUMENT, (name, k)
            if not H.real:
                assert f(H.h, 8) == _lib.NO_DEVICE
        buf = np.zeros((4, 2))
        assert L.icp_read_target_line_normals(None, 0, 4, C.c_void_p(buf.ctypes.data)) == _lib.BAD_ARGUMENT
        assert L.icp_read_target_line_normals(H.h, 0, 4, None) == _lib.BAD_ARGUMENT
        if not H.real:
            assert L.icp_read_target_line_normals(H.h, 0, 4, C.c_void_p(buf.ctypes.data)) == _lib.NO_DEVICE
        for name in UNGATED:
            f = getattr(L, name)
            assert f(None, sp, 4, C.byref(T), 1, C.byref(out), None, None) == _lib.BAD_ARGUMENT
            assert f(H.h, None, 4, C.byref(T), 1, C.byref(out), None, None) == _lib.BAD_ARGUMENT
            assert f(H.h, sp, 4, None, 1, C.byref(out), None, None) == _lib.BAD_ARGUMENT
            assert f(H.h, sp, 4, C.byref(T), 1, None, None, None) == _lib.BAD_ARGUMENT
            assert f(H.h, sp, TOO_MANY, C.byref(T), 1, C.byref(out), None, None) == _lib.BAD_ARGUMENT
            if not H.real:
                assert f(H.h, sp, 4, C.byref(T), 1, C.byref(out), None, None) == _lib.NO_DEVICE
        for name in GATED:
            f = getattr(L, name)
            for r in (float("nan"), -1.0, float("-inf"), -1e-300):
                assert f(H.h, sp, 4, C.byref(T), 1, r, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT, (name, r)
            assert f(None, sp, 4, C.byref(T), 1, 1.0, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT
            assert f(H.h, None, 4, C.byref(T), 1, 1.0, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT
            assert f(H.h, sp, 4, None, 1, 1.0, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT
            assert f(H.h, sp, 4, C.byref(T), 1, 1.0, None, None, None, None) == _lib.BAD_ARGUMENT
            assert f(H.h, sp, TOO_MANY, C.byref(T), 1, 1.0, C.byref(out), None, None, None) == _lib.BAD_ARGUMENT
            if not H.real:  # valid arguments reach the device check only now; 0 and +inf are valid bounds
                for r in (0.0, 1.0, float("inf")):
                    assert f(H.h, sp, 4, C.byref(T), 1, r, C.byref(out), None, None, None) == _lib.NO_DEVICE, (name, r)
    finally:
        H.close()


def test_python_layer_refuses_a_3d_handle_and_a_bad_bound_before_the_library():
    icp3 = object.__new__(I.Icp3d)  # (no handle is reached: the dimension is checked first)
    icp3._h = C.c_void_p()
    with pytest.raises(ValueError):
        icp3.compute_line_normals(8)
    with pytest.raises(ValueError):
        icp3.update_line_normals(8)
    with pytest.raises(ValueError):
        icp3.read_line_normals(0, 1)
    with pytest.raises(ValueError):
        icp3.estimate_point_to_line(np.zeros((3, 3)), I.Transform(), 1)
    with pytest.raises(ValueError):
        icp3.estimate_point_to_line(np.zeros((3, 3)), I.Transform(), 1, max_correspondence_distance=1.0)
    icp2 = object.__new__(I.Icp2d)  # (the bound is checked before the handle is used)
    icp2._h = C.c_void_p()
    for r in (-1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError):
            icp2.estimate_point_to_line(np.zeros((3, 2)), I.Transform(), 1, max_correspondence_distance=r)
        with pytest.raises(ValueError):
            icp2.estimate_point_to_line(np.zeros((3, 2)), I.Transform(), 1, return_info=True,
                                        max_correspondence_distance=r)


def test_scan2d_uses_the_line_residual_only_when_asked():
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

    class Plain(Fake):
        compute_line_normals = None  # (a factory without the extension keeps working when it is not asked for)
        estimate_point_to_line = None

    Ts0, inv0, path0 = harness.run_scan2d(GOLDEN, max_iter=3, icp_factory=Plain, max_frames=3)
    assert [e[0] for e in log] == ["new", "estimate"] * 3
    del log[:]
    Ts, inv, path = harness.run_scan2d(GOLDEN, max_iter=3, icp_factory=Fake, max_frames=3, point_to_line=7)
    want = []
    for k in (2, 3, 4):  # (001 is the fixed source; every later frame: a new handle, its normals, the line estimate)
        want += [("new", len(load_golden(k))), ("compute_line_normals", 7), ("estimate_point_to_line", 3)]
    assert log == want
    assert np.array_equal(path, path0) and len(Ts) == len(Ts0) == 3
    del log[:]
    harness.run_scan2d(GOLDEN, max_iter=3, icp_factory=Fake, max_frames=2)  # (the default, with a factory that has both)
    assert [e[0] for e in log] == ["new", "estimate"] * 2
    ap_help = subprocess.run([shutil.which("python") or "python", "-m", "icp_rust_amd.harness", "--help"], cwd=ROOT,
                             capture_output=True, text=True, timeout=300)
    assert ap_help.returncode == 0 and "--point-to-line" in ap_help.stdout


# ------------------------------------------------------------------ the definition, restated

def test_restated_normals_on_a_vertical_line_a_diagonal_and_too_few_points():
    rng = np.random.default_rng(1)
    y = rng.uniform(-1, 1, 40)
    n = line_normals_numpy(np.stack([np.full(40, 3.0), y], axis=1), 5)
    assert np.array_equal(n, np.tile([1.0, 0.0], (40, 1)))  # exactly: a[0][1] == 0, no rotation, column 0
    x = rng.uniform(-1, 1, 40)
    n = line_normals_numpy(np.stack([x, -x], axis=1), 6)
    assert np.max(np.abs(n - np.ones(2) / np.sqrt(2.0))) < 1e-12  # the first non-zero of (n_y, n_x) is positive
    assert np.max(np.abs(np.hypot(n[:, 0], n[:, 1]) - 1.0)) < 1e-12
    assert np.array_equal(line_normals_numpy(np.array([[0.0, 0.0], [1.0, 2.0]]), 3), np.zeros((2, 2)))
    # coincident points: a zero covariance, no rotation, and the tie of the diagonals takes column 0
    assert np.array_equal(line_normals_numpy(np.array([[1.0, 1.0]] * 5), 4), np.tile([1.0, 0.0], (5, 1)))


# ------------------------------------------------------------------ the CPU statement of the estimator

@pytest.fixture(scope="module")
def threads():
    O.set_threads(16)
    yield
    O.set_threads(1)


@pytest.mark.parametrize("seed,m,n", SEEDS)
def test_cpu_statement_on_independent_samples_beats_point_to_point(threads, seed, m, n):
    """scan and target are independent samples of the same walls (2 mm noise): the pairs differ along the wall by up to
    the sample spacing, which the line residual does not see.  Bound: 2e-3, the noise scale."""
    dst, src, Tt = outline_pair(seed, m, n)
    normals = line_normals_numpy(dst, 10)
    rc, T, _, inner = oracle_point_to_line(dst, normals, src, I.Transform(), 6)
    assert rc == O.OK and inner.sum() > 0
    rc, Tq, _, _ = O.icp_estimate(2, dst, src, O.transform_identity(), 6, use_kdtree=True)
    assert rc == O.OK
    ep, eq = pose_error(T, Tt), pose_error(Tq, Tt)
    print(f"seed {seed}: point-to-line {ep:.3g}, point-to-point {eq:.3g}")
    assert ep < 2e-3 and ep < eq, (ep, eq)


def test_cpu_statement_returns_the_identity_on_a_single_wall():
    """every normal is (1, 0): y and theta are unobserved, the normal equations are exactly singular and no update is
    produced at all"""
    rng = np.random.default_rng(9)
    wall = np.ascontiguousarray(np.stack([np.full(800, 3.0), rng.uniform(-3, 3, 800)], axis=1))
    src = wall[rng.integers(0, 800, 300)].copy()
    src[:, 0] += rng.normal(-0.02, 2e-3, 300)
    normals = line_normals_numpy(wall, 8)
    assert np.array_equal(normals, np.tile([1.0, 0.0], (800, 1)))
    rc, T, _, inner = oracle_point_to_line(wall, normals, src, I.Transform(), 3)
    assert rc == O.OK and inner.tolist() == [0, 0, 0]
    assert np.array_equal(T.as_array(), O.transform_identity().as_array())


def test_cpu_statement_on_the_golden_scans_gives_the_documented_inner_counts(threads):
    src = load_golden(1)
    # (the poses: the left fold's bits, recorded before one update became orc_p2pl_update)
    bits = {2: [0x3feffff9eaca0d20, 0xbf63bb11cece1558, 0x3f63bb11cece1558, 0x3feffff9eaca0d20, 0xbfd8d0227359d12a,
                0xbfdbfde9d6520519],
            10: [0x3feffff9875e0687, 0xbf6459d2050cbf77, 0x3f6459d2050cbf77, 0x3feffff9875e0687, 0xbfe3c7e1054a9e52,
                 0x3fcb5bb17c1fce82]}
    for k, want in ((2, [8, 5, 3]), (10, [8, 5, 4, 1])):
        dst = load_golden(k)
        rc, T, _, inner = oracle_point_to_line(dst, line_normals_numpy(dst, GOLDEN_K), src, I.Transform(), 20)
        assert rc == O.OK
        assert inner.tolist() == want + [0] * (20 - len(want)), (k, inner.tolist())
        assert T.as_array().view(np.uint64).tolist() == bits[k], k


# ------------------------------------------------------------------ the kernels' resources

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


# (VGPRs, scratch bytes per lane) of the 2-D kernels as the build reported them while each had a body of its own in
# p2line.hip, before csrc/normal_single_device.hpp put one body behind them and their 3-D twins
LINE_KERNELS_BEFORE_SHARING = {
    "p2plane.hip": {"k_line_normals": (54, 0), "k_line_gather": (22, 0)},
    "gate_plane.hip": {"k_lngate_stage": (72, 0)},
}
# every kernel of the two translation units the 2-D kernels live in, beside their 3-D twins
KERNELS = {
    "p2plane.hip": ("k_line_normals", "k_line_gather", "k_target_normals", "k_p2pl_gather", "k_p2pl_residual",
                    "k_p2pl_accumulate"),
    "gate_plane.hip": ("k_lngate_stage", "k_plgate_stage", "k_compact_chunks", "k_plgate_place"),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_line_kernels_do_not_spill_and_leave_room_for_four_waves_per_simd():
    """exactly the kernels of p2plane.hip and gate_plane.hip, which hold the 2-D kernels beside their 3-D twins; no
    scratch and at most 128 VGPRs in each; the 2-D kernels need no more than before they shared a body with the twins; the
    names stay clear of the budgeted search / evaluation kernels (tests/test_registers.py) and of the fragments the other
    file's kernels are counted by"""
    from test_registers import BUDGET

    for src, frags in KERNELS.items():
        regs = _usage(src)
        kernels = [k for k in regs if not k.endswith("#scratch")]
        for frag in frags:
            assert len([k for k in kernels if frag in k]) == 1, (frag, kernels)
        assert len(kernels) == len(frags), kernels
        others = [f for other, fs in KERNELS.items() if other != src for f in fs if f not in frags]
        for k in kernels:
            assert regs.get(k + "#scratch", 0) == 0, (k, regs.get(k + "#scratch"))
            assert regs[k] <= 128, (k, regs[k])
            assert not any(frag in k for frag in BUDGET), k
            assert not any(frag in k for frag in others + ["k_gate_stage"]), k
        for frag, (vgprs, scratch) in LINE_KERNELS_BEFORE_SHARING[src].items():
            name = [k for k in kernels if frag in k][0]
            assert regs[name] <= vgprs, f"{name}: {regs[name]} VGPRs > {vgprs}"
            assert regs.get(name + "#scratch", 0) <= scratch, f"{name}: scratch"
