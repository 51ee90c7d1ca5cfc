"""CPU-side checks of the batched point-to-plane pose quality (icp_batch_evaluate_point_to_plane[_device],
include/icp_mi355x.h section 20): declared, exported and bound, the counters and the LDS plan's accessor in the debug
header; ABI version still 8; every argument error -- a 2-D batch, k outside [3, 16], a bad bound, null outputs, a range
outside the packed arrays -- rejected before the device is touched, count == 0 a successful no-op; the Python layer's
refusals and return shapes (with a library that is not the real one); the LDS plan at its corners and its invariants at
every m (DESIGN.md section 9o derives the figures); the kernel's cross-compile for gfx950 within the budget of the
1024-thread kernels, and the four instantiations of p2plane_batch.hip within theirs now that the normals' rounds live in
one header for the line and the plane kernels (normal_batch_device.hpp); and what the call is for, on the CPU: 64 hypotheses of a thinned corridor and of a closed room
(imported by tests/test_gpu_plane_quality_batch.py), scored by the numpy restatement with the oracle's normals."""
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
NEW = ("icp_batch_evaluate_point_to_plane", "icp_batch_evaluate_point_to_plane_device")
DEBUG = ("icp_batch_plane_quality_counters", "icp_debug_plane_quality_batch_plan")
GRANT = 160 * 1024 - 256  # the dynamic LDS a one-workgroup kernel asks for (163 584 bytes)
FOLD = 10 * 256 * 8 + 256 * 8 + 256 * 4 + 4 * 96  # FoldLds<10> and the four group records: 23 936 bytes
INF = float("inf")


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
        assert s in public and s in _lib.SIGNATURES and hasattr(L, s) and hasattr(I.lib(), s), s
    for s in DEBUG:
        assert s in debug and s not in public and s in _lib.SIGNATURES and hasattr(L, s), s
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "quality_plane_batch.hip" in mk and "p2plane_device.hpp" in mk
    for name in ("evaluate_point_to_plane", "evaluate_point_to_plane_packed", "plane_quality_counters"):
        assert callable(getattr(I.IcpBatch, name)), name


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


# ------------------------------------------------------------------ the boundary

def _batch(dim=3):
    b = C.c_void_p()
    assert I.lib().icp_batch_create(C.byref(b), dim, -1) == _lib.OK  # (no device use: works without a GPU)
    return b


def _call(b, src, dst, items, k=8, r=1.0, out=True, status=True, entry=NEW[0], count=None):
    count = len(items) if count is None else count
    arr = (_lib.BatchItem * max(len(items), 1))()
    for i, (f, n, g, m) in enumerate(items):
        arr[i].src_first, arr[i].n, arr[i].dst_first, arr[i].m = f, n, g, m
        I.lib().icp_transform_identity(C.byref(arr[i].init))
    o = (_lib.PlaneQualityStruct * max(count, 1))() if out else None
    st = np.zeros(max(count, 1), dtype=np.int32)
    sp = C.c_void_p(src.ctypes.data) if src is not None else None
    dp = C.c_void_p(dst.ctypes.data) if dst is not None else None
    return getattr(I.lib(), entry)(b, sp, 0 if src is None else len(src), dp, 0 if dst is None else len(dst),
                                   arr if items else None, count, k, r, o,
                                   C.c_void_p(st.ctypes.data) if status else None)


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
        # null clouds with points claimed
        arr = (_lib.BatchItem * 1)()
        o, st = (_lib.PlaneQualityStruct * 1)(), np.zeros(1, dtype=np.int32)
        assert getattr(I.lib(), entry)(b, None, 10, C.c_void_p(dst.ctypes.data), 20, arr, 1, 8, 1.0, o,
                                       C.c_void_p(st.ctypes.data)) == _lib.BAD_ARGUMENT
        assert getattr(I.lib(), entry)(b, C.c_void_p(src.ctypes.data), 10, None, 20, arr, 1, 8, 1.0, o,
                                       C.c_void_p(st.ctypes.data)) == _lib.BAD_ARGUMENT
        # count == 0 is a successful no-op whatever the other pointers are, at the ends of k and of the bound too
        for k in (3, 8, 16):
            for r in (0.0, 1.0, INF):
                assert _call(b, None, None, [], k=k, r=r, count=0, out=False, status=False, entry=entry) == _lib.OK
        if I.lib().icp_device_count() == 0:  # valid arguments reach the device check only now
            for k, r in ((8, 1.0), (3, 0.0), (16, INF)):
                assert _call(b, src, dst, good, k=k, r=r, entry=entry) == _lib.NO_DEVICE, (k, r)
        out = (C.c_uint64 * 4)(9, 9, 9, 9)
        assert I.lib().icp_batch_plane_quality_counters(b, out) == _lib.OK and list(out) == [0, 0, 0, 0]
        assert I.lib().icp_batch_plane_quality_counters(None, out) == _lib.BAD_ARGUMENT
        assert I.lib().icp_batch_plane_quality_counters(b, None) == _lib.BAD_ARGUMENT
        for name in ("icp_batch_line_quality_counters", "icp_batch_plane_counters", "icp_batch_plane_gated_counters"):
            assert getattr(I.lib(), name)(b, out) == _lib.OK and list(out) == [0, 0, 0, 0], name  # (no other counter moved)
    finally:
        I.lib().icp_batch_destroy(b)
        I.lib().icp_batch_destroy(b2)


# ------------------------------------------------------------------ the Python layer

def test_python_layer_refuses_before_the_library_is_reached():
    B2 = object.__new__(I.IcpBatch)  # (no batch object is reached: the dimension is checked first)
    B2.DIM, B2._b, B2._device = 2, None, None
    with pytest.raises(ValueError):
        B2.evaluate_point_to_plane([np.zeros((3, 2))], [np.zeros((3, 2))], None)
    with pytest.raises(ValueError):
        B2.evaluate_point_to_plane_packed(np.zeros((3, 2)), np.zeros((3, 2)), [])
    B = object.__new__(I.IcpBatch)
    B.DIM, B._b, B._device = 3, None, None
    one = ([np.zeros((3, 3))], [np.zeros((3, 3))], None)
    for k in (2, 17):
        with pytest.raises(ValueError):
            B.evaluate_point_to_plane(*one, k=k)
    for r in (-1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError):
            B.evaluate_point_to_plane(*one, max_correspondence_distance=r)
        with pytest.raises(ValueError):
            B.evaluate_point_to_plane_packed(np.zeros((3, 3)), np.zeros((3, 3)), [(0, 3, 0, 3, I.Transform())], 8, r)
    with pytest.raises(ValueError):
        B.evaluate_point_to_plane([np.zeros((3, 3))], [], None)
    with pytest.raises(ValueError):
        B.evaluate_point_to_plane([np.zeros((3, 3))], [np.zeros((3, 3))], [I.Transform(), I.Transform()])
    real = I.IcpBatch(3)
    assert real.evaluate_point_to_plane([], [], []) == []
    assert real.plane_quality_counters() == (0, 0, 0, 0)
    assert real.plane_counters() == (0, 0, 0, 0) and real.evaluate_counters() == (0, 0, 0)
    real.close()


class _FakeLib:
    """Stands in for the library: records the host entry's arguments, answers item i with n = its n, inliers = i,
    plane_rmse = i + 0.5 and the statuses handed to it."""

    def __init__(self, statuses):
        self.statuses, self.calls, self.real = statuses, [], I.lib()

    def __getattr__(self, name):  # (the host-only pose algebra stays the library's)
        return getattr(self.real, name)

    def icp_batch_evaluate_point_to_plane(self, b, src, src_points, dst, dst_points, arr, count, k, r, out, status):
        self.calls.append((src_points, dst_points, count, k, r))
        st = np.ctypeslib.as_array(C.cast(status, C.POINTER(C.c_int32)), shape=(count,))
        st[:] = self.statuses[:count]
        for i in range(count):
            out[i].n, out[i].inliers, out[i].plane_rmse = int(arr[i].n), i, i + 0.5
        return _lib.OK


def test_python_return_shapes_with_a_fake_library(monkeypatch):
    fake = _FakeLib([_lib.OK, _lib.NAN_INPUT, _lib.OK])
    monkeypatch.setattr(api_module, "lib", lambda: fake)
    B = object.__new__(I.IcpBatch)
    B.DIM, B._b, B._device = 3, C.c_void_p(), None
    srcs = [np.zeros((4, 3)), np.ones((2, 3)), np.zeros((0, 3))]
    dsts = [np.zeros((5, 3)), np.ones((6, 3)), np.ones((3, 3))]
    qs, status = B.evaluate_point_to_plane(srcs, dsts, None, k=5, max_correspondence_distance=0.25, allow_failures=True,
                                           return_status=True)
    assert fake.calls == [(6, 14, 3, 5, 0.25)]
    assert [q is None for q in qs] == [False, True, False] and status.tolist() == [0, _lib.NAN_INPUT, 0]
    assert isinstance(qs[0], I.PlaneQuality) and qs[0].n == 4 and qs[2].n == 0 and qs[2].inliers == 2
    assert qs[2].plane_rmse == 2.5 and qs[0].as_array().shape == (18,)
    with pytest.raises(I.IcpError, match="item 1"):
        B.evaluate_point_to_plane(srcs, dsts, None, k=5)
    fake.statuses = [_lib.OK] * 3
    qs = B.evaluate_point_to_plane_packed(np.zeros((4, 3)), np.zeros((9, 3)), [(0, 4, 0, 9, I.Transform())] * 3)
    assert len(qs) == 3 and all(isinstance(q, I.PlaneQuality) for q in qs)
    assert fake.calls[-1] == (4, 9, 3, 10, INF)  # (k defaults to 10, the bound to +inf)
    B._b = None  # (nothing to destroy)


# ------------------------------------------------------------------ the LDS plan

def _plan(m):
    out = (C.c_uint32 * 4)()
    assert I.lib().icp_debug_plane_quality_batch_plan(m, out) == _lib.OK
    return tuple(out)  # lists per round, shared bytes, fixed bytes, dynamic LDS


def _keys(m):
    keys = 64
    while keys < m:
        keys *= 2
    return 8 * keys


def test_lds_plan_at_its_corners_and_its_invariants_at_every_m():
    """the figures DESIGN.md section 9o derives: with mp = m rounded up to 64, fixed = 24 mp (x | y | z) + 16 (mp + 4)
    (screen records) + 24 mp (normals) + 256 (control words); the shared region holds in turn the sort keys (8 B x next
    power of two of m), the lists (192 B each, a multiple of 64 of them) and the fold (23 936 B)"""
    assert FOLD == 23936
    assert _plan(1) == (64, FOLD, 4416, 28352)  # the fold sizes the region
    assert _plan(1024) == (448, 448 * 192, 65856, 151872) and -(-1024 // 448) == 3
    assert _plan(2048) == (128, 128 * 192, 131392, 155968) and 128 * 192 >= FOLD and -(-2048 // 128) == 16
    assert 155968 <= GRANT == 163584
    for m in range(1, 2049):
        lists, shared, fixed, lds = _plan(m)
        mp = (m + 63) // 64 * 64
        assert fixed == 64 * mp + 64 + 256, m
        assert lds == fixed + shared <= GRANT, m
        assert lists % 64 == 0 and 64 <= lists <= min(1024, mp), m
        assert shared >= lists * 192 and shared >= FOLD and shared >= _keys(m), m
        assert 1024 // 64 * 6 * 8 <= fixed - 256, m  # the box's wave minima, in front of the shared region
        # the rounds of the normals are the estimate kernel's wherever that has room for as many lists
        est = (C.c_uint32 * 4)()
        assert I.lib().icp_debug_plane_batch_plan(1024, m, est) == _lib.OK
        assert lists >= est[0], (m, lists, est[0])
    out = (C.c_uint32 * 4)()
    for m in (0, 2049, 4096):
        assert I.lib().icp_debug_plane_quality_batch_plan(m, out) == _lib.BAD_ARGUMENT
    assert I.lib().icp_debug_plane_quality_batch_plan(8, None) == _lib.BAD_ARGUMENT


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
def test_plane_quality_batch_kernel_cross_compiles_within_its_budget():
    """exactly one kernel in quality_plane_batch.hip; 1024 threads: at most 128 registers per thread, at most 96 bytes
    per lane of scratch, the cap the other 1024-thread kernels are held to (it compiles to 90 VGPRs and 0 bytes), and
    no static LDS on top of the dynamic plan.  The name stays clear of the budgeted search / evaluation kernels
    (tests/test_registers.py)."""
    from test_registers import BUDGET

    use = _usage("quality_plane_batch.hip")
    assert len(use) == 1 and "k_plane_quality_batch" in list(use)[0], list(use)
    for k, u in use.items():
        print(k, u)
        assert not any(frag in k for frag in BUDGET), k
        assert u["vgpr"] <= 128 and u["scratch"] <= 96 and u["lds"] == 0, (k, u)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_plane_estimate_batch_kernels_keep_their_budgets_with_the_normals_in_the_shared_header():
    """p2plane_batch.hip still holds exactly its four instantiations, within the budgets tests/test_plane_batch_abi.py
    and tests/test_plane_batch_gated_abi.py state: 512 threads: 256 VGPRs and no scratch; 1024 threads: 128 VGPRs and 96
    bytes per lane; no static LDS"""
    use = _usage("p2plane_batch.hip")
    assert len(use) == 4, list(use)
    for kernel in ("k_plane_estimate_batch", "k_plane_estimate_gated_batch"):
        for b, vgpr, scratch in ((512, 256, 0), (1024, 128, 96)):
            names = [k for k in use if "%sILj%dE" % (kernel, b) in k]
            assert len(names) == 1, (kernel, b, list(use))
            u = use[names[0]]
            print(names[0], u)
            assert u["vgpr"] <= vgpr and u["scratch"] <= scratch and u["lds"] == 0, (names[0], u)
    # one statement of the normals' rounds, in a header, in none of the .hip files: the line and the plane kernels, the
    # estimates and the qualities, all call csrc/normal_batch_device.hpp: normals_of_sorted_targets<DIM>
    name = "void normals_of_sorted_targets"
    for src in sorted(f for f in os.listdir(CSRC) if f.endswith(".hip")):
        text = open(os.path.join(CSRC, src)).read()
        assert name not in text and "_normals_of_sorted_targets" not in text, src
    where = [h for h in sorted(os.listdir(CSRC)) if h.endswith((".hpp", ".inc"))
             and "normals_of_sorted_targets(const" in open(os.path.join(CSRC, h)).read()]
    assert where == ["normal_batch_device.hpp"], where
    assert open(os.path.join(CSRC, "normal_batch_device.hpp")).read().count(name + "(const") == 1
    for src in ("p2line_batch.hip", "p2plane_batch.hip", "quality_line.hip", "quality_plane_batch.hip"):
        assert '#include "normal_batch_device.hpp"' in open(os.path.join(CSRC, src)).read(), src


# ------------------------------------------------------------------ what it is for (shared with the GPU file)

SCENE_K = 8
SCENE_R = 0.5
TRUE_AT = 17  # the position of the true pose among the hypotheses
SCENE_POSE = [0.03, -0.02, 0.01]


def _wall_y(y):
    x, z = np.meshgrid(np.linspace(-10.0, 10.0, 81), np.linspace(0.0, 2.0, 9), indexing="ij")
    return np.stack([x.ravel(), np.full(x.size, y), z.ravel()], axis=1)


def _wall_x(x):
    y, z = np.meshgrid(np.linspace(-1.75, 1.75, 15), np.linspace(0.0, 2.0, 9), indexing="ij")
    return np.stack([np.full(y.size, x), y.ravel(), z.ravel()], axis=1)


def thin_corridor():
    """two walls y = +-2, x in [-10, 10], z in [0, 2], on a 0.25 grid: 1458 targets, one workgroup's worth"""
    return np.ascontiguousarray(np.concatenate([_wall_y(-2.0), _wall_y(2.0)]))


def thin_room():
    """the corridor plus the end walls x = +-10, y in [-1.75, 1.75]: 1728 targets"""
    return np.ascontiguousarray(np.concatenate([thin_corridor(), _wall_x(-10.0), _wall_x(10.0)]))


def hypotheses():
    """64 poses: the true one at TRUE_AT, the others off it by up to 5 cm and 0.03 rad, at least 1 cm in y (across the
    corridor's walls: a hypothesis that differs along the corridor only is one the plane residual cannot rank)"""
    rng = np.random.default_rng(9)
    Ts = []
    for i in range(64):
        dx, dth = rng.uniform(-0.05, 0.05), rng.uniform(-0.03, 0.03)
        dy = rng.uniform(0.01, 0.05) * (1 if rng.integers(0, 2) else -1)
        Ts.append(I.Transform(SCENE_POSE) if i == TRUE_AT else
                  I.Transform([SCENE_POSE[0] + dx, SCENE_POSE[1] + dy, SCENE_POSE[2] + dth]))
    return Ts


def scene_scan(dst):
    """every second target moved by the inverse of the true pose: evaluated at that pose it lies on the map"""
    from test_p2plane import moved

    return np.ascontiguousarray(moved(np.ascontiguousarray(dst[::2]), I.Transform(SCENE_POSE).inverse()))


def weak_direction(f):
    """of the float fields in as_array order: the eigenvector of lmin of the translation block"""
    info = np.asarray(f[7:16]).reshape(3, 3)
    return np.linalg.eigh(info[:2, :2])[1][:, 0]


def assert_scene(name, fields):
    """the bars of DESIGN.md section 9h on the 64 hypotheses' float fields (as_array order): the true pose has the least
    plane_rmse; at it the corridor's translation block has lmin / lmax <= 1e-6 with the weak direction along x, the
    room's >= 1e-2"""
    rmse = np.array([f[3] for f in fields])
    best = int(np.argmin(rmse))
    f = fields[TRUE_AT]
    lmin, lmax = f[16], f[17]
    print(f"{name}: argmin {best}, plane_rmse there {rmse[best]:.3g}, next {np.sort(rmse)[1]:.3g}, lmin {lmin:.6g}, "
          f"lmax {lmax:.6g}, ratio {lmin / lmax:.3g}, weak {weak_direction(f)}")
    assert best == TRUE_AT and rmse[TRUE_AT] < np.sort(rmse)[1]
    assert lmax > 0.0
    if name == "corridor":
        assert lmin / lmax <= 1e-6
        assert abs(weak_direction(f)[0]) >= 0.999
    else:
        assert lmin / lmax >= 1e-2


@pytest.mark.parametrize("name", ["corridor", "room"])
def test_the_true_pose_wins_and_the_corridor_is_not_observed_along_its_axis(name):
    """the reference alone meets the bars the GPU test sets: the oracle's normals and exact search, the numpy
    restatement of section 13"""
    import oracle_ffi as O
    from test_gpu_plane_quality import oracle_idx, restate

    dst = thin_corridor() if name == "corridor" else thin_room()
    assert len(dst) == (1458 if name == "corridor" else 1728) and len(dst) <= 2048
    src = scene_scan(dst)
    assert len(src) <= 1024
    nrm = O.p2pl_normals(dst, SCENE_K)
    fields = []
    for T in hypotheses():
        rc, cnt, f = restate(dst, nrm, src, T, SCENE_R, oracle_idx(dst, src, T))
        assert rc == _lib.OK and cnt == len(src)  # (every point within 0.5 m of its match)
        fields.append(f)
    assert_scene(name, fields)
