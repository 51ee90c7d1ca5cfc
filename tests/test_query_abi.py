"""CPU-side checks of the neighbour queries of arbitrary points and of the removal by mask (icp_query_neighbours[_device],
icp_count_within[_device], icp_remove_targets[_device], icp_grid_remove_counters, icp_query_counters:
include/icp_mi355x.h section 24): the numpy restatements of the three definitions (the arbiters of
tests/test_gpu_query.py) against plain Python loops; declared, exported and bound; ABI version still 8; every
argument-only error rejected before the device is touched; the Python refusals; the kernels' registers, LDS and scratch
(hipcc cross-compiles without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import icp_rust_amd as I
import tie_clouds as TC
from icp_rust_amd import _lib
from test_crop_abi import HIPCC, ROOT, _Handle, declared
from test_outlier_abi import new_index_of

PUBLIC = ("icp_query_neighbours", "icp_query_neighbours_device", "icp_count_within", "icp_count_within_device",
          "icp_remove_targets", "icp_remove_targets_device")
DEBUG = ("icp_grid_remove_counters", "icp_query_counters", "icp_query_force_order")
GONE = 0xFFFFFFFF
FULL = 0xFFFFFFFF  # the cap that gives the full count
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


# ---------------------------------------------------------------------- the rules, restated ----
def pose_of(transform):
    """(r00, r01, r10, r11, tx, ty) of a Transform, None for None"""
    if transform is None:
        return None
    p = transform.pose
    return tuple(np.float64(v) for v in (p.r00, p.r01, p.r10, p.r11, p.tx, p.ty))


def moved_queries(q, transform):
    """the query points under the pose: px = (r00 x + r01 y) + tx, py = (r10 x + r11 y) + ty, z kept; numpy forms every
    product and sum on its own (no FMA).  None: the coordinates as given, NOT a product with the identity."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    pose = pose_of(transform)
    if pose is None:
        return q
    r00, r01, r10, r11, tx, ty = pose
    p = q.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        p[:, 0] = (r00 * q[:, 0] + r01 * q[:, 1]) + tx
        p[:, 1] = (r10 * q[:, 0] + r11 * q[:, 1]) + ty
    return p


def d2_block(p, t):
    """d2 of the points p against every target: dx dx + dy dy (+ dz dz) with dx = p - t, a left fold"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = p[:, None, :] - t[None, :, :]
        dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        return dd + d[..., 2] * d[..., 2] if t.shape[1] == 3 else dd


def query_lists(t, q, k, transform=None):
    """section 24's lists: per query its min(k, m) nearest targets by (d2, index) among those whose d2 is not NaN; rows
    padded with (0xffffffff, +inf)"""
    t = np.ascontiguousarray(t, dtype=np.float64)
    p = moved_queries(q, transform)
    n, m = len(p), len(t)
    idx = np.full((n, k), GONE, dtype=np.uint32)
    d2 = np.full((n, k), np.inf)
    for at in range(0, n, 256):
        dd = d2_block(p[at:at + 256], t)
        for r in range(len(dd)):
            row = dd[r]
            cand = np.flatnonzero(~np.isnan(row))
            if len(cand) > max(k, 512):  # lexsort only the targets up to the k-th smallest d2, ties included
                kth = np.partition(row[cand], k - 1)[k - 1]
                cand = cand[row[cand] <= kth]
            order = cand[np.lexsort((cand, row[cand]))][:k]
            idx[at + r, :len(order)] = order
            d2[at + r, :len(order)] = row[order]
    return idx, d2


def count_within_ref(t, q, radius, cap=None, transform=None, strict=False):
    """counts[i] = min(cap, #{ j : d2(p_i, t_j) <= r * r }); q None: the targets themselves (strict: the WRONG `<`)"""
    t = np.ascontiguousarray(t, dtype=np.float64)
    p = t if q is None else moved_queries(q, transform)
    r = np.float64(radius)
    with np.errstate(over="ignore"):
        r2 = r * r
    counts = np.zeros(len(p), dtype=np.int64)
    for at in range(0, len(p), 256):
        dd = d2_block(p[at:at + 256], t)
        with np.errstate(invalid="ignore"):
            counts[at:at + 256] = ((dd < r2) if strict else (dd <= r2)).sum(1)
    return np.minimum(counts, FULL if cap is None else cap).astype(np.uint32)


def mask_keep(keep):
    """(kept, new_index) of icp_remove_targets: target i is kept iff keep[i] != 0"""
    kept = np.asarray(keep) != 0
    return kept, new_index_of(kept)


# ------------------------------------------------------- the restatements against plain loops ----
def _moved_loop(q, pose):
    out = []
    for row in q:
        c = [float(v) for v in row]
        if pose is not None:
            r00, r01, r10, r11, tx, ty = (float(v) for v in pose)
            x, y = c[0], c[1]
            c[0] = (r00 * x + r01 * y) + tx
            c[1] = (r10 * x + r11 * y) + ty
        out.append(c)
    return out


def _d2_loop(p, t):
    dx, dy = p[0] - float(t[0]), p[1] - float(t[1])
    dd = dx * dx + dy * dy
    if len(p) == 3:
        dz = p[2] - float(t[2])
        dd = dd + dz * dz
    return dd


def _loops(t, q, k, radius, cap, pose):
    lists, counts = [], []
    for p in _moved_loop(q, pose):
        d2 = [_d2_loop(p, tj) for tj in t]
        cand = sorted((j for j in range(len(t)) if d2[j] == d2[j]), key=lambda j: (d2[j], j))[:k]
        lists.append([(j, d2[j]) for j in cand])
        counts.append(min(cap, sum(1 for j in range(len(t)) if d2[j] <= radius * radius)))
    return lists, counts


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _queries_for(t, rng):
    """interior points, the targets themselves, points outside the box, a NaN and two infinite queries"""
    dim = t.shape[1]
    lo, hi = t.min(0), t.max(0)
    q = [rng.uniform(lo - 0.5, hi + 0.5, (12, dim)), t[: min(len(t), 5)], hi + rng.uniform(1.0, 50.0, (3, dim))]
    special = np.tile((lo + hi) / 2, (4, 1))
    special[0, 0] = NAN
    special[1, 1] = INF
    special[2, dim - 1] = -INF
    special[3, 0], special[3, 1] = INF, NAN
    return np.ascontiguousarray(np.concatenate(q + [special]))


@pytest.mark.parametrize("name", ["random2", "random3"] + list(TC.TINY_NAMES))
def test_the_restatements_agree_with_plain_loops(name):
    rng = np.random.default_rng(21)
    if name.startswith("random"):
        t, radius = np.ascontiguousarray(rng.normal(size=(150, int(name[-1])))), 0.6
    else:
        t, radius = TC.tiny(name).pts, TC.tiny(name).spacing
    q = _queries_for(t, rng)
    T = I.Transform([0.3, -0.2, 0.4])
    seen_padding = seen_cap_below = seen_cap_above = False
    for transform in (None, T, I.Transform()):
        pose = pose_of(transform)
        for k, r, cap in ((1, radius, 1), (5, 2 * radius, 3), (32, INF, 1000), (8, 0.0, 2)):
            lists, counts = _loops(t, q, k, r, cap, pose)
            idx, d2 = query_lists(t, q, k, transform)
            for i, row in enumerate(lists):
                assert idx[i, :len(row)].tolist() == [j for j, _ in row], (name, k, i)
                assert _same_bits(d2[i, :len(row)], [d for _, d in row]), (name, k, i)
                assert np.all(idx[i, len(row):] == GONE) and np.all(d2[i, len(row):] == INF)
                seen_padding |= len(row) < k
            got = count_within_ref(t, q, r, cap, transform)
            assert got.tolist() == counts, (name, r, cap)
            full = count_within_ref(t, q, r, None, transform)
            seen_cap_below |= bool(np.any(full > cap))
            seen_cap_above |= bool(np.any(full < cap))
    assert seen_padding and seen_cap_above and (seen_cap_below or len(t) == 1)
    # the NaN query lists nothing and counts nothing; the infinite ones (no NaN) list the targets 0 .. with d2 = +inf, and
    # count m exactly when r * r is +inf; under the identity POSE an infinite coordinate turns into a NaN (0 * inf)
    n = len(q)
    idx, d2 = query_lists(t, q, 3)
    kk = min(3, len(t))
    assert np.all(idx[n - 4] == GONE) and np.all(idx[n - 1] == GONE)
    for i in (n - 3, n - 2):
        assert idx[i, :kk].tolist() == list(range(kk)) and np.all(d2[i, :kk] == INF)
    assert count_within_ref(t, q, INF)[n - 4:].tolist() == [0, len(t), len(t), 0]
    assert count_within_ref(t, q, 1e300)[n - 4:].tolist() == [0, len(t), len(t), 0]  # (r * r overflows to +inf)
    assert count_within_ref(t, q, 1e100)[n - 4:].tolist() == [0, 0, 0, 0]
    idx, _ = query_lists(t, q, 3, I.Transform())
    assert np.all(idx[n - 3] == GONE)  # y = +inf: r00 x + r01 y = x + 0 * inf = NaN
    assert idx[n - 2, 0] == (0 if t.shape[1] == 3 else GONE)  # z = -inf is kept (3-D); y = -inf as above (2-D)
    # the targets as their own queries
    assert np.array_equal(count_within_ref(t, None, radius, 4), count_within_ref(t, t, radius, 4))


def test_mask_keep_is_the_truth_value_of_every_byte():
    keep = np.array([1, 0, 255, 2, 0, 0, 7], dtype=np.uint8)
    kept, index = mask_keep(keep)
    assert kept.tolist() == [True, False, True, True, False, False, True]
    assert index.tolist() == [0, GONE, 1, 2, GONE, GONE, 3]
    loop, at = [], 0
    for b in keep.tolist():
        loop.append(at if b != 0 else GONE)
        at += 1 if b != 0 else 0
    assert index.tolist() == loop
    assert mask_keep(np.zeros(5, dtype=bool))[1].tolist() == [GONE] * 5
    assert mask_keep(np.ones(5, dtype=bool))[1].tolist() == [0, 1, 2, 3, 4]


def test_a_lattice_radius_decides_between_less_and_less_or_equal():
    """on the slab (spacing 1/8) r = spacing has r * r equal to an attained d2, and the next double below it does not"""
    c = TC.cloud("slab")
    r = c.spacing
    below = np.nextafter(r, 0.0)
    assert r * r == c.spacing ** 2 and below * below < r * r
    at = count_within_ref(c.pts, None, r)
    assert at.max() == 6 and at.min() == 4  # itself and the lattice neighbours at one spacing
    assert np.all(count_within_ref(c.pts, None, r, strict=True) == 1)
    assert np.all(count_within_ref(c.pts, None, below) == 1)


# ----------------------------------------------------------------------------------- the ABI ----
def test_query_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    for s in PUBLIC:
        assert s in public, s
    for s in DEBUG:
        assert s in debug and s not in public, s
    L = C.CDLL(_lib.LIB_PATH)
    for s in PUBLIC + DEBUG:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    makefile = open(os.path.join(ROOT, "icp_rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bquery\.hip\b", makefile, flags=re.M)
    for cls in (I.Icp2d, I.Icp3d):
        for name in ("query", "count_within", "remove", "remove_counters", "query_counters"):
            assert callable(getattr(cls, name)), name
    header = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert re.search(r"^ \* 24\. EXTENSION", header, flags=re.M)


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def test_argument_errors_are_rejected_before_the_device_is_used():
    L = I.lib()
    q = np.zeros((4, 2))
    qp = C.c_void_p(q.ctypes.data)
    idx = np.full((4, 32), 7, dtype=np.uint32)
    ip = C.c_void_p(idx.ctypes.data)
    counts = np.full(4, 7, dtype=np.uint32)
    cp = C.c_void_p(counts.ctypes.data)
    keep = np.ones(4, dtype=np.uint8)
    kp = C.c_void_p(keep.ctypes.data)
    removed = C.c_size_t(7)
    pose = I.Transform().pose
    H = _Handle()
    try:
        for entry in (L.icp_query_neighbours, L.icp_query_neighbours_device):
            for k in (0, -1, 33, 1 << 20):
                assert entry(H.h, qp, 4, None, k, ip, None) == _lib.BAD_ARGUMENT, k
            assert entry(None, qp, 4, None, 3, ip, None) == _lib.BAD_ARGUMENT
            assert entry(H.h, None, 4, None, 3, ip, None) == _lib.BAD_ARGUMENT  # q is required with n > 0
            for n in (0xFFFFFFFF, 1 << 32, 1 << 40):
                assert entry(H.h, qp, n, None, 3, ip, None) == _lib.BAD_ARGUMENT, n
        for entry in (L.icp_count_within, L.icp_count_within_device):
            for r in (NAN, -1.0, -INF, -5e-324):
                assert entry(H.h, qp, 4, None, r, 3, cp) == _lib.BAD_ARGUMENT, r
            assert entry(H.h, qp, 4, None, 1.0, 0, cp) == _lib.BAD_ARGUMENT  # cap == 0
            assert entry(None, qp, 4, None, 1.0, 3, cp) == _lib.BAD_ARGUMENT
            assert entry(H.h, qp, 4, None, 1.0, 3, None) == _lib.BAD_ARGUMENT  # counts is required with n > 0
            assert entry(H.h, None, 4, C.byref(pose), 1.0, 3, cp) == _lib.BAD_ARGUMENT  # the targets take no pose
            for n in (0xFFFFFFFF, 1 << 32):
                assert entry(H.h, qp, n, None, 1.0, 3, cp) == _lib.BAD_ARGUMENT, n
        for entry in (L.icp_remove_targets, L.icp_remove_targets_device):
            assert entry(H.h, None, None, C.byref(removed)) == _lib.BAD_ARGUMENT
            assert entry(None, kp, None, C.byref(removed)) == _lib.BAD_ARGUMENT
        assert removed.value == 7 and np.all(idx == 7) and np.all(counts == 7)  # a refused call writes nothing
        if not H.real:  # valid arguments reach the device check only now
            for entry in (L.icp_query_neighbours, L.icp_query_neighbours_device):
                for k in (1, 16, 17, 32):
                    assert entry(H.h, qp, 4, None, k, ip, None) == _lib.NO_DEVICE
                assert entry(H.h, qp, 4, C.byref(pose), 3, None, None) == _lib.NO_DEVICE
                assert entry(H.h, None, 0, None, 3, None, None) == _lib.NO_DEVICE
            for entry in (L.icp_count_within, L.icp_count_within_device):
                for r in (0.0, 1.0, INF):
                    assert entry(H.h, qp, 4, None, r, 1, cp) == _lib.NO_DEVICE
                assert entry(H.h, qp, 4, C.byref(pose), 1.0, FULL, cp) == _lib.NO_DEVICE
                assert entry(H.h, None, 4, None, 1.0, 3, cp) == _lib.NO_DEVICE  # (n == m is the handle's to tell)
            for entry in (L.icp_remove_targets, L.icp_remove_targets_device):
                assert entry(H.h, kp, None, C.byref(removed)) == _lib.NO_DEVICE
            assert removed.value == 7
    finally:
        H.close()
    out = (C.c_uint64 * 2)()
    assert L.icp_grid_remove_counters(None, out) == _lib.BAD_ARGUMENT
    assert L.icp_query_counters(None, out) == _lib.BAD_ARGUMENT
    assert L.icp_query_force_order(None, 0) == _lib.BAD_ARGUMENT


def test_python_refuses_bad_arguments_before_any_handle_is_reached():
    for cls in (I.Icp2d, I.Icp3d):
        icp = object.__new__(cls)  # (no handle is reached: the arguments are checked first)
        icp._h = C.c_void_p()
        icp._device = None
        icp._own_stream = True
        pts = np.zeros((4, cls.DIM))
        for k in (0, 33, -1, 2.5):
            with pytest.raises(ValueError):
                icp.query(pts, k)
        for shape in ((4,), (4, 1), (4, 4)):
            with pytest.raises(ValueError):
                icp.query(np.zeros(shape), 3)
            with pytest.raises(ValueError):
                icp.count_within(np.zeros(shape), 1.0)
        for r in (NAN, -1.0, -INF):
            with pytest.raises(ValueError):
                icp.count_within(pts, r)
            with pytest.raises(ValueError):
                icp.count_within(None, r)
        for cap in (0, -1, 1.5, 1 << 32):
            with pytest.raises(ValueError):
                icp.count_within(pts, 1.0, cap=cap)
        with pytest.raises(ValueError):
            icp.count_within(None, 1.0, transform=I.Transform())
        for keep in (np.ones((2, 2)), np.float64(1.0)):
            with pytest.raises(ValueError):
                icp.remove(keep)


# ------------------------------------------------------------------------- kernel resources ----
# (VGPRs, LDS bytes per workgroup) of the list kernel per (DIM, KMAX), of the count kernel per DIM and of the mark kernel
# 
PINS = {"k_query_neighboursILi3ELi16E": (48, 12288), "k_query_neighboursILi3ELi32E": (48, 24576),
        "k_query_neighboursILi2ELi16E": (38, 12288), "k_query_neighboursILi2ELi32E": (38, 24576),
        "k_count_withinILi3E": (32, 0), "k_count_withinILi2E": (26, 0), "k_mask_marks": (17, 64)}


def _resources(src):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "icp_rust_amd", "csrc", src),
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        for key, pattern in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pattern, line)
            if m and name:
                res[name][key] = int(m.group(1))
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_query_kernels_do_not_spill_and_keep_their_registers_and_lds():
    """no scratch in any kernel of query.hip, for both DIM and both KMAX; every kernel at its recorded VGPR count and LDS
    size; the names stay clear of the budgeted kernels (tests/test_registers.py).  The kernels that share the search body
    and the block walk keep their own pins in test_outlier_abi.py, test_gated_plane_abi.py and test_line_abi.py."""
    from test_registers import BUDGET

    res = _resources("query.hip")
    for frag in PINS:
        assert len([k for k in res if frag in k]) == 1, (frag, list(res))
    for k, r in res.items():
        assert r["scratch"] == 0, (k, r)
        assert r["vgpr"] <= 128, (k, r)
        assert not any(frag in k for frag in BUDGET), k
    for frag, (vgpr, lds) in PINS.items():
        r = [res[k] for k in res if frag in k][0]
        assert (r["vgpr"], r["lds"]) == (vgpr, lds), (frag, r)
