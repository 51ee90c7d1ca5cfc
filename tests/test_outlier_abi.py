"""CPU-side checks of the neighbour lists and the two outlier filters (icp_target_neighbours[_device],
icp_remove_radius_outliers, icp_remove_statistical_outliers, icp_grid_outlier_counters: include/icp_mi355x.h section 23):
declared, exported and bound; ABI version still 8; every argument-only error rejected before the device is touched; the
Python refusals; run_scan_to_map filters between the thinning and the registration and only when asked; the numpy
restatements of the three definitions (the arbiters of tests/test_gpu_outlier.py) against plain Python loops; the inputs
of the GPU tests shown not to be vacuous, and the boundary inputs shown to decide the comparison operators, from the
restatements alone; the kernels' register and scratch use (hipcc cross-compiles without a GPU)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import icp_rust_amd as I
import tie_clouds as TC
from icp_rust_amd import _lib
from icp_rust_amd.scans import load_scan2d
from test_crop_abi import HIPCC, ROOT, _Handle, _usage, declared
from test_gpu_quality import fold

NEW = ("icp_target_neighbours", "icp_target_neighbours_device", "icp_remove_radius_outliers",
       "icp_remove_statistical_outliers", "icp_grid_outlier_counters")
GONE = 0xFFFFFFFF
NAN, INF = float("nan"), float("inf")
# the mid settings of the issue: (radius, min_neighbours) and (k, std_ratio) per cloud
RADIUS_SETTINGS = {"scan": ((30.0, 3), (50.0, 4), (80.0, 6)), "cloud3": ((0.1, 3), (0.2, 5), (0.3, 10))}
STAT_SETTINGS = {"scan": ((8, 1.0), (8, 2.0), (16, 1.0), (31, 2.0)), "cloud3": ((8, 1.0), (16, 2.0), (31, 0.0))}
TIE_NAMES = ("slab", "slab+far", "slabdup", "strip200x3", "strip200x3+x31", "strip200x3+split", "lat40x30", "stripdup")


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


# ------------------------------------------------------------------------------- the inputs ----
def golden_scan():
    return np.ascontiguousarray(load_scan2d(os.path.join(ROOT, "tests", "golden", "scans2d", "001.txt")))


def cloud3():
    """3 300 points: two planes and a volume in [-1, 1]^3, and 300 stragglers in [-3, 3]^3, permuted"""
    rng = np.random.default_rng(7)
    a = rng.uniform(-1.0, 1.0, (3000, 3))
    a[:1000, 2] = 0.0
    a[1000:2000, 0] = 1.0
    b = rng.uniform(-3.0, 3.0, (300, 3))
    p = np.concatenate([a, b])
    return np.ascontiguousarray(p[rng.permutation(len(p))])


def named(name):
    return golden_scan() if name == "scan" else cloud3()


# ---------------------------------------------------------------------- the rules, restated ----
def d2_rows(p, rows):
    """d2 of the targets `rows` against every target: dx dx + dy dy (+ dz dz), a left fold; numpy forms every product
    and sum on its own (no FMA)"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = p[rows][:, None, :] - p[None, :, :]
        dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        return dd + d[..., 2] * d[..., 2] if p.shape[1] == 3 else dd


def lists_of(p, k, first=0, count=None):
    """section 23's lists: per target of [first, first + count) its min(k, m) nearest targets, itself included, by
    (d2, index); rows padded with (0xffffffff, +inf)"""
    p = np.ascontiguousarray(p, dtype=np.float64)
    m = len(p)
    count = m - first if count is None else count
    idx = np.full((count, k), GONE, dtype=np.uint32)
    d2 = np.full((count, k), np.inf)
    kk = min(k, m)
    for at in range(0, count, 512):
        rows = np.arange(first + at, first + min(at + 512, count))
        dd = d2_rows(p, rows)
        if m > 512:  # lexsort only the targets up to the kk-th smallest d2 of a row, ties included: the same first kk
            kth = np.partition(dd, kk - 1, axis=1)[:, kk - 1]
            order = np.empty((len(rows), kk), dtype=np.int64)
            for r in range(len(rows)):
                near = np.flatnonzero(dd[r] <= kth[r])
                order[r] = near[np.lexsort((near, dd[r, near]))][:kk]
        else:
            order = np.lexsort((np.broadcast_to(np.arange(m), dd.shape), dd), axis=1)[:, :kk]
        idx[at:at + len(rows), :kk] = order
        d2[at:at + len(rows), :kk] = np.take_along_axis(dd, order, axis=1)
    return idx, d2


def radius_keep(p, radius, min_neighbours, strict=False):
    """kept iff #{ j : d2(i, j) <= r * r } >= min_neighbours, j over all targets, i included (strict: the WRONG `<`)"""
    p = np.ascontiguousarray(p, dtype=np.float64)
    r = np.float64(radius)
    with np.errstate(over="ignore"):
        r2 = r * r
    keep = np.zeros(len(p), dtype=bool)
    for at in range(0, len(p), 512):
        rows = np.arange(at, min(at + 512, len(p)))
        dd = d2_rows(p, rows)
        keep[rows] = ((dd < r2) if strict else (dd <= r2)).sum(1) >= min_neighbours
    return keep


_MEAN_DISTANCES = {}


def mean_distances(p, k):
    """u of the statistical rule (m >= 2): over the first ke entries, other than target i's own, of i's list of length
    ke + 1, the left fold of sqrt(d2) from the nearest, divided by ke"""
    m = len(p)
    ke = min(k, m - 1)
    key = (p.shape, ke, hash(p.tobytes()))  # (the settings of one cloud share their lists)
    if key in _MEAN_DISTANCES:
        return _MEAN_DISTANCES[key]
    idx, d2 = lists_of(p, ke + 1)
    own = idx == np.arange(m, dtype=np.uint32)[:, None]
    drop = np.where(own.any(1), own.argmax(1), ke)  # (not listed: more than ke coincident targets in front; all d2 are 0)
    cols = np.arange(ke + 1)[None, :] != drop[:, None]
    r = np.sqrt(d2[cols].reshape(m, ke))
    s = r[:, 0].copy()
    for c in range(1, ke):
        s = s + r[:, c]
    u = s / np.float64(ke)
    u.setflags(write=False)
    _MEAN_DISTANCES[key] = u
    return u


def statistical_keep(p, k, std_ratio, at_least=False):
    """(keep, (mean, deviation, threshold)) of the statistical rule (at_least: the WRONG `>=` in place of `>`)"""
    p = np.ascontiguousarray(p, dtype=np.float64)
    m = len(p)
    if m <= 1:
        return np.ones(m, dtype=bool), (0.0, 0.0, 0.0)
    u = mean_distances(p, k)
    with np.errstate(over="ignore", invalid="ignore"):
        mean = fold(u) / np.float64(m)
        c = u - mean
        deviation = np.sqrt(fold(c * c) / np.float64(m - 1))
        t = np.float64(std_ratio) * deviation
        threshold = mean + t
        gone = (u >= threshold) if at_least else (u > threshold)
    return ~gone, (float(mean), float(deviation), float(threshold))


def new_index_of(mask):
    return np.where(mask, np.cumsum(mask) - 1, GONE).astype(np.uint32)


# ------------------------------------------------------- the restatements against plain loops ----
def _d2_loop(p, i, j):
    dx, dy = float(p[i, 0]) - float(p[j, 0]), float(p[i, 1]) - float(p[j, 1])
    dd = dx * dx + dy * dy
    if p.shape[1] == 3:
        dz = float(p[i, 2]) - float(p[j, 2])
        dd = dd + dz * dz
    return dd


def _fold_loop(v):
    v = [float(x) for x in v]
    if len(v) == 0:
        return 0.0
    if len(v) == 1:
        return v[0]
    while len(v) > 1:
        out = []
        for g in range(0, len(v), 256):
            grp = v[g:g + 256] + [0.0] * (256 - len(v[g:g + 256]))
            s = 128
            while s >= 1:
                for t in range(s):
                    grp[t] = grp[t] + grp[t + s]
                s //= 2
            out.append(grp[0])
        v = out
    return v[0]


def _loops(p, k, radius, need, ks, ratio):
    m = len(p)
    d2 = [[_d2_loop(p, i, j) for j in range(m)] for i in range(m)]
    order = [sorted(range(m), key=lambda j, i=i: (d2[i][j], j)) for i in range(m)]
    lists = [[(j, d2[i][j]) for j in order[i][:k]] for i in range(m)]
    by_radius = [sum(1 for j in range(m) if d2[i][j] <= radius * radius) >= need for i in range(m)]
    if m <= 1:
        return lists, by_radius, [True] * m, (0.0, 0.0, 0.0)
    ke = min(ks, m - 1)
    u = []
    for i in range(m):
        others = [j for j in order[i][:ke + 1] if j != i][:ke]
        s = math.sqrt(d2[i][others[0]])
        for j in others[1:]:
            s = s + math.sqrt(d2[i][j])
        u.append(s / float(ke))
    mean = _fold_loop(u) / float(m)
    deviation = math.sqrt(_fold_loop([(x - mean) * (x - mean) for x in u]) / float(m - 1))
    t = ratio * deviation
    threshold = mean + t
    return lists, by_radius, [not (x > threshold) for x in u], (mean, deviation, threshold)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("name", ["random2", "random3", "dups"] + list(TC.TINY_NAMES))
def test_the_restatements_agree_with_plain_loops(name):
    rng = np.random.default_rng(11)
    if name.startswith("random"):
        p, radius = rng.normal(size=(200, int(name[-1]))), 0.4
    elif name == "dups":  # more coincident targets than a list is long: a target need not be in its own list
        p, radius = np.repeat(rng.integers(0, 3, (8, 2)).astype(np.float64), 6, axis=0), 1.0
    else:
        p, radius = TC.tiny(name).pts, TC.tiny(name).spacing
    p = np.ascontiguousarray(p)
    for k, need, ks, ratio in ((1, 2, 1, 0.0), (5, 3, 4, 1.0), (32, 6, 31, -0.5)):
        lists, by_radius, by_stat, stats = _loops(p, k, radius, need, ks, ratio)
        idx, d2 = lists_of(p, k)
        kk = min(k, len(p))
        assert np.array_equal(idx[:, :kk], np.array([[j for j, _ in row] for row in lists], dtype=np.uint32))
        assert _same_bits(d2[:, :kk], np.array([[d for _, d in row] for row in lists]))
        assert np.all(idx[:, kk:] == GONE) and np.all(d2[:, kk:] == np.inf)
        assert np.array_equal(radius_keep(p, radius, need), by_radius)
        keep, got = statistical_keep(p, ks, ratio)
        assert np.array_equal(keep, by_stat) and _same_bits(got, stats), (got, stats)
    sub_idx, sub_d2 = lists_of(p, 3, first=len(p) // 2, count=len(p) - len(p) // 2)
    assert np.array_equal(sub_idx, lists_of(p, 3)[0][len(p) // 2:]) and _same_bits(sub_d2, lists_of(p, 3)[1][len(p) // 2:])


def test_fold_is_the_tree_and_not_a_left_fold():
    v = np.random.default_rng(2).normal(size=700) * 1e3
    assert _same_bits(fold(v), _fold_loop(v))
    assert fold(v) != np.cumsum(v)[-1]  # (the two orders differ on this input: the tree is observable)


# ------------------------------------------------------------------- the inputs are not vacuous ----
@pytest.mark.parametrize("name", ["scan", "cloud3"])
def test_every_mid_setting_removes_at_least_3_percent_and_keeps_at_least_half(name):
    p = named(name)
    assert p.shape == ((646, 2) if name == "scan" else (3300, 3))
    for r, need in RADIUS_SETTINGS[name]:
        share = radius_keep(p, r, need).mean()
        print(f"{name} radius {r} {need}: keeps {share:.3f}")
        assert 0.5 <= share <= 0.97, (r, need, share)
    for k, ratio in STAT_SETTINGS[name]:
        share = statistical_keep(p, k, ratio)[0].mean()
        print(f"{name} statistical {k} {ratio}: keeps {share:.3f}")
        assert 0.5 <= share <= 0.97, (k, ratio, share)


def test_the_slab_decides_between_less_and_less_or_equal():
    c = TC.cloud("slab")
    assert c.m == 1152 and c.spacing == 0.125
    right, wrong = radius_keep(c.pts, c.spacing, 5), radius_keep(c.pts, c.spacing, 5, strict=True)
    assert right.sum() == 1152 - 8 and not wrong.any()  # 99.3 % kept (all but the corners); `<` counts the point alone
    assert round(float(np.mean(right != wrong)), 3) == 0.993
    assert not radius_keep(c.pts, c.spacing, 7).any()  # (an interior point has 6 within one spacing, itself included)
    right, wrong = radius_keep(c.pts, 2 * c.spacing, 20), radius_keep(c.pts, 2 * c.spacing, 20, strict=True)
    assert round(float(right.mean()), 2) == 0.84 and not wrong.any()


def test_the_unit_cube_decides_between_greater_and_greater_or_equal():
    p = np.ascontiguousarray(TC.box(2, 2, 2).astype(np.float64))
    assert np.all(mean_distances(p, 3) == 1.0)
    keep, stats = statistical_keep(p, 3, 0.0)
    assert stats == (1.0, 0.0, 1.0) and keep.all()
    assert not statistical_keep(p, 3, 0.0, at_least=True)[0].any()


def test_a_nan_threshold_keeps_everything():
    p = np.ascontiguousarray(np.random.default_rng(4).normal(size=(50, 3)))
    keep, stats = statistical_keep(p, 4, INF)
    assert stats[2] == INF and keep.all()
    keep, stats = statistical_keep(np.ascontiguousarray(TC.box(2, 2, 2).astype(np.float64)), 3, INF)  # inf * 0
    assert math.isnan(stats[2]) and keep.all()
    p[7, 1] = 1e308  # an infinite u: the mean is infinite, the deviation and the threshold NaN
    keep, stats = statistical_keep(p, 4, 1.0)
    assert stats[0] == INF and math.isnan(stats[1]) and math.isnan(stats[2]) and keep.all()


# ----------------------------------------------------------------------------------- the ABI ----
def test_outlier_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    for s in NEW[:4]:
        assert s in public, s
    assert "icp_grid_outlier_counters" in debug and "icp_grid_outlier_counters" not in public
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    makefile = open(os.path.join(ROOT, "icp_rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\boutlier\.hip\b", makefile, flags=re.M)
    for cls in (I.Icp2d, I.Icp3d):
        for name in ("neighbours", "remove_radius_outliers", "remove_statistical_outliers", "outlier_counters"):
            assert callable(getattr(cls, name)), name
    assert callable(I.remove_radius_outliers) and callable(I.remove_statistical_outliers)
    header = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert re.search(r"^ \* 23\. EXTENSION", header, flags=re.M)


def test_abi_version_is_still_8():
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8


def test_argument_errors_are_rejected_before_the_device_is_used():
    L = I.lib()
    removed = C.c_size_t(7)
    stats = (C.c_double * 3)(7.0, 7.0, 7.0)
    H = _Handle()
    try:
        for entry in (L.icp_target_neighbours, L.icp_target_neighbours_device):
            for k in (0, -1, 33, 1 << 20):
                assert entry(H.h, k, 0, 0, None, None) == _lib.BAD_ARGUMENT, k
            assert entry(None, 3, 0, 0, None, None) == _lib.BAD_ARGUMENT
        for r in (NAN, -1.0, -INF, -5e-324):
            assert L.icp_remove_radius_outliers(H.h, r, 3, None, C.byref(removed)) == _lib.BAD_ARGUMENT, r
        assert L.icp_remove_radius_outliers(None, 1.0, 3, None, C.byref(removed)) == _lib.BAD_ARGUMENT
        for k in (0, -3, 32, 33):
            assert L.icp_remove_statistical_outliers(H.h, k, 1.0, None, C.byref(removed), stats) == _lib.BAD_ARGUMENT, k
        assert L.icp_remove_statistical_outliers(H.h, 8, NAN, None, C.byref(removed), stats) == _lib.BAD_ARGUMENT
        assert L.icp_remove_statistical_outliers(None, 8, 1.0, None, C.byref(removed), stats) == _lib.BAD_ARGUMENT
        assert removed.value == 7 and list(stats) == [7.0, 7.0, 7.0]  # a refused call writes nothing
        if not H.real:  # valid arguments reach the device check only now
            assert L.icp_target_neighbours(H.h, 32, 0, 0, None, None) == _lib.NO_DEVICE
            assert L.icp_target_neighbours_device(H.h, 1, 0, 0, None, None) == _lib.NO_DEVICE
            for r in (0.0, 1.0, INF):
                assert L.icp_remove_radius_outliers(H.h, r, 3, None, C.byref(removed)) == _lib.NO_DEVICE
            for k, ratio in ((1, 0.0), (31, -INF), (8, INF)):
                assert L.icp_remove_statistical_outliers(H.h, k, ratio, None, C.byref(removed), stats) == _lib.NO_DEVICE
    finally:
        H.close()
    out = (C.c_uint64 * 2)()
    assert L.icp_grid_outlier_counters(None, out) == _lib.BAD_ARGUMENT


def test_python_refuses_bad_arguments_before_any_handle_is_reached():
    for cls in (I.Icp2d, I.Icp3d):
        icp = object.__new__(cls)  # (no handle is reached: the arguments are checked first)
        icp._h = C.c_void_p()
        for r in (NAN, -1.0):
            with pytest.raises(ValueError):
                icp.remove_radius_outliers(r, 3)
        with pytest.raises(ValueError):
            icp.remove_radius_outliers(1.0, -1)
        for k in (0, 32, 2.5):
            with pytest.raises(ValueError):
                icp.remove_statistical_outliers(k, 1.0)
        with pytest.raises(ValueError):
            icp.remove_statistical_outliers(8, NAN)
        for k in (0, 33, -1):
            with pytest.raises(ValueError):
                icp.neighbours(k)
    pts = np.zeros((4, 3))
    for r in (NAN, -0.5):
        with pytest.raises(ValueError):
            I.remove_radius_outliers(pts, r, 3)
    for k, ratio in ((0, 1.0), (32, 1.0), (8, NAN)):
        with pytest.raises(ValueError):
            I.remove_statistical_outliers(pts, k, ratio)
    for shape in ((4,), (4, 1), (4, 4)):
        with pytest.raises(ValueError):
            I.remove_radius_outliers(np.zeros(shape), 1.0, 2)
        with pytest.raises(ValueError):
            I.remove_statistical_outliers(np.zeros(shape), 4, 1.0)


# ------------------------------------------------------------------------------- the harness ----
def test_scan_to_map_filters_between_the_thinning_and_the_registration_and_only_when_asked(monkeypatch):
    from icp_rust_amd import harness, synth

    log = []

    class Fake:
        def __init__(self, dst):
            log.append(("create", len(dst)))

        def estimate(self, src, T, max_iter, **kw):
            log.append(("estimate", len(src)))
            return I.Transform([0.25, -0.5, 0.01])

        def append(self, pts, T):
            log.append(("append", len(pts)))

    def fail(*a, **k):
        raise AssertionError("remove_statistical_outliers is called only with scan_outliers")

    def thinned(scan, v):
        log.append(("voxel", len(scan)))
        return scan[::2]

    def filtered(scan, k, ratio):
        log.append(("outliers", len(scan), k, ratio))
        return scan[:len(scan) - 5]

    packets = synth.synthetic_scan3d_packets(4 * synth.PACKETS_PER_FRAME)
    monkeypatch.setattr(harness, "remove_statistical_outliers", fail)
    monkeypatch.setattr(harness, "voxel_downsample", thinned)
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2)  # the default sequence makes no new call
    assert [e[0] for e in log] == ["create"] + ["estimate", "append"] * 3
    full = [e[1] for e in log if e[0] in ("create", "append")]
    del log[:]
    monkeypatch.setattr(harness, "remove_statistical_outliers", filtered)
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, scan_voxel=0.25, scan_outliers=(8, 1.5))
    assert [e[0] for e in log] == ["voxel", "outliers", "create"] + ["voxel", "outliers", "estimate", "append"] * 3
    halves = [(n + 1) // 2 for n in full]
    assert [e[1:] for e in log if e[0] == "outliers"] == [(n, 8, 1.5) for n in halves]  # frame 0 too, after the thin
    assert [e[1] for e in log if e[0] in ("create", "append")] == [n - 5 for n in halves]
    assert [e[1] for e in log if e[0] == "estimate"] == [n - 5 for n in halves[1:]]
    del log[:]
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, scan_outliers=(16, 2.0))
    assert [e[0] for e in log] == ["outliers", "create"] + ["outliers", "estimate", "append"] * 3
    assert [e[1:] for e in log if e[0] == "outliers"] == [(n, 16, 2.0) for n in full]


# ------------------------------------------------------------------------- kernel resources ----
# VGPRs of the list kernel per (DIM, KMAX) and of the radius kernel per DIM
PINS = {"k_target_neighboursILi3ELi16E": 49, "k_target_neighboursILi3ELi32E": 49, "k_target_neighboursILi2ELi16E": 39,
        "k_target_neighboursILi2ELi32E": 39, "k_radius_markILi3E": 30, "k_radius_markILi2E": 22}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_outlier_kernels_do_not_spill_and_keep_their_registers():
    """no scratch in any kernel of outlier.hip, for both DIM and both KMAX; the list and radius kernels at their recorded
    VGPR counts, the others at most 128; the names stay clear of the budgeted kernels (tests/test_registers.py).  The
    normals kernels, which share the search body, keep their pins in test_gated_plane_abi.py / test_line_abi.py."""
    from test_registers import BUDGET

    regs = _usage("outlier.hip")
    kernels = [k for k in regs if not k.endswith("#scratch")]
    for frag in tuple(PINS) + ("k_stat_level", "k_stat_scalar", "k_outlier_count", "k_fold_levelILi1E"):
        assert len([k for k in kernels if frag in k]) == 1, (frag, kernels)
    for k in kernels:
        assert regs.get(k + "#scratch", 0) == 0, (k, regs.get(k + "#scratch"))
        assert regs[k] <= 128, (k, regs[k])
        assert not any(frag in k for frag in BUDGET), k
    for frag, want in PINS.items():
        got = [regs[k] for k in kernels if frag in k][0]
        assert got == want, (frag, got, want)
