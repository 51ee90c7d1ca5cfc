"""CPU-side checks of voxel centroids (icp_voxel_centroids[_device]: include/icp_mi355x.h section 25): declared, exported
and bound; ABI version still 8; the numpy restatement of the rule (centroids_of, the arbiter of tests/test_gpu_voxel_mean.py)
against a dict-based loop and against exact sums; the -0.0 cases; every argument error rejected before the device is
touched; the Python refusals; run_scan_to_map routes the scans through the centroids only when asked; the kernels'
register and scratch use (hipcc cross-compiles without a GPU)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import icp_rust_amd as I
from icp_rust_amd import _lib
from test_crop_abi import HIPCC, ROOT, _usage, declared
from test_voxel_abi import BAD_SIZES, boundary_input, kept_index_of, special_input

NEW = ("icp_voxel_centroids", "icp_voxel_centroids_device")
GONE = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def built():
    I.build()


# ------------------------------------------------------------------------ the rule, restated ----
def fold(v):
    """the fold of section 9 (as tests/test_gpu_quality.py restates it): n == 1 -> v[0], else groups of 256 padded with
    +0.0, g[i] += g[i + s] for s = 128 .. 1 inside each, level after level"""
    v = np.asarray(v, dtype=np.float64).ravel()
    if v.size == 1:
        return v[0]
    while v.size > 1:
        g = np.concatenate([v, np.zeros((-v.size) % 256)]).reshape(-1, 256)
        s = 128
        while s >= 1:
            g = g[:, :s] + g[:, s:2 * s]
            s //= 2
        v = g[:, 0]
    return v[0]


def _fold_rows(rows):
    """section 9's tree over every row of an (m, 256) array of values padded with +0.0: g[i] += g[i + s], s = 128 .. 1"""
    s = 128
    while s >= 1:
        rows = rows[:, :s] + rows[:, s:2 * s]
        s //= 2
    return rows[:, 0]


def centroids_of(p, v):
    """the rule of section 25 in numpy: (mean, count, first_index, voxel_of).  Membership and order are
    kept_index_of's (section 22); per voxel and axis the fold of section 9 over the members in ascending index, then one
    division by the count.  Voxels of up to 256 members are one group of the tree each (folded many rows at a time);
    larger ones go through fold."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    n, dim = p.shape
    first = kept_index_of(p, v)
    voxel_of = np.full(n, GONE, dtype=np.uint32)
    if len(first) == 0:
        return np.zeros((0, dim)), np.zeros(0, dtype=np.uint32), first, voxel_of
    ok = np.isfinite(p).all(axis=1)
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.floor(p / np.float64(v)) + 0.0
    _, lowest, inverse = np.unique(c[ok], axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(lowest), dtype=np.int64)
    rank[np.argsort(lowest, kind="stable")] = np.arange(len(lowest))
    voxel_of[ok] = rank[inverse.ravel()]
    members = np.flatnonzero(ok)
    order = members[np.argsort(voxel_of[members], kind="stable")]  # by (voxel, index)
    count = np.bincount(voxel_of[members].astype(np.int64), minlength=len(first)).astype(np.uint32)
    start = np.concatenate([[0], np.cumsum(count.astype(np.int64))])
    assert np.array_equal(order[start[:-1]], first)
    mean = np.empty((len(first), dim))
    one = np.flatnonzero(count == 1)
    mean[one] = p[order[start[one]]]  # the fold of one value is the value; x / 1.0 is x
    group = np.flatnonzero((count >= 2) & (count <= 256))
    with np.errstate(over="ignore", invalid="ignore"):
        for lo in range(0, len(group), 4096):
            g = group[lo:lo + 4096]
            col = np.arange(256)[None, :]
            inside = col < count[g][:, None]
            src = order[np.minimum(start[g][:, None] + col, len(order) - 1)]
            for a in range(dim):
                rows = np.where(inside, p[src, a], 0.0)
                mean[g, a] = _fold_rows(rows) / count[g].astype(np.float64)
        for r in np.flatnonzero(count > 256):
            idx = order[start[r]:start[r + 1]]
            for a in range(dim):
                mean[r, a] = fold(p[idx, a]) / np.float64(count[r])
    return mean, count, first, voxel_of


def centroids_by_dict(p, v):
    """the same rule as a plain loop: a dict from the cell to the list of member indices, in order of first appearance"""
    p = np.asarray(p, dtype=np.float64)
    cells, voxel_of = {}, np.full(len(p), GONE, dtype=np.uint32)
    for i, row in enumerate(p):
        if not np.isfinite(row).all():
            continue
        with np.errstate(over="ignore"):
            cell = tuple(float(np.floor(x / np.float64(v))) for x in row)
        cells.setdefault(cell, []).append(i)
    ranks = {cell: r for r, cell in enumerate(cells)}
    for cell, idx in cells.items():
        voxel_of[idx] = ranks[cell]
    mean = np.zeros((len(cells), p.shape[1]))
    with np.errstate(over="ignore", invalid="ignore"):
        for cell, idx in cells.items():
            for a in range(p.shape[1]):
                mean[ranks[cell], a] = fold(p[idx, a]) / np.float64(len(idx))
    count = np.array([len(idx) for idx in cells.values()], dtype=np.uint32)
    first = np.array([idx[0] for idx in cells.values()], dtype=np.int64)
    return mean, count, first, voxel_of


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_the_restatement_agrees_with_the_dict_loop():
    rng = np.random.default_rng(3)
    for dim in (2, 3):
        crowded = rng.uniform(0.0, 1.0, (900, dim)) * np.where(rng.random((900, 1)) < 0.7, 0.2, 3.0)  # voxels above 256
        for p, v in ((rng.normal(size=(3000, dim)) * 2.0, 0.5), (boundary_input(dim), 0.1), (special_input(dim), 0.1),
                     (special_input(dim), 1e-3), (special_input(dim), 1e300), (rng.integers(-3, 3, (500, dim)) * 0.25, 0.25),
                     (crowded, 0.25)):
            got, want = centroids_of(p, v), centroids_by_dict(p, v)
            assert _same_bytes(got[0], want[0]), (dim, v)
            for g, w in zip(got[1:], want[1:]):
                assert np.array_equal(g, w), (dim, v)
            assert 0 < len(want[0]) < len(p)
            assert got[1].sum() == np.count_nonzero(got[3] != GONE)
        assert centroids_of(crowded, 0.25)[1].max() > 256


def test_the_restatement_is_as_accurate_as_its_tree_allows():
    """against math.fsum / c.  The bound is derived: a value passes 8 additions per level of the tree (s = 128 .. 1), each
    with a relative error of at most u = 2^-53, over L = ceil(log256 c) levels, and the division adds one more rounding:
    |mean - exact| <= ((1 + u)^(8 L + 1) - 1) sum|x| / c <= (8 L + 1) u 1.01 sum|x| / c"""
    rng = np.random.default_rng(11)
    u = 2.0 ** -53
    seen = set()
    clouds = [(rng.normal(size=(4000, 3)) * 2.0 + rng.normal(size=(1, 3)) * 100.0, 0.5),
              (rng.normal(size=(4000, 3)) * 0.3 + rng.normal(size=(1, 3)) * 100.0, 1.0),
              (rng.uniform(0.05, 0.95, (70_000, 3)) + np.array([[-7.0, 0.0, 123.0]]), 1.0)]  # one voxel, three levels
    for p, v in clouds:
        mean, count, first, voxel_of = centroids_of(p, v)
        for r in np.argsort(count)[::-1][:40]:
            idx = np.flatnonzero(voxel_of == r)
            c = len(idx)
            assert c == count[r]
            levels, left = 0, c
            while left > 1:
                levels, left = levels + 1, -(-left // 256)
            seen.add(levels)
            for a in range(3):
                x = [float(t) for t in p[idx, a]]
                exact = math.fsum(x) / c
                bound = (8 * levels + 1) * u * 1.01 * math.fsum(abs(t) for t in x) / c
                assert abs(float(mean[r, a]) - exact) <= bound, (c, a, mean[r, a], exact, bound)
    assert {1, 2, 3} <= seen  # voxels of one, two and three levels of the tree


def test_a_lone_negative_zero_stays_and_two_of_them_give_a_positive_zero():
    lone = np.array([[-0.0, 0.25, -0.0], [5.0, 5.0, 5.0]])
    mean, count, _, _ = centroids_of(lone, 1.0)
    assert np.array_equal(count, [1, 1]) and _same_bytes(mean, lone)
    assert np.signbit(mean[0, 0]) and np.signbit(mean[0, 2])
    pair = np.array([[-0.0, 0.25, -0.0], [5.0, 5.0, 5.0], [-0.0, 0.75, -0.0]])
    mean, count, first, voxel_of = centroids_of(pair, 1.0)
    assert np.array_equal(count, [2, 1]) and np.array_equal(first, [0, 1]) and np.array_equal(voxel_of, [0, 1, 0])
    assert mean[0, 0] == 0.0 and not np.signbit(mean[0, 0]) and not np.signbit(mean[0, 2]) and mean[0, 1] == 0.5
    for dim in (2, 3):
        got, want = centroids_of(pair[:, :dim], 1.0), centroids_by_dict(pair[:, :dim], 1.0)
        assert _same_bytes(got[0], want[0])


# ----------------------------------------------------------------------------------- the ABI ----
def test_centroid_symbols_are_declared_exported_and_bound():
    public, debug = declared("icp_mi355x.h"), declared("icp_mi355x_debug.h")
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s in public and s not in debug, s
        assert s in _lib.SIGNATURES and hasattr(L, s), s
        assert hasattr(I.lib(), s)
    text = open(os.path.join(ROOT, "include", "icp_mi355x.h")).read()
    assert int(re.search(r"#define\s+ICP_ABI_VERSION\s+(\d+)", text).group(1)) == 8
    assert I.lib().icp_abi_version() == 8
    makefile = open(os.path.join(ROOT, "icp_rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bvoxel_mean\.hip\b", makefile, flags=re.M)
    assert re.search(r"^HDRS\s*:=.*\bvoxel_device\.hpp\b", makefile, flags=re.M)
    assert callable(I.voxel_centroids)


def _centroids(entry, dim, pts, n, v, voxels, outs=(None, None, None, None)):
    f = getattr(I.lib(), entry)
    p = C.c_void_p(pts.ctypes.data) if pts is not None else None
    k = C.byref(voxels) if voxels is not None else None
    o = [C.c_void_p(a.ctypes.data) if a is not None else None for a in outs]
    if entry == "icp_voxel_centroids":
        return f(dim, p, n, v, o[0], o[1], o[2], o[3], k, -1)
    return f(dim, p, n, v, o[0], o[1], o[2], o[3], k, -1, None)


@pytest.mark.parametrize("entry", NEW)
def test_centroid_argument_errors_are_rejected_before_the_device_is_used(entry):
    pts = np.zeros((4, 3))
    voxels = C.c_size_t(7)
    mean, words = np.full((4, 3), 9.0), [np.full(4, 9, dtype=np.uint32) for _ in range(3)]
    outs = (mean, *words)  # (host arrays: a refused call must not write them, and never reads them as device memory)
    for dim in (1, 4, 0, -2):
        assert _centroids(entry, dim, pts, 4, 0.5, voxels, outs) == _lib.BAD_ARGUMENT, dim
    for v in BAD_SIZES + (float("-inf"), 2e-308):
        assert _centroids(entry, 3, pts, 4, v, voxels, outs) == _lib.BAD_ARGUMENT, v
    assert _centroids(entry, 3, pts, 4, 0.5, None, outs) == _lib.BAD_ARGUMENT
    assert _centroids(entry, 3, None, 4, 0.5, voxels, outs) == _lib.BAD_ARGUMENT
    assert _centroids(entry, 3, pts, 0xFFFFFFFF, 0.5, voxels, outs) == _lib.BAD_ARGUMENT  # (decided on n alone)
    # means or counts of more than 2^27 points: the limit of the sort underneath, decided on n and the pointers alone
    for k in (0, 1):
        asked = tuple(a if j == k else None for j, a in enumerate(outs))
        assert _centroids(entry, 3, pts, (1 << 27) + 1, 0.5, voxels, asked) == _lib.BAD_ARGUMENT, k
    f = getattr(I.lib(), entry)
    tail = (C.byref(voxels), -2) if entry == "icp_voxel_centroids" else (C.byref(voxels), -2, None)
    assert f(3, C.c_void_p(pts.ctypes.data), 4, 0.5, None, None, None, None, *tail) == _lib.BAD_ARGUMENT
    assert voxels.value == 7 and np.all(mean == 9.0) and all(np.all(w == 9) for w in words)  # nothing written
    if I.lib().icp_device_count() == 0:
        # valid arguments reach the device check only now; DBL_MIN and DBL_MAX are valid sizes, and so is n == 0
        for dim, v, n in ((2, 0.5, 4), (3, 2.2250738585072014e-308, 4), (3, 1.7976931348623157e308, 4), (3, 0.5, 0)):
            assert _centroids(entry, dim, pts, n, v, voxels) == _lib.NO_DEVICE, (dim, v, n)
        # ... and so are 2^27 points with means, and more when only the indices and the map are asked for
        assert _centroids(entry, 3, pts, 1 << 27, 0.5, voxels, outs) == _lib.NO_DEVICE
        assert _centroids(entry, 3, pts, (1 << 27) + 1, 0.5, voxels, (None, None, words[1], words[2])) == _lib.NO_DEVICE


def test_python_refuses_a_bad_size_or_shape_before_any_device_use():
    for v in BAD_SIZES + (-1e-9,):
        with pytest.raises(ValueError):
            I.voxel_centroids(np.zeros((4, 3)), v)
    for shape in ((4,), (4, 1), (4, 4), (2, 2, 3)):
        with pytest.raises(ValueError):
            I.voxel_centroids(np.zeros(shape), 0.5, return_counts=True)


def test_python_refuses_device_tensors_the_kernels_would_misread():
    class FakeTensor:
        is_cuda = True

        def __init__(self, shape, dtype="torch.float64", contiguous=True):
            self.shape, self.dtype, self._c = shape, dtype, contiguous

        def data_ptr(self):
            raise AssertionError("a refused tensor is never read")

        def dim(self):
            return len(self.shape)

        def is_contiguous(self):
            return self._c

    pytest.importorskip("torch")
    for t in (FakeTensor((8, 3), dtype="torch.float32"), FakeTensor((8, 3), contiguous=False), FakeTensor((8, 4)),
              FakeTensor((8,))):
        with pytest.raises(ValueError):
            I.voxel_centroids(t, 0.5)
    with pytest.raises(ValueError):
        I.voxel_centroids(FakeTensor((8, 3)), float("nan"))


# ------------------------------------------------------------------------------- the harness ----
def test_scan_to_map_takes_centroids_of_every_scan_only_when_asked(monkeypatch):
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
        raise AssertionError("not called")

    calls = {"centroids": [], "downsample": []}

    def centroids(scan, v):
        calls["centroids"].append((len(scan), v))
        return centroids_of(scan, v)[0]

    def thinned(scan, v):
        calls["downsample"].append((len(scan), v))
        return scan[kept_index_of(scan, v)]

    packets = synth.synthetic_scan3d_packets(4 * synth.PACKETS_PER_FRAME)
    # the default: neither function is called without scan_voxel, and only voxel_downsample with it
    monkeypatch.setattr(harness, "voxel_centroids", fail)
    monkeypatch.setattr(harness, "voxel_downsample", fail)
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2)
    full = [e[1] for e in log if e[0] in ("create", "append")]
    assert [e[0] for e in log] == ["create"] + ["estimate", "append"] * 3
    del log[:]
    monkeypatch.setattr(harness, "voxel_downsample", thinned)
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, scan_voxel=0.25)
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, scan_voxel=0.25, scan_voxel_centroids=False)
    assert calls["downsample"] == [(n, 0.25) for n in full] * 2 and calls["centroids"] == []
    del log[:], calls["downsample"][:]
    # the flag: every frame, frame 0 included, through voxel_centroids and none through voxel_downsample
    monkeypatch.setattr(harness, "voxel_centroids", centroids)
    monkeypatch.setattr(harness, "voxel_downsample", fail)
    harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, scan_voxel=0.25, scan_voxel_centroids=True)
    assert calls["centroids"] == [(n, 0.25) for n in full]
    assert [e[0] for e in log] == ["create"] + ["estimate", "append"] * 3
    sizes = [e[1] for e in log]
    assert sizes[0] < full[0] and sizes[1] == sizes[2] < full[1]  # the estimate and the append see the centroids
    # the flag without a size
    with pytest.raises(ValueError):
        harness.run_scan_to_map(packets, icp_factory=Fake, max_iter=2, scan_voxel_centroids=True)
    with pytest.raises(SystemExit):
        harness.main(["scan2map", "--scan-voxel-centroids"])


# ------------------------------------------------------------------------- kernel resources ----
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_centroid_kernels_do_not_spill_and_leave_room_for_four_waves_per_simd():
    """no scratch and at most 128 VGPRs (512 per lane of a SIMD: four waves) in every kernel of voxel_mean.hip; the names
    stay clear of the budgeted search / evaluation kernels (tests/test_registers.py)"""
    from test_registers import BUDGET

    regs = _usage("voxel_mean.hip")
    kernels = [k for k in regs if not k.endswith("#scratch")]
    for frag in ("k_vm_place", "k_vm_keyILi2E", "k_vm_keyILi3E", "k_vm_starts", "k_vm_foldILi2E", "k_vm_foldILi3E",
                 "k_vm_itemsILi2E", "k_vm_itemsILi3E", "k_vm_topILi2E", "k_vm_topILi3E", "k_compact_chunks"):
        assert len([k for k in kernels if frag in k]) == 1, (frag, kernels)
    for k in kernels:
        assert regs.get(k + "#scratch", 0) == 0, (k, regs.get(k + "#scratch"))
        assert regs[k] <= 128, (k, regs[k])
        assert not any(frag in k for frag in BUDGET), k
