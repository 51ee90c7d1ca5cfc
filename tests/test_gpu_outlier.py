"""EXTENSION beyond the reference (include/icp_mi355x.h section 23): the exact k-nearest target lists and the two
neighbourhood outlier filters, held to the numpy restatements of tests/test_outlier_abi.py bit for bit (lists: idx, and
d2 as uint64; filters: new_index, removed, the kept cloud's bytes, the statistics' bits), and to the crop's contract
(tests/test_gpu_crop.py): afterwards the handle is a fresh Icp*::new on the kept cloud."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import icp_rust_amd as I
import tie_clouds as TC
from icp_rust_amd import _lib
from icp_rust_amd.scans import load_scan2d
from test_gpu_crop import _cls, _same_bytes, assert_equals_fresh
from test_gpu_crop import keep_mask as disc_mask
from test_outlier_abi import (GONE, INF, RADIUS_SETTINGS, ROOT, STAT_SETTINGS, TIE_NAMES, cloud3, golden_scan, lists_of,
                              new_index_of, radius_keep, statistical_keep)
from test_voxel_abi import keep_mask as voxel_mask

pytestmark = pytest.mark.gpu

KS = (1, 3, 16, 17, 32)


@functools.lru_cache(maxsize=None)
def points(name):
    if name == "scan":
        p = golden_scan()
    elif name == "cloud3":
        p = cloud3()
    elif name == "grid3":  # above the 8 192 targets where the grid is the engine of the searches
        p = np.ascontiguousarray(np.random.default_rng(12).normal(size=(9_000, 3)) * np.array([4.0, 4.0, 0.5]))
    else:
        p = TC.by_name(name).pts
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference_lists(name):
    """the 32 nearest of every target, once per cloud: the lists of a smaller k are their first k columns"""
    idx, d2 = lists_of(points(name), 32)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


def assert_lists(got, want, what=""):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float64
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64)), what


def by_device(icp, k, first, count):
    import torch

    d_idx = torch.full((max(count, 1), k), 7, dtype=torch.int32, device="cuda")
    d_d2 = torch.full((max(count, 1), k), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = I.lib().icp_target_neighbours_device(icp._h, k, first, count, C.c_void_p(d_idx.data_ptr()),
                                              C.c_void_p(d_d2.data_ptr()))
    assert rc == _lib.OK
    icp.synchronize()
    return d_idx[:count].cpu().numpy().view(np.uint32), d_d2[:count].cpu().numpy()


# ------------------------------------------------------------------------------------ the lists ----
@pytest.mark.parametrize("name", TIE_NAMES + TC.TINY_NAMES + ("scan", "cloud3"))
def test_lists_equal_the_restatement_bit_for_bit(name):
    """exact ties at every place of a list (the lattices), far offsets and a slack beyond the cloud (+far, +x31, +split),
    coincident targets (slabdup, stripdup), clouds with m < k (the tiny ones: padded tails), both KMAX"""
    p = points(name)
    want = reference_lists(name)
    icp = _cls(p.shape[1])(p)
    for k in KS:
        assert_lists(icp.neighbours(k), (want[0][:, :k], want[1][:, :k]), (name, k))
    if len(p) < 32:
        got = icp.neighbours(32)
        assert np.all(got[0][:, len(p):] == GONE) and np.all(got[1][:, len(p):] == INF)
    assert_lists(by_device(icp, 17, 0, len(p)), (want[0][:, :17], want[1][:, :17]), name)
    icp.close()


@pytest.mark.parametrize("name", ["scan", "cloud3", "grid3"])
def test_sub_ranges_host_and_device(name):
    p = points(name)
    m = len(p)
    want = reference_lists(name)
    icp = _cls(p.shape[1])(p)
    for first in (0, 63, 64, 65, m - 1):
        for count in (0, 63, 64, 65, m - 1):
            if first + count > m:
                continue
            k = 5 if (first + count) % 2 else 20
            rows = slice(first, first + count)
            assert_lists(icp.neighbours(k, first, count), (want[0][rows, :k], want[1][rows, :k]), (first, count))
            assert_lists(by_device(icp, k, first, count), (want[0][rows, :k], want[1][rows, :k]), (first, count))
    idx = np.zeros((m, 4), dtype=np.uint32)  # either output may be NULL
    assert I.lib().icp_target_neighbours(icp._h, 4, 0, m, C.c_void_p(idx.ctypes.data), None) == _lib.OK
    assert np.array_equal(idx, want[0][:, :4])
    d2 = np.zeros((m, 4))
    assert I.lib().icp_target_neighbours(icp._h, 4, 0, m, None, C.c_void_p(d2.ctypes.data)) == _lib.OK
    assert np.array_equal(d2.view(np.uint64), np.ascontiguousarray(want[1][:, :4]).view(np.uint64))
    icp.close()


def test_list_statuses_that_read_the_handle():
    p = points("cloud3")
    icp = I.Icp3d(p)
    L = I.lib()
    assert L.icp_target_neighbours(icp._h, 3, len(p), 0, None, None) == _lib.OK  # count == 0
    assert L.icp_target_neighbours(icp._h, 3, len(p), 1, None, None) == _lib.BAD_ARGUMENT
    assert L.icp_target_neighbours_device(icp._h, 3, 1, len(p), None, None) == _lib.BAD_ARGUMENT
    assert L.icp_target_neighbours(icp._h, 3, 2 ** 63, 2 ** 63, None, None) == _lib.BAD_ARGUMENT  # (first + count wraps)
    icp.close()
    empty = I.Icp3d(np.zeros((0, 3)))
    assert L.icp_target_neighbours(empty._h, 3, 0, 0, None, None) == _lib.EMPTY_DST
    empty.close()
    bad = p.copy()
    bad[5, 1] = np.inf  # an infinite target: the handle has no grid, and compute_normals refuses it alike
    nogrid = I.Icp3d(bad)
    assert L.icp_compute_target_normals(nogrid._h, 5) == _lib.BAD_ARGUMENT
    assert L.icp_target_neighbours(nogrid._h, 3, 0, 1, None, None) == _lib.BAD_ARGUMENT
    removed = C.c_size_t(0)
    assert L.icp_remove_radius_outliers(nogrid._h, 1.0, 2, None, C.byref(removed)) == _lib.BAD_ARGUMENT
    assert L.icp_remove_statistical_outliers(nogrid._h, 4, 1.0, None, C.byref(removed), None) == _lib.BAD_ARGUMENT
    nogrid.close()


def test_lists_after_an_append_that_moves_the_records_and_a_crop_that_rebuilds_the_grid():
    p = points("grid3")
    rng = np.random.default_rng(13)
    extra = np.ascontiguousarray(p[rng.choice(len(p), 700, replace=False)] + rng.normal(size=(700, 3)) * 0.01)
    icp = I.Icp3d(p)
    icp.append(extra)
    assert icp.append_counters() == (1, 0)
    cloud = np.ascontiguousarray(np.concatenate([p, extra]))
    fresh = I.Icp3d(cloud)
    want = lists_of(cloud, 20)
    for k in (7, 20):
        got = icp.neighbours(k)
        assert_lists(got, fresh.neighbours(k), k)
        assert_lists(got, (want[0][:, :k], want[1][:, :k]), k)
    fresh.close()
    mask = disc_mask(cloud, (0.0, 0.0), 3.0)
    assert 0 < mask.sum() < len(cloud) / 1.5
    icp.crop((0.0, 0.0), 3.0)
    assert icp.crop_counters() == (0, 1)
    kept = np.ascontiguousarray(cloud[mask])
    fresh = I.Icp3d(kept)
    want = lists_of(kept, 20)
    for k in (7, 20):
        got = icp.neighbours(k)
        assert_lists(got, fresh.neighbours(k), k)
        assert_lists(got, (want[0][:, :k], want[1][:, :k]), k)
    fresh.close()
    icp.close()


def test_lists_of_a_handle_whose_engine_is_the_sweep_and_of_one_on_the_grid():
    """a handle below the grid's threshold has a grid all the same: the lists are served from it"""
    for name, mode in (("cloud3", I.NN_BRUTE), ("grid3", I.NN_GRID)):
        p = points(name)
        icp = I.Icp3d(p)
        assert I.lib().icp_get_nn_mode(icp._h) in (I.NN_AUTO, mode)
        want = reference_lists(name)
        assert_lists(icp.neighbours(9), (want[0][:, :9], want[1][:, :9]), name)
        forced = I.Icp3d(p, nn_mode=I.NN_BRUTE)
        assert_lists(forced.neighbours(9), (want[0][:, :9], want[1][:, :9]), name)
        forced.close()
        icp.close()


# ---------------------------------------------------------------------------- the radius filter ----
def assert_removal(icp, p, mask, got):
    removed, index = got
    assert removed == len(p) - mask.sum() and icp.m == icp.target_count == mask.sum()
    assert np.array_equal(index, new_index_of(mask))
    if mask.any():
        assert _same_bytes(icp.read_targets(), p[mask])


def assert_radius(p, radius, need):
    mask = radius_keep(p, radius, need)
    icp = _cls(p.shape[1])(p)
    assert_removal(icp, p, mask, icp.remove_radius_outliers(radius, need, return_index=True))
    moved = not mask.sum() < len(p) / 1.5
    want = (0, 0) if mask.all() else ((1, 0) if moved and mask.any() else (0, 1))
    assert icp.outlier_counters() == want and icp.crop_counters() == (0, 0) and icp.thin_counters() == (0, 0)
    icp.close()
    return mask


@pytest.mark.parametrize("name", ["scan", "cloud3"])
def test_radius_filter_equals_the_restatement_at_the_mid_settings(name):
    p = points(name)
    for radius, need in RADIUS_SETTINGS[name]:
        mask = assert_radius(p, radius, need)
        assert 0.03 * len(p) <= len(p) - mask.sum() and mask.sum() >= 0.5 * len(p)


def test_radius_filter_on_the_boundary_inputs():
    c = TC.cloud("slab")
    assert assert_radius(c.pts, c.spacing, 5).sum() == c.m - 8  # `<=`: an exact d2 == r * r counts
    assert not assert_radius(c.pts, c.spacing, 7).any()
    assert round(float(assert_radius(c.pts, 2 * c.spacing, 20).mean()), 2) == 0.84
    for name in ("slab+far", "strip200x3+x31", "strip200x3+split", "lat40x30"):
        c = TC.cloud(name)
        assert 0 < assert_radius(c.pts, c.spacing, 5).sum() < c.m, name


def test_radius_filter_at_the_edges_of_its_arguments():
    dup = TC.cloud("stripdup")  # every point three times: at radius 0 only coincident points count
    assert assert_radius(dup.pts, 0.0, 3).all()
    assert not assert_radius(dup.pts, 0.0, 4).any()
    for name in ("scan", "cloud3"):
        p = points(name)
        m = len(p)
        assert assert_radius(p, INF, m).all()
        assert not assert_radius(p, INF, m + 1).any()
        assert assert_radius(p, 1e6, m).all()  # a finite radius larger than the whole cloud
        assert not assert_radius(p, 1e6, m + 1).any()
        assert not assert_radius(p, 1e300, 2 ** 40).any()
        assert assert_radius(p, 0.0, 0).all() and assert_radius(p, 0.0, 1).all()
        assert assert_radius(p[:1], 1.0, 1).all() and not assert_radius(p[:1], 1.0, 2).any()  # m == 1


# ----------------------------------------------------------------------- the statistical filter ----
def assert_statistical(p, k, ratio):
    mask, stats = statistical_keep(p, k, ratio)
    icp = _cls(p.shape[1])(p)
    removed, index, got = icp.remove_statistical_outliers(k, ratio, return_index=True, return_stats=True)
    assert np.array_equal(np.array(got).view(np.uint64), np.array(stats).view(np.uint64)), (got, stats)
    assert_removal(icp, p, mask, (removed, index))
    icp.close()
    return mask, stats


@pytest.mark.parametrize("name", ["scan", "cloud3"])
def test_statistical_filter_equals_the_restatement_at_the_mid_settings(name):
    p = points(name)
    for k, ratio in STAT_SETTINGS[name]:
        mask, _ = assert_statistical(p, k, ratio)
        assert 0.03 * len(p) <= len(p) - mask.sum() and mask.sum() >= 0.5 * len(p)
    for ratio in (0.0, -1.0, INF, -INF):
        mask, stats = assert_statistical(p, 8, ratio)
        assert mask.all() if ratio == INF else (not mask.any() if ratio == -INF else not mask.all())


def test_statistical_filter_at_the_edges_of_the_tree_and_of_k():
    p = points("cloud3")
    mask, stats = assert_statistical(p[:1], 8, 1.0)  # m == 1: nothing removed, the statistics are +0.0
    assert mask.all() and stats == (0.0, 0.0, 0.0)
    assert_statistical(p[:2], 8, 1.0)  # ke = 1
    assert_statistical(p[:2], 8, -1.0)
    for m in (256, 257, 513):  # one group, two groups of the tree
        for k in (1, 5, 31):
            assert_statistical(p[:m], k, 0.5)
    for m in (5, 17, 31):  # k >= m: ke = m - 1
        assert_statistical(p[:m], 31, 0.0)
    for name in ("slab", "stripdup", "strip200x3+split", "five2", "cube"):
        c = TC.by_name(name)
        assert_statistical(c.pts, 6, 0.0)
        assert_statistical(c.pts, 2, 1.0)  # (stripdup: u == 0 for every target)


def test_statistical_filter_keeps_the_unit_cube_at_ratio_zero():
    """every u is 1, the mean 1, the deviation 0, the threshold 1: `u > threshold` removes nothing (`>=` would remove
    all eight)"""
    p = np.ascontiguousarray(TC.box(2, 2, 2).astype(np.float64))
    mask, stats = assert_statistical(p, 3, 0.0)
    assert mask.all() and stats == (1.0, 0.0, 1.0)
    mask, stats = assert_statistical(p, 3, INF)  # inf * 0: a NaN threshold keeps everything
    assert mask.all() and math.isnan(stats[2])


def test_an_infinite_mean_distance_gives_a_nan_threshold_and_nothing_is_removed():
    """One coordinate at 1e308: the d2 of that target to any other overflows to +inf, a distance like any other; its u
    is +inf, so the mean is +inf, u - mean is NaN for that target, the deviation and the threshold are NaN, and
    !(u > NaN) keeps every target.  Nothing is removed: the documented behaviour, not an error."""
    p = points("cloud3")[:400].copy()
    p[123, 1] = 1e308
    mask, stats = assert_statistical(p, 8, 1.0)
    assert mask.all() and stats[0] == INF and math.isnan(stats[1]) and math.isnan(stats[2])
    want = lists_of(p, 4)
    icp = I.Icp3d(p)
    assert_lists(icp.neighbours(4), want)
    assert want[1][123, 1] == INF and want[1][123, 0] == 0.0
    icp.close()


# ------------------------------------------------------------------- after either filter ----
def _filters(name):
    radius, need = RADIUS_SETTINGS[name][1]
    k, ratio = STAT_SETTINGS[name][1]
    return (("radius", lambda icp: icp.remove_radius_outliers(radius, need), lambda p: radius_keep(p, radius, need)),
            ("statistical", lambda icp: icp.remove_statistical_outliers(k, ratio),
             lambda p: statistical_keep(p, k, ratio)[0]))


@pytest.mark.parametrize("name", ["scan", "cloud3", "grid3"])
def test_the_handle_equals_a_fresh_one_on_the_kept_cloud(name):
    rng = np.random.default_rng(17)
    p = points(name)
    dim = p.shape[1]
    if name == "scan":
        src = np.ascontiguousarray(load_scan2d(os.path.join(ROOT, "tests", "golden", "scans2d", "002.txt")))
        q = src
    else:
        src = np.ascontiguousarray(p[rng.choice(len(p), 2_000, replace=False)] + rng.normal(size=(1, dim)) * 0.01)
        q = np.ascontiguousarray(rng.normal(size=(1_500, dim)))
    setting = "scan" if name == "scan" else "cloud3"
    for what, apply, rule in _filters(setting):
        mask = rule(p)
        assert 0 < mask.sum() < len(p), what
        icp = _cls(dim)(p)
        if dim == 3:
            icp.compute_normals(8)
            normals = icp.read_normals()
        else:
            icp.compute_line_normals(8)
            normals = icp.read_line_normals()
        assert apply(icp) == len(p) - mask.sum()
        moved = not mask.sum() < len(p) / 1.5
        assert icp.outlier_counters() == ((1, 0) if moved else (0, 1)), what
        got = icp.read_normals() if dim == 3 else icp.read_line_normals()
        assert _same_bytes(got, normals[mask]), what  # carried over
        kept = np.ascontiguousarray(p[mask])
        assert_equals_fresh(icp, kept, dim, q, src, I.Transform([0.01, 0.02, -0.01]), brute=len(p) < 8_192)
        if name == "grid3":  # (the lists of the moved records against a fresh handle's: both are the device's)
            fresh = I.Icp3d(kept)
            assert_lists(icp.neighbours(6), fresh.neighbours(6), what)
            fresh.close()
        else:
            assert_lists(icp.neighbours(6), lists_of(kept, 6), what)
        icp.close()


def test_nothing_removed_leaves_the_handle_borrowing_and_everything_removed_takes_an_append():
    import torch

    p = points("cloud3")
    d_p = torch.from_numpy(np.array(p)).cuda()
    icp = I.Icp3d(d_p)
    removed, index = icp.remove_radius_outliers(0.5, 1, return_index=True)
    assert removed == 0 and np.array_equal(index, np.arange(len(p), dtype=np.uint32))
    removed, index, stats = icp.remove_statistical_outliers(8, INF, return_index=True, return_stats=True)
    assert removed == 0 and np.array_equal(index, np.arange(len(p), dtype=np.uint32)) and stats[2] == INF
    assert icp.outlier_counters() == (0, 0) and icp._keep is d_p and icp.target_count == len(p)
    d_p[5, 0] = 123.0  # still reading the caller's tensor
    torch.cuda.synchronize()
    assert icp.read_targets(5, 1)[0, 0] == 123.0
    d_p[5, 0] = float(p[5, 0])
    torch.cuda.synchronize()
    removed, index = icp.remove_radius_outliers(0.5, len(p) + 1, return_index=True)
    assert removed == len(p) and icp.target_count == 0 and np.all(index == GONE) and icp._keep is None
    assert _same_bytes(d_p.cpu().numpy(), p)  # a borrowed cloud is never written
    assert icp.outlier_counters() == (0, 1)
    extra = np.ascontiguousarray(p[:2_000] + 0.25)
    icp.append(extra)
    rng = np.random.default_rng(3)
    assert_equals_fresh(icp, extra, 3, np.ascontiguousarray(rng.normal(size=(500, 3))), extra[:600] + 0.01,
                        I.Transform([0.01, 0.0, 0.0]), brute=True)
    mask = statistical_keep(extra, 8, 1.0)[0]
    assert icp.remove_statistical_outliers(8, 1.0) == len(extra) - mask.sum() > 0
    assert _same_bytes(icp.read_targets(), extra[mask])
    icp.close()


def test_one_chain_of_append_filter_thin_crop_and_a_plane_registration():
    rng = np.random.default_rng(23)
    # (6 000 targets: the sweep is the engine until the append takes the cloud past 8 192, where the grid takes over)
    base, extra = np.array(points("grid3")[:6_000]), np.array(points("cloud3")) * np.array([3.0, 3.0, 0.4])
    icp = I.Icp3d(base)
    icp.compute_normals(8)
    icp.append(extra)
    icp.update_normals(8)
    normals = icp.read_normals()
    cloud = np.ascontiguousarray(np.concatenate([base, extra]))
    for step in ("statistical", "thin", "crop"):
        if step == "statistical":
            mask = statistical_keep(cloud, 10, 1.0)[0]
            removed = icp.remove_statistical_outliers(10, 1.0)
        elif step == "thin":
            mask = voxel_mask(cloud, 0.3)
            removed = icp.thin(0.3)
        else:
            mask = disc_mask(cloud, (0.5, -0.5), 6.0)
            removed = icp.crop((0.5, -0.5), 6.0)
        assert removed == len(cloud) - mask.sum() > 0, step
        cloud, normals = np.ascontiguousarray(cloud[mask]), normals[mask]
    assert _same_bytes(icp.read_targets(), cloud) and _same_bytes(icp.read_normals(), normals)
    assert sum(icp.outlier_counters()) == sum(icp.thin_counters()) == sum(icp.crop_counters()) == 1
    src = np.ascontiguousarray(cloud[rng.choice(len(cloud), 1_500, replace=False)] + rng.normal(0, 1e-3, (1_500, 3)))
    init = I.Transform([0.02, -0.01, 0.005])
    icp.compute_normals(8)
    fresh = I.Icp3d(cloud)
    fresh.compute_normals(8)
    assert _same_bytes(icp.read_normals(), fresh.read_normals())
    a = icp.estimate_point_to_plane(src, init, 6, return_info=True)
    b = fresh.estimate_point_to_plane(src, init, 6, return_info=True)
    assert _same_bytes(a[0].as_array(), b[0].as_array()) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    fresh.close()
    icp.close()


def test_the_same_calls_on_two_handles_give_the_same_bytes():
    p = points("grid3")
    a, b = I.Icp3d(p), I.Icp3d(p)
    la, lb = a.neighbours(32), b.neighbours(32)
    assert _same_bytes(la[0], lb[0]) and _same_bytes(la[1], lb[1])
    ra = a.remove_statistical_outliers(16, 1.0, return_index=True, return_stats=True)
    rb = b.remove_statistical_outliers(16, 1.0, return_index=True, return_stats=True)
    assert ra[0] == rb[0] > 0 and _same_bytes(ra[1], rb[1]) and _same_bytes(np.array(ra[2]), np.array(rb[2]))
    ra, rb = a.remove_radius_outliers(0.3, 6, return_index=True), b.remove_radius_outliers(0.3, 6, return_index=True)
    assert ra[0] == rb[0] > 0 and _same_bytes(ra[1], rb[1])
    assert _same_bytes(a.read_targets(), b.read_targets())
    a.close()
    b.close()


# ----------------------------------------------------------------------- module-level functions ----
@pytest.mark.parametrize("name", ["scan", "cloud3"])
def test_module_level_filters_agree_with_the_handle_path(name):
    import torch

    p = points(name)
    d_p = torch.from_numpy(np.array(p)).cuda()
    radius, need = RADIUS_SETTINGS[name][0]
    k, ratio = STAT_SETTINGS[name][0]
    for call, mask in ((lambda x, **kw: I.remove_radius_outliers(x, radius, need, **kw), radius_keep(p, radius, need)),
                       (lambda x, **kw: I.remove_statistical_outliers(x, k, ratio, **kw),
                        statistical_keep(p, k, ratio)[0])):
        want = np.flatnonzero(mask)
        out, idx = call(p, return_index=True)
        assert idx.dtype == np.uint32 and np.array_equal(idx, want) and _same_bytes(out, p[mask])
        assert _same_bytes(call(p), p[mask])
        d_out, d_idx = call(d_p, return_index=True)
        assert d_out.is_cuda and d_idx.is_cuda
        assert _same_bytes(d_out.cpu().numpy(), p[mask]) and np.array_equal(d_idx.cpu().numpy(), want)
    assert len(I.remove_radius_outliers(np.zeros((0, 3)), 1.0, 2)) == 0
