"""The stable compaction behind the handle removals (compact_device.hpp: tiles of 1 024 = four rounds of 256 = four
waves of 64 per round) at its own edges: target counts one either side of a wave, a round and a tile, and masks that
empty a lane, a wave's first lane everywhere, a whole round or a whole tile.  icp_remove_targets runs k_mask_marks,
k_crop_place, k_crop_rec_mark and k_crop_rec_place; the two outlier filters run k_outlier_count in both of its modes.
Every expectation is numpy's: the cumsum restatement of new_index, cloud[keep], and a fresh handle on the kept cloud."""
import numpy as np
import pytest

import icp_rust_amd as I
from test_gpu_crop import _cloud, _cls, _same_bytes, new_index_of
from test_gpu_outlier import assert_radius, assert_statistical, points
from test_p2plane import room

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)


def masks(m, rng):
    """(name, keep) for a cloud of m targets: element 0, the last, lane 0 of every wave, the second round, the second
    tile (clouds that reach into a third), all but the last, and a random mask that keeps under 2/3.  A round the cloud
    ends before drops what there is of it."""
    out = []

    def add(name, drop=None, keep=None):
        k = np.ones(m, dtype=bool) if keep is None else keep
        if drop is not None:
            k[drop] = False
        out.append((name, k))

    add("first", drop=[0])
    add("last", drop=[m - 1])
    add("lane0", drop=slice(0, m, 64))
    add("round", drop=slice(256, 512))
    if m >= 2049:
        add("tile", drop=slice(1024, 2048))
    only_last = np.zeros(m, dtype=bool)
    only_last[m - 1] = True
    add("only-last", keep=only_last)
    r = rng.uniform(size=m) < 0.5
    while r.sum() * 1.5 >= m:  # (keeps under 2/3: the grid is rebuilt)
        r[np.flatnonzero(r)[0]] = False
    add("random", keep=r)
    return out


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("dim", [2, 3])
def test_remove_by_mask_at_the_edges_of_wave_round_and_tile(dim, m):
    rng = np.random.default_rng(9000 * dim + m)
    cloud = _cloud(rng, m, dim)
    q = _cloud(rng, 500, dim)
    for name, keep in masks(m, rng):
        what = (dim, m, name)
        kept = int(keep.sum())
        icp = _cls(dim)(cloud, nn_mode=I.NN_GRID)  # (the grid at every size: the searches read the records)
        removed, index = icp.remove(keep, return_index=True)
        if kept == m:  # (the round of a cloud that ends before it) nothing to remove: the handle is left as it was
            assert removed == 0 and np.array_equal(index, np.arange(m, dtype=np.uint32)), what
            assert icp.remove_counters() == (0, 0) and icp.target_count == m, what
            icp.close()
            continue
        assert removed == m - kept and icp.m == icp.target_count == kept, what
        assert index.dtype == np.uint32 and np.array_equal(index, new_index_of(keep)), what
        moved = kept > 0 and not kept < m / 1.5
        assert icp.remove_counters() == ((1, 0) if moved else (0, 1)), what
        rest = np.ascontiguousarray(cloud[keep])
        assert _same_bytes(icp.read_targets(), rest), what
        if kept > 0:
            fresh = _cls(dim)(rest, nn_mode=I.NN_GRID)
            assert np.array_equal(icp.nn_search(q), fresh.nn_search(q)), what
            fresh.close()
        icp.close()


@pytest.mark.parametrize("extra", [1, 2, 1025])
def test_normals_that_end_inside_or_at_the_edge_of_a_tile_follow_their_targets(extra):
    """normals on 1 024 targets and an append without an update: the place launch counts the survivors among the first
    normals_m targets at element normals_m, the first of the second tile"""
    normals_m = 1024
    rng = np.random.default_rng(300 + extra)
    base, more = room(rng, normals_m), room(rng, extra)
    cloud = np.ascontiguousarray(np.concatenate([base, more]))
    m = len(cloud)
    for drop in (0, normals_m - 1, normals_m):
        what = (extra, drop)
        icp = I.Icp3d(base)
        icp.compute_normals(8)
        before = icp.read_normals()
        icp.append(more)
        keep = np.ones(m, dtype=bool)
        keep[drop] = False
        removed, index = icp.remove(keep, return_index=True)
        assert removed == 1 and np.array_equal(index, new_index_of(keep)), what
        assert _same_bytes(icp.read_targets(), cloud[keep]), what
        had = int(keep[:normals_m].sum())
        if had < m - 1:  # the appended targets that were kept have no normal yet
            with pytest.raises(I.IcpError):
                icp.read_normals()
            icp.update_normals(8)
        want = before[keep[:normals_m]]
        assert _same_bytes(icp.read_normals()[:had], want), what
        # a second removal: the handle's count of normals was right, and they still follow
        now = np.ascontiguousarray(cloud[keep])
        normals = icp.read_normals()
        again = np.ones(len(now), dtype=bool)
        again[[0, had - 1]] = False
        removed, index = icp.remove(again, return_index=True)
        assert removed == 2 and np.array_equal(index, new_index_of(again)), what
        assert _same_bytes(icp.read_targets(), now[again]), what
        assert _same_bytes(icp.read_normals(), normals[again]), what
        icp.close()


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_outlier_filters_either_side_of_a_tile(m):
    """k_outlier_count's two modes: the radius filter's mark words, and u against the threshold"""
    p = np.ascontiguousarray(points("cloud3")[:m])
    mask = assert_radius(p, 0.3, 5)
    assert 0 < mask.sum() < m
    mask, _ = assert_statistical(p, 8, 1.0)
    assert 0 < mask.sum() < m
