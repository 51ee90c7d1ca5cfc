"""EXTENSION beyond the reference (include/icp_mi355x.h section 24): neighbour lists and radius counts of ARBITRARY points
against a handle's targets, and the removal of targets by the caller's mask -- held to the numpy restatements of
tests/test_query_abi.py bit for bit (idx; d2 as uint64; counts; new_index; the kept cloud's bytes), to the calls that
exist already (neighbours, nn_search, remove_radius_outliers) and to the crop's contract (tests/test_gpu_crop.py):
after a removal the handle is a fresh Icp*::new on the kept cloud.  There is no tolerance anywhere."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import icp_rust_amd as I
import tie_clouds as TC
from icp_rust_amd import _lib
from icp_rust_amd.scans import load_scan2d
from test_gpu_crop import _cls, _same_bytes, assert_equals_fresh
from test_gpu_crop import keep_mask as disc_mask
from test_outlier_abi import ROOT, golden_scan, new_index_of, radius_keep
from test_query_abi import FULL, GONE, INF, NAN, count_within_ref, mask_keep, query_lists
from test_voxel_abi import keep_mask as voxel_mask

pytestmark = pytest.mark.gpu

KS = (1, 5, 16, 17, 32)  # both KMAX variants and their boundary
POSE = (0.21, -0.13, 0.37)
CELL_ORDER_FROM = 250_000  # the adopted threshold: calls with at least this many points are sorted
LATTICES = ("slab", "slabdup", "lat40x30", "stripdup", "slab+far", "strip200x3+split")


def _transform(param):
    return None if param is None else I.Transform(list(param))


# ------------------------------------------------------------------------------- the inputs ----
def mixed_queries(t, rng, interior):
    """interior points; points outside each face of the box, near and far; points at tie_clouds.FAR and at 2^40 times the
    box's extent; some targets themselves; one NaN and one +inf query"""
    dim = t.shape[1]
    lo, hi = t.min(0), t.max(0)
    ext = float(np.max(hi - lo)) or 1.0
    q = [rng.uniform(lo, hi, (interior, dim)), t[rng.integers(0, len(t), 40)]]
    for axis in range(dim):
        for side, off in ((-1, 0.3), (1, 0.3), (-1, 5.0), (1, 5.0)):
            f = rng.uniform(lo, hi, (6, dim))
            f[:, axis] = (lo[axis] if side < 0 else hi[axis]) + side * off * ext * rng.uniform(0.5, 1.0, 6)
            q.append(f)
    centre = (lo + hi) / 2
    far = np.tile(centre, (6, 1))
    far[0] += np.array(TC.FAR[:dim], dtype=np.float64)
    far[1] -= np.array(TC.FAR[:dim], dtype=np.float64)
    far[2, 0] += 2.0 ** 40 * ext
    far[3, 1] -= 2.0 ** 40 * ext
    far[4] += 2.0 ** 40 * ext
    far[5, dim - 1] += 2.0 ** 40 * ext
    special = np.tile(centre, (2, 1))
    special[0, 1] = NAN
    special[1, 0] = INF
    return np.ascontiguousarray(np.concatenate(q + [far, special]))


@functools.lru_cache(maxsize=None)
def case(name):
    """(targets, queries) of a named case, read-only"""
    rng = np.random.default_rng(31)
    if name == "scan":  # a golden 2-D scan pair: frame 001 as the map, frame 002 and the mix as the queries
        t = golden_scan()
        scan = np.ascontiguousarray(load_scan2d(os.path.join(ROOT, "tests", "golden", "scans2d", "002.txt")))
        q = np.concatenate([scan, mixed_queries(t, rng, 50)])
    elif name == "random3":  # 3 000 targets, 2 000 queries
        t = np.ascontiguousarray(rng.normal(size=(3_000, 3)) * np.array([4.0, 3.0, 0.5]))
        mix = mixed_queries(t, rng, 0)
        q = np.concatenate([rng.normal(size=(2_000 - len(mix), 3)) * np.array([4.5, 3.5, 0.7]), mix])
        assert len(q) == 2_000
    elif name == "tiny3":  # m = 3: a row of k = 8 ends in padding
        t = TC.tiny("three3").pts
        q = mixed_queries(t, rng, 20)
    else:  # a lattice: its midpoints along every axis and along all at once (many equal d2), and every (duplicated) target
        c = TC.cloud(name)
        t = c.pts
        half = c.spacing / 2
        mids = [t + half * np.eye(c.dim)[a] for a in range(c.dim)] + [t + half]
        q = np.concatenate([t] + mids + [mixed_queries(t, rng, 10)])
    t, q = np.ascontiguousarray(t), np.ascontiguousarray(q)
    t.setflags(write=False)
    q.setflags(write=False)
    return t, q


@functools.lru_cache(maxsize=None)
def reference_lists(name, pose):
    """the 32 nearest of every query of a case, once: the lists of a smaller k are their first k columns"""
    t, q = case(name)
    idx, d2 = query_lists(t, q, 32, _transform(pose))
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


def assert_lists(got, want, what=""):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.float64
    assert got[0].shape == want[0].shape, what
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64)), what


def on_device(icp, q, k, transform=None):
    import torch

    idx, d2 = icp.query(torch.from_numpy(np.array(q)).cuda(), k, transform)
    assert idx.is_cuda and d2.is_cuda
    return idx.cpu().numpy().view(np.uint32), d2.cpu().numpy()


# ------------------------------------------------------------------------------------ 1. the lists ----
@pytest.mark.parametrize("name,pose", [("scan", POSE), ("scan", None), ("random3", None), ("random3", POSE)] +
                         [(n, None) for n in LATTICES] + [("slab", POSE), ("lat40x30", POSE)])
def test_lists_equal_the_restatement_bit_for_bit(name, pose):
    t, q = case(name)
    want = reference_lists(name, pose)
    assert np.isnan(q).any(axis=1).sum() == 1 and np.isinf(q).any(axis=1).sum() == 1
    if name in LATTICES and pose is None:  # the lattice midpoints: ties at the k-th place decide rows (a pose rounds them away)
        tied = np.mean(want[1][:, 4] == want[1][:, 5])
        assert tied > 0.2, tied
    icp = _cls(t.shape[1])(t)
    T = _transform(pose)
    for k in KS:
        assert_lists(icp.query(q, k, T), (want[0][:, :k], want[1][:, :k]), (name, k))
    assert_lists(on_device(icp, q, 17, T), (want[0][:, :17], want[1][:, :17]), name)
    assert icp.query_counters() == (0, len(KS) + 1)
    icp.close()


def test_the_special_queries_get_what_the_two_rules_give():
    t, q = case("random3")
    icp = I.Icp3d(t)
    idx, d2 = icp.query(q[-2:], 4)
    assert np.all(idx[0] == GONE) and np.all(d2[0] == INF)  # a NaN coordinate: padding only
    assert idx[1].tolist() == [0, 1, 2, 3] and np.all(d2[1] == INF)  # +inf: every d2 is +inf, by index
    idx, d2 = icp.query(q[-2:], 4, I.Transform())  # under the identity POSE 0 * inf is a NaN
    assert np.all(idx == GONE) and np.all(d2 == INF)
    big = np.array([[1e200, 0.0, 0.0], [0.0, 0.0, -1e160]])  # finite, but every d2 overflows: again by index
    idx, d2 = icp.query(big, 3)
    assert idx.tolist() == [[0, 1, 2], [0, 1, 2]] and np.all(d2 == INF)
    assert_lists((idx, d2), query_lists(t, big, 3))
    icp.close()


def test_rows_end_in_padding_when_there_are_fewer_targets_than_k():
    t, q = case("tiny3")
    icp = I.Icp3d(t)
    idx, d2 = icp.query(q, 8)
    assert_lists((idx, d2), query_lists(t, q, 8))
    finite = np.isfinite(q).all(axis=1)
    assert np.all(idx[finite, :3] != GONE) and np.all(idx[:, 3:] == GONE) and np.all(d2[:, 3:] == INF)
    assert_lists(on_device(icp, q, 8), (idx, d2))
    for k in (1, 3, 4, 32):
        assert_lists(icp.query(q, k), query_lists(t, q, k), k)
    icp.close()


def test_either_output_may_be_null_and_no_points_is_a_no_op():
    t, q = case("random3")
    want = reference_lists("random3", None)
    icp = I.Icp3d(t)
    L = I.lib()
    idx = np.zeros((len(q), 4), dtype=np.uint32)
    assert L.icp_query_neighbours(icp._h, C.c_void_p(q.ctypes.data), len(q), None, 4, C.c_void_p(idx.ctypes.data),
                                  None) == _lib.OK
    assert np.array_equal(idx, want[0][:, :4])
    d2 = np.zeros((len(q), 4))
    assert L.icp_query_neighbours(icp._h, C.c_void_p(q.ctypes.data), len(q), None, 4, None,
                                  C.c_void_p(d2.ctypes.data)) == _lib.OK
    assert np.array_equal(d2.view(np.uint64), np.ascontiguousarray(want[1][:, :4]).view(np.uint64))
    got = icp.query(np.zeros((0, 3)), 5)
    assert got[0].shape == (0, 5) and got[1].shape == (0, 5)
    assert icp.count_within(np.zeros((0, 3)), 1.0).shape == (0,)
    icp.close()


def test_statuses_that_read_the_handle():
    t, q = case("random3")
    L = I.lib()
    qp = C.c_void_p(q.ctypes.data)
    counts = np.zeros(len(t) + 1, dtype=np.uint32)
    cp = C.c_void_p(counts.ctypes.data)
    icp = I.Icp3d(t)
    assert L.icp_count_within(icp._h, None, len(t) - 1, None, 1.0, 3, cp) == _lib.BAD_ARGUMENT  # the targets: n == m
    assert L.icp_count_within(icp._h, None, len(t) + 1, None, 1.0, 3, cp) == _lib.BAD_ARGUMENT
    assert L.icp_count_within(icp._h, None, len(t), None, 1.0, 3, cp) == _lib.OK
    icp.close()
    empty = I.Icp3d(np.zeros((0, 3)))
    assert L.icp_query_neighbours(empty._h, qp, 4, None, 3, None, None) == _lib.EMPTY_DST
    assert L.icp_query_neighbours(empty._h, None, 0, None, 3, None, None) == _lib.EMPTY_DST
    assert L.icp_count_within(empty._h, qp, 4, None, 1.0, 3, cp) == _lib.EMPTY_DST
    assert empty.remove(np.zeros(0, dtype=bool)) == 0  # m == 0: a successful no-op
    empty.close()
    bad = np.array(t)
    bad[5, 1] = INF  # an infinite target: the handle has no grid
    nogrid = I.Icp3d(bad)
    assert L.icp_query_neighbours(nogrid._h, qp, 4, None, 3, None, None) == _lib.BAD_ARGUMENT
    assert L.icp_count_within(nogrid._h, qp, 4, None, 1.0, 3, cp) == _lib.BAD_ARGUMENT
    # ... but a removal needs none, like a crop: remove the infinite target and the handle is a fresh one on the rest
    keep = np.isfinite(bad).all(axis=1)
    assert nogrid.remove(keep) == 1 and nogrid.remove_counters() == (0, 1)
    rest = np.ascontiguousarray(bad[keep])
    assert _same_bytes(nogrid.read_targets(), rest)
    assert_lists(nogrid.query(q[:300], 6), query_lists(rest, q[:300], 6))
    nogrid.close()


# ------------------------------------------------ 2. cross-checks against the calls that exist ----
@pytest.mark.parametrize("name", ["scan", "random3", "slab", "slabdup", "lat40x30", "stripdup", "slab+far"])
def test_the_targets_as_queries_give_the_lists_of_neighbours(name):
    t, _ = case(name)
    icp = _cls(t.shape[1])(t)
    for k in (1, 7, 16, 20):
        assert_lists(icp.query(t, k), icp.neighbours(k), (name, k))
    icp.close()


@pytest.mark.parametrize("name", ["scan", "random3", "grid3", "slab", "slabdup", "lat40x30", "stripdup"])
def test_k_1_gives_the_index_of_nn_search(name):
    """on the lattices the queries are midpoints and duplicated targets: the nearest is decided by the lowest index"""
    if name == "grid3":  # above the 8 192 targets where the grid is the engine of nn_search
        rng = np.random.default_rng(12)
        t = np.ascontiguousarray(rng.normal(size=(9_000, 3)) * np.array([4.0, 4.0, 0.5]))
        q = np.ascontiguousarray(rng.normal(size=(2_000, 3)) * np.array([5.0, 5.0, 1.0]))
    else:
        t, q = case(name)
        q = np.ascontiguousarray(q[np.isfinite(q).all(axis=1)])
        q = np.ascontiguousarray(q[np.abs(q - t.mean(0)).max(axis=1) < 2.0 ** 30])  # (tie_clouds.FAR stays in)
    icp = _cls(t.shape[1])(t)
    idx, d2 = icp.query(q, 1)
    assert np.array_equal(idx[:, 0], icp.nn_search(q)), name
    if name in ("slab", "slabdup", "lat40x30", "stripdup"):
        want = query_lists(t, q, 2)
        assert np.mean(want[1][:, 0] == want[1][:, 1]) > 0.5  # the nearest IS a tie for most rows
        assert np.array_equal(idx[:, 0], want[0][:, 0])
    icp.close()


# ----------------------------------------------------------- 3. cell order against caller order ----
def test_a_call_in_cell_order_equals_the_same_queries_in_chunks_in_the_caller_s_order():
    rng = np.random.default_rng(41)
    t = np.ascontiguousarray(rng.normal(size=(20_000, 3)) * np.array([6.0, 5.0, 0.8]))
    n = CELL_ORDER_FROM + 4_463
    q = rng.normal(size=(n, 3)) * np.array([7.0, 6.0, 1.2])
    q[rng.integers(0, n, 50)] = t[rng.integers(0, len(t), 50)]
    q[12_345, 2], q[54_321, 0], q[60_000, 1] = NAN, INF, 2.0 ** 45
    q = np.ascontiguousarray(q)
    T = I.Transform(list(POSE))
    icp = I.Icp3d(t)
    whole = icp.query(q, 8, T)
    assert icp.query_counters() == (1, 0)
    parts = [icp.query(q[at:at + 100_000], 8, T) for at in range(0, n, 100_000)]
    assert icp.query_counters() == (1, len(parts)) and len(parts) == 3
    assert_lists(whole, (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])))
    special = np.array([12_345, 54_321, 60_000])
    rows = np.sort(np.concatenate([rng.choice(np.setdiff1d(np.arange(n), special), 1_997, replace=False), special]))
    assert len(np.unique(rows)) == 2_000
    want = query_lists(t, q[rows], 8, T)
    assert_lists((whole[0][rows], whole[1][rows]), want)
    # ... and so do the counts, and the device entry
    for cap in (3, None):
        counts = icp.count_within(q, 0.4, T, cap=cap)
        chunks = np.concatenate([icp.count_within(q[at:at + 100_000], 0.4, T, cap=cap) for at in range(0, n, 100_000)])
        assert np.array_equal(counts, chunks)
        assert np.array_equal(counts[rows], count_within_ref(t, q[rows], 0.4, cap, T))
    assert icp.query_counters() == (3, 3 + 6)
    assert_lists(on_device(icp, q, 8, T), whole)
    assert icp.query_counters() == (4, 9)
    icp.close()


# ------------------------------------------------------------------------------- 4. the counts ----
def assert_counts(icp, t, q, radius, caps, T=None):
    full = count_within_ref(t, q, radius, None, T)
    for cap in caps:
        got = icp.count_within(q, radius, T, cap=cap)
        assert got.dtype == np.uint32 and np.array_equal(got, np.minimum(full, FULL if cap is None else cap)), (radius, cap)
    return full


@pytest.mark.parametrize("name,pose", [("scan", POSE), ("random3", None), ("random3", POSE), ("slab", None),
                                        ("stripdup", None), ("slab+far", None), ("strip200x3+split", None)])
def test_counts_equal_the_restatement(name, pose):
    t, q = case(name)
    T = _transform(pose)
    icp = _cls(t.shape[1])(t)
    small = {"scan": 40.0, "random3": 0.5}.get(name, 0.3)
    for radius in (0.0, small, INF, 1e200, 30.0 * small):
        full = assert_counts(icp, t, q, radius, (None,), T)
        typical = int(np.median(full[full > 0])) if np.any(full > 0) else 1
        assert_counts(icp, t, q, radius, (1, max(typical - 1, 1), typical, typical + 1, len(t), len(t) + 1, FULL), T)
        if radius == small:
            assert 1 < typical < len(t)
    nan_row, inf_row = len(q) - 2, len(q) - 1
    got = icp.count_within(q, INF, T)  # (x = +inf stays infinite under this pose: both of its products are infinite)
    assert got[nan_row] == 0 and got[inf_row] == len(t) == count_within_ref(t, q[inf_row:], INF, None, T)[0]
    assert icp.count_within(q, 1e100, T)[inf_row] == 0
    icp.close()


@pytest.mark.parametrize("name", ["slab", "lat40x30", "slab+far"])
def test_a_radius_whose_square_is_an_attained_d2_counts_it_and_the_next_double_below_does_not(name):
    c = TC.cloud(name)
    icp = _cls(c.dim)(c.pts)
    q = np.ascontiguousarray(np.concatenate([c.pts, c.pts + c.spacing * np.eye(c.dim)[0]]))
    for steps in (1, 2, 5):
        r = steps * c.spacing
        below = np.nextafter(r, 0.0)
        at, under = count_within_ref(c.pts, q, r), count_within_ref(c.pts, q, below)
        assert np.all(at > under)  # `<=` against `<` decides every row
        assert np.array_equal(under, count_within_ref(c.pts, q, r, strict=True))
        assert np.array_equal(icp.count_within(q, r), at) and np.array_equal(icp.count_within(q, below), under)
        assert np.array_equal(icp.count_within(None, r), count_within_ref(c.pts, None, r))
        assert np.array_equal(icp.count_within(None, below), count_within_ref(c.pts, None, below))
    icp.close()


def test_a_far_query_whose_radius_is_exactly_its_distance_to_the_nearest_target():
    c = TC.cloud("slab")
    t = c.pts
    corner = t[np.lexsort((t[:, 2], t[:, 1], -t[:, 0]))[0]]  # a target on the face x = max
    assert corner[0] == t[:, 0].max()
    icp = I.Icp3d(t)
    # 2^20: inside the block walk's reach, d2 is exact and the one target counts; 2^43: the targets of the face are no
    # longer told apart (48 of them at d2 = 2^86); 2^60: the whole axis is taken, and all 1 152 targets sit at d2 = 2^120
    for e, hits in ((20, 1), (43, 48), (60, c.m)):
        q = np.ascontiguousarray(np.stack([corner + [2.0 ** e, 0, 0], corner - [2.0 ** e + corner[0] - t[:, 0].min(), 0, 0]]))
        r = 2.0 ** e
        want = count_within_ref(t, q, r)
        assert want.tolist() == [hits, hits], (e, want)
        assert count_within_ref(t, q, np.nextafter(r, 0.0)).tolist() == [0, 0]
        assert icp.count_within(q, r).tolist() == [hits, hits], e
        assert icp.count_within(q, r, cap=1).tolist() == [1, 1], e
        assert icp.count_within(q, np.nextafter(r, 0.0)).tolist() == [0, 0], e
        wide = np.nextafter(r, INF)
        assert np.array_equal(icp.count_within(q, wide), count_within_ref(t, q, wide)), e
        lists = icp.query(q, 3)
        assert_lists(lists, query_lists(t, q, 3), e)
        assert lists[1][0, 0] == r * r
    icp.close()


@pytest.mark.parametrize("name,radius,need", [("scan", 50.0, 4), ("random3", 0.4, 5), ("slab", 0.125, 5),
                                               ("slabdup", 0.0, 3)])
def test_the_targets_counted_around_themselves_give_the_keep_rule_of_the_radius_filter(name, radius, need):
    t, _ = case(name)
    a, b = _cls(t.shape[1])(t), _cls(t.shape[1])(t)
    counts = a.count_within(None, radius, cap=need)
    assert np.array_equal(counts, count_within_ref(t, None, radius, need))
    assert np.array_equal(a.count_within(None, radius), count_within_ref(t, None, radius))
    assert np.array_equal(a.count_within(None, radius), a.count_within(np.array(t), radius))
    keep = counts >= need
    assert np.array_equal(keep, radius_keep(t, radius, need)) and 0 < keep.sum()
    removed, index = b.remove_radius_outliers(radius, need, return_index=True)
    assert np.array_equal(keep, index != GONE) and removed == len(t) - keep.sum()
    # the composition: query, decide, remove leaves the handle the filter leaves
    got = a.remove(keep, return_index=True)
    assert got[0] == removed and np.array_equal(got[1], index)
    assert _same_bytes(a.read_targets(), b.read_targets())
    if removed:
        assert sum(a.remove_counters()) == 1 and a.outlier_counters() == (0, 0)
        assert sum(b.outlier_counters()) == 1 and b.remove_counters() == (0, 0)
    a.close()
    b.close()


# ------------------------------------------------------------------------------ 5. the removal ----
def _mapped(dim, rng):
    """a handle with normals on a base cloud and an append, (handle, cloud, normals)"""
    if dim == 3:
        base = np.ascontiguousarray(rng.normal(size=(9_000, 3)) * np.array([4.0, 4.0, 0.5]))
        extra = np.ascontiguousarray(rng.normal(size=(1_500, 3)) * np.array([3.0, 3.0, 0.4]))
    else:
        base = golden_scan()
        extra = np.ascontiguousarray(base[rng.integers(0, len(base), 200)] + rng.normal(size=(200, 2)))
    icp = _cls(dim)(base)
    if dim == 3:
        icp.compute_normals(8)
        icp.append(extra)
        icp.update_normals(8)
        normals = icp.read_normals()
    else:
        icp.compute_line_normals(8)
        icp.append(extra)
        icp.update_line_normals(8)
        normals = icp.read_line_normals()
    return icp, np.ascontiguousarray(np.concatenate([base, extra])), normals


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("share", [0.9, 0.4])
def test_a_random_mask_leaves_a_fresh_handle_on_the_kept_cloud(dim, share):
    rng = np.random.default_rng(53 + dim)
    icp, cloud, normals = _mapped(dim, rng)
    keep = (rng.uniform(size=len(cloud)) < share).astype(np.uint8) * rng.integers(1, 256, len(cloud)).astype(np.uint8)
    kept, index = mask_keep(keep)
    assert 0 < kept.sum() < len(cloud)
    removed, got = icp.remove(keep, return_index=True)
    assert removed == len(cloud) - kept.sum() and icp.m == icp.target_count == kept.sum()
    assert got.dtype == np.uint32 and np.array_equal(got, index)
    moved = not kept.sum() < len(cloud) / 1.5
    assert icp.remove_counters() == ((1, 0) if moved else (0, 1))
    assert icp.crop_counters() == icp.thin_counters() == icp.outlier_counters() == (0, 0)
    rest = np.ascontiguousarray(cloud[kept])
    assert _same_bytes(icp.read_targets(), rest)
    after = icp.read_normals() if dim == 3 else icp.read_line_normals()
    assert _same_bytes(after, normals[kept])  # carried over
    q = np.ascontiguousarray(rng.normal(size=(1_500, dim)) * 4.0)
    src = np.ascontiguousarray(rest[rng.choice(len(rest), min(2_000, len(rest)), replace=False)] + 0.01)
    assert_equals_fresh(icp, rest, dim, q, src, I.Transform([0.01, 0.02, -0.01]), brute=len(cloud) < 8_192)
    fresh = _cls(dim)(rest)
    assert_lists(icp.query(q, 6), fresh.query(q, 6))
    assert np.array_equal(icp.count_within(q, 0.5, cap=9), fresh.count_within(q, 0.5, cap=9))
    fresh.close()
    icp.close()


def test_all_ones_leaves_the_handle_borrowing_and_all_zeros_takes_an_append():
    import torch

    rng = np.random.default_rng(59)
    p = np.ascontiguousarray(rng.normal(size=(5_000, 3)))
    d_p = torch.from_numpy(p).cuda()
    icp = I.Icp3d(d_p)
    for ones in (np.ones(len(p), dtype=bool), np.full(len(p), 255, dtype=np.uint8), torch.ones(len(p), dtype=torch.bool, device="cuda")):
        removed, index = icp.remove(ones, return_index=True)
        assert removed == 0 and np.array_equal(index, np.arange(len(p), dtype=np.uint32))
    assert icp.remove_counters() == (0, 0) and icp._keep is d_p and icp.target_count == len(p)
    d_p[5, 0] = 123.0  # still reading the caller's tensor
    torch.cuda.synchronize()
    assert icp.read_targets(5, 1)[0, 0] == 123.0
    d_p[5, 0] = float(p[5, 0])
    torch.cuda.synchronize()
    removed, index = icp.remove(np.zeros(len(p), dtype=np.uint8), return_index=True)
    assert removed == len(p) and icp.target_count == 0 and np.all(index == GONE) and icp._keep is None
    assert _same_bytes(d_p.cpu().numpy(), p)  # a borrowed cloud is never written
    assert icp.remove_counters() == (0, 1)
    extra = np.ascontiguousarray(p[:2_000] + 0.25)
    icp.append(extra)
    assert_equals_fresh(icp, extra, 3, np.ascontiguousarray(rng.normal(size=(500, 3))), extra[:600] + 0.01,
                        I.Transform([0.01, 0.0, 0.0]), brute=True)
    assert_lists(icp.query(p[:500], 5), query_lists(extra, p[:500], 5))
    icp.close()


def test_python_refuses_a_mask_of_the_wrong_length():
    t, _ = case("random3")
    icp = I.Icp3d(t)
    for n in (len(t) - 1, len(t) + 1, 0):
        with pytest.raises(ValueError):
            icp.remove(np.ones(n, dtype=bool))
    assert icp.target_count == len(t) and icp.remove_counters() == (0, 0)
    icp.close()


# ---------------------------------------------------------------- 6. the handle is not disturbed ----
def test_an_estimate_after_a_query_returns_the_bits_it_returns_without_the_query():
    rng = np.random.default_rng(61)
    t = np.ascontiguousarray(rng.normal(size=(20_000, 3)) * np.array([6.0, 5.0, 0.8]))
    n = CELL_ORDER_FROM + 3_000  # (above 65 536 source points an estimate folds in the order of its own snapshot)
    src = np.ascontiguousarray(t[rng.integers(0, len(t), n)] + rng.normal(size=(n, 3)) * 0.02)
    q = np.ascontiguousarray(rng.normal(size=(n, 3)) * 5.0)
    init, pose = I.Transform([0.03, -0.02, 0.01]), I.Transform(list(POSE))
    a, b = I.Icp3d(t), I.Icp3d(t)
    first = [h.estimate(src, init, 3, return_info=True) for h in (a, b)]
    assert _same_bytes(first[0][0].as_array(), first[1][0].as_array())
    order = a.last_fold_order(n)
    assert not np.array_equal(order, np.arange(n))
    a.query(q, 8, pose)  # in cell order: the call takes the handle's sort
    a.count_within(src, 0.3, pose, cap=4)
    a.query(q[:500], 8)  # in the caller's order
    assert a.query_counters() == (2, 1)
    assert np.array_equal(a.last_fold_order(n), np.arange(n))  # (the header says so: the identity until the next estimate)
    second = [h.estimate(src, first[0][0], 4, return_info=True) for h in (a, b)]
    assert _same_bytes(second[0][0].as_array(), second[1][0].as_array())
    assert np.array_equal(second[0][1], second[1][1]) and np.array_equal(second[0][2], second[1][2])
    assert np.array_equal(a.last_fold_order(n), b.last_fold_order(n))
    a.close()
    b.close()


def test_after_an_append_a_crop_and_a_thin_a_query_equals_a_fresh_handle_s():
    rng = np.random.default_rng(67)
    base = np.ascontiguousarray(rng.normal(size=(9_000, 3)) * np.array([4.0, 4.0, 0.5]))
    extra = np.ascontiguousarray(base[rng.choice(len(base), 700, replace=False)] + rng.normal(size=(700, 3)) * 0.01)
    q = mixed_queries(base, rng, 1_200)
    T = I.Transform(list(POSE))
    icp = I.Icp3d(base)
    cloud = base
    for step in ("append", "crop", "thin"):
        if step == "append":
            icp.append(extra)
            cloud = np.concatenate([base, extra])
        elif step == "crop":
            icp.crop((0.5, -0.5), 5.0)
            cloud = cloud[disc_mask(cloud, (0.5, -0.5), 5.0)]
        else:
            icp.thin(0.25)
            cloud = cloud[voxel_mask(cloud, 0.25)]
        cloud = np.ascontiguousarray(cloud)
        assert _same_bytes(icp.read_targets(), cloud), step
        fresh = I.Icp3d(cloud)
        for pose in (None, T):
            got = icp.query(q, 9, pose)
            assert_lists(got, fresh.query(q, 9, pose), step)
            assert_lists(got, query_lists(cloud, q, 9, pose), step)
            assert np.array_equal(icp.count_within(q, 0.6, pose, cap=7), count_within_ref(cloud, q, 0.6, 7, pose)), step
        fresh.close()
    icp.close()


# --------------------------------------------------------------------------- 7. the device entries ----
@pytest.mark.parametrize("name", ["scan", "random3"])
def test_device_tensors_in_and_out_equal_the_host_entries_and_repeat_their_bytes(name):
    import torch

    t, q = case(name)
    T = I.Transform(list(POSE))
    icp = _cls(t.shape[1])(torch.from_numpy(np.array(t)).cuda())
    d_q = torch.from_numpy(np.array(q)).cuda()
    for pose in (None, T):
        for k in (3, 20):
            host = icp.query(q, k, pose)
            for _ in range(2):
                idx, d2 = icp.query(d_q, k, pose)
                assert idx.is_cuda and d2.is_cuda and idx.dtype == torch.int32 and d2.dtype == torch.float64
                assert_lists((idx.cpu().numpy().view(np.uint32), d2.cpu().numpy()), host, (name, k))
        for cap in (2, None):
            host = icp.count_within(q, 0.5 if name == "random3" else 40.0, pose, cap=cap)
            for _ in range(2):
                counts = icp.count_within(d_q, 0.5 if name == "random3" else 40.0, pose, cap=cap)
                assert counts.is_cuda and counts.dtype == torch.int32
                assert np.array_equal(counts.cpu().numpy().view(np.uint32), host)
    assert _same_bytes(d_q.cpu().numpy(), q)  # the queries are never written
    rng = np.random.default_rng(71)
    keep = rng.uniform(size=len(t)) < 0.8
    other = _cls(t.shape[1])(t)
    want = other.remove(keep, return_index=True)
    got = icp.remove(torch.from_numpy(keep).cuda(), return_index=True)
    assert got[0] == want[0] == len(t) - keep.sum() and np.array_equal(got[1], want[1])
    assert np.array_equal(got[1], new_index_of(keep))
    assert _same_bytes(icp.read_targets(), other.read_targets()) and _same_bytes(icp.read_targets(), t[keep])
    assert icp.remove_counters() == other.remove_counters()
    with pytest.raises(ValueError):
        icp.remove(torch.ones(int(keep.sum()), dtype=torch.float32, device="cuda"))
    other.close()
    icp.close()
