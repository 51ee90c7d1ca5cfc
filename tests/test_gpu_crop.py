"""EXTENSION beyond the reference (include/icp_mi355x.h section 11): the sliding-window map.  icp_crop_targets keeps the
targets of a handle inside a disc of the xy plane; the checkable contract is the one of an append (tests/test_map.py):
afterwards the handle is a fresh Icp*::new on the cloud it now holds -- which numpy (the keep rule) and the oracle
(everything else) can compute."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib, harness, synth
from parity_util import oracle_in_device_order
from test_map import OracleMap, moved
from test_p2plane import room

pytestmark = pytest.mark.gpu
GONE = 0xFFFFFFFF


def keep_mask(dst, center, radius):
    """the keep rule, restated: dx = x - cx, dy = y - cy, d2 = dx dx + dy dy (numpy evaluates every product and sum on
    its own: no FMA), kept iff d2 <= r * r (false for a NaN d2)"""
    dst = np.asarray(dst, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = dst[:, 0] - np.float64(center[0]), dst[:, 1] - np.float64(center[1])
        d2 = dx * dx + dy * dy
        return d2 <= np.float64(radius) * np.float64(radius)


def new_index_of(mask):
    return np.where(mask, np.cumsum(mask) - 1, GONE).astype(np.uint32)


def _cloud(rng, m, dim=3):
    return np.ascontiguousarray(rng.normal(size=(m, dim)) * np.array([20.0, 20.0, 2.0][:dim]))


def _cls(dim):
    return I.Icp3d if dim == 3 else I.Icp2d


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equals_fresh(icp, cloud, dim, q, src, init, brute=False, fresh_mode=None):
    """searches and a registration (at most 65 536 source points: the caller's fold order) of `icp` equal those of a
    fresh handle on `cloud`, bit for bit"""
    assert icp.target_count == len(cloud)
    assert _same_bytes(icp.read_targets(), cloud)
    fresh = _cls(dim)(cloud) if fresh_mode is None else _cls(dim)(cloud, nn_mode=fresh_mode)
    assert I.lib().icp_get_nn_mode(icp._h) == I.lib().icp_get_nn_mode(fresh._h)
    got = icp.nn_search(q)
    assert np.array_equal(got, fresh.nn_search(q))
    if brute:
        rc, want = O.nn_brute(cloud, q)
        assert rc == O.OK and np.array_equal(got, want)
    assert len(src) <= 65536
    a = icp.estimate(src, init, 5, return_info=True)
    b = fresh.estimate(src, init, 5, return_info=True)
    assert _same_bytes(a[0].as_array(), b[0].as_array())
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    fresh.close()


# ------------------------------------------------------------------ fresh-handle equality ----
SIZES = [(2, 3_000), (3, 3_000), (2, 8_000), (3, 8_000), (2, 8_500), (3, 8_500), (2, 200_000), (3, 200_000),
         (3, (1 << 23) + 50_000)]


@pytest.mark.parametrize("dim,m", SIZES)
def test_crop_equals_a_fresh_handle_on_the_kept_cloud(dim, m):
    """covers: the sweep as engine; one target count either side of the size where the grid takes over (8 192: the crop
    of 8 500 lands below it); the grid; more than 2^23 targets (more than one chunk of tile counts)"""
    rng = np.random.default_rng(7000 * dim + m)
    dst = _cloud(rng, m, dim)
    center, radius = (1.0, -2.0), 45.0
    mask = keep_mask(dst, center, radius)
    assert 0.85 * m < mask.sum() < 0.97 * m
    kept = np.ascontiguousarray(dst[mask])
    icp = _cls(dim)(dst)
    removed, index = icp.crop(center, radius, return_index=True)
    assert removed == m - mask.sum() and icp.m == icp.target_count == mask.sum()
    assert np.array_equal(index, new_index_of(mask))
    q = _cloud(rng, 3000, dim)
    src = kept[rng.choice(len(kept), 20_000 if m >= 20_000 else 2_000, replace=False)] + rng.normal(size=(1, dim)) * 0.01
    init = I.Transform([0.05, 0.02, -0.01])
    assert_equals_fresh(icp, kept, dim, q, src, init, brute=m <= 10_000)
    if m == 200_000:
        # a source cloud above 65 536 points folds in the order of the handle's grid cells: the cropped handle keeps the
        # grid of its last full build -- it equals the oracle in ITS fold order (as tests/test_map.py does for appends)
        assert icp.crop_counters() == (1, 0)
        big = kept[rng.choice(len(kept), 150_000, replace=False)]
        big = np.concatenate([big, big[:50_000] + 0.003]) + rng.normal(size=(200_000, dim)) * 0.01
        T0 = I.Transform([0.02, -0.01, 0.004])
        T, idx, inner = icp.estimate(big, T0, 4, return_info=True)
        O.set_threads(16)
        try:
            rc, oT, oidx, oinner = oracle_in_device_order(icp, dim, kept, big, O.transform_new(np.array([0.02, -0.01, 0.004])), 4)
        finally:
            O.set_threads(1)
        assert rc == O.OK
        assert np.array_equal(idx, oidx) and np.array_equal(inner, oinner)
        assert _same_bytes(T.as_array(), oT.as_array())
    icp.close()


# ------------------------------------------------------------------------ both grid paths ----
def test_moved_and_rebuilt_crops_both_equal_a_fresh_handle_and_the_next_append_is_incremental():
    rng = np.random.default_rng(41)
    base = synth.box_cloud(synth.SEED + 21, 90_000, synth.ROOM_LO, synth.ROOM_HI)
    icp = I.Icp3d(base)
    q = synth.box_cloud(synth.SEED + 22, 30_000, synth.ROOM_LO, synth.ROOM_HI) + rng.normal(size=(30_000, 3)) * 0.02
    init = I.Transform([0.02, -0.01, 0.004])

    def src_of(cloud):
        return cloud[rng.choice(len(cloud), 20_000, replace=False)] + rng.normal(size=(20_000, 3)) * 0.01

    # thin: the corners of the room beyond 3.9 m of the centre go (kept well above m_full / 1.5): moved
    mask = keep_mask(base, (0.1, -0.1), 3.9)
    assert 0.8 * len(base) < mask.sum() < len(base)
    assert icp.crop((0.1, -0.1), 3.9) == len(base) - mask.sum()
    cloud = np.ascontiguousarray(base[mask])
    assert icp.crop_counters() == (1, 0)
    assert_equals_fresh(icp, cloud, 3, q, src_of(cloud), init, fresh_mode=I.NN_GRID)
    # the next append is still served by moving the records, and still equals a fresh handle
    extra = synth.box_cloud(synth.SEED + 23, 5_000, synth.ROOM_LO * 0.5, synth.ROOM_HI * 0.5)
    before = icp.append_counters()
    icp.append(extra)
    assert icp.append_counters() == (before[0] + 1, before[1])
    cloud = np.ascontiguousarray(np.concatenate([cloud, extra]))
    assert_equals_fresh(icp, cloud, 3, q, src_of(cloud), init, fresh_mode=I.NN_GRID)
    # a second thin crop on the appended handle: moved again
    mask = keep_mask(cloud, (-0.1, 0.1), 3.8)
    assert icp.crop((-0.1, 0.1), 3.8) == len(cloud) - mask.sum() > 0
    cloud = np.ascontiguousarray(cloud[mask])
    assert icp.crop_counters() == (2, 0)
    assert_equals_fresh(icp, cloud, 3, q, src_of(cloud), init, fresh_mode=I.NN_GRID)
    # deep: kept < m_full / 1.5 (m_full = the 90 000 of the last full build): rebuilt
    mask = keep_mask(cloud, (0.5, 0.5), 2.2)
    assert 20_000 < mask.sum() < 90_000 / 1.5
    assert icp.crop((0.5, 0.5), 2.2) == len(cloud) - mask.sum()
    cloud = np.ascontiguousarray(cloud[mask])
    assert icp.crop_counters() == (2, 1)
    assert_equals_fresh(icp, cloud, 3, q, src_of(cloud), init, fresh_mode=I.NN_GRID)
    rc, want = O.nn_brute(cloud, q[:3000])
    assert rc == O.OK and np.array_equal(icp.nn_search(q[:3000]), want)
    icp.close()


# ---------------------------------------------------------------------------- interleaving ----
def test_appends_crops_and_estimates_interleaved_track_the_oracle():
    """a handle that has already searched (cell-sorted snapshot, previous matches, window predictions, speculation
    state) keeps returning the oracle's results as its cloud grows and shrinks"""
    rng = np.random.default_rng(77)
    world = synth.box_cloud(synth.SEED + 5, 60_000, synth.ROOM_LO, synth.ROOM_HI)
    parts = np.array_split(world, 3)
    scan = world[rng.choice(len(world), 20_000, replace=False)] + rng.normal(size=(20_000, 3)) * 0.01
    T = I.Transform([0.05, -0.04, 0.01])
    init = O.Pose(*T.pose.as_tuple())
    icp = I.Icp3d(parts[0])
    dst = parts[0]

    def check():
        Tg, idx, inner = icp.estimate(scan, T, 3, return_info=True)
        rc, oT, oidx, oinner = oracle_in_device_order(icp, 3, dst, scan, init, 3)
        assert rc == O.OK
        assert np.array_equal(idx, oidx) and np.array_equal(inner, oinner)
        assert _same_bytes(Tg.as_array(), oT.as_array())

    icp.append(parts[1])
    dst = np.concatenate([dst, parts[1]])
    check()
    for center, radius, part in (((0.3, -0.2), 3.7, parts[2]), ((-0.4, 0.1), 3.3, None)):
        mask = keep_mask(dst, center, radius)
        assert icp.crop(center, radius) == len(dst) - mask.sum() > 0
        dst = np.ascontiguousarray(dst[mask])
        check()
        if part is not None:
            icp.append(part)
            dst = np.ascontiguousarray(np.concatenate([dst, part]))
    assert _same_bytes(icp.read_targets(), dst)
    icp.close()


# --------------------------------------------------------------------------------- normals ----
def test_kept_targets_keep_their_normals_and_point_to_plane_runs_without_recomputation():
    rng = np.random.default_rng(77)
    dst = room(rng, 30_000)
    src = dst[rng.integers(0, len(dst), 12_000)] + rng.normal(0, 1e-3, (12_000, 3))
    Tt = I.Transform([0.05, -0.04, 0.015])
    icp = I.Icp3d(dst)
    icp.compute_normals(10)
    before = icp.read_normals()
    center, radius = (0.2, 0.1), 3.6
    mask = keep_mask(dst, center, radius)
    assert 0.7 * len(dst) < mask.sum() < len(dst)
    assert icp.crop(center, radius) == len(dst) - mask.sum()
    normals = icp.read_normals()
    assert _same_bytes(normals, before[mask])
    kept = np.ascontiguousarray(dst[mask])
    src = moved(src[keep_mask(src, center, radius - 0.2)], Tt.inverse())
    T, idx, inner = icp.estimate_point_to_plane(src, I.Transform(), 8, return_info=True)
    O.set_threads(16)
    try:
        rc, oT, oidx, oinner = O.p2pl_estimate(O.KdTree(kept), normals, src, O.transform_identity(), 8)
    finally:
        O.set_threads(1)
    assert rc == O.OK
    assert np.array_equal(idx, oidx) and np.array_equal(inner, oinner)
    assert np.max(np.abs(T.as_array() - oT.as_array())) < 1e-9  # (tests/test_p2plane.py: tree sums vs left folds)
    icp.close()


def test_crop_after_an_append_without_an_update_leaves_exactly_the_new_kept_targets_without_normals():
    rng = np.random.default_rng(5)
    dst, extra = room(rng, 9_000), room(rng, 2_000)
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    before = icp.read_normals()
    icp.append(extra)
    cloud = np.concatenate([dst, extra])
    center, radius = (-0.1, 0.3), 3.5
    mask = keep_mask(cloud, center, radius)
    assert mask[:9_000].sum() < 9_000 and mask[9_000:].sum() < 2_000
    assert icp.crop(center, radius) == len(cloud) - mask.sum()
    kept = np.ascontiguousarray(cloud[mask])
    with pytest.raises(I.IcpError) as e:  # the appended targets that were kept have no normal yet
        icp.estimate_point_to_plane(dst[:100], I.Transform(), 1)
    assert e.value.status == _lib.BAD_ARGUMENT
    with pytest.raises(I.IcpError):
        icp.read_normals()
    icp.update_normals(8)
    got = icp.read_normals()
    had = int(mask[:9_000].sum())
    assert _same_bytes(got[:had], before[mask[:9_000]])  # the normals that existed: unchanged
    O.set_threads(16)
    try:
        want = O.p2pl_normals_update(kept, had, 8, got)
    finally:
        O.set_threads(1)
    assert np.max(np.abs(got - want)) < 1e-9  # (tests/test_p2plane.py: the appended targets' normals, to rounding)
    assert icp.estimate_point_to_plane(kept[:500], I.Transform(), 2) is not None
    icp.close()


# ----------------------------------------------------------------------------------- edges ----
def test_an_infinite_radius_changes_nothing_and_the_handle_keeps_borrowing():
    import torch

    rng = np.random.default_rng(9)
    base, q = _cloud(rng, 12_000), _cloud(rng, 2_000)
    d_base = torch.from_numpy(base).cuda()
    icp = I.Icp3d(d_base)
    removed, index = icp.crop((0.0, 0.0), float("inf"), return_index=True)
    assert removed == 0 and np.array_equal(index, np.arange(12_000, dtype=np.uint32))
    assert icp.crop_counters() == (0, 0) and icp.append_counters() == (0, 0)
    assert icp._keep is d_base and icp.target_count == 12_000
    # still reading the caller's tensor: what the caller writes there is what the handle returns
    d_base[5, 0] = 123.0
    torch.cuda.synchronize()
    assert icp.read_targets(5, 1)[0, 0] == 123.0
    d_base[5, 0] = float(base[5, 0])
    torch.cuda.synchronize()
    rc, want = O.nn_brute(base, q)
    assert np.array_equal(icp.nn_search(q), want)
    icp.close()


def test_a_borrowed_device_cloud_is_never_written_and_moves_into_the_handle():
    import torch

    rng = np.random.default_rng(10)
    base, q = _cloud(rng, 12_000), _cloud(rng, 2_000)
    d_base = torch.from_numpy(base).cuda()
    icp = I.Icp3d(d_base)
    mask = keep_mask(base, (3.0, 3.0), 30.0)
    assert icp.crop((3.0, 3.0), 30.0) == 12_000 - mask.sum() > 0
    assert icp._keep is None
    assert _same_bytes(d_base.cpu().numpy(), base)
    d_base.zero_()  # the handle no longer reads the caller's buffer
    torch.cuda.synchronize()
    kept = np.ascontiguousarray(base[mask])
    assert _same_bytes(icp.read_targets(), kept)
    rc, want = O.nn_brute(kept, q)
    assert np.array_equal(icp.nn_search(q), want)
    icp.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_targets_with_a_nan_x_or_y_are_removed_at_any_radius(dim):
    rng = np.random.default_rng(11 + dim)
    dst = _cloud(rng, 9_000, dim)
    dst[17, 0] = np.nan
    dst[4_000, 1] = np.nan
    dst[8_999, 0] = dst[8_999, 1] = np.nan
    icp = _cls(dim)(dst)
    removed, index = icp.crop((0.0, 0.0), float("inf"), return_index=True)
    mask = keep_mask(dst, (0.0, 0.0), float("inf"))
    assert removed == 3 and mask.sum() == 8_997
    assert np.array_equal(index, new_index_of(mask))
    kept = np.ascontiguousarray(dst[mask])
    q = _cloud(rng, 1_500, dim)
    src = kept[:2_000] + 0.01
    assert_equals_fresh(icp, kept, dim, q, src, I.Transform([0.01, 0.0, 0.0]), brute=True)
    icp.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_radius_zero_keeps_exactly_the_targets_with_those_xy(dim):
    rng = np.random.default_rng(21 + dim)
    dst = _cloud(rng, 10_000, dim)
    dst[[5, 700, 9_999], :2] = dst[123, :2]
    center = dst[123, :2].copy()
    icp = _cls(dim)(dst)
    removed, index = icp.crop(center, 0.0, return_index=True)
    assert removed == 10_000 - 4
    want = np.full(10_000, GONE, dtype=np.uint32)
    want[[5, 123, 700, 9_999]] = [0, 1, 2, 3]
    assert np.array_equal(index, want)
    assert _same_bytes(icp.read_targets(), dst[[5, 123, 700, 9_999]])
    rc, nn = O.nn_brute(dst[[5, 123, 700, 9_999]], dst[:50])
    assert np.array_equal(icp.nn_search(dst[:50]), nn)
    icp.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_crop_everything_then_append(dim):
    rng = np.random.default_rng(31 + dim)
    dst, extra, q = _cloud(rng, 20_000, dim), _cloud(rng, 9_000, dim), _cloud(rng, 2_000, dim)
    icp = _cls(dim)(dst)
    removed, index = icp.crop((1e6, 1e6), 1.0, return_index=True)
    assert removed == 20_000 and icp.target_count == 0 and icp.m == 0
    assert np.all(index == GONE)
    with pytest.raises(I.IcpError) as e:
        icp.estimate(q, I.Transform(), 3)
    assert e.value.status == _lib.EMPTY_DST
    assert icp.crop((0.0, 0.0), 1.0) == 0  # an empty cloud: nothing to do
    icp.append(extra)
    src = extra[:2_000] + 0.01
    assert_equals_fresh(icp, extra, dim, q, src, I.Transform([0.01, 0.0, 0.0]), brute=True)
    icp.close()


def test_two_handles_cropped_alike_hold_identical_bytes():
    rng = np.random.default_rng(51)
    dst = _cloud(rng, 150_000)
    a, b = I.Icp3d(dst), I.Icp3d(dst)
    ra, ia = a.crop((2.0, 1.0), 40.0, return_index=True)
    rb, ib = b.crop((2.0, 1.0), 40.0, return_index=True)
    assert ra == rb > 0 and _same_bytes(ia, ib)
    assert _same_bytes(a.read_targets(), b.read_targets())
    src = dst[:30_000] + 0.01
    Ta, xa, na = a.estimate(src, I.Transform(), 4, return_info=True)
    Tb, xb, nb = b.estimate(src, I.Transform(), 4, return_info=True)
    assert _same_bytes(Ta.as_array(), Tb.as_array()) and _same_bytes(xa, xb) and _same_bytes(na, nb)
    a.close()
    b.close()


# ----------------------------------------------------------------------------------- multi ----
@pytest.mark.parametrize("world", [2, 4])
def test_crop_across_virtual_ranks_equals_one_handle(world):
    rng = np.random.default_rng(100 + world)
    dst = synth.box_cloud(synth.SEED + 61, 60_000, synth.ROOM_LO, synth.ROOM_HI)
    src = dst[rng.choice(len(dst), 20_000, replace=False)] + rng.normal(size=(20_000, 3)) * 0.01
    center, radius = (0.2, -0.3), 3.6
    mask = keep_mask(dst, center, radius)
    one = I.Icp3d(dst, nn_mode=I.NN_GRID)
    multi = I.IcpMulti(dst, [0] * world)
    assert one.crop(center, radius) == multi.crop(center, radius) == len(dst) - mask.sum() > 0
    assert multi.target_count == one.target_count == mask.sum()
    T0 = I.Transform([0.02, -0.01, 0.004])
    T1, idx1, inner1 = one.estimate(src, T0, 5, return_info=True)
    T, idx, inner = multi.estimate(src, T0, 5, return_info=True)
    assert _same_bytes(T.as_array(), T1.as_array())
    assert np.array_equal(idx, idx1) and np.array_equal(inner, inner1)
    multi.close()
    one.close()


# ------------------------------------------------------------------------------------ loop ----
class OracleWindowMap(OracleMap):
    """OracleMap with the sliding window restated: crop is a numpy mask by the keep rule (tests only)"""

    def __call__(self, dst):
        self.removed = []
        return super().__call__(dst)

    def crop(self, center, radius):
        mask = keep_mask(self.dst, center, radius)
        self.removed.append(int(len(self.dst) - mask.sum()))
        self.dst = np.ascontiguousarray(self.dst[mask])


def test_scan_to_map_with_a_window_on_gpu_matches_the_oracle_bit_for_bit():
    pk = synth.synthetic_scan3d_packets(5 * 30)
    R = 4.0  # (the room's corners lie 4.24 m from its centre: every frame's append brings points the window lets go of)
    Os, opath, oworld = harness.run_scan_to_map(pk, step=30, max_iter=5, icp_factory=OracleWindowMap(tree_order=True),
                                                map_radius=R)
    assert len(Os) == 4 and len([r for r in oworld.removed if r > 0]) >= 2, oworld.removed
    Ts, path, world = harness.run_scan_to_map(pk, step=30, max_iter=5, map_radius=R)
    assert len(Ts) == 4
    for a, b in zip(Ts, Os):
        assert _same_bytes(a.as_array(), b.as_array())
    assert _same_bytes(path, opath)
    assert _same_bytes(world.read_targets(), oworld.dst)
    _, _, grown = harness.run_scan_to_map(pk, step=30, max_iter=5)
    assert world.target_count < grown.target_count
    assert sum(world.crop_counters()) == len([r for r in oworld.removed if r > 0])
