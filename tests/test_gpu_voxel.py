"""EXTENSION beyond the reference (include/icp_mi355x.h section 22): voxel thinning -- the first point of every voxel, in
order.  The stand-alone calls are held to the numpy restatement of the rule (tests/test_voxel_abi.py: kept_index_of),
byte for byte; icp_thin_targets to the crop's contract (tests/test_gpu_crop.py): afterwards the handle is a fresh
Icp*::new on the kept cloud."""
import ctypes as C

import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib, harness, synth
from parity_util import oracle_in_device_order
from test_gpu_crop import GONE, OracleWindowMap, _cloud, _cls, _same_bytes, assert_equals_fresh, new_index_of
from test_gpu_crop import keep_mask as disc_mask
from test_map import moved
from test_p2plane import room
from test_voxel_abi import boundary_input, keep_mask, kept_index_of, special_input

pytestmark = pytest.mark.gpu


def by_host(p, v):
    out, idx = I.voxel_downsample(p, v, return_index=True)
    assert out.dtype == np.float64 and idx.dtype == np.uint32
    return out, idx


def by_device(p, v):
    import torch

    out, idx = I.voxel_downsample(torch.from_numpy(np.ascontiguousarray(p)).cuda(), v, return_index=True)
    assert out.is_cuda and idx.is_cuda and out.dtype == torch.float64
    return out.cpu().numpy(), idx.cpu().numpy().view(np.uint32)


def assert_is_the_restatement(p, v, entries=(by_host, by_device)):
    want = kept_index_of(p, v)
    for entry in entries:
        out, idx = entry(p, v)
        assert len(idx) == len(out) == len(want), (entry.__name__, len(idx), len(want))
        assert np.array_equal(idx, want), entry.__name__
        assert _same_bytes(out, p[want]), entry.__name__  # (bytes: a kept -0.0 stays -0.0)
    return want


# ------------------------------------------------------------------------- the stand-alone call ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097, 200_000])
@pytest.mark.parametrize("dim", [2, 3])
def test_downsample_equals_the_restatement(dim, n):
    """sizes around a wave, a tile of 1 024 and several tiles; rows with NaN, +-inf and +-0.0 among the points"""
    rng = np.random.default_rng(100 * n + dim)
    p = np.ascontiguousarray(rng.normal(size=(n, dim)) * 2.0)
    if n >= 63:
        for row, x in zip(rng.choice(n, 8, replace=False), (np.nan, np.inf, -np.inf, 0.0, -0.0, -0.0, 0.0, np.nan)):
            p[row, rng.integers(dim)] = x
    want = assert_is_the_restatement(p, 0.5)
    assert n == 1 or len(want) < n


@pytest.mark.parametrize("name", ["boundary", "specials", "overflow", "one_voxel", "distinct"])
@pytest.mark.parametrize("dim", [2, 3])
def test_downsample_of_the_inputs_that_catch_a_wrong_rule(dim, name):
    if name == "boundary":  # a product with 1 / v instead of the division merges other neighbours
        p, v = boundary_input(dim), 0.1
    elif name == "specials":
        p, v = special_input(dim), 0.1
    elif name == "overflow":  # 1e308 / 1e-3 = +inf: a cell coordinate like any other (rows 9 and 11, and once more)
        p, v = np.concatenate([special_input(dim), special_input(dim)[[9, 11]]]), 1e-3
    elif name == "one_voxel":  # every atomicMin of the insert falls on one word
        p, v = np.random.default_rng(1).uniform(0.0, 1.0, (65_536, dim)), 1.0
    else:  # no two points share a voxel
        k = np.random.default_rng(2).permutation(70_001)
        p, v = np.zeros((70_001, dim)), 0.25
        p[:, 0], p[:, dim - 1] = k * 0.25 + 0.125, (k % 7) * 0.25
    want = assert_is_the_restatement(np.ascontiguousarray(p), v)
    if name == "one_voxel":
        assert np.array_equal(want, [0])
    if name == "distinct":
        assert len(want) == len(p)
    if name == "overflow":
        assert p[9, 0] == p[11, 0] == 1e308 and 9 in want and 11 in want
        assert len(p) - 2 not in want and len(p) - 1 not in want  # a second point of a voxel at +inf goes like any other


@pytest.mark.parametrize("dim", [2, 3])
def test_out_and_kept_index_are_each_optional(dim):
    import torch

    p = np.ascontiguousarray(np.random.default_rng(5 + dim).normal(size=(5_000, dim)))
    want = kept_index_of(p, 0.25)
    d_p = torch.from_numpy(p).cuda()
    for with_out, with_idx in ((True, False), (False, True), (False, False)):
        out, idx, kept = np.zeros((5_000, dim)), np.zeros(5_000, dtype=np.uint32), C.c_size_t(0)
        rc = I.lib().icp_voxel_downsample(dim, C.c_void_p(p.ctypes.data), 5_000, 0.25,
                                          C.c_void_p(out.ctypes.data) if with_out else None,
                                          C.c_void_p(idx.ctypes.data) if with_idx else None, C.byref(kept), -1)
        assert rc == _lib.OK and kept.value == len(want)
        assert not with_out or _same_bytes(out[:len(want)], p[want])
        assert not with_idx or np.array_equal(idx[:len(want)], want)
        d_out, d_idx, kept = torch.zeros_like(d_p), torch.zeros(5_000, dtype=torch.int32, device="cuda"), C.c_size_t(0)
        rc = I.lib().icp_voxel_downsample_device(dim, C.c_void_p(d_p.data_ptr()), 5_000, 0.25,
                                                 C.c_void_p(d_out.data_ptr()) if with_out else None,
                                                 C.c_void_p(d_idx.data_ptr()) if with_idx else None, C.byref(kept), -1,
                                                 None)
        assert rc == _lib.OK and kept.value == len(want)
        assert not with_out or _same_bytes(d_out[:len(want)].cpu().numpy(), p[want])
        assert not with_idx or np.array_equal(d_idx[:len(want)].cpu().numpy().view(np.uint32), want)
    kept = C.c_size_t(7)
    assert I.lib().icp_voxel_downsample(dim, None, 0, 0.25, None, None, C.byref(kept), -1) == _lib.OK and kept.value == 0
    assert len(I.voxel_downsample(np.zeros((0, dim)), 0.25)) == 0


def test_downsample_past_one_chunk_of_tile_counts():
    """2^23 + 1025 points: more than 8 192 tiles, so the chunk sums carry; the points pair up in voxels along x, so the
    kept indices are the even ones (no large numpy sort)"""
    import torch

    n, v = (1 << 23) + 1025, 0.5
    i = torch.arange(n, device="cuda", dtype=torch.int64)
    d_p = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    d_p[:, 0] = (i // 2).double() * v + 0.25 * v  # (exact: multiples of 1 / 8 far below 2^53)
    d_p[:, 1], d_p[:, 2] = 0.3, -0.7
    out, idx = I.voxel_downsample(d_p, v, return_index=True)
    assert len(out) == len(idx) == (n + 1) // 2
    assert torch.equal(idx.long(), torch.arange(0, n, 2, device="cuda"))
    assert torch.equal(out, d_p[0::2])
    I.lib().icp_trim_pool()  # (the table of 2^25 words goes back)


def test_two_calls_on_the_same_input_give_identical_bytes():
    import torch

    rng = np.random.default_rng(8)
    p = np.ascontiguousarray(rng.normal(size=(300_000, 3)) * 3.0)
    a, b = by_host(p, 0.3), by_host(p, 0.3)
    assert _same_bytes(a[0], b[0]) and _same_bytes(a[1], b[1])
    d_p = torch.from_numpy(p).cuda()
    with torch.cuda.stream(torch.cuda.Stream()):
        c = I.voxel_downsample(d_p, 0.3, return_index=True)
    d = I.voxel_downsample(d_p, 0.3, return_index=True)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])
    assert _same_bytes(c[0].cpu().numpy(), a[0]) and np.array_equal(c[1].cpu().numpy().view(np.uint32), a[1])
    assert _same_bytes(d_p.cpu().numpy(), p)  # the input is never written


# --------------------------------------------------------------------- thin == a fresh handle ----
# dim, m, v, the kept share (computed on the CPU with the restatement), what the grid does
THINS = [(2, 200_000, 0.1, (0.82, 0.84), "moved"), (2, 200_000, 0.25, (0.43, 0.45), "rebuilt"),
         (3, 200_000, 0.5, (0.74, 0.75), "moved"), (3, 200_000, 1.0, (0.30, 0.32), "rebuilt"),
         (3, 8_500, 2.0, (0.53, 0.55), "rebuilt"),  # ends below the 8 192 targets where the grid takes over
         (2, 3_000, 1.0, None, None), (3, 3_000, 1.0, None, None)]  # the sweep as engine


@pytest.mark.parametrize("dim,m,v,share,path", THINS)
def test_thin_equals_a_fresh_handle_on_the_kept_cloud(dim, m, v, share, path):
    rng = np.random.default_rng(7000 * dim + m)
    dst = _cloud(rng, m, dim)
    mask = keep_mask(dst, v)
    if share:
        assert share[0] * m < mask.sum() < share[1] * m
    assert 0 < mask.sum() < m
    kept = np.ascontiguousarray(dst[mask])
    icp = _cls(dim)(dst)
    removed, index = icp.thin(v, return_index=True)
    assert removed == m - mask.sum() and icp.m == icp.target_count == mask.sum()
    assert np.array_equal(index, new_index_of(mask))
    assert icp.crop_counters() == (0, 0)  # the crop's counters count crops
    if path:
        assert icp.thin_counters() == ((1, 0) if path == "moved" else (0, 1))
    else:
        assert sum(icp.thin_counters()) == 1
    q = _cloud(rng, 3000, dim)
    src = kept[rng.choice(len(kept), 20_000 if m >= 20_000 else 2_000, replace=False)] + rng.normal(size=(1, dim)) * 0.01
    init = I.Transform([0.05, 0.02, -0.01])
    assert_equals_fresh(icp, kept, dim, q, src, init, brute=m <= 10_000)
    if path == "moved":  # the next append is still served by moving the records, and still equals a fresh handle
        extra = np.ascontiguousarray(kept[:4_000] + 0.01)
        before = icp.append_counters()
        icp.append(extra)
        assert icp.append_counters() == (before[0] + 1, before[1])
        assert_equals_fresh(icp, np.ascontiguousarray(np.concatenate([kept, extra])), dim, q, src, init)
    left = icp.read_targets()  # thin again: nothing goes but what the append brought into occupied voxels
    assert icp.thin(v) == len(left) - len(kept_index_of(left, v))
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
    mask = keep_mask(dst, 0.05)
    assert 0.6 * len(dst) < mask.sum() < 0.8 * len(dst)
    assert icp.thin(0.05) == len(dst) - mask.sum()
    normals = icp.read_normals()
    assert _same_bytes(normals, before[mask])
    kept = np.ascontiguousarray(dst[mask])
    src = moved(src, Tt.inverse())
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


def test_thin_after_an_append_without_an_update_leaves_exactly_the_new_kept_targets_without_normals():
    rng = np.random.default_rng(5)
    dst, extra = room(rng, 9_000), room(rng, 2_000)
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    before = icp.read_normals()
    icp.append(extra)
    cloud = np.concatenate([dst, extra])
    mask = keep_mask(cloud, 0.1)
    assert 0 < mask[:9_000].sum() < 9_000 and 0 < mask[9_000:].sum() < 2_000
    assert icp.thin(0.1) == len(cloud) - mask.sum()
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
def test_a_size_that_removes_nothing_changes_nothing_and_a_borrowed_cloud_is_never_written():
    import torch

    rng = np.random.default_rng(9)
    base, q = _cloud(rng, 12_000), _cloud(rng, 2_000)
    d_base = torch.from_numpy(base).cuda()
    icp = I.Icp3d(d_base)
    assert len(kept_index_of(base, 1e-9)) == 12_000
    removed, index = icp.thin(1e-9, return_index=True)
    assert removed == 0 and np.array_equal(index, np.arange(12_000, dtype=np.uint32))
    assert icp.thin_counters() == (0, 0) and icp.crop_counters() == (0, 0) and icp.append_counters() == (0, 0)
    assert icp._keep is d_base and icp.target_count == 12_000
    d_base[5, 0] = 123.0  # still reading the caller's tensor
    torch.cuda.synchronize()
    assert icp.read_targets(5, 1)[0, 0] == 123.0
    d_base[5, 0] = float(base[5, 0])
    torch.cuda.synchronize()
    mask = keep_mask(base, 2.0)
    assert icp.thin(2.0) == 12_000 - mask.sum() > 0
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
def test_thin_to_one_point_then_append(dim):
    rng = np.random.default_rng(31 + dim)
    dst = np.ascontiguousarray(rng.uniform(1.0, 9.0, (20_000, dim)))
    extra, q = _cloud(rng, 9_000, dim), _cloud(rng, 2_000, dim)
    icp = _cls(dim)(dst)
    removed, index = icp.thin(10.0, return_index=True)
    assert removed == 19_999 and icp.target_count == 1 and index[0] == 0 and np.all(index[1:] == GONE)
    assert _same_bytes(icp.read_targets(), dst[:1])
    icp.append(extra)
    cloud = np.ascontiguousarray(np.concatenate([dst[:1], extra]))
    assert_equals_fresh(icp, cloud, dim, q, extra[:2_000] + 0.01, I.Transform([0.01, 0.0, 0.0]), brute=True)
    icp.close()


def test_a_thin_after_an_append_keeps_the_old_map_and_drops_the_new_points_in_occupied_voxels():
    rng = np.random.default_rng(61)
    v = 0.5
    base = _cloud(rng, 150_000)
    icp = I.Icp3d(base)
    icp.thin(v)
    old = np.ascontiguousarray(base[keep_mask(base, v)])
    assert _same_bytes(icp.read_targets(), old)
    again = np.ascontiguousarray(old + rng.normal(size=old.shape) * 1e-3)  # the same place seen once more: 1 mm of noise
    icp.append(again)
    removed, index = icp.thin(v, return_index=True)
    m = len(old)
    assert np.array_equal(index[:m], np.arange(m, dtype=np.uint32))  # every old map point stays where it is
    old_cells = {tuple(c) for c in np.floor(old / v)}
    in_occupied = np.array([tuple(c) in old_cells for c in np.floor(again / v)])
    assert 0.9 * m < in_occupied.sum() < m  # (a few cross into a voxel the map had not filled)
    assert np.all(index[m:][in_occupied] == GONE)
    assert np.array_equal(index, new_index_of(keep_mask(np.concatenate([old, again]), v)))
    assert removed == m - np.count_nonzero(index[m:] != GONE) and icp.target_count == 2 * m - removed
    icp.close()


def test_two_handles_thinned_alike_hold_identical_bytes():
    dst = _cloud(np.random.default_rng(51), 150_000)
    a, b = I.Icp3d(dst), I.Icp3d(dst)
    ra, ia = a.thin(0.7, return_index=True)
    rb, ib = b.thin(0.7, return_index=True)
    assert ra == rb > 0 and _same_bytes(ia, ib)
    assert _same_bytes(a.read_targets(), b.read_targets())
    a.close()
    b.close()


# ----------------------------------------------------------------------------------- multi ----
def test_thin_across_two_virtual_ranks_equals_one_handle():
    rng = np.random.default_rng(102)
    dst = synth.box_cloud(synth.SEED + 61, 60_000, synth.ROOM_LO, synth.ROOM_HI)
    src = dst[rng.choice(len(dst), 20_000, replace=False)] + rng.normal(size=(20_000, 3)) * 0.01
    mask = keep_mask(dst, 0.05)
    one = I.Icp3d(dst, nn_mode=I.NN_GRID)
    multi = I.IcpMulti(dst, [0, 0])
    assert one.thin(0.05) == multi.thin(0.05) == len(dst) - mask.sum() > 0
    assert multi.target_count == one.target_count == mask.sum()
    T0 = I.Transform([0.02, -0.01, 0.004])
    T1, idx1, inner1 = one.estimate(src, T0, 5, return_info=True)
    T, idx, inner = multi.estimate(src, T0, 5, return_info=True)
    assert _same_bytes(T.as_array(), T1.as_array())
    assert np.array_equal(idx, idx1) and np.array_equal(inner, inner1)
    multi.close()
    one.close()


# ---------------------------------------------------------------------------- interleaving ----
def test_appends_thins_crops_and_estimates_interleaved_track_the_oracle():
    """a handle that has already searched keeps returning the oracle's results as its cloud grows, is thinned and is
    cropped (tests/test_gpu_crop.py: test_appends_crops_and_estimates_interleaved_track_the_oracle, with thins)"""
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
    for v, center, radius, part in ((0.04, (0.3, -0.2), 3.7, parts[2]), (0.08, (-0.4, 0.1), 3.3, None)):
        mask = keep_mask(dst, v)
        assert icp.thin(v) == len(dst) - mask.sum() > 0
        dst = np.ascontiguousarray(dst[mask])
        check()
        mask = disc_mask(dst, center, radius)
        assert icp.crop(center, radius) == len(dst) - mask.sum() > 0
        dst = np.ascontiguousarray(dst[mask])
        if part is not None:
            icp.append(part)
            dst = np.ascontiguousarray(np.concatenate([dst, part]))
        else:
            check()
    assert sum(icp.thin_counters()) == 2 and sum(icp.crop_counters()) == 2
    assert _same_bytes(icp.read_targets(), dst)
    icp.close()


# ------------------------------------------------------------------------------------ loop ----
class OracleVoxelMap(OracleWindowMap):
    """OracleWindowMap with the thinning restated: thin is a numpy mask by the rule (tests only)"""

    def __call__(self, dst):
        self.thinned = []
        return super().__call__(dst)

    def thin(self, v):
        mask = keep_mask(self.dst, v)
        self.thinned.append(int(len(self.dst) - mask.sum()))
        self.dst = np.ascontiguousarray(self.dst[mask])


def test_scan_to_map_with_voxels_on_gpu_matches_the_oracle_bit_for_bit(monkeypatch):
    pk = synth.synthetic_scan3d_packets(5 * 30)
    kw = dict(step=30, max_iter=5, scan_voxel=0.05, map_voxel=0.1, map_radius=4.0)
    Ts, path, world = harness.run_scan_to_map(pk, **kw)  # (scans of about 11 000 points: the caller's fold order)
    with monkeypatch.context() as mp:
        mp.setattr(harness, "voxel_downsample", lambda scan, v: np.ascontiguousarray(scan[kept_index_of(scan, v)]))
        Os, opath, oworld = harness.run_scan_to_map(pk, icp_factory=OracleVoxelMap(tree_order=True), **kw)
    assert len(Ts) == len(Os) == 4 and all(r > 0 for r in oworld.thinned), oworld.thinned
    for a, b in zip(Ts, Os):
        assert _same_bytes(a.as_array(), b.as_array())
    assert _same_bytes(path, opath)
    assert _same_bytes(world.read_targets(), oworld.dst)
    assert sum(world.thin_counters()) == 4
    _, _, grown = harness.run_scan_to_map(pk, step=30, max_iter=5)
    assert world.target_count < grown.target_count
