"""Gated point-to-plane registration (Icp3d.estimate_point_to_plane(..., max_correspondence_distance=r):
icp_estimate_point_to_plane_gated[_device], icp_gate_plane_pairs_device and icp_multi_estimate_point_to_plane_gated of
include/icp_mi355x.h section 12).
  * the gate alone against numpy (every operation rounded on its own), at the tile's edges and on the chunk-sum path;
  * r = +inf returns the bits of estimate_point_to_plane;
  * a finite r against a bit-exact restatement on the same handle (one ungated iteration at a time on the kept points)
    and against the CPU statement of the definition (oracle: orc_p2pl_estimate, chained the same way);
  * the gate helps on a scan that holds an object the map does not; few inliers; state neutrality; virtual ranks."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from parity_util import oracle_plane_in_device_order
from test_p2plane import moved, room

pytestmark = pytest.mark.gpu

INF = float("inf")


def bits(T):
    return np.asarray(T.as_array(), dtype=np.float64).view(np.uint64)


def blob_scene(seed, n=3000, m=6000, share=0.55):
    """a room of m targets; the scan: n points, `share` of them a Gaussian blob (sigma 0.3) at (2.2, -2.2, 0.8) that the
    room does not hold, the rest room samples with 1e-3 noise; true pose (0.10, -0.08, 0.03)"""
    rng = np.random.default_rng(seed)
    dst = room(rng, m)
    k = int(n * share)
    world = np.concatenate([np.array([2.2, -2.2, 0.8]) + rng.normal(size=(k, 3)) * 0.3,
                            dst[rng.integers(0, m, n - k)] + rng.normal(size=(n - k, 3)) * 1e-3])
    Tt = I.Transform([0.10, -0.08, 0.03])
    src = np.ascontiguousarray(moved(rng.permutation(world), Tt.inverse()))
    return dst, src, Tt


def d2_of(src, T, b):
    """section 12's d2, every operation rounded on its own"""
    r00, r10, r01, r11, tx, ty = T.pose.as_tuple()
    qx = (r00 * src[:, 0] + r01 * src[:, 1]) + tx
    qy = (r10 * src[:, 0] + r11 * src[:, 1]) + ty
    ex, ey, dz = qx - b[:, 0], qy - b[:, 1], src[:, 2] - b[:, 2]
    return qx, qy, dz, (ex * ex + ey * ey) + dz * dz


@pytest.fixture(scope="module")
def scene5():
    dst, src, Tt = blob_scene(5)
    icp = I.Icp3d(dst)
    icp.compute_normals(10)
    yield icp, dst, src, Tt
    icp.close()


# ------------------------------------------------------------------ the gate alone

@pytest.fixture(scope="module")
def stage_handle():
    rng = np.random.default_rng(11)
    dst = room(rng, 2048)
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    yield icp, dst, icp.read_normals()
    icp.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_stage_call_equals_numpy(stage_handle, n):
    import torch

    icp, dst, normals = stage_handle
    m = len(dst)
    rng = np.random.default_rng(1000 + n)
    T = I.Transform([0.05, -0.03, 0.2])
    idx = rng.integers(0, m, n).astype(np.int32)
    # near their (random) partner or far from it, half and half: r = 0.05 separates them
    src = dst[idx] + rng.normal(size=(n, 3)) * np.where(rng.random(n) < 0.5, 0.01, 0.5)[:, None]
    src = np.ascontiguousarray(moved(src, T.inverse()))
    if n >= 64:
        src[n // 2, 1] = np.nan  # a NaN source point is dropped at every finite or infinite bound
    d_src, d_idx = torch.from_numpy(src).cuda(), torch.from_numpy(idx).cuda()
    b, nj = dst[idx], normals[idx]
    qx, qy, dz, d2 = d2_of(src, T, b)
    want = np.stack([qx, qy, b[:, 0], b[:, 1], dz, nj[:, 0], nj[:, 1], nj[:, 2]], 1)
    for r in (0.05, 0.0, INF):
        with np.errstate(invalid="ignore"):
            mask = d2 <= r * r
        d_pairs = torch.full((n, 8), -7.0, dtype=torch.float64, device="cuda")
        d_kept = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        kept = icp.gate_plane_pairs_device(d_src, T, d_idx, r, d_pairs, d_kept)
        print(f"n={n} r={r}: kept {kept} of {n}")
        assert kept == int(mask.sum()), (n, r, kept, int(mask.sum()))
        pos = d_kept.cpu().numpy()
        assert np.array_equal(pos[:kept], np.flatnonzero(mask)), (n, r)
        assert np.all(pos[kept:] == -1)  # nothing is written behind the survivors
        got = d_pairs.cpu().numpy()
        assert np.array_equal(got[:kept].view(np.uint64), want[mask].view(np.uint64)), (n, r)
        assert np.all(got[kept:] == -7.0)
        # without the positions: the same pairs
        d_pairs2 = torch.full((n, 8), -7.0, dtype=torch.float64, device="cuda")
        assert icp.gate_plane_pairs_device(d_src, T, d_idx, r, d_pairs2) == kept
        assert torch.equal(d_pairs2, d_pairs)
        if r == 0.05 and n >= 64:
            assert 0.25 * n < kept < 0.75 * n, (n, kept)
        if r == INF:
            assert kept == n - (1 if n >= 64 else 0)


def test_stage_call_on_the_chunk_sum_path(stage_handle):
    """the smallest n whose last tile has a whole chunk of tiles (8 192 tiles of 1 024 points) and one more tile in front of
    it: 2^23 + 1025.  Only the count and the positions are checked."""
    import torch

    icp, dst, _ = stage_handle
    m = len(dst)
    n = (1 << 23) + 1025
    T = I.Transform()
    rng = np.random.default_rng(3)
    block = 4096  # (divides neither 2^23 + 1025 nor the tile into equal survivor counts: 1 keep in 3, then 2 in 5)
    j = np.arange(block) % m
    off = np.where((np.arange(block) % 3 == 0) | (np.arange(block) % 5 == 1), 0.001, 1.0)
    tile = dst[j] + np.stack([np.zeros(block), np.zeros(block), off], 1)
    reps = -(-n // block)
    d_src = torch.from_numpy(np.ascontiguousarray(tile)).cuda().repeat(reps, 1)[:n].contiguous()
    # idx = arange % m, and the block is a multiple of m: the partner of point i is dst[i % m]
    assert block % m == 0
    d_idx = (torch.arange(n, dtype=torch.int64, device="cuda") % m).to(torch.int32)
    d_pairs = torch.empty((n, 8), dtype=torch.float64, device="cuda")
    d_kept = torch.empty((n,), dtype=torch.int32, device="cuda")
    kept = icp.gate_plane_pairs_device(d_src, T, d_idx, 0.01, d_pairs, d_kept)
    keep_block = off < 0.5
    want = torch.from_numpy(np.tile(keep_block, reps)[:n]).cuda().nonzero().flatten().to(torch.int32)
    assert kept == want.shape[0], (kept, want.shape[0])
    assert torch.equal(d_kept[:kept], want)
    del d_pairs, d_kept, d_src, d_idx, want
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ +inf equals the ungated call

@pytest.mark.parametrize("n", [2, 65, 1025, 12000])
def test_an_infinite_bound_returns_the_bits_of_the_ungated_call(scene5, n):
    import torch

    icp, dst, _, Tt = scene5
    rng = np.random.default_rng(n)
    src = np.ascontiguousarray(moved(dst[rng.integers(0, len(dst), n)] + rng.normal(size=(n, 3)) * 2e-3, Tt.inverse()))
    T0, idx0, inner0 = icp.estimate_point_to_plane(src, I.Transform(), 4, return_info=True)
    d_src = torch.from_numpy(src).cuda()
    for s in (src, d_src):
        T, idx, inner, inl = icp.estimate_point_to_plane(s, I.Transform(), 4, return_info=True,
                                                         max_correspondence_distance=INF)
        assert np.array_equal(bits(T), bits(T0)), (n, T.as_array(), T0.as_array())
        assert np.array_equal(idx, idx0) and np.array_equal(inner, inner0), (n, inner, inner0)
        assert np.array_equal(inl, np.full(4, n)), (n, inl)
        T1 = icp.estimate_point_to_plane(s, I.Transform(), 4, max_correspondence_distance=INF)  # (without the info)
        assert np.array_equal(bits(T1), bits(T0))
    if n >= 65:
        assert inner0.sum() > 0


# ------------------------------------------------------------------ a finite bound against two restatements

def chain(icp, src, max_iter, r, step):
    """the definition, one outer iteration at a time: the kept points of iteration k are those whose match under T_k
    (evaluate's indices: the same exact search) lies within r; `step(src[keep], T_k)` = (T_{k+1}, inner count)"""
    dst = icp.read_targets()
    T = I.Transform()
    inner, inl = np.zeros(max_iter, dtype=np.uint32), np.zeros(max_iter, dtype=np.uint32)
    for k in range(max_iter):
        _, idx = icp.evaluate(src, T, INF, return_indices=True)
        _, _, _, d2 = d2_of(src, T, dst[idx])
        with np.errstate(invalid="ignore"):
            keep = d2 <= r * r
        inl[k] = keep.sum()
        T, inner[k] = step(np.ascontiguousarray(src[keep]), T)
    return T, inner, inl


def test_a_finite_bound_equals_the_restatement_on_the_same_handle_bit_for_bit(scene5):
    icp, dst, src, Tt = scene5
    T, idx, inner, inl = icp.estimate_point_to_plane(src, I.Transform(), 10, return_info=True,
                                                     max_correspondence_distance=0.25)

    def step(kept, Tk):
        Tn, _, inner_k = icp.estimate_point_to_plane(kept, Tk, 1, return_info=True)
        return Tn, inner_k[0]

    rT, rinner, rinl = chain(icp, src, 10, 0.25, step)
    print("inliers", inl.tolist(), "inner", inner.tolist())
    assert np.array_equal(inl, rinl), (inl, rinl)
    assert np.array_equal(inner, rinner), (inner, rinner)
    assert np.array_equal(bits(T), bits(rT)), (T.as_array(), rT.as_array())
    assert len(set(inl.tolist())) > 1  # the gate changes while the loop runs
    # the indices are those of ALL points at the pose the last iteration started from
    Tb = icp.estimate_point_to_plane(src, I.Transform(), 9, max_correspondence_distance=0.25)
    _, want_idx = icp.evaluate(src, Tb, INF, return_indices=True)
    assert np.array_equal(idx, want_idx)


def test_a_finite_bound_tracks_the_cpu_statement(scene5):
    icp, dst, src, Tt = scene5
    T, _, inner, inl = icp.estimate_point_to_plane(src, I.Transform(), 10, return_info=True,
                                                   max_correspondence_distance=0.25)
    normals = icp.read_normals()
    tree = O.KdTree(dst)

    def step(kept, Tk):
        rc, oT, _, oinner = O.p2pl_estimate(tree, normals, kept, O.Pose(*Tk.pose.as_tuple()), 1)
        assert rc == O.OK
        return I.Transform.from_pose(oT), oinner[0]

    oT, oinner, oinl = chain(icp, src, 10, 0.25, step)
    assert np.array_equal(inl, oinl), (inl, oinl)
    assert np.array_equal(inner, oinner), (inner, oinner)
    err = np.max(np.abs(T.as_array() - oT.as_array()))
    print("against the CPU statement:", err)
    assert err < 1e-9  # tests/test_p2plane.py's bar for tree sums against left folds

    def tree_step(kept, Tk):  # the same step with its sums in the tree of reduce_geometry(kept): equal to the bit
        rc, tT, _, tinner = oracle_plane_in_device_order(icp, tree, normals, kept, Tk, 1)
        assert rc == O.OK
        return I.Transform.from_pose(tT), tinner[0]

    tT, tinner, tinl = chain(icp, src, 10, 0.25, tree_step)
    assert np.array_equal(inl, tinl) and np.array_equal(inner, tinner), (inner, tinner)
    assert np.array_equal(bits(T), bits(tT)), (T.as_array(), tT.as_array())


@pytest.mark.parametrize("seed", [5, 6, 7])
def test_the_gate_helps_on_a_scan_with_an_object_the_map_does_not_hold(seed):
    """the CPU statement (orc_p2pl_estimate, chained on the kept points) gives an ungated error of 0.358-0.375 and a
    ratio of 13.8-21.7 on these three scenes: the bars (0.1, a fifth) leave a margin of about 3"""
    dst, src, Tt = blob_scene(seed)
    icp = I.Icp3d(dst)
    icp.compute_normals(10)
    truth = Tt.as_array()
    plain = np.abs(icp.estimate_point_to_plane(src, I.Transform(), 10).as_array() - truth).max()
    gated = np.abs(icp.estimate_point_to_plane(src, I.Transform(), 10, max_correspondence_distance=0.25).as_array()
                   - truth).max()
    icp.close()
    print(f"seed {seed}: ungated error {plain:.4f}, gated {gated:.4f}, ratio {plain / gated:.1f}")
    assert plain > 0.1, plain
    assert gated < plain / 5, (gated, plain)


# ------------------------------------------------------------------ edges and state

def test_zero_and_one_inlier_leave_the_pose_alone(scene5):
    icp, dst, src, Tt = scene5
    init = I.Transform([0.01, 0.02, 0.005])
    far = np.ascontiguousarray(src[:200] + np.array([0.0, 0.0, 50.0]))
    T, _, inner, inl = icp.estimate_point_to_plane(far, init, 3, return_info=True, max_correspondence_distance=0.25)
    assert np.array_equal(bits(T), bits(init)) and inner.tolist() == [0, 0, 0] and inl.tolist() == [0, 0, 0]
    one = far.copy()
    one[17] = moved(dst[5:6], init.inverse())[0]  # lands on a target exactly up to rounding
    T, _, inner, inl = icp.estimate_point_to_plane(one, init, 3, return_info=True, max_correspondence_distance=0.25)
    assert np.array_equal(bits(T), bits(init)) and inner.tolist() == [0, 0, 0] and inl.tolist() == [1, 1, 1]


def test_gated_and_ungated_calls_do_not_disturb_each_other_and_normals_must_be_current():
    dst, src, Tt = blob_scene(8, n=1500, m=3000)
    icp = I.Icp3d(dst)
    with pytest.raises(I.IcpError):  # normals first
        icp.estimate_point_to_plane(src, I.Transform(), 2, max_correspondence_distance=0.25)
    icp.compute_normals(8)
    fresh = I.Icp3d(dst)
    fresh.compute_normals(8)
    alone_gated = fresh.estimate_point_to_plane(src, I.Transform(), 4, return_info=True, max_correspondence_distance=0.25)
    fresh.close()
    alone_plain = icp.estimate_point_to_plane(src, I.Transform(), 4, return_info=True)  # (the first call of its handle)
    for _ in range(2):
        g = icp.estimate_point_to_plane(src, I.Transform(), 4, return_info=True, max_correspondence_distance=0.25)
        p = icp.estimate_point_to_plane(src, I.Transform(), 4, return_info=True)
        assert np.array_equal(bits(g[0]), bits(alone_gated[0]))
        assert all(np.array_equal(a, b) for a, b in zip(g[1:], alone_gated[1:]))
        assert np.array_equal(bits(p[0]), bits(alone_plain[0]))
        assert all(np.array_equal(a, b) for a, b in zip(p[1:], alone_plain[1:]))
    rng = np.random.default_rng(9)
    icp.append(room(rng, 900) + np.array([0.0, 0.0, 0.001]))
    with pytest.raises(I.IcpError):  # the appended targets have no normal yet
        icp.estimate_point_to_plane(src, I.Transform(), 2, max_correspondence_distance=0.25)
    icp.update_normals(8)
    T, _, inner, inl = icp.estimate_point_to_plane(src, I.Transform(), 4, return_info=True,
                                                   max_correspondence_distance=0.25)
    assert inner.sum() > 0 and np.all(inl > 0) and np.all(inl < len(src))
    icp.close()


@pytest.mark.parametrize("world", [1, 2, 4])
def test_gated_point_to_plane_across_virtual_ranks_equals_one_handle(scene5, world):
    icp, dst, src, Tt = scene5
    T1, idx1, inner1, inl1 = icp.estimate_point_to_plane(src, I.Transform(), 5, return_info=True,
                                                         max_correspondence_distance=0.25)
    multi = I.IcpMulti(dst, [0] * world)
    multi.compute_target_normals(10)
    T, idx, inner, inl = multi.estimate_point_to_plane(src, I.Transform(), 5, return_info=True,
                                                       max_correspondence_distance=0.25)
    Tp, idxp, innerp = multi.estimate_point_to_plane(src, I.Transform(), 5, return_info=True)  # (ungated: as before)
    P1 = icp.estimate_point_to_plane(src, I.Transform(), 5, return_info=True)
    multi.close()
    assert np.array_equal(bits(T), bits(T1)), (T.as_array(), T1.as_array())
    assert np.array_equal(idx, idx1) and np.array_equal(inner, inner1) and np.array_equal(inl, inl1)
    assert inner.sum() > 0 and len(set(inl.tolist())) > 1
    assert np.array_equal(bits(Tp), bits(P1[0])) and np.array_equal(idxp, P1[1]) and np.array_equal(innerp, P1[2])
