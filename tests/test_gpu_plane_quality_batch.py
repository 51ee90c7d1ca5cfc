"""Batched point-to-plane pose quality (IcpBatch.evaluate_point_to_plane*, include/icp_mi355x.h section 20) against the
single sequence: every item's status, n, inliers and float fields equal, bit for bit, what a fresh Icp3d(dst_i) returns
after compute_normals(k) from evaluate_point_to_plane(src_i, T_i, r) -- whichever way the batch served it (a workgroup of
the one launch, normals included, or one by one); three items against the numpy restatement of section 13 directly; and
what the call is for: 64 hypotheses of a corridor and of a room ranked by plane_rmse, with the information the plane
residual gives next to the c I of the point residual's batch."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
import tie_clouds as TC
from icp_rust_amd import _lib
from test_gpu_batch import random_item
from test_gpu_plane_quality import NFLOATS, oracle_idx, restate, same_bits, scan_of
from test_p2plane import moved, room
from test_plane_quality_batch_abi import (SCENE_K, SCENE_R, TRUE_AT, assert_scene, hypotheses, scene_scan, thin_corridor,
                                          thin_room)

pytestmark = pytest.mark.gpu

M_PLANE, N_PLANE = 2048, 1024  # the largest item a workgroup serves
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.set_threads(16)
    yield
    O.set_threads(1)


def single(dst, src, T, k, r):
    """(status, inliers, float fields) of the single sequence on a fresh handle"""
    icp = None
    try:
        icp = I.Icp3d(dst)
        icp.compute_normals(k)
        q = icp.evaluate_point_to_plane(src, T, r)
        return _lib.OK, q.inliers, q.as_array()
    except I.IcpError as e:
        return e.status, None, None
    finally:
        if icp is not None:
            icp.close()


def assert_items_match(srcs, dsts, Ts, k, r, got):
    qs, status = got
    assert len(qs) == len(srcs)
    for i, (s, d, T) in enumerate(zip(srcs, dsts, Ts)):
        rc, inl, arr = single(d, s, T, k, r)
        assert status[i] == rc, (i, status[i], rc)
        if rc != _lib.OK:
            assert qs[i] is None
            continue
        assert qs[i].n == len(s) and qs[i].inliers == inl, (i, qs[i].inliers, inl)
        assert np.array_equal(qs[i].as_array(), arr), (i, qs[i].as_array(), arr)


def fits(n, m):
    return 1 <= n <= N_PLANE and 1 <= m <= M_PLANE


def nearest_d2(dst, q):
    """squared distance of every q to its nearest dst, by brute force"""
    d = q[:, None, :] - dst[None, :, :]
    return np.min((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)


# ------------------------------------------------------------------ (1) shape edges

def test_edges_of_the_fold_tree_of_the_list_rounds_and_of_the_limits():
    ns = [1, 2, 3, 255, 256, 257, 512, 513, 1023, 1024, 1025]
    ms = [1, 2, 3, 5, 63, 64, 65, 129, 1024, 2047, 2048, 2049]
    # every n with an m and every m with an n, then more crossings of the edges of both: 40 items
    shapes = [(n, ms[(3 * i + 5) % len(ms)]) for i, n in enumerate(ns)]
    shapes += [(ns[(5 * i + 4) % len(ns)], m) for i, m in enumerate(ms)]
    shapes += [(1024, 2048), (1025, 2049), (1, 1), (512, 2048), (513, 2047), (1023, 65), (256, 64), (257, 5), (2, 3),
               (3, 2), (255, 1), (1024, 1024), (513, 129), (1024, 1), (1025, 64), (512, 2049), (257, 2048)]
    assert len(shapes) == 40
    assert {n for n, _ in shapes} == set(ns) and {m for _, m in shapes} == set(ms)
    rng = np.random.default_rng(3100)
    srcs, dsts, Ts = [], [], []
    for n, m in shapes:
        dst = room(rng, m)
        T = I.Transform([rng.normal(0.0, 0.1), rng.normal(0.0, 0.1), rng.normal(0.0, 0.02)])
        srcs.append(scan_of(rng, dst, n, T))
        dsts.append(dst)
        Ts.append(T)
    # a bound that keeps about half of all the points
    r = float(np.sqrt(np.median(np.concatenate([nearest_d2(d, moved(s, T)) for s, d, T in zip(srcs, dsts, Ts)]))))
    B = I.IcpBatch(3)
    got = B.evaluate_point_to_plane(srcs, dsts, Ts, k=8, max_correspondence_distance=r, allow_failures=True,
                                    return_status=True)
    assert_items_match(srcs, dsts, Ts, 8, r, got)
    assert all(st == _lib.OK for st in got[1])
    share = sum(q.inliers for q in got[0]) / sum(q.n for q in got[0])
    served, one_by_one, launches, refused = B.plane_quality_counters()
    inside = sum(fits(n, m) for n, m in shapes)
    print(f"r {r:.4g}, inlier share {share:.3f}, inside the limits {inside}, served {served}, one by one {one_by_one}")
    assert 0.4 <= share <= 0.6
    # every item inside the limits in the one launch, none handed back, those outside one by one
    assert (served, one_by_one, launches, refused) == (inside, len(shapes) - inside, 1, 0)
    # (the other calls' counters are their own)
    assert B.evaluate_counters() == (0, 0, 0) and B.plane_counters() == (0, 0, 0, 0)
    assert B.plane_gated_counters() == (0, 0, 0, 0) and B.counters() == (0, 0, 0, 0)
    B.close()


# ------------------------------------------------------------------ (2) neighbourhood size

@pytest.mark.parametrize("k", [3, 16])
def test_neighbourhood_size_at_its_ends_and_clamped_and_too_few_targets(k):
    rng = np.random.default_rng(3200 + k)
    items = [random_item(rng, 3, n=200, m=5), random_item(rng, 3, n=700, m=5), random_item(rng, 3, n=200, m=300),
             random_item(rng, 3, n=700, m=300), random_item(rng, 3, n=40, m=2), random_item(rng, 3, n=300, m=1)]
    srcs, dsts, Ts = zip(*items)  # (m = 5 with k = 16: k > m, clamped; m < 3: zero normals, a valid result)
    B = I.IcpBatch(3)
    got = B.evaluate_point_to_plane(srcs, dsts, Ts, k=k, allow_failures=True, return_status=True)
    assert_items_match(srcs, dsts, Ts, k, INF, got)
    assert B.plane_quality_counters() == (6, 0, 1, 0)
    for i in (4, 5):
        q = got[0][i]
        assert got[1][i] == _lib.OK and q.inliers == q.n and not q.information.any() and not q.translation_eig.any()
        assert q.plane_sum_r2 == 0.0 and q.plane_rmse == 0.0 and q.error == 0.0 and q.huber_error == 0.0
        assert q.inlier_sum_d2 > 0.0
    B.close()


# ------------------------------------------------------------------ (3) bounds

@pytest.fixture(scope="module")
def bound_items():
    rng = np.random.default_rng(3300)
    return list(zip(*[random_item(rng, 3, n=n, m=m) for n, m in ((300, 400), (1000, 1500), (2, 700))]))


@pytest.mark.parametrize("r", [0.0, 0.3, INF])
def test_bounds_and_the_fields_shared_with_the_point_batch(bound_items, r):
    srcs, dsts, Ts = bound_items
    B = I.IcpBatch(3)
    got = B.evaluate_point_to_plane(srcs, dsts, Ts, k=8, max_correspondence_distance=r, return_status=True)
    assert_items_match(srcs, dsts, Ts, 8, r, got)
    if r == 0.0:
        assert all(q.inliers == 0 and q.plane_rmse == 0.0 and q.error > 0.0 and not q.information.any() for q in got[0])
    if r == INF:
        assert all(q.inliers == q.n for q in got[0])
    for q, p in zip(got[0], B.evaluate(srcs, dsts, Ts, r)):  # the point residual's batch: the same three fields' bits
        assert q.inliers == p.inliers
        assert same_bits([q.inlier_sum_d2, q.inlier_rmse, q.fitness], [p.inlier_sum_d2, p.inlier_rmse, p.fitness])
    B.close()


# ------------------------------------------------------------------ (4) the tie rule

TIE_ROWS = 300
TIE_POSE = [0.02, -0.015, 0.01]


@pytest.mark.parametrize("name,k", TC.PLANE_CASES, ids=[f"{name}-k{k}" for name, k in TC.PLANE_CASES])
def test_items_equal_the_single_calls_at_ties(name, k):
    """the sweep over the x-sorted targets against the grid kernel on lattice clouds, where the k-th place is a tie for
    many rows: 300 rows of the cloud seen from a small pose, scored a fraction of a lattice spacing off it (at the pose
    itself every residual is zero and the sums would not depend on the normals)"""
    c = TC.cloud(name)
    assert c.dim == 3 and c.m <= M_PLANE
    assert TC.moved_share(c, k) > 0  # a wrong tie rule changes normals the result depends on
    rows = np.random.default_rng(TC.SEED + 1).choice(c.m, TIE_ROWS, replace=False)
    T = I.Transform(TIE_POSE)
    src = np.ascontiguousarray(moved(np.ascontiguousarray(c.pts[rows]), T.inverse()))
    Ti = I.Transform([max(0.3 * c.spacing, 0.004), -max(0.2 * c.spacing, 0.003), 0.0]) * T
    r = INF  # (the offset is many spacings of the split cloud's fine lattice: every pair counts, test_bounds has the gate)
    B = I.IcpBatch(3)
    got = B.evaluate_point_to_plane([src], [c.pts], [Ti], k=k, max_correspondence_distance=r, return_status=True)
    assert B.plane_quality_counters() == (1, 0, 1, 0)  # by the batch kernel, not one by one through the grid kernel
    B.close()
    assert_items_match([src], [c.pts], [Ti], k, r, got)
    assert got[0][0].inliers == TIE_ROWS and got[0][0].information.any()


# ------------------------------------------------------------------ (5) the restatement

def test_batched_items_equal_the_restated_definition_directly():
    """not through the single call's sums: the fresh handle's targets and normals, the oracle's exact indices (which
    the single call's indices are held to first), the numpy restatement of section 13"""
    dst = room(np.random.default_rng(3400), 1500)
    rng = np.random.default_rng(3401)
    T = I.Transform([0.12, -0.07, 0.04])
    srcs = [scan_of(rng, dst, n, T) for n in (2, 257, 1024)]
    icp = I.Icp3d(dst)
    icp.compute_normals(8)
    targets, nrm = icp.read_targets(), icp.read_normals()
    assert np.array_equal(targets, dst)
    oidx = [oracle_idx(dst, s, T) for s in srcs]
    for s, want in zip(srcs, oidx):
        _, idx = icp.evaluate_point_to_plane(s, T, 0.03, return_indices=True)
        assert np.array_equal(idx, want), len(s)
    icp.close()
    B = I.IcpBatch(3)
    qs = B.evaluate_point_to_plane(srcs, [dst] * 3, T, k=8, max_correspondence_distance=0.03)
    assert B.plane_quality_counters() == (3, 0, 1, 0)
    B.close()
    for s, ix, q in zip(srcs, oidx, qs):
        rc, cnt, want = restate(targets, nrm, s, T, 0.03, ix)
        assert rc == _lib.OK and q.n == len(s) and q.inliers == cnt, (len(s), q.inliers, cnt)
        assert len(want) == NFLOATS and same_bits(q.as_array(), want), (len(s), q.as_array(), want)
        if len(s) > 2:
            assert 0 < cnt < len(s)


# ------------------------------------------------------------------ (6) hypotheses

def test_hypotheses_share_one_range_and_each_equals_its_single_call():
    rng = np.random.default_rng(3500)
    dst = room(rng, 1500)
    src = np.ascontiguousarray(dst[rng.integers(0, len(dst), 650)] + rng.normal(0, 1e-3, (650, 3)))
    Ts = [I.Transform([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1)]) for _ in range(64)]
    B = I.IcpBatch(3)
    got = B.evaluate_point_to_plane_packed(src, dst, [(0, len(src), 0, len(dst), T) for T in Ts], k=8,
                                           max_correspondence_distance=0.2, return_status=True)
    assert B.plane_quality_counters() == (64, 0, 1, 0)
    B.close()
    assert_items_match([src] * 64, [dst] * 64, Ts, 8, 0.2, got)


# ------------------------------------------------------------------ (7) a mixed batch

def mixed_items():
    rng = np.random.default_rng(3600)
    items = [random_item(rng, 3, n=300, m=400)]
    s, d, T = random_item(rng, 3, n=300, m=400)
    s[3, 2] = np.nan
    items.append((s, d, T))  # 1: a NaN source coordinate: ICP_NAN_INPUT, decided from the workgroup's record
    s, d, T = random_item(rng, 3, n=200, m=300)
    d[17, 2] = np.nan
    items.append((s, d, T))  # 2: a NaN target coordinate: handed back, the single call's status and bits
    _, d, T = random_item(rng, 3, n=1, m=30)
    items.append((np.zeros((0, 3)), d, T))  # 3: n = 0: ICP_OK and zeros
    s, _, T = random_item(rng, 3, n=40, m=10)
    items.append((s, np.zeros((0, 3)), T))  # 4: m = 0: ICP_EMPTY_DST
    items.append(random_item(rng, 3, n=50, m=2))  # 5: m = 2: zero normals
    floor = np.ascontiguousarray(np.stack([rng.uniform(-3, 3, 900), rng.uniform(-3, 3, 900), np.full(900, 0.5)], axis=1))
    s = floor[rng.integers(0, 900, 600)].copy()
    s[:, 2] += rng.normal(0.02, 2e-3, len(s))
    items.append((s, floor, I.Transform()))  # 6: all targets in one plane z = const: normals (0, 0, 1)
    t = np.linspace(-3, 3, 500)
    line = np.ascontiguousarray(np.stack([t, 0.5 * t + 1.0, 0.25 * t - 0.5], axis=1))
    s = line[rng.integers(0, 500, 350)] + rng.normal(0.0, 5e-3, size=(350, 3))
    items.append((np.ascontiguousarray(s), line, I.Transform([0.01, -0.01, 0.002])))  # 7: collinear targets
    base = room(rng, 400)
    dup = np.ascontiguousarray(np.repeat(base, 3, axis=0)[rng.permutation(1200)])
    s = base[rng.integers(0, 400, 500)] + rng.normal(0.0, 2e-3, size=(500, 3))
    items.append((np.ascontiguousarray(s), dup, I.Transform([0.02, 0.01, -0.005])))  # 8: every target three times
    items.append(random_item(rng, 3, n=900, m=1500))
    return items


def test_statuses_and_bits_in_a_mixed_batch():
    srcs, dsts, Ts = zip(*mixed_items())
    B = I.IcpBatch(3)
    got = B.evaluate_point_to_plane(srcs, dsts, Ts, k=8, max_correspondence_distance=0.5, allow_failures=True,
                                    return_status=True)
    assert_items_match(srcs, dsts, Ts, 8, 0.5, got)
    status = got[1].tolist()
    assert status[:2] == [_lib.OK, _lib.NAN_INPUT] and status[3:5] == [_lib.OK, _lib.EMPTY_DST]
    # (item 2, the NaN target: whatever the single call makes of such a cloud -- assert_items_match compared status and
    # bits; the workgroup hands it back, counted below)
    assert status[5:] == [_lib.OK] * 5
    assert got[0][3].n == 0 and got[0][3].inliers == 0 and not got[0][3].as_array().any()
    q = got[0][5]  # m = 2: zero normals, all-zero plane sums and information
    assert q.plane_sum_r2 == 0.0 and q.error == 0.0 and q.huber_error == 0.0 and not q.information.any()
    q = got[0][6]  # one plane z = const: the normals have no xy part beyond rounding, the translation is not observed
    assert q.inliers == q.n and q.translation_eig[1] <= 1e-12 * q.n and q.plane_rmse > 0.01
    # n = 0, m = 0 and the handed-back NaN target one by one, the other seven in the launch
    assert B.plane_quality_counters() == (7, 3, 1, 0)
    with pytest.raises(I.IcpError, match="item 1"):
        B.evaluate_point_to_plane(srcs, dsts, Ts, k=8, max_correspondence_distance=0.5)
    B.close()


# ------------------------------------------------------------------ (8) entries

def test_device_entry_equals_host_entry_twice_and_an_estimate_batch_around_them_keeps_its_bits():
    import torch

    rng = np.random.default_rng(3700)
    B = I.IcpBatch(3)
    est = [random_item(rng, 3, n=n, m=m) for n, m in ((300, 400), (900, 1500), (40, 70))]
    before = B.estimate_point_to_plane(*zip(*est), 10, k=8, return_info=True)
    for count in (24, 5, 40):  # grow, shrink, grow: the batch's buffers are reused and resized
        items = [random_item(rng, 3, n=int(rng.integers(1, 1025)), m=int(rng.integers(1, 800))) for _ in range(count)]
        srcs, dsts, Ts = zip(*items)
        src, dst = np.concatenate(srcs), np.concatenate(dsts)
        sf, df = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(d) for d in dsts])
        packed = [(sf[i], len(srcs[i]), df[i], len(dsts[i]), Ts[i]) for i in range(count)]
        host = B.evaluate_point_to_plane_packed(src, dst, packed, 8, 0.5, return_status=True)
        again = B.evaluate_point_to_plane_packed(src, dst, packed, 8, 0.5, return_status=True)
        d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        ptrs = (d_src.data_ptr(), d_dst.data_ptr())
        dev = B.evaluate_point_to_plane_packed(d_src, d_dst, packed, 8, 0.5, return_status=True)
        assert (d_src.data_ptr(), d_dst.data_ptr()) == ptrs  # borrowed in place ...
        assert np.array_equal(d_src.cpu().numpy(), src) and np.array_equal(d_dst.cpu().numpy(), dst)  # ... and left alone
        for other in (again, dev):
            for i in range(count):
                assert host[0][i].inliers == other[0][i].inliers, i
                assert np.array_equal(host[0][i].as_array(), other[0][i].as_array()), i
            assert np.array_equal(host[1], other[1])
        if count == 5:
            assert_items_match(srcs, dsts, Ts, 8, 0.5, host)
    assert B.plane_quality_counters() == (3 * (24 + 5 + 40), 0, 9, 0)
    after = B.estimate_point_to_plane(*zip(*est), 10, k=8, return_info=True)
    for i in range(len(est)):
        assert same_bits(before[0][i].as_array(), after[0][i].as_array()) and np.array_equal(before[1][i], after[1][i]), i
    assert np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3])
    assert sum(B.plane_counters()[:2]) == 2 * len(est)
    B.close()


# ------------------------------------------------------------------ (9) what it is for

def test_hypotheses_are_ranked_and_the_corridor_is_not_observed_along_its_axis():
    """the scenes and bars of tests/test_plane_quality_batch_abi.py (DESIGN.md section 9h's), which the numpy restatement
    meets on the CPU: 64 poses around the true one for a thinned corridor and for the closed room, all 128 in one
    launch; the point residual's batch on the same items has c I for its translation block, whatever the scene"""
    scenes = [("corridor", thin_corridor()), ("room", thin_room())]
    Ts = hypotheses()
    srcs = [scene_scan(dst) for _, dst in scenes]
    src, dst = np.concatenate(srcs), np.concatenate([d for _, d in scenes])
    packed, sf, df = [], 0, 0
    for s, (_, d) in zip(srcs, scenes):
        packed += [(sf, len(s), df, len(d), T) for T in Ts]
        sf, df = sf + len(s), df + len(d)
    B = I.IcpBatch(3)
    qs = B.evaluate_point_to_plane_packed(src, dst, packed, SCENE_K, SCENE_R)
    assert B.plane_quality_counters() == (128, 0, 1, 0)
    pp = B.evaluate_packed(src, dst, packed, SCENE_R)
    B.close()
    for j, ((name, d), s) in enumerate(zip(scenes, srcs)):
        mine = qs[64 * j:64 * j + 64]
        assert all(q.inliers == q.n == len(s) for q in mine)
        assert_scene(name, [q.as_array() for q in mine])
        rc, inl, arr = single(d, s, Ts[TRUE_AT], SCENE_K, SCENE_R)  # the true pose's item against its single sequence
        assert rc == _lib.OK and inl == len(s) and np.array_equal(mine[TRUE_AT].as_array(), arr)
        for p in pp[64 * j:64 * j + 64]:
            assert p.information[0][0] == p.information[1][1] == float(p.inliers)
