"""Batched point-to-plane registration (IcpBatch.estimate_point_to_plane*, include/icp_mi355x.h section 18) against the
single call: every item's status, pose, indices and inner counts equal, bit for bit, what a fresh Icp3d(dst_i) returns
after compute_normals(k) from estimate_point_to_plane(src_i, init_i, max_iter) -- whichever way the batch served it (a
workgroup of the batch launch, normals included, or one by one)."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
import tie_clouds as TC
from icp_rust_amd import _lib
from parity_util import oracle_plane_in_device_order
from test_gpu_batch import random_item
from test_p2plane import moved, room

pytestmark = pytest.mark.gpu

M_PLANE = 2048  # the largest target count a workgroup serves
N_PLANE = 1024


def single(dst, src, init, max_iter, k):
    """(status, pose, indices, inner counts) of the single call on a fresh handle"""
    icp = None
    try:
        icp = I.Icp3d(dst)
        icp.compute_normals(k)
        T, idx, inner = icp.estimate_point_to_plane(src, init, max_iter, return_info=True)
        return _lib.OK, T.as_array(), idx, inner
    except I.IcpError as e:
        return e.status, None, None, None
    finally:
        if icp is not None:
            icp.close()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def assert_items_match(srcs, dsts, inits, max_iter, k, got):
    Ts, idxs, inner, status = got
    assert len(Ts) == len(srcs)
    for i, (s, d, T0) in enumerate(zip(srcs, dsts, inits)):
        rc, pose, idx, inn = single(d, s, T0, max_iter, k)
        assert status[i] == rc, (i, status[i], rc)
        if rc != _lib.OK:
            assert Ts[i] is None
            continue
        assert np.array_equal(Ts[i].as_array(), pose) and same_bits(Ts[i].as_array(), pose), i
        assert np.array_equal(idxs[i], idx), i
        assert np.array_equal(inner[i], inn), i


def fits(n, m):
    return 1 <= n <= N_PLANE and 1 <= m <= M_PLANE


def test_edges_of_the_fold_tree_and_of_the_limits():
    ns = [1, 2, 3, 63, 64, 65, 511, 512, 513, 768, 769, 1023, 1024, 1025]
    ms = [1, 2, 3, 4, 64, 65, M_PLANE - 1, M_PLANE, M_PLANE + 1]
    # every n with an m and every m with an n, then more crossings of the edges of both: 40 items (the shapes of
    # test_gpu_line_batch.py)
    shapes = [(n, ms[(3 * i + 5) % len(ms)]) for i, n in enumerate(ns)]
    shapes += [(ns[(5 * i + 4) % len(ns)], m) for i, m in enumerate(ms)]
    shapes += [(1024, M_PLANE), (1025, M_PLANE + 1), (1, 1), (512, M_PLANE), (513, M_PLANE - 1), (1023, 65), (768, 64),
               (769, 4), (2, 3), (3, 2), (64, 1), (65, M_PLANE), (511, 3), (1024, 1), (63, M_PLANE - 1), (1025, 64),
               (512, M_PLANE + 1)]
    assert len(shapes) == 40
    rng = np.random.default_rng(2500)
    items = [random_item(rng, 3, n=n, m=m) for n, m in shapes]
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(3)
    got = B.estimate_point_to_plane(srcs, dsts, inits, 20, k=8, return_info=True, allow_failures=True)
    assert_items_match(srcs, dsts, inits, 20, 8, got)
    served, one_by_one, launches, refused = B.plane_counters()
    inside = sum(fits(n, m) for n, m in shapes)
    handed_back = one_by_one - (len(shapes) - inside)
    print(f"inside the limits {inside}, served {served}, one by one {one_by_one}, handed back {handed_back}")
    assert refused == 0 and launches == 2 and served + one_by_one == len(shapes)
    assert handed_back >= 0          # every item outside the limits is counted one by one
    # finite coordinates and small rotations: none of the three hand-back reasons can occur, 0 expected; the cap only
    # keeps the test from passing through the fallback
    assert 32 * handed_back <= inside
    assert B.counters() == (0, 0, 0, 0) and B.line_counters() == (0, 0, 0, 0)  # (the other batches' counters are their own)
    B.close()


@pytest.mark.parametrize("k", [3, 16])
def test_neighbourhood_size_at_its_ends_and_clamped(k):
    rng = np.random.default_rng(2600 + k)
    items = [random_item(rng, 3, n=200, m=5), random_item(rng, 3, n=700, m=5), random_item(rng, 3, n=200, m=300),
             random_item(rng, 3, n=700, m=300)]  # (m = 5 with k = 16: k > m, clamped)
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(3)
    got = B.estimate_point_to_plane(srcs, dsts, inits, 20, k=k, return_info=True, allow_failures=True)
    assert_items_match(srcs, dsts, inits, 20, k, got)
    assert B.plane_counters()[:2] == (4, 0)
    B.close()


TIE_ROWS = 300
TIE_POSE = [0.02, -0.015, 0.01]
TIE_ITER = 4


@pytest.mark.parametrize("name,k", TC.PLANE_CASES, ids=[f"{name}-k{k}" for name, k in TC.PLANE_CASES])
def test_items_equal_the_single_calls_at_ties(name, k):
    """the sweep over the x-sorted targets with d^2 = (dx dx + dy dy) + dz dz against the grid kernel on lattice clouds,
    where the k-th place is a tie for many rows: 300 rows of the cloud seen from a small pose, the estimate started a
    fraction of a lattice spacing off it (at the pose itself every residual is zero and the result would not depend on
    the normals; at least 4 / 3 mm, so that on the fine lattice of the split cloud too the first update is above the
    threshold under which the inner loop stops)"""
    c = TC.cloud(name)
    assert c.dim == 3 and c.m <= 1152
    assert TC.moved_share(c, k) > 0  # a wrong tie rule changes normals the result depends on
    rows = np.random.default_rng(TC.SEED + 1).choice(c.m, TIE_ROWS, replace=False)
    T = I.Transform(TIE_POSE)
    src = np.ascontiguousarray(moved(np.ascontiguousarray(c.pts[rows]), T.inverse()))
    Ti = I.Transform([max(0.3 * c.spacing, 0.004), -max(0.2 * c.spacing, 0.003), 0.0]) * T
    rc, pose, idx, inner = single(c.pts, src, Ti, TIE_ITER, k)
    assert rc == _lib.OK
    B = I.IcpBatch(3)
    Ts, idxs, inn, st = B.estimate_point_to_plane([src], [c.pts], [Ti], TIE_ITER, k=k, return_info=True)
    assert B.plane_counters() == (1, 0, 1, 0)  # by the batch kernel, not one by one through the grid kernel
    B.close()
    print(f"{name} k={k}: inner counts {inner.tolist()}")
    assert st[0] == _lib.OK and same_bits(Ts[0].as_array(), pose), (Ts[0].as_array(), pose)
    assert np.array_equal(idxs[0], idx) and np.array_equal(inn[0], inner)


def test_room_scenes_equal_the_cpu_statement():
    """one call of 25 items: five room scenes at n = 2, 3, 65, 513, 1024, each bit-equal to the CPU statement with its
    sums in the tree of icp_reduce_geometry(n), fed the normals read from a fresh handle"""
    rng = np.random.default_rng(2700)
    ns = [2, 3, 65, 513, 1024]
    scenes = [room(rng, m) for m in (300, 700, 1100, 1600, 2048)]
    Tt = I.Transform([0.03, -0.02, 0.01])
    srcs, dsts = [], []
    for dst in scenes:
        for n in ns:
            s = dst[rng.integers(0, len(dst), n)] + rng.normal(0, 1e-3, (n, 3))
            srcs.append(np.ascontiguousarray(moved(s, Tt.inverse())))
            dsts.append(dst)
    B = I.IcpBatch(3)
    Ts, idxs, inner, status = B.estimate_point_to_plane(srcs, dsts, None, 8, k=10, return_info=True)
    assert B.plane_counters() == (25, 0, 2, 0)
    B.close()
    O.set_threads(16)
    try:
        for j, dst in enumerate(scenes):
            icp = I.Icp3d(dst)
            icp.compute_normals(10)
            normals = icp.read_normals()
            tree = O.KdTree(dst)
            for q in range(len(ns)):
                i = j * len(ns) + q
                rc, oT, oidx, oinner = oracle_plane_in_device_order(icp, tree, normals, srcs[i], I.Transform(), 8)
                assert rc == O.OK and status[i] == _lib.OK
                assert np.array_equal(idxs[i], oidx) and np.array_equal(inner[i], oinner), i
                assert same_bits(Ts[i].as_array(), oT.as_array()), (i, Ts[i].as_array(), oT.as_array())
            icp.close()
    finally:
        O.set_threads(1)
    print("inner counts:", inner.tolist())


def test_hypotheses_share_one_range_and_each_equals_its_single_call():
    rng = np.random.default_rng(2800)
    dst = room(rng, 1500)
    src = dst[rng.integers(0, len(dst), 650)] + rng.normal(0, 1e-3, (650, 3))
    inits = [I.Transform([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1)]) for _ in range(64)]
    B = I.IcpBatch(3)
    got = B.estimate_point_to_plane_packed(src, dst, [(0, len(src), 0, len(dst), T) for T in inits], 20, k=8,
                                           return_info=True, allow_failures=True)
    assert_items_match([src] * 64, [dst] * 64, inits, 20, 8, got)
    served, one_by_one, launches, refused = B.plane_counters()
    assert (served + one_by_one, launches, refused) == (64, 1, 0)
    B.close()


def mixed_items():
    rng = np.random.default_rng(2900)
    items = [random_item(rng, 3, n=300, m=400)]
    s, d, T = random_item(rng, 3, n=300, m=400)
    s[3, 2] = np.nan
    items.append((s, d, T))  # 1: a NaN source coordinate: ICP_NAN_INPUT
    s, d, T = random_item(rng, 3, n=200, m=300)
    d[17, 2] = np.nan
    items.append((s, d, T))  # 2: a NaN target coordinate: handed back, the single call's status
    _, d, T = random_item(rng, 3, n=1, m=30)
    items.append((np.zeros((0, 3)), d, T))  # 3: n = 0
    s, _, T = random_item(rng, 3, n=40, m=10)
    items.append((s, np.zeros((0, 3)), T))  # 4: m = 0: ICP_EMPTY_DST
    items.append(random_item(rng, 3, n=50, m=2))  # 5: m = 2: zero normals, no update
    floor = np.ascontiguousarray(np.stack([rng.uniform(-3, 3, 900), rng.uniform(-3, 3, 900), np.full(900, 0.5)], axis=1))
    s = floor[rng.integers(0, 900, 600)].copy()
    s[:, 2] += rng.normal(0.02, 2e-3, len(s))
    items.append((s, floor, I.Transform()))  # 6: all targets in one plane z = const: singular, no update
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
    srcs, dsts, inits = zip(*mixed_items())
    B = I.IcpBatch(3)
    got = B.estimate_point_to_plane(srcs, dsts, inits, 20, k=8, return_info=True, allow_failures=True)
    assert_items_match(srcs, dsts, inits, 20, 8, got)
    status = got[3]
    assert status[0] == _lib.OK and status[1] == _lib.NAN_INPUT and status[3] == _lib.OK and status[4] == _lib.EMPTY_DST
    # (item 2, the NaN target: whatever the single call makes of such a cloud -- assert_items_match compared status and
    # bits; the workgroup hands it back, counted below)
    assert status[5:].tolist() == [_lib.OK] * 5
    for i in (5, 6):  # zero normals / a single plane: no update, the pose stays the initial one
        assert got[2][i].tolist() == [0] * 20 and np.array_equal(got[0][i].as_array(), inits[i].as_array()), i
    served, one_by_one = B.plane_counters()[:2]
    assert served + one_by_one == len(srcs) and one_by_one >= 3  # (n = 0, m = 0 and the NaN target go one by one)
    with pytest.raises(I.IcpError, match="item 1"):
        B.estimate_point_to_plane(srcs, dsts, inits, 20, k=8)
    # no outer iteration for the whole call: every item one by one, each as its single call
    before = B.plane_counters()
    got0 = B.estimate_point_to_plane(srcs, dsts, inits, 0, k=8, return_info=True, allow_failures=True)
    assert_items_match(srcs, dsts, inits, 0, 8, got0)
    assert got0[2].shape == (len(srcs), 0)
    after = B.plane_counters()
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (0, len(srcs), 0)
    B.close()


def test_device_entry_equals_host_entry_twice_and_buffers_are_reused():
    import torch

    rng = np.random.default_rng(3000)
    B = I.IcpBatch(3)
    for count in (24, 5, 40):  # grow, shrink, grow: the batch's buffers are reused and resized
        items = [random_item(rng, 3, n=int(rng.integers(1, 1025)), m=int(rng.integers(1, 800))) for _ in range(count)]
        srcs, dsts, inits = zip(*items)
        src, dst = np.concatenate(srcs), np.concatenate(dsts)
        sf, df = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(d) for d in dsts])
        packed = [(sf[i], len(srcs[i]), df[i], len(dsts[i]), inits[i]) for i in range(count)]
        host = B.estimate_point_to_plane_packed(src, dst, packed, 20, k=8, return_info=True)
        again = B.estimate_point_to_plane_packed(src, dst, packed, 20, k=8, return_info=True)
        d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        ptrs = (d_src.data_ptr(), d_dst.data_ptr())
        dev = B.estimate_point_to_plane_packed(d_src, d_dst, packed, 20, k=8, return_info=True)
        assert (d_src.data_ptr(), d_dst.data_ptr()) == ptrs  # borrowed in place ...
        assert np.array_equal(d_src.cpu().numpy(), src) and np.array_equal(d_dst.cpu().numpy(), dst)  # ... and left alone
        for other in (again, dev):
            for i in range(count):
                assert np.array_equal(host[0][i].as_array(), other[0][i].as_array()), i
                assert np.array_equal(host[1][i], other[1][i]), i
            assert np.array_equal(host[2], other[2]) and np.array_equal(host[3], other[3])
        if count == 5:
            assert_items_match(srcs, dsts, inits, 20, 8, host)
    B.close()
