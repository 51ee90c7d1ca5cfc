"""Batched point-to-line registration (IcpBatch.estimate_point_to_line*, include/icp_mi355x.h section 15) against the
single call: every item's status, pose, indices and inner counts equal, bit for bit, what a fresh Icp2d(dst_i) returns
after compute_line_normals(k) from estimate_point_to_line(src_i, init_i, max_iter) -- whichever way the batch served it
(a workgroup of the batch launch, normals included, or one by one)."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from test_gpu_batch import random_item
from test_line_abi import GOLDEN_K, load_golden, oracle_point_to_line

pytestmark = pytest.mark.gpu

M_LINE = 2048  # the largest target count a workgroup serves
N_LINE = 1024


def single(dst, src, init, max_iter, k):
    """(status, pose, indices, inner counts) of the single call on a fresh handle"""
    icp = I.Icp2d(dst)
    try:
        icp.compute_line_normals(k)
        T, idx, inner = icp.estimate_point_to_line(src, init, max_iter, return_info=True)
        return _lib.OK, T.as_array(), idx, inner
    except I.IcpError as e:
        return e.status, None, None, None
    finally:
        icp.close()


def assert_items_match(srcs, dsts, inits, max_iter, k, got):
    Ts, idxs, inner, status = got
    assert len(Ts) == len(srcs)
    for i, (s, d, T0) in enumerate(zip(srcs, dsts, inits)):
        rc, pose, idx, inn = single(d, s, T0, max_iter, k)
        assert status[i] == rc, (i, status[i], rc)
        if rc != _lib.OK:
            assert Ts[i] is None
            continue
        assert np.array_equal(Ts[i].as_array(), pose), i
        assert np.array_equal(idxs[i], idx), i
        assert np.array_equal(inner[i], inn), i


def fits(n, m):
    return 1 <= n <= N_LINE and 1 <= m <= M_LINE


def test_edges_of_the_fold_tree_and_of_the_limits():
    ns = [1, 2, 3, 63, 64, 65, 511, 512, 513, 768, 769, 1023, 1024, 1025]
    ms = [1, 2, 3, 4, 64, 65, M_LINE - 1, M_LINE, M_LINE + 1]
    # every n with an m and every m with an n, then more crossings of the edges of both: 40 items
    shapes = [(n, ms[(3 * i + 5) % len(ms)]) for i, n in enumerate(ns)]
    shapes += [(ns[(5 * i + 4) % len(ns)], m) for i, m in enumerate(ms)]
    shapes += [(1024, M_LINE), (1025, M_LINE + 1), (1, 1), (512, M_LINE), (513, M_LINE - 1), (1023, 65), (768, 64),
               (769, 4), (2, 3), (3, 2), (64, 1), (65, M_LINE), (511, 3), (1024, 1), (63, M_LINE - 1), (1025, 64),
               (512, M_LINE + 1)]
    assert len(shapes) == 40
    rng = np.random.default_rng(1500)
    items = [random_item(rng, 2, n=n, m=m) for n, m in shapes]
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(2)
    got = B.estimate_point_to_line(srcs, dsts, inits, 20, k=8, return_info=True, allow_failures=True)
    assert_items_match(srcs, dsts, inits, 20, 8, got)
    served, one_by_one, launches, refused = B.line_counters()
    inside = sum(fits(n, m) for n, m in shapes)
    handed_back = one_by_one - (len(shapes) - inside)
    print(f"inside the limits {inside}, served {served}, one by one {one_by_one}, handed back {handed_back}")
    assert refused == 0 and launches == 2 and served + one_by_one == len(shapes)
    assert handed_back >= 0          # every item outside the limits is counted one by one
    assert 32 * handed_back <= inside  # of those inside, at most 1 in 32 may be handed back
    assert B.counters() == (0, 0, 0, 0)  # (the point batch's counters are its own)
    B.close()


@pytest.mark.parametrize("k", [3, 16])
def test_neighbourhood_size_at_its_ends_and_clamped(k):
    rng = np.random.default_rng(1600 + k)
    items = [random_item(rng, 2, n=200, m=5), random_item(rng, 2, n=700, m=5), random_item(rng, 2, n=200, m=300),
             random_item(rng, 2, n=700, m=300)]  # (m = 5 with k = 16: k > m, clamped)
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(2)
    got = B.estimate_point_to_line(srcs, dsts, inits, 20, k=k, return_info=True, allow_failures=True)
    assert_items_match(srcs, dsts, inits, 20, k, got)
    assert B.line_counters()[:2] == (4, 0)
    B.close()


def test_golden_scan_pairs_and_the_cpu_statement():
    scans = [load_golden(j) for j in range(1, 12)]
    srcs = scans[:10] + [scans[0]]   # 001 -> 002 ... 010 -> 011, and 001 -> 010
    dsts = scans[1:11] + [scans[9]]
    ident = [I.Transform() for _ in srcs]
    B = I.IcpBatch(2)
    got = B.estimate_point_to_line(srcs, dsts, ident, 20, k=GOLDEN_K, return_info=True)
    assert_items_match(srcs, dsts, ident, 20, GOLDEN_K, got)
    assert B.line_counters()[:2] == (len(srcs), 0)  # no hand-back
    B.close()
    print("inner counts:", [got[2][i].tolist() for i in range(len(srcs))])
    O.set_threads(16)
    try:
        for i in (0, 10):  # 001 -> 002 and 001 -> 010 against the CPU statement fed the device's normals
            icp = I.Icp2d(dsts[i])
            icp.compute_line_normals(GOLDEN_K)
            normals = icp.read_line_normals()
            icp.close()
            rc, oT, oidx, oinner = oracle_point_to_line(dsts[i], normals, srcs[i], I.Transform(), 20)
            assert rc == O.OK
            assert np.array_equal(got[1][i], oidx) and np.array_equal(got[2][i], oinner), i
            assert float(np.max(np.abs(got[0][i].as_array() - oT.as_array()))) < 1e-9, i
    finally:
        O.set_threads(1)


def test_hypotheses_share_one_range_and_each_equals_its_single_call():
    src, dst = load_golden(5), load_golden(6)
    rng = np.random.default_rng(7)
    inits = [I.Transform([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.4, 0.4)]) for _ in range(64)]
    B = I.IcpBatch(2)
    got = B.estimate_point_to_line_packed(src, dst, [(0, len(src), 0, len(dst), T) for T in inits], 20, k=GOLDEN_K,
                                          return_info=True, allow_failures=True)
    assert_items_match([src] * 64, [dst] * 64, inits, 20, GOLDEN_K, got)
    served, one_by_one, launches, refused = B.line_counters()
    assert (served + one_by_one, launches, refused) == (64, 1, 0)
    B.close()


def mixed_items():
    rng = np.random.default_rng(1700)
    items = [random_item(rng, 2, n=300, m=400)]
    s, d, T = random_item(rng, 2, n=300, m=400)
    s[3, 1] = np.nan
    items.append((s, d, T))  # a NaN source coordinate: ICP_NAN_INPUT
    _, d, T = random_item(rng, 2, n=1, m=30)
    items.append((np.zeros((0, 2)), d, T))  # n = 0
    s, _, T = random_item(rng, 2, n=40, m=10)
    items.append((s, np.zeros((0, 2)), T))  # m = 0: ICP_EMPTY_DST
    wall = np.ascontiguousarray(np.stack([np.full(900, 3.0), rng.uniform(-3, 3, 900)], axis=1))
    s = wall[rng.integers(0, 900, 600)].copy()
    s[:, 0] += rng.normal(-0.02, 2e-3, len(s))
    items.append((s, wall, I.Transform()))  # a single wall: all normals (1, 0), singular, no update
    line = np.ascontiguousarray(np.stack([np.linspace(-3, 3, 500), 0.5 * np.linspace(-3, 3, 500) + 1.0], axis=1))
    s = line[rng.integers(0, 500, 350)] + rng.normal(0.0, 5e-3, size=(350, 2))
    items.append((np.ascontiguousarray(s), line, I.Transform([0.01, -0.01, 0.002])))  # collinear targets
    items.append(random_item(rng, 2, n=900, m=1500))
    return items


def test_statuses_and_bits_in_a_mixed_batch():
    srcs, dsts, inits = zip(*mixed_items())
    B = I.IcpBatch(2)
    got = B.estimate_point_to_line(srcs, dsts, inits, 20, k=8, return_info=True, allow_failures=True)
    assert_items_match(srcs, dsts, inits, 20, 8, got)
    status = got[3]
    assert status.tolist() == [_lib.OK, _lib.NAN_INPUT, _lib.OK, _lib.EMPTY_DST, _lib.OK, _lib.OK, _lib.OK]
    assert got[2][4].tolist() == [0] * 20 and np.array_equal(got[0][4].as_array(), I.Transform().as_array())
    served, one_by_one = B.line_counters()[:2]
    assert served + one_by_one == len(srcs) and one_by_one >= 2  # (n = 0 and m = 0 go one by one)
    with pytest.raises(I.IcpError, match="item 1"):
        B.estimate_point_to_line(srcs, dsts, inits, 20, k=8)
    # no outer iteration for the whole call: every item one by one, each as its single call
    before = B.line_counters()
    got0 = B.estimate_point_to_line(srcs, dsts, inits, 0, k=8, return_info=True, allow_failures=True)
    assert_items_match(srcs, dsts, inits, 0, 8, got0)
    assert got0[2].shape == (len(srcs), 0)
    after = B.line_counters()
    assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (0, len(srcs), 0)
    B.close()


def test_device_entry_equals_host_entry_twice_and_buffers_are_reused():
    import torch

    rng = np.random.default_rng(1800)
    B = I.IcpBatch(2)
    for count in (24, 5, 40):  # grow, shrink, grow: the batch's buffers are reused and resized
        items = [random_item(rng, 2, n=int(rng.integers(1, 1025)), m=int(rng.integers(1, 800))) for _ in range(count)]
        srcs, dsts, inits = zip(*items)
        src, dst = np.concatenate(srcs), np.concatenate(dsts)
        sf, df = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(d) for d in dsts])
        packed = [(sf[i], len(srcs[i]), df[i], len(dsts[i]), inits[i]) for i in range(count)]
        host = B.estimate_point_to_line_packed(src, dst, packed, 20, k=8, return_info=True)
        again = B.estimate_point_to_line_packed(src, dst, packed, 20, k=8, return_info=True)
        dev = B.estimate_point_to_line_packed(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), packed, 20, k=8,
                                              return_info=True)
        for other in (again, dev):
            for i in range(count):
                assert np.array_equal(host[0][i].as_array(), other[0][i].as_array()), i
                assert np.array_equal(host[1][i], other[1][i]), i
            assert np.array_equal(host[2], other[2]) and np.array_equal(host[3], other[3])
        if count == 5:
            assert_items_match(srcs, dsts, inits, 20, 8, host)
    B.close()
