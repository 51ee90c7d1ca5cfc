"""Batched small registrations (IcpBatch, icp_batch_* of include/icp_mi355x.h section 8) against the single call: every
item's pose, indices and inner counts equal, bit for bit, what Icp{2,3}d(dst_i).estimate(src_i, init_i, max_iter)
returns on a handle of its own -- whichever way the batch served it (a workgroup of the batch launch, or one by one)."""
import os

import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from icp_rust_amd.scans import load_scan2d
from parity_util import oracle_in_device_order

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCANS = os.path.join(ROOT, "tests", "golden", "scans2d")


def single(dim, dst, src, init, max_iter):
    """(status, pose bits, indices, inner counts) of the single call on a fresh handle"""
    icp = (I.Icp2d if dim == 2 else I.Icp3d)(dst)
    try:
        T, idx, inner = icp.estimate(src, init, max_iter, return_info=True)
        return _lib.OK, T.as_array(), idx, inner
    except I.IcpError as e:
        return e.status, None, None, None
    finally:
        icp.close()


def assert_items_match(dim, srcs, dsts, inits, max_iter, got):
    Ts, idxs, inner, status = got
    for i, (s, d, T0) in enumerate(zip(srcs, dsts, inits)):
        rc, pose, idx, inn = single(dim, d, s, T0, max_iter)
        assert status[i] == rc, (i, status[i], rc)
        if rc != _lib.OK:
            assert Ts[i] is None
            continue
        assert np.array_equal(Ts[i].as_array(), pose), i
        assert np.array_equal(idxs[i], idx), i
        assert np.array_equal(inner[i], inn), i


def random_item(rng, dim, n=None, m=None):
    n = int(rng.integers(1, 1025)) if n is None else n
    m = int(rng.integers(1, 2049)) if m is None else m
    dst = rng.uniform(-20.0, 20.0, size=(m, dim))
    src = dst[rng.integers(0, m, size=n)].copy()
    th, t = rng.normal(0.0, 0.05), rng.normal(0.0, 0.5, size=2)
    c, s = np.cos(th), np.sin(th)
    x, y = src[:, 0].copy(), src[:, 1].copy()
    src[:, 0], src[:, 1] = c * x - s * y + t[0], s * x + c * y + t[1]
    src += rng.normal(0.0, 0.01, size=src.shape)
    init = I.Transform([rng.normal(0.0, 0.1), rng.normal(0.0, 0.1), rng.normal(0.0, 0.02)])
    return src, dst, init


@pytest.mark.parametrize("dim", [2, 3])
def test_random_items_in_one_call_equal_their_single_calls(dim):
    rng = np.random.default_rng(100 + dim)
    fixed_n = [1, 2, 100, 512, 513, 700, 768, 769, 1000, 1024]  # every workgroup size and its edges
    items = [random_item(rng, dim, n=fixed_n[k] if k < len(fixed_n) else None) for k in range(300)]
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(dim)
    got = B.estimate(srcs, dsts, inits, 20, return_info=True, allow_failures=True)
    assert_items_match(dim, srcs, dsts, inits, 20, got)
    served, one_by_one, launches, refused = B.counters()
    assert refused == 0 and launches == 3 and served + one_by_one == 300 and served >= 290
    # a sample against the CPU oracle, folded in the order the single call folded
    Ts, idxs, inner, status = got
    for i in range(0, 300, 37):
        icp = (I.Icp2d if dim == 2 else I.Icp3d)(dsts[i])
        icp.estimate(srcs[i], inits[i], 20)
        rc, oT, oidx, oinner = oracle_in_device_order(icp, dim, dsts[i], srcs[i], O.Pose(*inits[i].pose.as_tuple()), 20)
        icp.close()
        assert rc == O.OK
        assert np.array_equal(Ts[i].as_array(), oT.as_array()), i
        assert np.array_equal(idxs[i], oidx) and np.array_equal(inner[i], oinner), i


def golden_scans():
    return [load_scan2d(os.path.join(SCANS, f"{k:03d}.txt")) for k in range(1, 41)]


def test_consecutive_golden_scan_pairs_cold_and_warm():
    scans = golden_scans()
    srcs, dsts = scans[:-1], scans[1:]
    B = I.IcpBatch(2)
    ident = [I.Transform() for _ in srcs]
    assert_items_match(2, srcs, dsts, ident, 20, B.estimate(srcs, dsts, ident, 20, return_info=True, allow_failures=True))
    # the reference's scan2d loop: 001 is the fixed source, frame k warm-starts from frame k-1's pose
    from icp_rust_amd import harness

    Ts, _, _ = harness.run_scan2d(SCANS)
    warm = [I.Transform()] + Ts[:-1]
    srcs, dsts = [scans[0]] * len(Ts), scans[1:1 + len(Ts)]
    got = B.estimate(srcs, dsts, warm, 20, return_info=True, allow_failures=True)
    assert_items_match(2, srcs, dsts, warm, 20, got)
    assert all(np.array_equal(a.as_array(), b.as_array()) for a, b in zip(got[0], Ts))


def test_hypotheses_share_one_range_and_each_equals_its_single_call():
    scans = golden_scans()
    src, dst = scans[4], scans[5]
    rng = np.random.default_rng(7)
    inits = [I.Transform([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.4, 0.4)]) for _ in range(256)]
    B = I.IcpBatch(2)
    Ts, errs = B.estimate_hypotheses(src, dst, inits, 20)
    _, idxs, inner, status = B.estimate_packed(src, dst, [(0, len(src), 0, len(dst), T) for T in inits], 20,
                                               return_info=True, allow_failures=True)
    assert_items_match(2, [src] * 256, [dst] * 256, inits, 20, (Ts, idxs, inner, status))
    for k in range(0, 256, 51):
        assert errs[k] == I.huber_error(Ts[k], src, dst[idxs[k].astype(np.int64)])
    assert np.all(np.isfinite(errs))


def equal_run_pair(n):
    """the cloud of test_gpu_parity's run of equal residuals at the median (the smaller workgroups hand it back)"""
    rng = np.random.default_rng(n)
    side = int(np.ceil(np.sqrt(n)))
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    dst = (np.stack([gx.ravel(), gy.ravel()], axis=1)[:n] * 4.0 + rng.integers(0, 8, size=(n, 2)) / 8.0).astype(np.float64)
    off = np.empty((n, 2))
    k = max(int(0.4 * n), 160)
    off[:k] = (0.5, 0.25)
    h = (n - k) // 2
    off[k:k + h] = (0.5, 0.25) - rng.integers(1, 64, size=(h, 2)) / 128.0
    off[k + h:] = (0.5, 0.25) + rng.integers(1, 64, size=(n - k - h, 2)) / 128.0
    return dst + off, dst


def test_mixed_batch_of_edge_items_keeps_every_single_call_status_and_bits():
    rng = np.random.default_rng(5)
    items, kernel = [], []  # kernel[i]: the batch launch serves item i (else one by one)

    def add(item, in_kernel):
        items.append(item)
        kernel.append(in_kernel)

    add(random_item(rng, 2), True)
    add(random_item(rng, 2, n=5000, m=3000), False)  # beyond one workgroup
    s, d = equal_run_pair(600)
    add((s, d, I.Transform()), False)  # handed back by its workgroup
    add(random_item(rng, 2), True)
    s, d, T = random_item(rng, 2, n=300, m=400)
    d[17] = np.nan
    add((s, d, T), True)  # a NaN target: the box skips it, as build_grid does
    s, d, T = random_item(rng, 2, n=300, m=400)
    s[3, 1] = np.nan
    add((s, d, T), True)  # a NaN source: ICP_NAN_INPUT from the workgroup
    s, d, T = random_item(rng, 2, n=50, m=10)
    d[:] = np.nan
    add((s, d, T), False)  # no finite box: not served by the workgroup
    s, _, T = random_item(rng, 2, n=40, m=10)
    add((s, np.zeros((0, 2)), T), False)  # m = 0: ICP_EMPTY_DST
    _, d, T = random_item(rng, 2, n=1, m=30)
    add((np.zeros((0, 2)), d, T), False)  # n = 0
    add(random_item(rng, 2, n=1, m=30), True)
    add(random_item(rng, 2), True)
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(2)
    got = B.estimate(srcs, dsts, inits, 20, return_info=True, allow_failures=True)
    assert_items_match(2, srcs, dsts, inits, 20, got)
    status = got[3]
    assert status[5] == _lib.NAN_INPUT and status[7] == _lib.EMPTY_DST and status[8] == _lib.OK
    served, one_by_one, _, refused = B.counters()
    assert refused == 0 and (served, one_by_one) == (sum(kernel), len(kernel) - sum(kernel))
    with pytest.raises(I.IcpError, match="item 5"):
        B.estimate(srcs, dsts, inits, 20)


def test_no_iterations_and_no_items():
    rng = np.random.default_rng(9)
    items = [random_item(rng, 2) for _ in range(5)]
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(2)
    got = B.estimate(srcs, dsts, inits, 0, return_info=True)
    for i in range(5):
        rc, pose, idx, inner = single(2, dsts[i], srcs[i], inits[i], 0)
        assert rc == _lib.OK and np.array_equal(got[0][i].as_array(), pose) and np.array_equal(got[1][i], idx)
        assert got[2].shape == (5, 0)
    assert B.estimate([], [], [], 20) == []
    assert B.counters() == (0, 5, 0, 0)


def test_device_entry_equals_host_entry_and_buffers_are_reused():
    import torch

    rng = np.random.default_rng(11)
    B = I.IcpBatch(3)
    for count in (40, 7, 90):  # grow, shrink, grow: the batch's buffers are reused and resized
        items = [random_item(rng, 3) for _ in range(count)]
        srcs, dsts, inits = zip(*items)
        src, dst = np.concatenate(srcs), np.concatenate(dsts)
        sf, df = np.cumsum([0] + [len(s) for s in srcs]), np.cumsum([0] + [len(d) for d in dsts])
        packed = [(sf[i], len(srcs[i]), df[i], len(dsts[i]), inits[i]) for i in range(count)]
        host = B.estimate_packed(src, dst, packed, 20, return_info=True)
        dev = B.estimate_packed(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), packed, 20, return_info=True)
        for i in range(count):
            assert np.array_equal(host[0][i].as_array(), dev[0][i].as_array())
            assert np.array_equal(host[1][i], dev[1][i])
        assert np.array_equal(host[2], dev[2]) and np.array_equal(host[3], dev[3])
        if count == 7:
            assert_items_match(3, srcs, dsts, inits, 20, host)


def test_same_batch_twice_gives_the_same_bits():
    rng = np.random.default_rng(13)
    items = [random_item(rng, 2) for _ in range(64)]
    srcs, dsts, inits = zip(*items)
    B = I.IcpBatch(2)
    a = B.estimate(srcs, dsts, inits, 20, return_info=True)
    b = B.estimate(srcs, dsts, inits, 20, return_info=True)
    for i in range(64):
        assert np.array_equal(a[0][i].as_array(), b[0][i].as_array()) and np.array_equal(a[1][i], b[1][i])
    assert np.array_equal(a[2], b[2])
