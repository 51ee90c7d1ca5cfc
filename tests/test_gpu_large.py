"""Clouds past 2^23 points, at the sizes bench.py's large lines run (gn_large: 64M pairs, nn_large: 2^24 x 2^24).

Past 2^23 points the reduction tree stops growing (common.hpp: reduce_geometry caps it at kTreeMaxBlocks = 2 048
blocks) and its threads fold more than eight points each: nine at 2^23 + 1, sixteen at 2^24, sixty-four at 64M.  The
evaluations there are checked against the oracle's tree variant bit for bit, and one update against an independent
long-double restatement of the reference (tests/test_wgn_reference.py derives the bound); the grid search against the
kd-tree; a rank that owns more than 256 tree blocks (the pipelined and in-launch sharded paths refuse it) against one
handle.  Host threads of the oracle: 16 at most (O.set_threads)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import synth
from parity_util import apply_pose, gn_large_pairs, oracle_in_device_order, oracle_loop, reference_wgn_update_identity
from test_wgn_reference import U, fold_depth_tree, rel_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def delta(before, after):
    return tuple(y - x for x, y in zip(before, after))


def device_estimate(a, b):
    """estimate_transform (src/lib.rs:59-84) through estimate_transform_device on a fresh handle, twice -- cold, then
    with the predictions of the first call, as bench.gn_large times it.  Both must give the same bits.  Returns
    (pose as an array, updates applied, path counters of the second call: window started, window missed, short
    pipeline, radix path, ...)."""
    icp = I.Icp3d(torch.zeros((1, 3), dtype=torch.float64, device="cuda"))
    try:
        d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        T0, applied0 = icp.estimate_transform_device(d_a, d_b)
        c0 = I.gn_path_counters(icp)
        T, applied = icp.estimate_transform_device(d_a, d_b)
        c1 = I.gn_path_counters(icp)
        del d_a, d_b
    finally:
        icp.close()
        torch.cuda.empty_cache()
    assert applied0 == applied and np.array_equal(T0.as_array(), T.as_array())
    return T.as_array(), applied, delta(c0, c1)


_oracle = {}


def oracle_estimate(n, heavy):
    """oracle_loop of gn_large_pairs(n, n + heavy, heavy), kept for the tests that look at the same pairs again"""
    if (n, heavy) not in _oracle:
        a, b = gn_large_pairs(n, n + heavy, heavy)
        oT, applied = oracle_loop(a, b)
        _oracle[(n, heavy)] = (oT.as_array(), applied)
    return _oracle[(n, heavy)]


# 2^23 + 1: the first size past the cap; 2^24: nn_large's; 2^26: gn_large's (64 pairs per thread)
@pytest.mark.parametrize("n,heavy", [(8_388_609, False), (16_777_216, False), (16_777_216, True), (67_108_864, False)])
def test_evaluations_past_the_tree_cap_equal_the_tree_oracle(n, heavy):
    """estimate_transform on pairs shaped like bench.gn_large (heavy: 10 % outliers, medians away from zero): the
    applied count and the pose of the oracle folding in the capped tree, bit for bit.  Above 4M pairs the refined
    windows (a 2^18 sample, windows narrowing as 1 / n) decide the medians: on the clean pairs they serve every
    evaluation without a miss."""
    blocks, threads = I.reduce_geometry(n)
    assert blocks == 2048 and threads == 512 and n > 8 * blocks * threads
    a, b = gn_large_pairs(n, n + heavy, heavy)
    got, applied, (tried, missed, short, radix, _, _) = device_estimate(a, b)
    del a, b
    oT, oapplied = oracle_estimate(n, heavy)
    assert applied == oapplied and applied >= 1, (applied, oapplied)
    assert np.array_equal(got, oT), (got, oT)
    evals = applied + 1  # (every update is followed by one more evaluation, whichever rule ends the loop)
    if heavy:
        assert tried - missed + short + radix >= evals, (tried, missed, short, radix)
    else:
        assert (tried, missed, short, radix) == (evals, 0, 0, 0)


def test_three_digit_radix_pipeline_past_the_tree_cap():
    """With the refined windows switched off (ICP_GN_NO_REFINE, read once per process: a child process) the radix
    pipeline with its third 12-bit digit serves 2^24 pairs alone -- what a failed refinement falls back to: the same
    bits as the oracle."""
    n = 16_777_216
    code = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import test_gpu_large as L\n"
        "a, b = L.gn_large_pairs(%d, %d)\n"
        "got, applied, c = L.device_estimate(a, b)\n"
        "print('result', applied, ' '.join(float(x).hex() for x in got), ' '.join(str(x) for x in c[:4]))\n"
    ) % (ROOT, HERE, n, n)
    env = dict(os.environ, ICP_GN_NO_REFINE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("result ")][-1].split()
    applied, got = int(line[1]), np.array([float.fromhex(x) for x in line[2:8]])
    tried, missed, short, radix = (int(x) for x in line[8:12])
    assert tried == 0 and short == applied + 1 and radix == 0, (tried, missed, short, radix)
    oT, oapplied = oracle_estimate(n, False)
    assert applied == oapplied and np.array_equal(got, oT), (got, oT)


@pytest.mark.parametrize("heavy", [False, True])
def test_one_update_past_the_tree_cap_against_the_longdouble_reference(heavy):
    """weighted_gauss_newton_update at the identity pose on 9M pairs (2 048 blocks, threads folding eight or nine): the
    device's four medians are the exact order statistics (its stddevs, bit for bit), and its update is within
    cond * (D + 8) * u of the long-double witness, D the depth of the device's tree (tests/test_wgn_reference.py).
    This does not share the tree oracle's fold: a block folded twice or dropped is 1e-4 of delta off."""
    n = 9_000_000
    a, b = gn_large_pairs(n, 3, heavy)
    want, sd, cond = reference_wgn_update_identity(a, b, skeel=True)
    assert cond < 10.0, cond
    T = I.Transform()
    assert np.array_equal(I.residual_stddevs(T, a, b), sd)
    got = I.weighted_gauss_newton_update(T, a, b)
    assert got is not None
    bound = cond * (fold_depth_tree(n) + 8) * U
    assert rel_err(got, want) <= bound, (got, want, rel_err(got, want), bound)


def _spacing(dst):
    return float(np.prod(dst.max(0) - dst.min(0)) / len(dst)) ** (1.0 / 3.0)


def test_search_at_nn_large_size_equals_the_kdtree_along_a_chain():
    """bench.nn_large's clouds (2^24 x 2^24, the 1M pair's box scaled by 16^(1/3): the same density) through
    prepare_source_device / correspond_device along a chain of poses -- the identity (the seeded first search), two
    small steps (warm searches, certificates), a jump of 30 NN spacings, a small step: every index is the kd-tree's,
    `a` the moved xy, `b` the matched target's xy.  Then three outer iterations of estimate equal the oracle's in
    the device's fold order: pose, indices, inner counts."""
    n = 1 << 24
    s = 16.0 ** (1.0 / 3.0)
    src, dst = synth.synthetic_pair(n, n, lo=synth.BOX_LO * s, hi=synth.BOX_HI * s)
    icp = I.Icp3d(dst)
    assert I.lib().icp_get_nn_mode(icp._h) == I.NN_GRID
    O.set_threads(16)
    try:
        tree = O.KdTree(dst)
        rng = np.random.default_rng(24)
        spacing, reach = _spacing(dst), float(np.abs(src[:, :2]).max())
        params = [np.zeros(3)]
        for st in (1e-3, 1e-4, 30.0, 1e-3):  # in NN spacings
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            step = st * spacing * d
            step[2] = step[2] / reach  # the rotation moves the farthest query by about as much
            params.append(params[-1] + step)
        d_q = torch.from_numpy(src).cuda()
        idx = torch.empty(n, dtype=torch.int32, device="cuda")
        a = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        b = torch.empty_like(a)
        icp.prepare_source_device(d_q, I.Transform(params[0]))
        moved = src.copy()
        for prm in params:
            T = I.Transform(prm)
            icp.correspond_device(d_q, T, a, b, idx)
            icp.synchronize()
            moved[:, :2] = apply_pose(T, src)
            rc, want = tree.search(moved)
            assert rc == O.OK
            got = idx.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want), (prm, int((got != want).sum()))
            assert np.array_equal(a.cpu().numpy(), moved[:, :2])
            assert np.array_equal(b.cpu().numpy(), dst[want][:, :2])
        assert I.nn_cert_counters(icp)[0] >= 1  # certificates were checked on the small steps
        del d_q, idx, a, b, tree, moved
        torch.cuda.empty_cache()
        Tg, idxg, innerg = icp.estimate(src, I.Transform(), 3, return_info=True)
        rc, oT, oidx, oinner = oracle_in_device_order(icp, 3, dst, src, O.transform_identity(), 3)
    finally:
        O.set_threads(1)
        icp.close()
    assert rc == O.OK
    assert np.array_equal(idxg, oidx)
    assert np.array_equal(innerg, oinner)
    assert np.array_equal(Tg.as_array(), oT.as_array())


def test_odd_sized_search_and_estimate_past_the_tree_cap():
    """20 000 003 queries against 3 000 001 targets (a last tree block of three points, nine or ten per thread):
    estimate equals the oracle's in the device's fold order -- pose, indices, inner counts"""
    src, dst = synth.synthetic_pair(20_000_003, 3_000_001)
    icp = I.Icp3d(dst)
    O.set_threads(16)
    try:
        T, idx, inner = icp.estimate(src, I.Transform(), 3, return_info=True)
        rc, oT, oidx, oinner = oracle_in_device_order(icp, 3, dst, src, O.transform_identity(), 3)
    finally:
        O.set_threads(1)
        icp.close()
    assert rc == O.OK
    assert np.array_equal(idx, oidx)
    assert np.array_equal(inner, oinner)
    assert np.array_equal(T.as_array(), oT.as_array())


@pytest.mark.parametrize("world,n", [(2, 4_200_000), (3, 9_000_001)])
def test_ranks_of_more_than_256_blocks_equal_one_handle(world, n):
    """IcpMulti with every rank on cuda:0, each rank owning more than 256 tree blocks: 513 at 2 x 4.2M, 683 at
    3 x 9M (the tree capped at 2 048 blocks of over 4 096 points).  The pipelined evaluation (pipe.hip) and the
    in-launch sharded loop refuse such a rank; the stage calls serve it, sharded.  Pose, indices and inner counts are
    one handle's bit for bit -- and at 9M the one handle's are the oracle's in the device's fold order."""
    m = 1_000_000
    src, dst = synth.synthetic_pair(n, m)
    blocks, _ = I.reduce_geometry(n)
    assert blocks // world > 256
    init = I.Transform([0.01, -0.02, 0.001])
    one = I.Icp3d(dst)
    T1, idx1, inner1 = one.estimate(src, init, 3, return_info=True)
    if n > 1 << 23:
        O.set_threads(16)
        try:
            rc, oT, oidx, oinner = oracle_in_device_order(one, 3, dst, src, O.Pose.from_array(init.as_array()), 3)
        finally:
            O.set_threads(1)
        assert rc == O.OK
        assert np.array_equal(idx1, oidx) and np.array_equal(inner1, oinner)
        assert np.array_equal(T1.as_array(), oT.as_array())
    one.close()
    multi = I.IcpMulti(dst, [0] * world)
    try:
        T, idx, inner = multi.estimate(src, init, 3, return_info=True)
        sharded, replicated = multi.counters()
        launches, _, _ = multi.loop_counters()
        piped = multi.pipe_iterations()
    finally:
        multi.close()
    assert np.array_equal(T.as_array(), T1.as_array())
    assert np.array_equal(inner, inner1) and np.array_equal(idx, idx1)
    assert piped == 0 and launches == 0, (piped, launches)
    assert sharded >= 1, (sharded, replicated, inner.tolist())
