"""The wave's part of the block sums (gn_device.hpp: block_reduce_waves) folds its 19 sums as a PACKED tree: after the
step with offset 32 the upper half of a register carries another sum, after 16 every row of 16 lanes carries one.  The
operands and their order are those of the plain tree v[l] += v[l + off], off = 32 .. 1, which the oracle's tree variant
states -- so every result must still be the oracle's, bit for bit.  The other suites hold every evaluation to that
already, on inputs whose sums hardly depend on which lane met which; this file adds inputs on which a wrong pairing
of lanes cannot hide:

  * coordinates of magnitude 2^((i mod 64) mod 40) with random signs and full mantissas -- neighbouring lanes differ
    by a factor of two, rows of 16 by 2^16, so nearly every addition of the tree rounds.  That the block sums DO
    depend on the pairing is asserted on the CPU first (the oracle with the lanes' index bits swapped -- the tree's
    steps taken in another order -- and with another block size);
  * the smallest shapes at which the tree can go wrong: ragged last waves, one block and two, and the sizes either
    side of the one-workgroup estimate (1024) and of the inner loop in one launch (4096);
  * one NaN and one infinite residual in lane 37 of wave 5 -- row 2 of the wave, whose sums the packed tree leaves in
    lane 32.

Each size goes through one evaluation of the stage pipeline (weighted_gauss_newton_update: the one-workgroup kernel up
to 1024 pairs, the window launches beyond), through estimate_transform_device (from 4096 pairs on the inner loop in one
launch, k_gn_loop; at 4095 the window launches stepped from the host) and through one Icp3d.estimate(..., 2)."""
import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from parity_util import apply_pose, oracle_in_device_order, oracle_loop

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 127, 511, 512, 513, 4_095, 4_096, 4_097, 8_191]
POSE = (0.02, 0.01, -0.003)  # the pose of the single evaluation
HOT = 5 * 64 + 37            # lane 37 of wave 5 of block 0


def opose(T):
    return O.Pose(*T.pose.as_tuple())


def hostile_pairs(n, seed=None):
    """a: +-[1, 2) 2^((i mod 64) mod 40); b: a moved by a small pose, plus noise of 5 % of a's magnitude"""
    rng = np.random.default_rng(n if seed is None else seed)
    e = ((np.arange(n) % 64) % 40).astype(np.int64)[:, None]
    a = np.ldexp(1.0 + rng.random((n, 2)), e) * rng.choice([-1.0, 1.0], size=(n, 2))
    b = apply_pose(O.transform_new(np.array([0.4, -0.3, 0.02])), a) + np.ldexp(rng.normal(size=(n, 2)) * 0.05, e)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def swap_lane_bits(n, p, q):
    """the permutation of 0 .. n - 1 (n a multiple of 64) that swaps bits p and q of every lane index: folding the
    permuted pairs is folding the original ones with the tree's steps 2^p and 2^q in each other's place"""
    i = np.arange(n)
    bp, bq = (i >> p) & 1, (i >> q) & 1
    return i ^ ((bp ^ bq) << p) ^ ((bp ^ bq) << q)


@pytest.fixture(scope="module")
def cases():
    """per size: the pairs, and what the oracle makes of them in the device's tree (computed once, never changed)"""
    out = {}
    for n in SIZES:
        a, b = hostile_pairs(n)
        blocks, threads = I.reduce_geometry(n)
        rc, want, _ = O.weighted_gauss_newton_update_tree(opose(I.Transform(POSE)), a, b, blocks, threads)
        out[n] = dict(a=a, b=b, geometry=(blocks, threads), update=(rc, want), loop=oracle_loop(a, b))
        for v in (a, b, want):
            v.setflags(write=False)
    return out


def test_the_block_sums_of_these_pairs_depend_on_the_pairing_of_lanes():
    """the condition of this file's power, on the CPU: the oracle's block sums change when two steps of the wave tree
    trade places (every pair of neighbouring steps, and the two packed ones against a row step), and its totals change
    with the block size"""
    T = opose(I.Transform(POSE))
    for n in (512, 4096):
        a, b = hostile_pairs(n)
        blocks, threads = I.reduce_geometry(n)
        assert threads == 512 and blocks == n // 512
        base = O.wgn_tree_partials(T, a, b, blocks, threads)
        assert np.all(np.isfinite(base))
        touched = np.zeros(base.shape[1], dtype=bool)
        for p, q in ((5, 4), (4, 3), (3, 2), (2, 1), (1, 0), (5, 3), (4, 0)):
            perm = swap_lane_bits(n, p, q)
            other = O.wgn_tree_partials(T, np.ascontiguousarray(a[perm]), np.ascontiguousarray(b[perm]), blocks, threads)
            differ = other != base
            touched |= differ.any(axis=0)
            print(f"n {n}: steps {1 << p} and {1 << q} swapped: {int(differ.sum())} of {base.size} block sums differ")
            # (a sum that a few lanes of the largest magnitude dominate can round to the same bits either way: a fifth of
            # them moving is several sums per block, a wrong pairing cannot pass in all of them at every size)
            assert differ.sum() >= base.size // 5, (n, p, q, int(differ.sum()))
        if n == 4096:
            assert touched.all(), touched  # every one of the 19 sums is moved by some swap
        rc0, d0, e0 = O.weighted_gauss_newton_update_tree(T, a, b, blocks, 512)
        rc1, d1, e1 = O.weighted_gauss_newton_update_tree(T, a, b, 2 * blocks, 256)
        assert rc0 == O.OK and rc1 == O.OK
        assert not np.array_equal(d0, d1) or e0 != e1, n


@pytest.mark.parametrize("n", SIZES)
def test_one_evaluation_equals_the_tree_oracle(cases, n):
    c = cases[n]
    rc, want = c["update"]
    for _ in range(2):  # (the second evaluation finds the windows the first one left predicted)
        got = I.weighted_gauss_newton_update(I.Transform(POSE), c["a"], c["b"])
        if rc != O.OK:
            assert got is None
        else:
            assert got is not None and np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("n", SIZES)
def test_the_inner_loop_equals_the_tree_oracle(cases, n):
    import torch

    c = cases[n]
    oT, oapplied = c["loop"]
    icp = I.Icp3d(torch.zeros((1, 3), dtype=torch.float64, device="cuda"))
    try:
        d_a, d_b = torch.tensor(c["a"], device="cuda"), torch.tensor(c["b"], device="cuda")
        for _ in range(2):  # (cold windows, then predicted ones)
            l0 = I.gn_loop_counters(icp)
            T, applied = icp.estimate_transform_device(d_a, d_b)
            l1 = I.gn_loop_counters(icp)
            print("n", n, "applied", applied, "k_gn_loop launches, evaluations, hand-backs:", tuple(y - x for x, y in zip(l0, l1)))
            assert applied == oapplied
            assert np.array_equal(T.as_array(), oT.as_array()), (T.as_array(), oT.as_array())
    finally:
        icp.close()
    # and through the host arrays' entry (the scratch handle)
    T, applied = I.estimate_transform(c["a"], c["b"], return_inner_iters=True)
    assert applied == oapplied and np.array_equal(T.as_array(), oT.as_array())


@pytest.mark.parametrize("n", SIZES)
def test_two_iterations_of_icp_equal_the_oracle(cases, n):
    """the same coordinates as clouds: the targets are the pairs' b in another order, z a small offset of its own"""
    c = cases[n]
    rng = np.random.default_rng(7 * n + 1)
    src = np.ascontiguousarray(np.concatenate([c["a"], rng.normal(size=(n, 1))], axis=1))
    dst = np.ascontiguousarray(np.concatenate([c["b"], rng.normal(size=(n, 1))], axis=1)[rng.permutation(n)])
    icp = I.Icp3d(dst)
    try:
        T, idx, inner = icp.estimate(src, I.Transform(), 2, return_info=True)
        rc, oT, oidx, oinner = oracle_in_device_order(icp, 3, dst, src, O.transform_identity(), 2)
    finally:
        icp.close()
    assert rc == O.OK
    assert np.array_equal(idx, oidx)
    assert np.array_equal(inner, oinner), (inner, oinner)
    assert np.array_equal(T.as_array(), oT.as_array()), (T.as_array(), oT.as_array())


@pytest.mark.parametrize("n", [513, 4_097])
def test_a_nan_residual_in_an_upper_row_is_reported(cases, n):  # the reference panics, src/stats.rs:12
    a, b = cases[n]["a"], cases[n]["b"].copy()
    b[HOT, 1] = np.nan
    with pytest.raises(I.IcpError) as e:
        I.weighted_gauss_newton_update(I.Transform(POSE), a, b)
    assert e.value.status == _lib.NAN_INPUT
    with pytest.raises(I.IcpError) as e:
        I.estimate_transform(a, b)
    assert e.value.status == _lib.NAN_INPUT
    # and the next call is served normally
    rc, want = cases[n]["update"]
    assert rc == O.OK and np.array_equal(I.weighted_gauss_newton_update(I.Transform(POSE), a, cases[n]["b"]), want)


@pytest.mark.parametrize("n", [513, 4_097])
def test_an_infinite_residual_in_an_upper_row_gives_what_the_oracle_gives(cases, n):
    """an infinite residual has the Huber weight 0, and 0 times infinity is NaN: the sums it enters are NaN (the Huber
    error is +inf), in the oracle and on the device alike -- whatever the oracle makes of them (no update, or an update
    of NaNs) is what the device must make of them, and of the loop around them"""
    a, b = cases[n]["a"], cases[n]["b"].copy()
    b[HOT, 0] = np.inf
    T = I.Transform(POSE)
    blocks, threads = cases[n]["geometry"]
    rc, want, _ = O.weighted_gauss_newton_update_tree(opose(T), a, b, blocks, threads)
    assert rc in (O.OK, O.NONE)
    for _ in range(2):
        got = I.weighted_gauss_newton_update(T, a, b)
        if rc == O.NONE:
            assert got is None
        else:
            assert got is not None and np.array_equal(got, want, equal_nan=True), (got, want)
    oT, oapplied = oracle_loop(a, b)
    gT, applied = I.estimate_transform(a, b, return_inner_iters=True)
    assert applied == oapplied and np.array_equal(gT.as_array(), oT.as_array(), equal_nan=True)
