"""The finishing launch of a filed-candidate evaluation runs one workgroup per dimension (gn_win.hip: k_win_pick,
k_win_pick2): each resolves, lists and selects its own dimension and folds half of the block sums; the one that draws
the second ticket of the pair combines both and releases the result.  These cases aim at what that split can break:
a miss in one dimension only, odd and even counts, ties, NaN input, the ticket reused call after call, the two
contexts of a handle and two handles side by side.  Every result is compared bit for bit with the oracle evaluated
in the device's reduction order, and icp_gn_filed_counters proves that the finishing launches in question ran (a handle
whose files were not usable takes the second pass for a while: `settle` waits that out first)."""
import os

import numpy as np
import pytest

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import synth
from parity_util import oracle_in_device_order

pytestmark = pytest.mark.gpu


def opose(T):
    return O.Pose(*[float(x) for x in T.as_array()])


def pairs(n, seed, shift=(0.0, 0.0), spread=0.05):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 2)) * 20
    Tt = O.transform_new(np.array([0.4, -0.3, 0.02]))
    b = O.transform_apply_many(Tt, a) + rng.normal(size=(n, 2)) * spread + np.asarray(shift)
    k = rng.integers(0, n, size=n // 10)
    b[k] += rng.normal(size=(len(k), 2)) * 5
    return a, b


def check(T, a, b):
    got = I.weighted_gauss_newton_update(T, a, b)
    blocks, threads = I.reduce_geometry(len(a))
    rc, want, _ = O.weighted_gauss_newton_update_tree(opose(T), a, b, blocks, threads)
    assert rc == O.OK and got is not None
    assert np.array_equal(got, want), (got, want)


def delta(before, after):
    return tuple(y - x for x, y in zip(before, after))


def filed(icp=None):
    return I.gn_filed_counters(icp)[0]


def settle():
    """run small window evaluations on the scratch handle until it files candidates again"""
    a, b = pairs(8_192, 99)
    for _ in range(80):
        if I.gn_filed_counters()[1] == 0:
            return
        check(T0, a, b)
    assert I.gn_filed_counters()[1] == 0


def check_estimate(icp, dim, dst, src, iters):
    T, idx, inner = icp.estimate(src, I.Transform(), iters, return_info=True)
    rc, oT, oidx, oinner = oracle_in_device_order(icp, dim, dst, src, O.transform_identity(), iters)
    assert rc == O.OK
    assert np.array_equal(idx, oidx)
    assert np.array_equal(inner, oinner)
    assert np.array_equal(T.as_array(), oT.as_array())


T0 = I.Transform([0.39, -0.31, 0.0199])


@pytest.mark.parametrize("dim", [0, 1])
def test_a_window_miss_in_one_dimension_only(dim):
    n = 200_000
    settle()
    a, b = pairs(n, 21 + dim)
    check(T0, a, b)  # the prediction
    check(T0, a, b)
    shift = [0.0, 0.0]
    shift[dim] = 1.5  # ~30 sigma: every order statistic of this dimension leaves its window, the other's stay
    a2, b2 = pairs(n, 21 + dim, shift=tuple(shift))
    c0, f0 = I.gn_path_counters(), filed()
    check(T0, a2, b2)
    tried, missed, _, radix, _, _ = delta(c0, I.gn_path_counters())
    assert tried == 1 and missed == 1 and radix == 0
    assert filed() - f0 == 1  # the split finish found the miss
    # and the next evaluations hit again
    c1 = I.gn_path_counters()
    for k in range(3):
        check(I.Transform([0.3901 + 1e-4 * k, -0.31, 0.0199]), a2, b2)
    tried, missed, _, _, _, _ = delta(c1, I.gn_path_counters())
    assert tried == 3 and missed == 0


@pytest.mark.parametrize("n", [4_096, 4_097, 65_536, 65_537, 262_143, 262_144, (1 << 20) - 1, 1 << 20])
def test_odd_and_even_counts(n):
    settle()
    a, b = pairs(n, n)
    check(T0, a, b)
    check(T0, a, b)
    c0, f0 = I.gn_path_counters(), filed()
    for k in range(3):
        check(I.Transform([0.39 + 1e-4 * k, -0.31, 0.0199 + 1e-6 * k]), a, b)
    tried, missed, _, _, _, _ = delta(c0, I.gn_path_counters())
    assert tried == 3 and missed == 0
    assert filed() - f0 >= 1


@pytest.mark.parametrize("dim", [0, 1])
def test_duplicate_residuals_in_one_dimension(dim):
    """A few hundred residuals of one exact value next to the median (ties inside one dimension's candidate list, which
    still fits), then a third of them on one value (the list overflows: a miss)."""
    n = 200_001
    rng = np.random.default_rng(7 + dim)
    a = rng.normal(size=(n, 2)) * 10
    r = rng.normal(size=(n, 2)) * 0.2
    settle()
    check(I.Transform(), a, a - r)
    check(I.Transform(), a, a - r)
    r2 = r.copy()
    r2[:400, dim] = np.median(r[:, dim]) + 1e-9
    f0 = filed()
    check(I.Transform(), a, a - r2)
    check(I.Transform(), a, a - r2)
    assert filed() - f0 >= 1  # ties inside one dimension's list, selected by the split finish
    k = n // 3
    r3 = r.copy()
    r3[:k, dim] = 0.0
    c0 = I.gn_path_counters()
    check(I.Transform(), a, a - r3)
    tried, missed, _, _, _, _ = delta(c0, I.gn_path_counters())
    assert tried == 1 and missed == 1
    check(T0, *pairs(n, 5))
    check(T0, *pairs(n, 5))


def test_nan_input_is_reported_and_the_next_calls_are_clean():
    n = 100_000
    settle()
    a, b = pairs(n, 31)
    check(T0, a, b)
    check(T0, a, b)
    bad = b.copy()
    bad[1234, 1] = np.nan
    with pytest.raises(I.IcpError):
        I.weighted_gauss_newton_update(T0, a, bad)
    f0 = filed()
    for k in range(3):
        check(I.Transform([0.39 + 1e-4 * k, -0.31, 0.0199]), a, b)
    assert filed() - f0 == 3


def test_many_consecutive_calls_on_one_handle():
    n = 150_000
    settle()
    a, b = pairs(n, 41)
    check(T0, a, b)
    c0, f0 = I.gn_path_counters(), filed()
    for k in range(40):
        check(I.Transform([0.39 + 2e-5 * k, -0.31 - 1e-5 * k, 0.0199]), a, b)
    tried, missed, _, _, _, _ = delta(c0, I.gn_path_counters())
    assert tried == 40 and missed == 0
    assert filed() - f0 == 40  # forty tickets of the pair drawn on one context


def test_two_handles_alternating():
    """Each estimate runs the paired finish (both contexts of the handle, k_win_pick2) and the single one."""
    src1, dst1 = synth.synthetic_pair(120_000, 100_000, seed=synth.SEED + 11)
    src2, dst2 = synth.synthetic_pair(90_000, 110_000, seed=synth.SEED + 12)
    h1, h2 = I.Icp3d(dst1), I.Icp3d(dst2)
    try:
        for _ in range(3):
            check_estimate(h1, 3, dst1, src1, 6)
            check_estimate(h2, 3, dst2, src2, 6)
        assert filed(h1) > 0 and filed(h2) > 0
    finally:
        h1.close()
        h2.close()


def test_the_frame_and_the_2d_golden_pair():
    pk = synth.synthetic_scan3d_packets(150)
    s3, d3 = synth.remove_invalid_values(pk[:75]), synth.remove_invalid_values(pk[75:150])
    icp3 = I.Icp3d(d3)
    try:
        for _ in range(2):
            check_estimate(icp3, 3, d3, s3, 20)
        assert filed(icp3) > 0
    finally:
        icp3.close()
    from icp_rust_amd.scans import load_scan2d
    g = os.path.join(os.path.dirname(__file__), "golden", "scans2d")
    s2, d2 = load_scan2d(os.path.join(g, "001.txt")), load_scan2d(os.path.join(g, "002.txt"))
    icp2 = I.Icp2d(d2)
    try:
        check_estimate(icp2, 2, d2, s2, 20)
    finally:
        icp2.close()
