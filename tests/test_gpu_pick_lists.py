"""The finishing launch of a window evaluation (gn_win.hip: k_win_pick / k_win_pick2) takes its candidates out of the
segments the first launch filed them in: every lister thread loads its own members, a scan of the listers' counts
places them in the dense lists the exact selections rank.  These cases shape the LISTS -- few segments, a ragged last
block, one pair per thread, one lister that holds every candidate, dimensions of very different counts, a median bin
beyond its cap, signed zeros on the median -- and hold the results to the oracle bit for bit.

Each constructed case is checked twice on the same pairs:
  * `estimate_transform_device` on a fresh handle against the oracle's estimate_transform with its sums folded in the
    device's tree (parity_util.oracle_loop): pose and applied updates, after a warm-up call that leaves the windows
    predicted;
  * ONE evaluation at the identity through the stage pipeline (`weighted_gauss_newton_update`, the launches
    k_win_hist_sums_bkt -> k_win_pick) against the oracle's tree evaluation, after a warm-up evaluation; the filed
    counter proves that k_win_pick finished it.  (A whole estimate_transform of up to 2^20 pairs runs its inner loop
    in one launch, gn_loop.hip, which keeps its own lists; the stage call is what reaches the finishing launch.)
Unless a case is built to overflow, the path counters must show the window pipeline serving the checked work: windows
started, none missed, no other pipeline.  The populations the constructions rely on are checked with numpy first.

Seeds: every generator below is seeded with the case's n (stated at each case); with them the build in front of this
file's first version serves every non-overflow case from its windows on an MI355X."""
import numpy as np
import pytest
import torch

import icp_rust_amd as I
import oracle_ffi as O
from parity_util import PPF34, oracle_in_device_order, oracle_loop

pytestmark = pytest.mark.gpu

THREADS = 512           # threads of a block of the reduction tree (icp_reduce_geometry)
F_WINDOW = 0.2          # half-width of a fine window in sigmas for clouds of up to 2^17 pairs (window_half_width)
FINE_BINS = 512         # bins of a fine window
CAP_MED = 1024          # median candidates the window pipeline keeps per dimension (kWinCapMed)


def delta(before, after):
    return tuple(y - x for x, y in zip(before, after))


def stats(v):
    """median, MAD and the width of a fine bin of the window predicted from them"""
    med = np.median(v)
    mad = np.median(np.abs(v - med))
    return med, mad, 2.0 * F_WINDOW * PPF34 * mad / FINE_BINS


def noisy_pairs(n, seed, sigma=0.1):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 2)) * 10
    r = rng.normal(size=(n, 2)) * sigma
    return a, r


def run_case(a, b, warm=None):
    """the two checks of the module's docstring; returns the counter deltas (estimate, stage) of the checked work.
    warm: other pairs (a, b) of the same size to predict the windows from -- the case is then one built to MISS, and
    the asserts on the counters are its own."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    overflow = warm is not None
    wa, wb = (np.ascontiguousarray(x) for x in warm) if overflow else (a, b)
    n = len(a)
    oT, oapplied = oracle_loop(a, b)
    icp = I.Icp3d(torch.zeros((1, 3), dtype=torch.float64, device="cuda"))
    try:
        d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        d_wa, d_wb = (d_a, d_b) if not overflow else (torch.from_numpy(wa).cuda(), torch.from_numpy(wb).cuda())
        icp.estimate_transform_device(d_wa, d_wb)  # warm-up: the windows of every evaluation kind are predicted
        c0 = I.gn_path_counters(icp)
        T, applied = icp.estimate_transform_device(d_a, d_b)
        est = delta(c0, I.gn_path_counters(icp))
    finally:
        icp.close()
    print("estimate_transform_device: window started, missed, short, radix =", est[:4], "applied", applied)
    assert applied == oapplied
    assert np.array_equal(T.as_array(), oT.as_array()), (T.as_array(), oT.as_array())
    # one evaluation through the stage pipeline
    Tid = I.Transform()
    blocks, threads = I.reduce_geometry(n)
    assert threads == THREADS
    rc, want, _ = O.weighted_gauss_newton_update_tree(O.transform_identity(), a, b, blocks, threads)
    assert rc == O.OK
    for _ in range(2):  # warm-up: the prediction, and narrow windows again if an earlier test left wide ones
        assert I.weighted_gauss_newton_update(Tid, wa, wb) is not None
    c0, f0 = I.gn_path_counters(), I.gn_filed_counters()
    got = I.weighted_gauss_newton_update(Tid, a, b)
    stage, filed = delta(c0, I.gn_path_counters()), delta(f0, I.gn_filed_counters())
    print("stage evaluation: window started, missed, short, radix =", stage[:4], "filed, second pass =", filed)
    assert got is not None and np.array_equal(got, want), (got, want)
    if not overflow:
        assert est[0] >= 1 and est[1] == 0 and est[2] == 0 and est[3] == 0, est
        assert stage[:4] == (1, 0, 0, 0), stage
        assert filed == (1, 0), filed  # finished by k_win_pick
    return est, stage


# n = 4096: eight tree blocks -- 248 of the 256 lister threads of each part have no segment; a fine bin holds one or two
# n = 4097, 5000: a ragged last block (one pair / 392 pairs in it)
# n = 131072: 256 blocks, one pair per thread, every lister busy
@pytest.mark.parametrize("n", [4096, 4097, 5000, 131072])
def test_lists_over_few_ragged_and_full_segments(n):
    a, r = noisy_pairs(n, n)  # seed: n
    blocks, _ = I.reduce_geometry(n)
    assert blocks == (n + THREADS - 1) // THREADS
    run_case(a, a - r)


def test_one_lister_holds_every_candidate():
    """n = 65536 (128 blocks, one pair per thread: block b folds the pairs [512 b, 512 b + 512)): every x residual
    within 4 fine bins of the median and within 5 of median -+ MAD lies in block 3, every such y residual in block 77.
    The candidates -- the median's bin, the ring's few bins on either side -- are therefore all ONE lister's, far more
    than it loads unrolled, and the other 255 listers of each part are empty."""
    n = 65536
    rng = np.random.default_rng(n)  # seed: n
    a = rng.normal(size=(n, 2)) * 10
    r = np.empty((n, 2))
    for d, blk in ((0, 3), (1, 77)):
        v = rng.normal(size=n) * 0.1
        med, mad, fine = stats(v)
        dist = np.abs(v - med)
        near = (dist <= 4 * fine) | (np.abs(dist - mad) <= 5 * fine)
        k = int(near.sum())
        assert 150 <= k <= THREADS, k  # the block holds them all; a lister of a hundred and more
        home = np.zeros(n, dtype=bool)
        home[blk * THREADS:blk * THREADS + k] = True
        r[home, d] = v[near]
        r[~home, d] = v[~near]
    b = a - r
    for d, blk in ((0, 3), (1, 77)):  # the populations as the device sees them (a - b, rounded)
        v = a[:, d] - b[:, d]
        med, mad, fine = stats(v)
        dist = np.abs(v - med)
        cand = np.flatnonzero((dist <= 2 * fine) | (np.abs(dist - mad) <= 3 * fine))
        assert len(cand) > 60 and np.all(cand // THREADS == blk), (len(cand), np.unique(cand // THREADS))
    run_case(a, b)


def test_dimensions_of_very_different_counts():
    """x: 400 distinct residuals inside a hundredth of the median's fine bin (hundreds of median candidates, below the
    cap); y: the middle element alone in a gap of four fine bins (one median candidate).  n odd: one middle rank."""
    n = 40_001
    a, r = noisy_pairs(n, n)  # seed: n
    for d in (0, 1):
        r[:, d] -= np.median(r[:, d])
    _, _, fine_x = stats(r[:, 0])
    order = np.argsort(np.abs(r[:, 0]))
    r[order[:400], 0] = (np.arange(400) - 199.5) * (0.01 * fine_x / 400)
    _, _, fine_y = stats(r[:, 1])
    order = np.argsort(np.abs(r[:, 1]))
    mid, rest = order[0], order[1:]
    r[mid, 1] = 0.0
    close = rest[np.abs(r[rest, 1]) < 2 * fine_y]
    r[close, 1] += np.where(r[close, 1] < 0, -2 * fine_y, 2 * fine_y)
    b = a - r
    vx, vy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    medx, _, fx = stats(vx)
    medy, _, fy = stats(vy)
    in_x = int(np.sum(np.abs(vx - medx) <= 0.02 * fx))
    assert 400 <= in_x < CAP_MED, in_x
    assert int(np.sum(np.abs(vy - medy) <= 1.5 * fy)) == 1
    run_case(a, b)


def test_duplicates_beyond_the_median_cap_fall_back_with_the_same_bits():
    """30 % of the x residuals are one value on the median: more candidates in the median's bin than the lists keep.
    The windows are predicted from a clean distribution of the same scale; the window pipeline must report a miss,
    and whatever serves the evaluation instead returns the oracle's bits."""
    n = 60_001
    a, r = noisy_pairs(n, n, sigma=0.2)  # seed: n
    clean = (a, a - r)
    r = r.copy()
    k = int(0.3 * n)
    h = (n - k) // 2
    r[:k, 0] = 0.0
    r[k:k + h, 0] = -np.abs(r[k:k + h, 0]) - 1e-3
    r[k + h:, 0] = np.abs(r[k + h:, 0]) + 1e-3
    assert k > CAP_MED and np.median(r[:, 0]) == 0.0
    est, stage = run_case(a, a - r, warm=clean)
    # the stage evaluation's window was tried and missed (tests/test_gpu_window.py holds the same sequence to the same
    # counts); how the whole estimate_transform gets past its miss is the inner loop's business: its bits are checked
    assert stage[0] == 1 and stage[1] == 1, stage
    # and the pipelines are back in their rest state afterwards
    a2, r2 = noisy_pairs(n, 3)
    run_case(a2, a2 - r2)


@pytest.mark.parametrize("n", [65_536, 65_537])
def test_signed_zeros_on_the_median(n):
    """a run of +0 / -0 sits exactly on the median of y, the rest splits evenly around it: middle_of at the edges"""
    a, r = noisy_pairs(n, n)  # seed: n
    z = 301
    h = (n - z) // 2
    r[:z, 1] = np.where(np.arange(z) % 2 == 0, 0.0, -0.0)
    r[z:z + h, 1] = -np.abs(r[z:z + h, 1]) - 1e-6
    r[z + h:, 1] = np.abs(r[z + h:, 1]) + 1e-6
    b = a.copy()
    b[:, 0] = a[:, 0] - r[:, 0]
    b[:, 1] = np.where(r[:, 1] == 0.0, a[:, 1], a[:, 1] - r[:, 1])  # (a - (+-0) == a: the residual is an exact zero there)
    v = a[:, 1] - b[:, 1]
    assert np.median(v) == 0.0 and int(np.sum(v == 0.0)) == z
    run_case(a, b)


def test_paired_finish_serves_both_evaluations_of_an_outer_iteration():
    """Icp3d.estimate, default two streams, on a synthetic pair above the cooperative search's size: once an inner loop
    has applied exactly one update the host bets on the next pose, and ONE launch of four workgroups (k_win_pick2)
    finishes the deciding evaluation and the next iteration's first.  Six iterations against the same-order oracle."""
    from icp_rust_amd import synth
    n = m = 70_000
    src, dst = synth.synthetic_pair(n, m)
    icp = I.Icp3d(dst)
    try:
        icp.estimate(src, I.Transform(), 6)  # warm-up: predictions, and how the inner loops of this pair end
        c0, f0 = I.gn_path_counters(icp), I.gn_filed_counters(icp)
        T, idx, inner = icp.estimate(src, I.Transform(), 6, return_info=True)
        path, filed = delta(c0, I.gn_path_counters(icp)), delta(f0, I.gn_filed_counters(icp))
        print("estimate: window started, missed, short, radix, bets won, lost =", path, "filed, second pass =", filed)
        rc, oT, oidx, oinner = oracle_in_device_order(icp, 3, dst, src, O.transform_identity(), 6)
    finally:
        icp.close()
    assert rc == O.OK
    assert np.array_equal(idx, oidx)
    assert np.array_equal(inner, oinner)
    assert np.array_equal(T.as_array(), oT.as_array())
    assert path[0] >= 6 and path[1] == 0 and path[2] == 0 and path[3] == 0, path
    assert path[4] >= 1, path  # a bet was won: its evaluations were finished in pairs
    assert filed[0] >= 2 and filed[1] == 0, filed
