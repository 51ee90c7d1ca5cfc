"""An independent witness for one weighted Gauss-Newton update at a size past 2^23 pairs: the reference's definition
(src/lib.rs:218-261, src/stats.rs, src/huber.rs) restated in numpy with every sum and the solve in np.longdouble
(parity_util.reference_wgn_update_identity), not derived from the oracle.  This CPU test shows that both of the
oracle's summation orders -- the reference's left fold and the device's tree -- land within the error bound below of
it; tests/test_gpu_large.py holds the device to the same bound.

The bound.  The residuals and the four medians are exact in f64 (the identity pose makes the residual a - b; order
statistics do not depend on how they are found), so all that differs between the witness and a f64 evaluation is the
rounding of the sums and the solve.  A sum folded to a depth of D additions, of terms each rounded a few times (the
products w g J_p J_q, or w J_p J_q and the factor g applied to the folded total), is off by at most (D + 8) u times the
sum of its terms' magnitudes, u = 2^-53, to first order.  A relative perturbation eps of every term moves delta by at
most eps times the Skeel condition number of the solve (computed by the witness: about 3 on these pairs, where at the
identity pose J^T r does not cancel), so
    max |delta - delta_ref| <= cond * (D + 8) * u * max |delta_ref|.
D is n for the left fold (3e-9 at 9M pairs) and, for the tree of icp_reduce_geometry, the pairs one thread folds plus
the two stages' 64-lane butterflies, wave folds and rows (K + 30: 1.4e-14 at 9M).  Folding any block of 4 096 pairs
twice, or dropping it, moves delta by about 1e-4 of itself; one pair, by about 1e-7."""
import numpy as np

import icp_rust_amd as I
import oracle_ffi as O
from parity_util import gn_large_pairs, reference_wgn_update_identity

U = 2.0 ** -53


def fold_depth_tree(n):
    """additions on the longest path of the device's tree (oracle_ffi.weighted_gauss_newton_update_tree's comment)"""
    blocks, threads = I.reduce_geometry(n)
    per_thread = -(-n // (blocks * threads))
    rows = -(-blocks // threads)  # block sums one thread of the second stage folds
    return per_thread + 6 + (threads // 64 - 1) + rows + 6 + (threads // 64 - 1)


def rel_err(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)) / np.max(np.abs(want)))


def test_both_oracle_fold_orders_meet_the_bound_of_the_longdouble_update_at_9m_pairs():
    n = 9_000_000  # even: the medians are means of two order statistics
    a, b = gn_large_pairs(n, 3)
    want, sd, cond = reference_wgn_update_identity(a, b, skeel=True)
    assert 1.0 <= cond < 10.0, cond  # (the premise of the bound: J^T r does not cancel at the identity pose)
    T = O.transform_identity()
    rc, osd = O.calc_stddevs(a - b)
    assert rc == O.OK and np.array_equal(osd, sd)  # the medians: exact on both sides
    rc, left = O.weighted_gauss_newton_update(T, a, b)
    assert rc == O.OK
    blocks, threads = I.reduce_geometry(n)
    assert blocks == 2048 and n > 4096 * blocks  # the tree is capped: threads fold more than eight pairs
    rc, tree, _ = O.weighted_gauss_newton_update_tree(T, a, b, blocks, threads)
    assert rc == O.OK
    bound_left = cond * (n + 8) * U
    bound_tree = cond * (fold_depth_tree(n) + 8) * U
    assert bound_tree < 1e-13 and bound_left < 1e-8
    assert rel_err(left, want) <= bound_left, (rel_err(left, want), bound_left)
    assert rel_err(tree, want) <= bound_tree, (rel_err(tree, want), bound_tree)
    # ... and the witness sees a dropped pair (what the bound is for)
    drop = np.ones(n, dtype=bool)
    drop[4_500_001] = False
    rc, short = O.weighted_gauss_newton_update_tree(T, np.ascontiguousarray(a[drop]), np.ascontiguousarray(b[drop]),
                                                    blocks, threads)[:2]
    assert rc == O.OK and rel_err(short, want) > 100 * bound_tree
