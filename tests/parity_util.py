"""Helpers of the -m gpu parity tests (test infrastructure)."""
import numpy as np

import icp_rust_amd as I
import oracle_ffi as O


def oracle_in_device_order(icp, dim, dst, src, init, max_iter, use_kdtree=True):
    """The oracle's Icp::estimate with its sums folded exactly as the LAST estimate call on `icp` folded
    them: the tree of icp_reduce_geometry over the source points in that call's fold order
    (icp_last_fold_order; the identity unless the call took a cell-sorted snapshot).  The oracle folds over
    the order of the cloud it is handed, so it is handed src[perm]; its indices go back to the caller's order.
    `init`: an oracle pose.  Returns (rc, pose, idx, inner) like O.icp_estimate."""
    src = np.ascontiguousarray(src, dtype=np.float64)
    n = len(src)
    perm, cell = icp.last_fold_order(n, with_cells=True)
    check_fold_order(perm, cell)
    blocks, threads = I.reduce_geometry(n)
    rc, oT, oidx_s, oinner = O.icp_estimate(dim, dst, np.ascontiguousarray(src[perm]), init, max_iter,
                                            use_kdtree=use_kdtree, sum_mode=1, reduce_blocks=blocks,
                                            reduce_threads=threads)
    oidx = np.empty_like(oidx_s)
    oidx[perm] = oidx_s
    return rc, oT, oidx, oinner


def oracle_plane_in_device_order(icp, dst, normals, src, init, max_iter):
    """The CPU statement of the scalar-residual estimator (orc_p2pl_estimate) with its thirteen sums folded in the
    tree of icp_reduce_geometry(len(src)): the bits of Icp3d.estimate_point_to_plane and, on lifted clouds [x, y, 0]
    with normals [nx, ny, 0], of Icp2d.estimate_point_to_line.  Unlike `estimate`, these calls fold in the CALLER's
    order: the pairs are gathered from d_src and idx as given (k_p2pl_gather / k_line_gather write pair i from source
    point i, and k_p2pl_accumulate's thread g folds pairs g, g + G, ...), so no permutation is taken from `icp` -- it
    is accepted only so that the call reads like oracle_in_device_order.  `dst`: the targets (m x 3) or an O.KdTree
    of them; `init`: an oracle pose or a Transform.  Returns (rc, pose, idx, inner) like O.p2pl_estimate."""
    src = np.ascontiguousarray(src, dtype=np.float64)
    tree = dst if isinstance(dst, O.KdTree) else O.KdTree(dst)
    init = O.Pose(*init.pose.as_tuple()) if hasattr(init, "pose") else init
    blocks, threads = I.reduce_geometry(len(src))
    return O.p2pl_estimate(tree, normals, src, init, max_iter, sum_mode=1, reduce_blocks=blocks,
                           reduce_threads=threads)


def check_fold_order(perm, cell):
    """a permutation, ascending by (sort key, original index): the stable order the header documents"""
    n = len(perm)
    assert np.array_equal(np.sort(perm), np.arange(n))
    if n > 1:
        c = cell.astype(np.int64)
        assert np.all(np.diff(c) >= 0)
        same = np.diff(c) == 0
        assert np.all(np.diff(perm)[same] > 0)


def apply_pose(T, pts):
    """Transform::transform (src/transform.rs:22-24) of many points at once, as the oracle does it for one:
    (r00 x + r01 y) + tx, with no fused multiply-add (numpy evaluates each product and sum on its own).  `T`: an
    oracle pose or a Transform."""
    p = getattr(T, "pose", T)
    x, y = pts[:, 0], pts[:, 1]
    return np.stack([(p.r00 * x + p.r01 * y) + p.tx, (p.r10 * x + p.r11 * y) + p.ty], axis=1)


def oracle_loop(a, b):
    """estimate_transform (src/lib.rs:59-84) with every sum folded in the tree of icp_reduce_geometry: the device's
    bits.  Returns (oracle pose, updates applied)."""
    blocks, threads = I.reduce_geometry(len(a))
    T = O.transform_identity()
    prev, applied = np.finfo(np.float64).max, 0
    if len(a) >= 2:
        for _ in range(200):
            rc, delta, err = O.weighted_gauss_newton_update_tree(T, a, b, blocks, threads)
            if rc != O.OK:
                break
            if (delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2] < 1e-6:
                break
            if err > prev:
                break
            prev = err
            T = O.transform_mul(O.transform_new(delta), T)
            applied += 1
    return T, applied


def gn_large_pairs(n, seed, heavy=False):
    """Pairs shaped like bench.py's gn_large line, drawn on the host: a uniform in [-40, 40)^2, b = a rotated by
    0.015 rad and moved by (0.3, -0.2), plus N(0, 0.05^2) noise.  `heavy`: 10 % of b are outliers thrown
    N(0, 5^2) around an offset of (4, -2.5), which also pulls the residuals' medians away from zero."""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, 2)) - 0.5) * 80.0
    c, s = np.cos(0.015), np.sin(0.015)
    b = np.empty_like(a)
    b[:, 0] = c * a[:, 0] - s * a[:, 1] + 0.3
    b[:, 1] = s * a[:, 0] + c * a[:, 1] - 0.2
    b += rng.normal(size=(n, 2)) * 0.05
    if heavy:
        k = rng.choice(n, size=n // 10, replace=False)
        b[k] += rng.normal(size=(len(k), 2)) * 5.0 + np.array([4.0, -2.5])
    return a, b


PPF34 = 1.482602218505602  # 1 / PPF(0.75), src/stats.rs:41
HUBER_K = 1.345            # src/lib.rs:32


def _median_f64(v):
    """stats::mutable_median (src/stats.rs:11-28): the middle order statistic, or the mean (b + c) / 2 of the two
    middle ones, rounded once in f64.  Order statistics are exact, whichever algorithm finds them."""
    n = len(v)
    if n % 2 == 1:
        return np.partition(v, n // 2)[n // 2]
    p = np.partition(v, (n // 2 - 1, n // 2))
    return (p[n // 2 - 1] + p[n // 2]) / 2.0


def reference_stddevs(a, b):
    """The residuals (r00 x + r01 y) + tx - d at the IDENTITY pose (= a - b exactly) and stats::calc_stddevs
    (src/stats.rs:30-60) of them: PPF34 * median(|r - median(r)|) per dimension, all in f64 as the reference
    rounds it.  Returns (residuals, stddevs)."""
    r = a - b
    sd = np.empty(2)
    for j in range(2):
        col = np.ascontiguousarray(r[:, j])
        m = _median_f64(col)
        sd[j] = PPF34 * _median_f64(np.abs(col - m))
    return r, sd


def reference_wgn_update_identity(a, b, skeel=False):
    """weighted_gauss_newton_update (src/lib.rs:218-261) at the identity pose, written from the reference's
    definition: the residuals and the four medians exactly in f64 (reference_stddevs), then the Huber weights
    (src/huber.rs: drho(e, k) = 1 for e <= k^2, else k / sqrt(e)), the sums of w g J^T J and w g J^T r and the
    3 x 3 solve -H^-1 g in np.longdouble.  At the identity J_x = (1, 0, -y), J_y = (0, 1, x).
    Returns (delta as longdouble[3], stddevs as f64[2]); with `skeel`, also the Skeel condition number
    || |H^-1| (|H|_abs |delta| + |g|_abs) ||_inf / ||delta||_inf of the solve, where |.|_abs are the sums of the
    terms' magnitudes: a relative perturbation eps of every term moves delta by at most eps times it."""
    L = np.longdouble
    r, sd = reference_stddevs(a, b)
    ax, ay = a[:, 0].astype(L), a[:, 1].astype(L)
    H = np.zeros((3, 3), dtype=L)
    g = np.zeros(3, dtype=L)
    Habs = np.zeros((3, 3), dtype=L)
    gabs = np.zeros(3, dtype=L)
    k = L(HUBER_K)
    for j in range(2):
        if sd[j] == 0.0:
            continue
        rj = r[:, j].astype(L)
        e = rj * rj
        w = np.where(e <= k * k, L(1), k / np.sqrt(np.maximum(e, k * k)))
        wg = w / L(sd[j])
        J = (L(1), L(0), -ay) if j == 0 else (L(0), L(1), ax)
        for p in range(3):
            wJp = wg * J[p]
            g[p] += np.sum(wJp * rj)
            if skeel:
                gabs[p] += np.sum(np.abs(wJp * rj))
            for q in range(p, 3):
                H[p, q] += np.sum(wJp * J[q])
                H[q, p] = H[p, q]
                if skeel:
                    Habs[p, q] += np.sum(np.abs(wJp * J[q]))
                    Habs[q, p] = Habs[p, q]
    delta = -_solve3_longdouble(H, g)
    if not skeel:
        return delta, sd
    Hinv = np.stack([_solve3_longdouble(H, e) for e in np.eye(3, dtype=L)], axis=1)
    cond = np.max(np.abs(Hinv) @ (Habs @ np.abs(delta) + gabs)) / np.max(np.abs(delta))
    return delta, sd, float(cond)


def _solve3_longdouble(H, g):
    """H^-1 g by the adjugate (numpy's solvers do not take longdouble)"""
    c = np.empty((3, 3), dtype=H.dtype)
    for i in range(3):
        for j in range(3):
            m = np.delete(np.delete(H, i, 0), j, 1)
            c[i, j] = (-1) ** (i + j) * (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])
    det = np.sum(H[0] * c[0])
    return (c.T @ g) / det


def plane_residuals_identity(st, idx, dst, normals):
    """n_q . (p - q) of the pairs (st[i], dst[idx[i]]) at the identity inner pose, in f64 with every operation
    rounded on its own and in the kernel's order: (nx ex + ny ey) + nz ez."""
    q, nq = dst[idx], normals[idx]
    return (nq[:, 0] * (st[:, 0] - q[:, 0]) + nq[:, 1] * (st[:, 1] - q[:, 1])) + nq[:, 2] * (st[:, 2] - q[:, 2])


def reference_plane_update(st, idx, dst, normals, skeel=False):
    """One update of the scalar-residual estimator at the identity inner pose, written from the definition at the
    top of icp_rust_amd/csrc/p2plane.hip (not from the oracle): residual r = n_q . (p - q), sigma = 1.4826 MAD(r),
    g = 1 / sigma, w = drho(r^2, 1.345), Jacobian row J = n_xy^T [I | (-p_y, p_x)^T] = (nx, ny, ny p_x - nx p_y),
    delta = -(sum w g J^T J)^-1 (sum w g J^T r), Huber error = sum rho(r^2).
    The residuals are taken in f64 (plane_residuals_identity) and sigma from their exact order statistics, both shared
    with the code under test; the weights, the twelve sums, the error and the adjugate solve are in np.longdouble.
    Returns (delta as longdouble[3], sigma, Huber error as longdouble); with `skeel`, also the Skeel condition number
    || |H^-1| (|H|_abs |delta| + |g|_abs) ||_inf / ||delta||_inf, where |.|_abs sum the terms' magnitudes with
    |J_2| taken as |ny p_x| + |nx p_y| (what the rounding of J_2's two products and their sum is relative to): a
    relative perturbation eps of every term's factors moves delta by at most eps times it.  sigma == 0: delta None."""
    L = np.longdouble
    st, dst, normals = (np.asarray(x, dtype=np.float64) for x in (st, dst, normals))
    idx = np.asarray(idx, dtype=np.int64)
    r = plane_residuals_identity(st, idx, dst, normals)
    col = np.ascontiguousarray(r)
    sigma = PPF34 * _median_f64(np.abs(col - _median_f64(col)))
    k = L(HUBER_K)
    rl = r.astype(L)
    e = rl * rl
    big = e > k * k
    root = np.sqrt(np.maximum(e, k * k))
    err = np.sum(np.where(big, 2 * k * root - k * k, e))
    if sigma == 0.0:
        return (None, sigma, err, None) if skeel else (None, sigma, err)
    wg = np.where(big, k / root, L(1)) / L(sigma)
    nq = normals[idx].astype(L)
    px, py = st[:, 0].astype(L), st[:, 1].astype(L)
    J = (nq[:, 0], nq[:, 1], nq[:, 1] * px - nq[:, 0] * py)
    Jabs = (np.abs(nq[:, 0]), np.abs(nq[:, 1]), np.abs(nq[:, 1] * px) + np.abs(nq[:, 0] * py))
    H, Habs = np.zeros((3, 3), dtype=L), np.zeros((3, 3), dtype=L)
    g, gabs = np.zeros(3, dtype=L), np.zeros(3, dtype=L)
    for p in range(3):
        g[p] = np.sum(wg * J[p] * rl)
        gabs[p] = np.sum(wg * Jabs[p] * np.abs(rl))
        for q in range(p, 3):
            H[p, q] = H[q, p] = np.sum(wg * J[p] * J[q])
            Habs[p, q] = Habs[q, p] = np.sum(wg * Jabs[p] * Jabs[q])
    delta = -_solve3_longdouble(H, g)
    if not skeel:
        return delta, sigma, err
    Hinv = np.stack([_solve3_longdouble(H, c) for c in np.eye(3, dtype=L)], axis=1)
    cond = np.max(np.abs(Hinv) @ (Habs @ np.abs(delta) + gabs)) / np.max(np.abs(delta))
    return delta, sigma, err, float(cond)
