"""Every 1-NN engine against exact_nn on the clouds of tests/blind_clouds.py, where the gap between the best and the
second-best target is below what the engines' f32 screens resolve (tests/test_blind_clouds.py shows that it is, and that
a screen without its margin goes wrong there): a dropped margin, a margin applied to the wrong length, an FMA or an
approximate square root that shifts a bound by an ulp changes an index here, and nowhere else in the suite.  All indices
must be equal; the unique queries are repeated (np.tile) up to the size at which an engine takes the kernel a case
names, to a total that is no multiple of 64.  Each case states the dispatch condition it relies on and asserts what
the library lets a test observe of it."""
import numpy as np
import pytest

import blind_clouds as B
import icp_rust_amd as I
from parity_util import apply_pose

pytestmark = pytest.mark.gpu

N_SHARED = 66_003  # > 65 536 = kGridCoopMaxN (common.hpp:494): one lane per query, the seeded and the warm walk
EXACT_T = (2.0 ** -3, -(2.0 ** -4))  # a translation under which every coordinate stays exact: ties survive
T0 = (0.02, -0.015, 0.004)


def _handle(dst, mode):
    icp = (I.Icp3d if dst.shape[1] == 3 else I.Icp2d)(dst, nn_mode=mode)
    # api.hip:531-535 (resolved_nn_mode): a forced mode is the engine, AUTO picks by m >= 8192
    assert I.lib().icp_get_nn_mode(icp._h) == mode
    return icp


def _translation(t):
    return I.Transform.from_rt(np.eye(2), np.asarray(t, dtype=np.float64))


def _moved(T, src):
    q = src.copy()
    q[:, :2] = apply_pose(T, src)  # Transform::transform as the contract states it, in numpy
    return q


class _Device:
    """the queries on the device and the three outputs of a search"""

    def __init__(self, q):
        import torch

        self.n = len(q)
        self.q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        self.idx = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.a = torch.empty((self.n, 2), dtype=torch.float64, device="cuda")
        self.b = torch.empty_like(self.a)

    def search(self, icp, T=None):
        """nn_search (no pose) or correspond_device (pose): (idx, a, b) on the host"""
        self.idx.fill_(-1)
        if T is None:
            icp.nn_search_device(self.q, self.idx)
            icp.synchronize()
            return self.idx.cpu().numpy().view(np.uint32), None, None
        icp.correspond_device(self.q, T, self.a, self.b, self.idx)
        icp.synchronize()
        return self.idx.cpu().numpy().view(np.uint32), self.a.cpu().numpy(), self.b.cpu().numpy()


def _equal(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:10]], want[bad[:10]])


def _under_the_exact_translation(c, q):
    """(source points, pose) with pose(source) == q bit for bit: the searches with a pose see the cloud's own queries"""
    src = q.copy()
    src[:, :2] -= EXACT_T
    T = _translation(EXACT_T)
    assert np.array_equal(_moved(T, src), q)
    return src, T


# ------------------------------------------------------------------------------------------------ the sweep --


def _sweep_plan(n, m):
    """(queries per lane, whether every chunk is whole tiles) as launch_nn_brute picks them (nn_brute.hip:666-684)"""
    r = 8 if n >= 900_000 else 4 if n >= 2 * 256 * 1024 else 2 if n >= 256 * 1024 else 1
    qblocks, granules = -(-n // (256 * r)), -(-m // 64)
    chunks = -(-2048 // qblocks) if qblocks < 2048 else 1
    chunks = max(1, min(chunks, granules, 64))
    per = -(-granules // chunks)
    if per >= 16:
        per = -(-per // 16) * 16
    return r, (per * 64) % 1024 == 0


# n < 262 144: R = 1, which only k_nn_brute_scr serves (nn_brute.hip:607: the dot-product screen needs R >= 2); from
# 262 144 / 524 288 / 900 000 on R = 2 / 4 / 8 (nn_brute.hip:666-669) and k_nn_brute_dot, the half diagonal of the box
# being far below 1e15 (nn_brute.hip:608).  The screen exists because the grid's box does (nn_brute.hip:565, 599).
@pytest.mark.parametrize("n,r", [(50_003, 1), (262_147, 2), (524_291, 4), (900_003, 8)])
@pytest.mark.parametrize("variant", ["plain", "offset"])
@pytest.mark.parametrize("dim", [2, 3])
def test_sweep_with_the_screen_in_front_equals_exact_nn(dim, variant, n, r):
    """FULL (chunks of whole tiles, nn_brute.hip:597) with the bulk padded to m = 16 384; not FULL with m = 3722 at
    every size, and with m = 7922 as built under one query per lane (at 2 / 4 / 8 per lane its 124 granules make
    chunks of 32: whole tiles again)"""
    assert n % 64 != 0
    full_seen = set()
    for bulk in (B.BULK, B.BULK_FULL, B.BULK_SMALL):
        c = B.cloud(dim, variant, bulk)
        q, want = B.tiled(c, n)
        plan = _sweep_plan(n, c.m)
        assert plan[0] == r and plan[1] == (bulk == B.BULK_FULL or (bulk == B.BULK and r > 1)), (plan, c)
        full_seen.add(plan[1])
        icp = _handle(c.dst, I.NN_BRUTE)
        dev = _Device(q)
        _equal(dev.search(icp)[0], want, (c, "nn_search"))
        src, T = _under_the_exact_translation(c, q)
        got, a, b = _Device(src).search(icp, T)
        _equal(got, want, (c, "correspond_device"))
        assert np.array_equal(a, q[:, :2]) and np.array_equal(b, c.dst[want][:, :2])
        icp.close()
    assert full_seen == {True, False}


# ------------------------------------------------------------------------------------------- the grid, cold --


# nn_search carries no pose and correspond_device finds no snapshot of the source (nothing was prepared): `sorted` is
# false (nn_grid.hip:2129), neither the seeded nor a warm walk applies (nn_grid.hip:2152-2153) and k_nn_grid<., ., COLD>
# runs (nn_grid.hip:2251-2275), four lanes per query up to 65 536 queries, one beyond (nn_grid.hip:2147).
@pytest.mark.parametrize("n", [10_003, N_SHARED])
@pytest.mark.parametrize("variant", ["plain", "offset"])
@pytest.mark.parametrize("dim", [2, 3])
def test_cold_grid_search_equals_exact_nn(dim, variant, n):
    assert n % 64 != 0 and (n <= 65_536) == (n == 10_003)
    c = B.cloud(dim, variant)
    q, want = B.tiled(c, n)
    icp = _handle(c.dst, I.NN_GRID)
    _equal(_Device(q).search(icp)[0], want, (c, "nn_search"))
    src, T = _under_the_exact_translation(c, q)
    got, a, b = _Device(src).search(icp, T)
    _equal(got, want, (c, "correspond_device"))
    assert np.array_equal(a, q[:, :2]) and np.array_equal(b, c.dst[want][:, :2])
    assert I.nn_cert_counters(icp)[0] == 0
    icp.close()


# ------------------------------------------------------------------------------- the grid, seeded then warm --


def _cert_plan(dst, poses):
    """Which kernel each search of a prepared snapshot beyond 65 536 points takes, restated from launch_nn_grid
    (nn_grid.hip:2152-2243): `seeded` (the first), `cert` (k_nn_cert + k_nn_walk_lists: the step from the previous pose
    is at most 0.01 of the smallest cell side and certificates exist), `leave` (k_nn_grid_warm<., true>: such a step,
    no certificates yet: the walk leaves them) or `coop` (k_nn_grid_warm_coop: every other warm search)"""
    lo, h, n = B._geometry(dst)
    reach = np.sqrt(sum(max(abs(lo[d]), abs(lo[d] + h[d] * n[d])) ** 2 for d in range(2)))
    plan, have_certs, last = [], False, None
    for T in poses:
        p = T.pose
        if last is None:
            plan.append("seeded")
        else:
            dr = np.sqrt((p.r00 - last.r00) ** 2 + (p.r01 - last.r01) ** 2 + (p.r10 - last.r10) ** 2 + (p.r11 - last.r11) ** 2)
            dt = np.sqrt((p.tx - last.tx) ** 2 + (p.ty - last.ty) ** 2)
            step = dr * reach + dt
            assert not 0.009 * h.min() < step < 0.011 * h.min(), "too close to the threshold to restate"
            certs = step <= 0.01 * h.min()  # (the previous search left its pose: every search of a snapshot does)
            if certs and have_certs:
                plan.append("cert")
            elif certs:
                plan.append("leave")
                have_certs = True
            else:
                plan.append("coop")
        last = p
    return plan


def _along_poses(c, poses, want_plan=None):
    """prepare_source_device, then one search per pose: indices, a and b against exact_nn of the moved queries"""
    q = B.tiled(c, N_SHARED)[0]
    reps = N_SHARED // c.nq + 1
    icp = _handle(c.dst, I.NN_GRID)
    dev = _Device(q)
    icp.prepare_source_device(dev.q, poses[0])
    counters = []
    for k, T in enumerate(poses):
        got, a, b = dev.search(icp, T)
        counters.append(I.nn_cert_counters(icp))
        moved = _moved(T, c.q)
        want = np.tile(B.nearest(c.dst, moved), reps)[:N_SHARED]
        _equal(got, want, (c, k, T.as_array()))
        assert np.array_equal(a, np.tile(moved[:, :2], (reps, 1))[:N_SHARED])
        assert np.array_equal(b, c.dst[want][:, :2])
    plan = _cert_plan(c.dst, poses)
    print(f"{c}: {plan}, certificate counters {counters}")
    # every search that the restated dispatch sends to k_nn_cert, and no other, counted as one that checked certificates
    assert [x[0] for x in counters] == list(np.cumsum([p == "cert" for p in plan]))
    if want_plan is not None:
        assert set(want_plan) <= set(plan), plan
    icp.close()
    return plan, counters


# A snapshot of the source beyond 65 536 points: the first search is k_nn_grid_seeded (nn_grid.hip:2152, 2227), the
# later ones start from the previous matches: k_nn_grid_warm_coop after a long step, k_nn_grid_warm<., true> and then
# k_nn_cert + k_nn_walk_lists after steps of at most a hundredth of a cell (nn_grid.hip:2191-2243; _cert_plan).
@pytest.mark.parametrize("variant", ["plain", "offset"])
@pytest.mark.parametrize("dim", [2, 3])
def test_seeded_then_warm_searches_equal_exact_nn(dim, variant):
    c = B.cloud(dim, variant)
    step = 2.0 ** -16  # a few knot steps: most knot queries move to another target, their f32 coordinates barely change
    if variant == "plain":
        poses = [I.Transform(), _translation(EXACT_T), I.Transform(np.array([0.3, -0.2, 1e-3])),
                 I.Transform(np.array([0.3 + step, -0.2, 1e-3]))]
    else:  # translations only: a rotation about the origin moves this cloud by far more than a cell
        poses = [I.Transform(), _translation(EXACT_T), _translation((0.3, -0.2)), _translation((0.3 + step, -0.2))]
    # ... and the same step where the queries still sit INSIDE their knots: back beside the identity, and once more
    poses += [_translation((step, 0.0)), _translation((2 * step, 0.0))]
    moved = _moved(poses[1], c.q)
    assert np.array_equal(moved[:, :2], c.q[:, :2] + EXACT_T)  # exact: the ties are still ties
    assert np.mean(B.exact_nn(c.dst, moved)[2]) >= 0.04
    # the step changes the answer: it is two steps and more of the knots from s = 2^-17 down, 65 % of them (measured:
    # 0.53 - 0.55 of the knot queries change their target from the identity to poses[4], 0.14 from there to poses[5])
    at = [B.nearest(c.dst, _moved(T, c.q))[c.knot_queries] for T in (poses[0], poses[4], poses[5])]
    assert np.mean(at[0] != at[1]) >= 0.3 and np.mean(at[1] != at[2]) >= 0.05
    _along_poses(c, poses, want_plan=["seeded", "coop", "leave", "cert"])


# Steps of a fraction of a cell, a repeated pose, one long jump, small steps again: after the second search every small
# step checks the certificates of the previous matches (k_nn_cert) and walks only where they fail (k_nn_walk_lists).
# No certificate of a knot query is sound here -- its rival is closer than the bound's own margin -- so each of them
# must fail and be searched again: the index equality is what proves it.
@pytest.mark.parametrize("variant", ["plain", "offset"])
@pytest.mark.parametrize("dim", [2, 3])
def test_certified_searches_equal_exact_nn_along_a_chain_of_small_steps(dim, variant):
    c = B.cloud(dim, variant)
    hmin = float(B._geometry(c.dst)[1].min())
    rng = np.random.default_rng(900 + dim)
    t, poses = np.zeros(2), [I.Transform()]
    for st in [1e-4, 1e-3, 0.0, 2e-3, 1e-4, 30.0, 1e-3, 1e-4, 0.0]:
        d = rng.normal(size=2)
        t = t + st * hmin * d / np.linalg.norm(d)
        poses.append(_translation(t))
    plan, counters = _along_poses(c, poses)
    assert counters[-1][0] >= 4 and plan[:6] == ["seeded", "leave", "cert", "cert", "cert", "cert"]
    assert plan[6] == "coop"  # the long jump


# ------------------------------------------------------------------------------------- the whole registration --


# estimate() beyond 65 536 source points on the grid engine: the seeded search (k = 1), the warm search (k = 2, 3) and,
# where the host's bet on the next pose holds twice in a row, the run-ahead warm search, enqueued before the host knows
# its pose (api.hip:1287, 1313: it needs an iteration after next, so k >= 3; launch_nn_grid_ahead, nn_grid.hip:2071-2111)
# -- against the sweep on the same points in the grid's fold order, as
# test_gpu_search_rows.test_estimate_on_the_shared_walk_equals_the_brute_force_engine arranges it.  Whether a run-ahead
# search is issued depends on the inner counts of the iterations before it (the bet is placed after an iteration of one
# update, api.hip:1257): on these clouds none is within three iterations and only the 3-D offset cloud sees one within
# six (inner counts 2, 1, 1, 3, 2, 0), so k = 6 is run as well and the counters are printed, not asserted.
@pytest.mark.parametrize("variant", ["plain", "offset"])
@pytest.mark.parametrize("dim", [2, 3])
def test_estimate_on_the_grid_equals_the_sweep_and_exact_nn(dim, variant):
    c = B.cloud(dim, variant)
    src = B.tiled(c, N_SHARED)[0]
    reps = N_SHARED // c.nq + 1
    start = I.Transform(np.array(T0)) if variant == "plain" else _translation(T0[:2])
    grid, brute = _handle(c.dst, I.NN_GRID), _handle(c.dst, I.NN_BRUTE)
    for k in (1, 2, 3, 6):
        T, idx, inner = grid.estimate(src, start, k, return_info=True)
        perm = grid.last_fold_order(len(src))
        assert np.array_equal(np.sort(perm), np.arange(len(src)))
        bT, bidx_s, binner = brute.estimate(np.ascontiguousarray(src[perm]), start, k, return_info=True)
        bidx = np.empty_like(bidx_s)
        bidx[perm] = bidx_s
        if k == 1:  # the search of k = 1 runs at the initial pose
            want = np.tile(B.nearest(c.dst, _moved(start, c.q)), reps)[:N_SHARED]
            _equal(idx, want, (c, "grid, k = 1"))
            _equal(bidx, want, (c, "sweep, k = 1"))
        _equal(idx, bidx, (c, k))
        assert np.array_equal(inner, binner), (k, inner, binner)
        assert T.as_array().tobytes() == bT.as_array().tobytes(), (k, T.as_array(), bT.as_array())
        print(f"{c}: k = {k}, inner counts {inner.tolist()}, run-ahead searches confirmed / discarded so far "
              f"{I.run_ahead_counters(grid)}, speculative searches {I.gn_path_counters(grid)[4:]}")
    grid.close()
    brute.close()


# --------------------------------------------------------------------------------- the one-workgroup kernels --


def _tiny_poses():
    return [I.Transform(), _translation((2.0 ** -18, -(2.0 ** -19))), I.Transform(np.array([1e-3, -2e-3, 1e-5])),
            _translation(EXACT_T)]


# n = 512 <= 1024 source and m = 600 <= 2048 target points on a handle left on AUTO: the whole estimate is one launch
# of k_tiny_estimate (gn_fast.hip:473-474), whose search is tiny_nearest (tiny_device.hpp): tiny_screen_bound and an f32
# bound on x along the x-sorted targets.
@pytest.mark.parametrize("dim", [2, 3])
def test_single_launch_estimate_equals_exact_nn_at_the_initial_pose(dim):
    c = B.cloud(dim, "tiny")
    assert (c.m, c.nq) == (600, 512)
    for T in _tiny_poses():
        icp = (I.Icp3d if dim == 3 else I.Icp2d)(c.dst)
        got, idx, inner = icp.estimate(c.q, T, 1, return_info=True)
        assert icp.single_launch_counters()[0] == 1, icp.single_launch_counters()
        _equal(idx, B.nearest(c.dst, _moved(T, c.q)), (c, T.as_array()))
        # five outer iterations: the warm walk from the previous match, against the host-driven path on a handle with
        # the single launch off (k_nn_tiny: f64 only)
        got, idx, inner = icp.estimate(c.q, T, 5, return_info=True)
        assert icp.single_launch_counters()[0] == 2, icp.single_launch_counters()
        plain = (I.Icp3d if dim == 3 else I.Icp2d)(c.dst)
        plain.set_single_launch(False)
        pT, pidx, pinner = plain.estimate(c.q, T, 5, return_info=True)
        assert plain.single_launch_counters()[0] == 0
        _equal(idx, pidx, (c, "five iterations", T.as_array()))
        assert np.array_equal(inner, pinner) and got.as_array().tobytes() == pT.as_array().tobytes()
        icp.close()
        plain.close()


# four items of 512 x 600 points: each fits a workgroup of the batch launch (api_batch.hip:93-94, 158), which runs the
# same tiny_nearest on a box it reduces itself (tiny_device.hpp: tiny_batch_box)
@pytest.mark.parametrize("dim", [2, 3])
def test_batch_estimate_equals_exact_nn_and_the_single_call(dim):
    c = B.cloud(dim, "tiny")
    poses = _tiny_poses()
    batch = I.IcpBatch(dim)
    for max_iter in (1, 5):
        Ts, idxs, inner, status = batch.estimate([c.q] * 4, [c.dst] * 4, poses, max_iter, return_info=True)
        for i, T in enumerate(poses):
            icp = (I.Icp3d if dim == 3 else I.Icp2d)(c.dst)
            sT, sidx, sinner = icp.estimate(c.q, T, max_iter, return_info=True)
            icp.close()
            if max_iter == 1:
                _equal(idxs[i], B.nearest(c.dst, _moved(T, c.q)), (c, i))
            _equal(idxs[i], sidx, (c, i, max_iter))
            assert np.array_equal(inner[i], sinner) and Ts[i].as_array().tobytes() == sT.as_array().tobytes()
    served, one_by_one, launches, refused = batch.counters()
    assert (served, one_by_one, launches, refused) == (8, 0, 2, 0)
    batch.close()


# the same through the point-to-line batch (api_batch.hip:97, 158: up to 1024 x 2048 points per workgroup, normals of
# k = 8 neighbours included): item against single call, bit for bit
def test_line_batch_estimate_equals_the_single_call():
    from test_gpu_line_batch import assert_items_match

    c = B.cloud(2, "tiny")
    poses = _tiny_poses()
    batch = I.IcpBatch(2)
    srcs, dsts = [c.q] * 4, [c.dst] * 4
    for max_iter in (1, 5):
        got = batch.estimate_point_to_line(srcs, dsts, poses, max_iter, k=8, return_info=True, allow_failures=True)
        assert_items_match(srcs, dsts, poses, max_iter, 8, got)
        assert np.all(got[3] == 0), got[3]
    assert batch.line_counters()[:2] == (8, 0)
    batch.close()
