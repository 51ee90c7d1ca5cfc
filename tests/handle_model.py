"""Model-based sequence tests (test infrastructure): ONE handle through every kind of call, in arbitrary order.

What is held: a handle's answer depends on the cloud and the normals it holds, never on how it got there -- not on the
appends and crops behind the cloud, the engine asked for, a reserve, the calls made before, a poisoned call, or the
previous owner of its pooled buffers.

Three pieces, none of which needs a GPU (`torch` is never imported here):

  * `Model`: what a handle holds, in numpy -- dimension, cloud, normals (m x 3 in both dimensions) with normals_m /
    normals_k, the engine asked for, alive or closed -- and its transitions (append, keep_rows -- the one behind crop,
    thin, the removal by mask and the two outlier filters --, normals, close / create).
  * `sequence(seed, profile)`: a list of plain-data steps (op name, sizes, sub-seed, parameters).  Every random draw of
    a step is keyed by the sub-seed the step carries, so the same list drives the GPU and any stand-in.
    `map_sequence(seed, profile)`: the same with thin, remove, radius_filter, stat_filter and the reads through the grid
    (neighbours, query, count_within) in the mix; their parameters come from the model's cloud.
  * `run(device, steps)`: applies each step to a Model and to `device` and compares, bit for bit unless stated, with
    the references the single-call tests already use (imported, not copied).  `device` is any object with the
    operation methods of `ReferenceDevice` below: on the GPU a thin adapter over Icp2d / Icp3d
    (tests/test_gpu_sequences.py), on a machine without one `ReferenceDevice` itself -- a second model that answers
    with the reference results (tests/test_handle_model.py, which also derives sabotaged stand-ins from it).

Replaying a failure: `run` raises `SequenceFailure` with the seed, the step number, what differed and the step list up
to there as a Python literal.  `run(device, steps[:k])` replays a prefix: paste the literal, cut it, run it again.
"""
import pprint

import numpy as np

import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from parity_util import check_fold_order, oracle_in_device_order, oracle_plane_in_device_order
from test_gpu_crop import keep_mask, new_index_of
from test_gpu_gated import restate as gated_restate, searcher
from test_gpu_plane_parity import oracle_chain
from test_gpu_quality import transformed
from test_line_abi import lift, line_normals_numpy, outline
from test_map import moved
from test_outlier_abi import lists_of, new_index_of as filter_index_of, radius_keep, statistical_keep
from test_p2plane import room
from test_query_abi import count_within_ref, mask_keep, moved_queries, query_lists
from test_voxel_abi import keep_mask as thin_mask

INF = float("inf")
TRUE_PARAM = (0.03, -0.02, 0.01)  # the pose every scan is moved by (tests/test_line_abi.py's)
BRUTE_MAX_M = 10_000              # nn_search: O.nn_brute up to here, the kd-tree beyond
# line normals: line_normals_numpy sorts rows x m distances in numpy.  Every row is restated up to the 6 000 x 6 000 of
# tests/test_gpu_line.py's largest full check; beyond that many pairs, the first and the last LINE_ENDS rows and a seeded
# sample of those between (every row is still held to unit length and the older rows to their bits)
LINE_WORK = 6_000 * 6_000
LINE_ENDS = 512
MODES = {"auto": I.NN_AUTO, "brute": I.NN_BRUTE, "grid": I.NN_GRID}
REMOVALS = ("crop", "thin", "remove", "radius_filter", "stat_filter")
READS = ("neighbours", "query", "count_within")
MUTATING = ("create", "append", "reserve", "set_nn_mode", "normals") + REMOVALS
# the restatements of the filters, of the full neighbour lists and of the counts around the targets themselves are
# quadratic in m (about 3 s each at 9 000 targets, 35 s at 30 000): the generator emits the filters up to here only, and
# the full-range lists and the counts around the targets up to its profile's "full_max", which is lower still
QUADRATIC_MAX_M = 12_000
SUB_ROWS = 512                    # neighbours of a larger cloud: a sub-range of this many rows (at most 1 024)
GONE = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ the model

class Model:
    """what one handle holds"""

    def __init__(self, dim, cloud):
        self.dim = dim
        self.cloud = np.ascontiguousarray(cloud, dtype=np.float64).reshape(-1, dim)
        self.normals = np.zeros((len(self.cloud), 3))
        self.normals_m = 0
        self.normals_k = 0
        self.mode = "auto"
        self.alive = True

    @property
    def m(self):
        return len(self.cloud)

    @property
    def stale(self):
        """the normal-residual calls and read_normals are refused"""
        return self.m == 0 or self.normals_m != self.m

    def append(self, points):
        self.cloud = np.ascontiguousarray(np.concatenate([self.cloud, points]))
        self.normals = np.concatenate([self.normals, np.zeros((len(points), 3))])

    def carried(self, mask):
        """the normals of the kept rows"""
        return self.normals[mask]

    def current(self, mask):
        """how many of the kept rows have current normals: the kept ones among the first normals_m"""
        return int(mask[:self.normals_m].sum())

    def keep_rows(self, mask):
        """every removal (crop, thin, mask, the two filters): kept rows keep their order and their normals; rows appended
        but not yet updated stay without"""
        self.normals = np.ascontiguousarray(self.carried(mask))
        self.normals_m = self.current(mask)
        self.cloud = np.ascontiguousarray(self.cloud[mask])

    def set_normals(self, normals, k):
        self.normals = np.ascontiguousarray(normals, dtype=np.float64).reshape(self.m, 3)
        self.normals_m, self.normals_k = self.m, k

    def lifted(self):
        return self.cloud if self.dim == 3 else lift(self.cloud)


# --------------------------------------------------------------------------------- data a step stands for

def make_cloud(dim, m, seed, shift=(0.0, 0.0), scale=1.0):
    """test_p2plane.room (3-D) / test_line_abi.outline (2-D), moved by `shift` in xy, then in units of 1 / `scale` m"""
    rng = np.random.default_rng(seed)
    c = room(rng, m) if dim == 3 else outline(rng, m)
    c[:, 0] += shift[0]
    c[:, 1] += shift[1]
    return np.ascontiguousarray(c * scale)


def make_scan(cloud, n, seed, sigma=0.004, pose=TRUE_PARAM):
    """n noisy samples of the CURRENT cloud in the frame that `pose` maps into the cloud's: registered from the
    identity, the inner loops have an update to apply"""
    rng = np.random.default_rng(seed)
    world = cloud[rng.integers(0, len(cloud), n)] + rng.normal(size=(n, cloud.shape[1])) * sigma
    return np.ascontiguousarray(moved(world, I.Transform(list(pose)).inverse()))


def make_queries(cloud, n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(cloud[rng.integers(0, len(cloud), n)] + rng.normal(size=(n, cloud.shape[1])) * 0.05)


def make_pairs(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-5.0, 5.0, size=(n, 2))
    b = moved(a, I.Transform([0.05, -0.02, 0.01])) + rng.normal(size=(n, 2)) * 0.01
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def make_mask(m, share, seed, dtype):
    """the keep mask of a `remove` step: about `share` of the m targets (1.0: all, 0.0: none); as uint8 the kept bytes
    take values from 1 to 255, not only 1"""
    rng = np.random.default_rng(seed)
    keep = rng.random(m) < share
    if dtype == "bool":
        return keep
    return np.where(keep, rng.integers(1, 256, m), 0).astype(np.uint8)


def make_read_queries(cloud, n, seed, pose):
    """the n points of a `query` / `count_within` step and the Transform they go in with: points around the CURRENT cloud
    (make_queries), given in the frame that `pose` maps into the cloud's"""
    if len(cloud):
        q = make_queries(cloud, n, seed)
    else:  # (an empty handle refuses the read: any points do)
        q = np.ascontiguousarray(np.random.default_rng(seed).normal(size=(n, cloud.shape[1])))
    if pose is None:
        return q, None
    T = I.Transform(list(pose))
    return np.ascontiguousarray(moved(q, T.inverse())), T


def appended_points(model, step):
    """the points of an append step as they arrive in the cloud: make_cloud moved by the step's pose; with "clip" also
    clipped into the bounding box of the cloud as it is -- inside the box the grid was built for, whatever was removed
    since"""
    pts = make_cloud(model.dim, step["k"], step["seed"], step.get("shift", (0.0, 0.0)))
    if step.get("pose") is not None:
        pts = moved(pts, I.Transform(step["pose"]))
    if step.get("clip") and model.m:
        pts = np.clip(pts, model.cloud.min(axis=0), model.cloud.max(axis=0))
    return np.ascontiguousarray(pts)


def opose(T):
    return O.Pose(*T.pose.as_tuple())


# the masks of the removals, shared by the generator, trace() and run(): each is restated once per process
_MASKS = {}


def removal_mask(cloud, step):
    """(keep mask, statistics or None) of a removal step on `cloud`, by the single-call tests' restatements:
    test_gpu_crop.keep_mask, test_voxel_abi.keep_mask, test_query_abi.mask_keep, test_outlier_abi.radius_keep and
    statistical_keep"""
    op = step["op"]
    if op == "crop":
        return keep_mask(cloud, step["center"], INF if step["radius"] == "inf" else step["radius"]), None
    if op == "thin":
        return thin_mask(cloud, step["v"]), None
    if op == "remove":
        return mask_keep(make_mask(len(cloud), step["share"], step["seed"], step["dtype"]))[0], None
    key = (op, step.get("radius"), step.get("need"), step.get("k"), step.get("ratio"), cloud.shape, hash(cloud.tobytes()))
    if key not in _MASKS:
        if len(_MASKS) > 64:
            _MASKS.clear()
        if op == "radius_filter":
            _MASKS[key] = (radius_keep(cloud, step["radius"], step["need"]), None)
        elif op == "stat_filter":
            _MASKS[key] = statistical_keep(cloud, step["k"], INF if step["ratio"] == "inf" else step["ratio"])
        else:
            raise ValueError(f"{op!r} is no removal")
    return _MASKS[key]


# ------------------------------------------------------------------------------------------ the references

def ref_search(cloud, q):
    """O.nn_brute up to BRUTE_MAX_M targets, O.KdTree.search beyond"""
    rc, idx = O.nn_brute(cloud, q) if len(cloud) <= BRUTE_MAX_M else O.KdTree(cloud).search(q)
    assert rc == O.OK
    return idx


def half_radius(cloud, src, T):
    """a finite bound that keeps about half the points at the pose T: sqrt(median d2) of the exact matches"""
    q = moved(src, T)
    d = q - cloud[ref_search(cloud, q).astype(np.int64)]
    return float(np.sqrt(np.median(np.sum(d * d, axis=1))))


def ref_estimate(fold_source, model, src, init, iters):
    """parity_util.oracle_in_device_order: (status, pose, indices, inner counts)"""
    rc, oT, oidx, oinner = oracle_in_device_order(fold_source, model.dim, model.cloud, src, opose(init), iters)
    return rc, oT.as_array(), oidx, oinner


def ref_gated(model, src, init, iters, r, perm):
    """test_gpu_gated.restate with the call's fold order: (pose, indices, inner counts, inlier counts)"""
    oT, oidx, oinner, oinl = gated_restate(model.dim, model.cloud, src, opose(init), iters, r, perm,
                                           searcher(model.cloud, model.m <= BRUTE_MAX_M))
    return oT.as_array(), oidx, oinner, oinl


class _PlaneTarget:
    """what test_gpu_plane_parity.oracle_chain asks of its `t`"""

    def __init__(self, model):
        self.dim, self.icp = model.dim, None
        self.tree = O.KdTree(model.lifted())
        self.normals = model.normals


def ref_normal_estimate(model, src, init, iters, r):
    """ungated: parity_util.oracle_plane_in_device_order with the model's normals; gated: the chained statement on
    the kept points (test_gpu_plane_parity.oracle_chain).  Returns (status, pose, indices, inner counts, inliers)."""
    t = _PlaneTarget(model)
    src3 = src if model.dim == 3 else lift(src)
    if r is None:
        rc, oT, oidx, oinner = oracle_plane_in_device_order(None, t.tree, t.normals, src3, init, iters)
        return rc, oT.as_array(), oidx, oinner, None
    oT, oidx, oinner, oinl = oracle_chain(t, src, init, iters, r)
    return O.OK, oT.as_array(), oidx, oinner, oinl


def ref_normals(model, k, rows=None):
    """O.p2pl_normals / test_line_abi.line_normals_numpy of the cloud as it is now, as m x 3; `rows`: those rows only"""
    if model.dim == 2:
        return lift(line_normals_numpy(model.cloud, k, rows))
    if rows is None:
        return O.p2pl_normals(model.cloud, k)
    first = int(rows[0])
    assert np.array_equal(rows, np.arange(first, model.m))
    return O.p2pl_normals_update(model.cloud, first, k, np.zeros((model.m, 3)))[first:]


def ref_quality(model, kind, src, T, r):
    """`restate` of test_gpu_quality.py, test_gpu_plane_quality.py and (behind test_gpu_line_quality.py)
    test_line_quality_abi.py on the oracle's exact matches: (status, n, inliers, float fields, indices)"""
    import test_gpu_plane_quality as PQ
    import test_gpu_quality as Q
    import test_line_quality_abi as LQ

    n = len(src)
    if np.isnan(src).any():
        oidx = np.zeros(n, dtype=np.uint32)
    else:
        oidx = ref_search(model.cloud, transformed(src, T))
    if kind == "point":
        rc, cnt, floats = Q.restate(model.dim, model.cloud, src, T, r, oidx)
    elif model.dim == 3:
        rc, cnt, floats = PQ.restate(model.cloud, model.normals, src, T, r, oidx)
    else:
        rc, cnt, floats = LQ.restate(model.cloud, np.ascontiguousarray(model.normals[:, :2]), src, T, r, oidx)
    return rc, n, cnt, floats, oidx


# -------------------------------------------------------------------- the stand-in: a second model, answering

class ReferenceDevice:
    """A device without a GPU: a second Model that answers every operation with the reference's result.  Its methods
    are the interface `run` drives; every array in and out is numpy, every pose an I.Transform, every status an
    icp_status.  `perm_of(n)` -> (fold order, sort keys) of an estimate over n points (default: the caller's order)."""

    model_cls = Model

    def __init__(self, perm_of=None):
        self.model = None
        self.perm_of = perm_of or (lambda n: (np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.uint32)))
        self.last_block = 0
        self.prev_idx = None
        self.after_poison = False
        self.cloud_before = None  # the cloud before the last removal; None after a create or an append

    # -- the transitions (the sabotaged stand-ins of tests/test_handle_model.py each change one line of one of these)
    def new_model(self, dim, cloud):
        return self.model_cls(dim, cloud)

    def searched_cloud(self):
        return self.model.cloud

    def gated_fold(self, perm):
        return perm

    def indices(self, idx):
        self.prev_idx, self.after_poison = idx, False
        return idx

    # -- life
    def create(self, dim, cloud, borrowed=False, trim=False):
        self.model = self.new_model(dim, cloud)
        self.cloud_before = None

    def close(self):
        self.model.alive = False

    # -- the cloud
    def target_count(self):
        return self.model.m

    def read_targets(self):
        return self.model.cloud.copy()

    def append(self, points, T=None):
        self.model.append(moved(points, T) if T is not None else points)
        self.last_block = len(points)
        self.cloud_before = None

    def index_of(self, mask):
        return new_index_of(mask)

    def remove_rows(self, mask):
        """what every removal ends in: (the number removed, new_index)"""
        index = self.index_of(mask)
        self.cloud_before = self.model.cloud
        self.model.keep_rows(mask)
        return int(len(mask) - mask.sum()), index

    def crop(self, center, radius):
        return self.remove_rows(keep_mask(self.model.cloud, center, radius))

    def thin_keep(self, cloud, v):
        return thin_mask(cloud, v)

    def thin(self, v):
        return self.remove_rows(self.thin_keep(self.model.cloud, v))

    def remove(self, keep, entry):
        return self.remove_rows(mask_keep(keep)[0])

    def radius_keep(self, cloud, radius, need):
        return radius_keep(cloud, radius, need)

    def radius_filter(self, radius, need):
        if self.model.m == 0:
            return 0, np.zeros(0, dtype=np.uint32)
        return self.remove_rows(self.radius_keep(self.model.cloud, radius, need))

    def stat_filter(self, k, ratio):
        mask, stats = statistical_keep(self.model.cloud, k, ratio)
        return self.remove_rows(mask) + (stats,)

    # -- reads through the grid: (status, ...); every one sees the cloud through searched_cloud()
    def neighbours(self, k, first, count):
        cloud = self.searched_cloud()
        if len(cloud) == 0:
            return _lib.EMPTY_DST, None, None
        return (_lib.OK,) + lists_of(cloud, k, first, len(cloud) - first if count is None else count)

    def query(self, q, k, T=None, order=None):
        cloud = self.searched_cloud()
        if len(cloud) == 0:
            return _lib.EMPTY_DST, None, None
        return (_lib.OK,) + query_lists(cloud, q, k, T)

    def count_within(self, q, radius, cap=None, T=None):
        cloud = self.searched_cloud()
        if len(cloud) == 0:
            return _lib.EMPTY_DST, None
        return _lib.OK, count_within_ref(cloud, q, radius, cap, T)

    def reserve(self, capacity):
        pass

    def set_nn_mode(self, mode):
        self.model.mode = mode

    def nn_search(self, q):
        return ref_search(self.searched_cloud(), q)

    # -- point-to-point
    def last_fold_order(self, n, with_cells=False):
        perm, cell = self.perm_of(n)
        return (perm, cell) if with_cells else perm

    def estimate(self, src, init, iters, r=None):
        bad = np.isnan(src).any(axis=1)  # (the oracle's searches are not asked about a NaN: the documented outcome)
        if r is None:
            rc, T, idx, inner = (O.NAN, None, None, None) if bad.any() else ref_estimate(self, self.model, src, init, iters)
            if rc != O.OK:
                self.after_poison = True
                return rc, None, None, None, None
            return rc, T, self.indices(idx), inner, None
        perm = self.gated_fold(self.perm_of(len(src))[0])
        perm = (np.cumsum(~bad) - 1)[perm[~bad[perm]]]  # a NaN point is never an inlier: the others, renumbered
        T, good, inner, inl = ref_gated(self.model, np.ascontiguousarray(src[~bad]), init, iters, r, perm)
        idx = np.zeros(len(src), dtype=np.uint32)
        idx[~bad] = good
        return _lib.OK, T, self.indices(idx), inner, inl

    def evaluate(self, kind, src, T, r):
        if kind == "normal" and self.model.stale:
            return _lib.BAD_ARGUMENT, len(src), 0, None, None
        rc, n, cnt, floats, idx = ref_quality(self.model, kind, src, T, r)
        if rc != _lib.OK:
            self.after_poison = True
            return rc, n, 0, None, None
        return rc, n, cnt, floats, self.indices(idx)

    # -- normals and the normal residual
    def normals(self, k, update):
        mo = self.model
        if update and mo.normals_m > 0 and mo.normals_k != k:
            return _lib.BAD_ARGUMENT
        if update and mo.normals_m > 0:
            new = ref_normals(mo, k, np.arange(mo.normals_m, mo.m))
            mo.set_normals(np.concatenate([mo.normals[:mo.normals_m], new]), k)
        else:
            mo.set_normals(ref_normals(mo, k), k)
        return _lib.OK

    def read_normals(self):
        if self.model.stale:
            return _lib.BAD_ARGUMENT, None
        return _lib.OK, self.model.normals.copy()

    def estimate_normal(self, src, init, iters, r=None):
        if self.model.stale:
            return _lib.BAD_ARGUMENT, None, None, None, None
        rc, T, idx, inner, inl = ref_normal_estimate(self.model, src, init, iters, r)
        if rc != O.OK:
            self.after_poison = True
            return rc, None, None, None, None
        return rc, T, self.indices(idx), inner, inl

    # -- the free function (the scratch handle)
    def free_update(self, T, a, b):
        blocks, threads = I.reduce_geometry(len(a))
        rc, delta, _ = O.weighted_gauss_newton_update_tree(opose(T), a, b, blocks, threads)
        return delta if rc == O.OK else None


# ------------------------------------------------------------------------------------------------ the checker

class SequenceFailure(AssertionError):
    """a step whose result differs from the reference: .seed, .step (its number), .what, .prefix (steps[:step + 1])"""

    def __init__(self, seed, step, what, prefix):
        self.seed, self.step, self.what, self.prefix = seed, step, what, prefix
        super().__init__(f"seed {seed}, step {step} ({prefix[-1]['op']}): {what}\n"
                         f"replay with run(device, steps) on\nsteps = {pprint.pformat(prefix, width=150)}")


def _need(cond, *what):
    if not cond:
        raise AssertionError(" ".join(str(w) for w in what))


def _radius(model, step, src, T):
    r = step["r"]
    if r is None or isinstance(r, float):
        return r
    return INF if r == "inf" else half_radius(model.cloud, src, T)


def _check_state(model, device):
    """after every mutating step: the count and the bytes of the cloud, and the normals -- refused while stale"""
    _need(device.target_count() == model.m, "target_count", device.target_count(), "model", model.m)
    if model.m:
        _need(same_bits(device.read_targets(), model.cloud), "read_targets differs from the model's bytes")
    rc, normals = device.read_normals()
    if model.stale:
        _need(rc == _lib.BAD_ARGUMENT, "read_normals on stale normals returned status", rc)
    else:
        _need(rc == _lib.OK, "read_normals refused with status", rc)
        _need(same_bits(normals, model.normals), "read_normals differs from the model's normals")


def _check_estimate(got, want, what, inliers=True):
    rc, T, idx, inner, inl = got
    orc, oT, oidx, oinner, oinl = want
    _need(rc == orc, what, "status", rc, "reference", orc)
    if orc != _lib.OK:
        return
    _need(np.array_equal(idx, oidx), what, "indices differ at", np.nonzero(idx != oidx)[0][:10])
    _need(np.array_equal(inner, oinner), what, "inner counts", inner.tolist(), "reference", oinner.tolist())
    if inliers and oinl is not None:
        _need(np.array_equal(inl, oinl), what, "inlier counts", inl.tolist(), "reference", oinl.tolist())
    _need(same_bits(T, oT), what, "pose", T, "reference", oT)


def _step_estimate(model, device, step, src):
    init = I.Transform()
    iters, n = step["iters"], len(src)
    r = _radius(model, step, src, init)
    got = device.estimate(src, init, iters, r)
    if r is None:
        _check_estimate(got, ref_estimate(device, model, src, init, iters) + (None,), "estimate")
        return
    _need(got[0] == _lib.OK, "gated estimate: status", got[0])
    perm, cell = device.last_fold_order(n, with_cells=True)
    check_fold_order(perm, cell)
    _check_estimate(got, (_lib.OK,) + ref_gated(model, src, init, iters, r, perm), f"gated estimate r={r}")
    if r == INF:  # ... and the bits of the ungated reference
        _need(np.all(got[4] == n), "r = inf: inlier counts", got[4].tolist())
        _check_estimate(got, ref_estimate(device, model, src, init, iters) + (None,), "gated estimate r=inf, ungated")


def _step_normal_estimate(model, device, step, src):
    init = I.Transform()
    if model.stale:  # refused with the documented status; nothing is computed
        r = {None: None, "inf": INF}.get(step["r"], 0.05)
        rc = device.estimate_normal(src, init, step["iters"], r)[0]
        _need(rc == _lib.BAD_ARGUMENT, "stale normals: status", rc, "documented", _lib.BAD_ARGUMENT)
        return
    r = _radius(model, step, src, init)
    got = device.estimate_normal(src, init, step["iters"], r)
    _check_estimate(got, ref_normal_estimate(model, src, init, step["iters"], r), f"normal estimate r={r}")


def _step_evaluate(model, device, step, src):
    T = I.Transform(list(TRUE_PARAM))
    kind = step["kind"]
    if kind == "normal" and model.stale:
        rc = device.evaluate(kind, src, T, INF)[0]
        _need(rc == _lib.BAD_ARGUMENT, "stale normals: status", rc, "documented", _lib.BAD_ARGUMENT)
        return
    r = _radius(model, step, src, T)
    rc, n, inliers, floats, gidx = device.evaluate(kind, src, T, r)
    orc, on, ocnt, ofloats, oidx = ref_quality(model, kind, src, T, r)
    what = f"evaluate {kind} r={r}:"
    _need(rc == orc == _lib.OK, what, "status", rc, "reference", orc)
    _need(np.array_equal(gidx, oidx), what, "indices differ at", np.nonzero(gidx != oidx)[0][:10])
    _need(n == on and inliers == ocnt, what, "n, inliers", n, inliers, "reference", on, ocnt)
    _need(same_bits(floats, ofloats), what, "fields", floats, "reference", ofloats)


def _step_poisoned(model, device, step, src):
    """one NaN source point: the status the single-call tests document, or dropped by a finite bound"""
    bad = src.copy()
    j = len(bad) // 3
    bad[j, step["seed"] % 2] = np.nan
    init, kind = I.Transform(), step["kind"]
    if kind in ("query", "count_within"):  # the NaN point lists nothing and counts nothing; every other row as restated
        T = I.Transform(list(TRUE_PARAM))
        if kind == "query":
            got = device.query(bad, step["k"], T, None)
            _check_lists(got, query_lists(model.cloud, bad, step["k"], T), "query with a NaN point")
            nan = np.isnan(moved_queries(bad, T)).any(axis=1)
            _need(nan[j] and np.all(got[1][nan] == GONE) and np.all(got[2][nan] == INF), "the NaN point's row is not padding")
        else:
            rc, counts = device.count_within(bad, step["radius"], step["cap"], T)
            _need(rc == _lib.OK, "count_within with a NaN point: status", rc)
            want = count_within_ref(model.cloud, bad, step["radius"], step["cap"], T)
            _need(np.array_equal(np.asarray(counts), want) and counts[j] == 0, "count_within with a NaN point differs")
        return
    if kind == "estimate":
        rc = device.estimate(bad, init, step["iters"], None)[0]
    elif kind == "normal":
        rc = device.estimate_normal(bad, init, step["iters"], None)[0]
    elif kind in ("evaluate", "evaluate_normal"):
        rc = device.evaluate("point" if kind == "evaluate" else "normal", bad, I.Transform(list(TRUE_PARAM)), INF)[0]
    else:  # "gated": test_gpu_gated.py::test_a_nan_source_point_is_dropped_by_a_finite_bound, against the restatement
        good = np.ascontiguousarray(np.delete(src, j, axis=0))
        r = half_radius(model.cloud, good, init)
        rc, T, idx, inner, inl = device.estimate(bad, init, step["iters"], r)
        _need(rc == _lib.OK, "a NaN point under a finite bound: status", rc)
        perm = device.last_fold_order(len(bad))
        _need(np.array_equal(perm, np.arange(len(bad))), "a source of", len(bad), "points folds in the caller's order")
        want = ref_gated(model, good, init, step["iters"], r, np.arange(len(good)))
        _check_estimate((rc, T, np.delete(idx, j), inner, inl), (_lib.OK,) + want, "gated estimate without the NaN point")
        return
    want = _lib.BAD_ARGUMENT if kind in ("normal", "evaluate_normal") and model.stale else _lib.NAN_INPUT
    _need(rc == want, f"poisoned {kind}: status", rc, "documented", want)


def _step_normals(model, device, step):
    k, update = step["k"], step["update"]
    first = model.normals_m if update else 0
    refused = update and model.normals_m > 0 and model.normals_k != k
    rc = device.normals(k, update)
    if refused:  # a different k: refused, and nothing changes (_check_state follows)
        _need(rc == _lib.BAD_ARGUMENT, "update with another k: status", rc)
        return
    _need(rc == _lib.OK, "normals: status", rc)
    rc, got = device.read_normals()
    _need(rc == _lib.OK and got.shape == (model.m, 3), "read_normals after the normals were computed: status", rc)
    _need(same_bits(got[:first], model.normals[:first]), "update: an older row changed")
    if model.dim == 2:
        _need(not got[:, 2].any(), "a line normal with nz != 0")
    rows = np.arange(first, model.m)
    if model.dim == 2 and len(rows) * model.m > LINE_WORK:
        rows = sample_rows(rows, LINE_WORK // model.m, step["seed"])
    want = ref_normals(model, k, None if len(rows) == model.m else rows)
    _need(np.allclose(np.linalg.norm(got[first:], axis=1), 1.0, rtol=0.0, atol=1e-12), "normals: not unit length")
    err = float(np.max(np.abs(got[rows] - want))) if len(rows) else 0.0
    _need(err < 1e-9, "normals differ from the CPU statement by", err)
    model.set_normals(got, k)  # the device's normals, as tests/test_gpu_plane_parity.py feeds the oracle


def _step_removal(model, device, step):
    """crop, thin, remove, radius_filter, stat_filter: the number removed, the whole new_index map and, for the statistical
    filter, its three statistics to the bit (as tests/test_gpu_outlier.py holds them); on an empty handle the documented
    return values: nothing removed, an empty map, statistics of +0.0.  _check_state follows."""
    op = step["op"]
    mask, stats = removal_mask(model.cloud, step)
    if op == "crop":
        got = device.crop(step["center"], INF if step["radius"] == "inf" else step["radius"])
    elif op == "thin":
        got = device.thin(step["v"])
    elif op == "remove":
        got = device.remove(make_mask(model.m, step["share"], step["seed"], step["dtype"]), step["entry"])
    elif op == "radius_filter":
        got = device.radius_filter(step["radius"], step["need"])
    else:
        got = device.stat_filter(step["k"], INF if step["ratio"] == "inf" else step["ratio"])
    removed, index = got[:2]
    want = int(len(mask) - mask.sum())
    _need(removed == want, f"{op} removed", removed, "model", want)
    index_of = new_index_of if op == "crop" else filter_index_of
    _need(np.array_equal(np.asarray(index), index_of(mask)), f"{op}: the index map differs")
    if op == "stat_filter":
        _need(np.array_equal(bits(got[2]), bits(stats)), "stat_filter: (mean, deviation, threshold)", got[2], "reference", stats)
    model.keep_rows(mask)


RESTATE_ROWS = 5_000  # a query of more points is restated on both ends and a seeded sample of 2 000 rows


def _check_lists(got, want, what, rows=None):
    """indices exactly, d2 to the bit, padding included"""
    rc, idx, d2 = got
    _need(rc == _lib.OK, what, "status", rc)
    if rows is not None:
        _need(idx.shape[0] > rows[-1], what, "rows", idx.shape)
        idx, d2 = idx[rows], d2[rows]
    widx, wd2 = want
    _need(idx.shape == widx.shape and d2.shape == wd2.shape, what, "shapes", idx.shape, d2.shape, "reference", widx.shape)
    _need(np.array_equal(idx, widx), what, "indices differ in rows", np.nonzero((idx != widx).any(axis=1))[0][:10])
    _need(same_bits(d2, wd2), what, "d2 differs in rows", np.nonzero((bits(d2) != bits(wd2)).any(axis=1))[0][:10])


def _step_read(model, device, step):
    """neighbours, query, count_within: the restated rows exactly; on an empty handle the status query.hip and outlier.hip
    document (ICP_EMPTY_DST)"""
    op, m = step["op"], model.m
    if op == "neighbours":
        k, first, count = step["k"], step["first"], step["count"]
        got = device.neighbours(k, first, count)
        if m == 0:
            _need(got[0] == _lib.EMPTY_DST, "neighbours on an empty handle: status", got[0])
            return
        _check_lists(got, lists_of(model.cloud, k, first, m - first if count is None else count), f"neighbours k={k}")
        return
    n = step["n"]
    q, T = (None, None) if n is None else make_read_queries(model.cloud, n, step["seed"], step.get("pose"))
    if op == "count_within":
        rc, counts = device.count_within(q, step["radius"], step["cap"], T)
        if m == 0:
            _need(rc == _lib.EMPTY_DST, "count_within on an empty handle: status", rc)
            return
        _need(rc == _lib.OK, "count_within: status", rc)
        want = count_within_ref(model.cloud, q, step["radius"], step["cap"], T)
        counts = np.asarray(counts)
        _need(np.array_equal(counts, want), "count_within differs at", np.nonzero(counts != want)[0][:10])
        return
    k, order = step["k"], step.get("order")
    got = device.query(q, k, T, order)
    if m == 0:
        _need(got[0] == _lib.EMPTY_DST, "query on an empty handle: status", got[0])
        return
    rows = None
    if n > RESTATE_ROWS:
        ends = np.concatenate([np.arange(64), np.arange(n - 64, n)])
        middle = np.random.default_rng(step["seed"]).choice(np.arange(64, n - 64), 2_000, replace=False)
        rows = np.unique(np.concatenate([ends, middle]))
    _check_lists(got, query_lists(model.cloud, q if rows is None else q[rows], k, T), f"query k={k} n={n} order={order}", rows)
    if order == "cell":  # ... and in full, byte for byte, the same call in the caller's order
        rc, idx, d2 = device.query(q, k, T, "caller")
        _need(rc == _lib.OK, "query in the caller's order: status", rc)
        _need(idx.tobytes() == got[1].tobytes() and d2.tobytes() == got[2].tobytes(), "the cell-ordered query differs from the "
              "same call in the caller's order")


def sample_rows(rows, count, seed):
    """both ends of `rows` and a seeded sample of the middle: about `count` rows, ascending"""
    ends = np.concatenate([rows[:LINE_ENDS], rows[-LINE_ENDS:]])
    middle = rows[LINE_ENDS:-LINE_ENDS]
    take = min(len(middle), max(count - len(ends), LINE_ENDS))
    return np.unique(np.concatenate([ends, np.random.default_rng(seed).choice(middle, take, replace=False)]))


def apply_step(models, devices, step):
    """one step on its handle's model and device; `models`: {handle key: Model}, updated in place"""
    key, op = step.get("h", 0), step["op"]
    device, model = devices[key], models.get(key)
    if op == "free_update":
        T = I.Transform(step["pose"])
        a, b = make_pairs(step["n"], step["seed"])
        got = device.free_update(T, a, b)
        blocks, threads = I.reduce_geometry(len(a))
        rc, want, _ = O.weighted_gauss_newton_update_tree(opose(T), a, b, blocks, threads)
        _need(rc == O.OK and got is not None and same_bits(got, want), "free update", got, "reference", want)
        return
    if op == "create":
        _need(model is None or not model.alive, "create on a live handle")
        model = models[key] = Model(step["dim"], make_cloud(step["dim"], step["m"], step["seed"], scale=step.get("scale", 1.0)))
        device.create(model.dim, model.cloud.copy(), borrowed=step.get("borrowed", False), trim=step.get("trim", False))
    elif op == "close":
        device.close()
        model.alive = False
        return
    else:
        _need(model is not None and model.alive, "a step on a closed handle")
    if op == "append":
        pts = make_cloud(model.dim, step["k"], step["seed"], step.get("shift", (0.0, 0.0)))
        T = I.Transform(step["pose"]) if step.get("pose") is not None else None
        if step.get("clip"):  # the points as they arrive in the cloud, handed over as they are
            pts, T = appended_points(model, step), None
        model.append(moved(pts, T) if T is not None else pts)
        device.append(pts.copy(), T)
    elif op in REMOVALS:
        _step_removal(model, device, step)
    elif op in READS:
        _step_read(model, device, step)
    elif op == "reserve":
        device.reserve(step["capacity"])
    elif op == "set_nn_mode":
        device.set_nn_mode(step["mode"])
        model.mode = step["mode"]
    elif op == "normals":
        _step_normals(model, device, step)
    elif op == "nn_search":
        q = make_queries(model.cloud, step["n"], step["seed"])
        got, want = device.nn_search(q), ref_search(model.cloud, q)
        _need(np.array_equal(got, want), "nn_search differs at", np.nonzero(got != want)[0][:10])
    elif op in ("estimate", "normal_estimate", "evaluate", "poisoned"):
        src = make_scan(model.cloud, step["n"], step["seed"], step.get("sigma", 0.004), step.get("pose", TRUE_PARAM))
        {"estimate": _step_estimate, "normal_estimate": _step_normal_estimate, "evaluate": _step_evaluate,
         "poisoned": _step_poisoned}[op](model, device, step, src)
    elif op != "create":
        raise ValueError(f"unknown op {op!r}")
    if op in MUTATING:
        _check_state(model, device)


def run(device, steps, seed=None, on_step=None):
    """Apply `steps` to a fresh Model and to `device` (or to {handle key: device}, for steps that carry "h") and
    compare after each; raises SequenceFailure at the first step that differs.  run(device, steps[:k]) replays a
    prefix.  `on_step(no, step, models)`, if given, is called after each step that passed (path confirmation).
    Returns the models."""
    devices = device if isinstance(device, dict) else {0: device}
    models = {}
    for no, step in enumerate(steps):
        try:
            apply_step(models, devices, step)
            if on_step is not None:
                on_step(no, step, models)
        except SequenceFailure:
            raise
        except Exception as e:  # a mismatch, or an error of the device: either way this step is the finding
            raise SequenceFailure(seed, no, f"{type(e).__name__}: {e}", list(steps[:no + 1])) from e
    return models


# --------------------------------------------------------------------------------------------- the generator

# Sizes come from the thresholds in the code, not from workloads.  Targets: below kTinyMaxM (2 048); between it and
# kGridMinM (8 192); just below 8 192, so that an append crosses it and a crop crosses back; 20-30 k for the grid.
# Sources: 1, 2, a wave (63-65), a block (511-513), the single-launch path and the gate's tile (1 024 / 1 025), the
# one-launch inner loop (from 4 096: 5 000), and one size above kGridCoopMaxN (65 536) for estimate and its gate.
PROFILES = {
    "gpu": dict(m_create=(7_800, 1_500, 24_000, 5_000), m_later=(1_800, 9_000, 5_000), near=(7_000, 8_192), m_max=30_000,
                n_sizes=(513, 1, 1_024, 64, 5_000, 2, 1_025, 63, 512, 65, 511), n_big=70_000, n_poison=1_025,
                nq=2_000,
                # the map sequences: a cloud a thin takes below near[1] and one a filter does; the large cloud; the second
                # life's; where the quadratic restatements end (QUADRATIC_MAX_M) and where the full-range reads do
                m_cross=(8_700, 8_250), m_stay=9_600, m_big=24_000, m_second=(1_800, 2_400, 3_000), quad_max=QUADRATIC_MAX_M,
                full_max=4_500, q_sizes=(2_000, 1, 64, 63, 65)),
    # the reduced profile of tests/test_handle_model.py: the same generator, every size scaled below the thresholds
    "cpu": dict(m_create=(1_300, 400, 2_600, 900), m_later=(500, 1_500, 900), near=(1_200, 1_400), m_max=3_000,
                n_sizes=(513, 1, 1_024, 64, 1_200, 2, 1_025, 63, 512, 65, 511), n_big=1_200, n_poison=257,
                nq=300,
                m_cross=(1_480, 1_430), m_stay=1_640, m_big=2_600, m_second=(500, 700, 900), quad_max=2_000, full_max=1_000,
                q_sizes=(300, 1, 64, 63, 65)),
}
# what follows a change of the cloud, in rotation (a form that needs current normals is preceded by what makes them so)
FORMS = ("nn_search", "estimate", "normal", "evaluate_inf", "estimate_half", "evaluate_normal_half", "poison_estimate",
         "normal_half", "estimate_inf", "evaluate_half", "reserve", "normal_inf", "poison_normal", "evaluate_normal_inf",
         "set_nn_mode", "poison_evaluate", "poison_gated", "poison_evaluate_normal")
NORMALS_K = (8, 10, 6)
# the second rotation, of the map sequences: the reads through the grid (and their poisoned forms)
MAP_READS = ("neighbours", "query", "count_cap", "query_pose", "poison_query", "count", "poison_count")
K_VALUES = (8, 1, 16, 17, 32)  # both kernel widths of the lists (KMAX 16 and 32) and their edges
MASK_FORMS = (("host", "bool"), ("device", "uint8"), ("host", "uint8"), ("device", "bool"))
FILTERS = ("radius_filter", "stat_filter")
READ_POSE = [0.03, -0.02, 0.01]
READ_POISON_N = 257  # the points of a poisoned read: four waves and one point
# the sequences tests/test_gpu_sequences.py runs, and tests/test_handle_model.py asserts the coverage conditions over
GPU_DIMS, GPU_SEEDS, GPU_INTERLEAVED_SEEDS = (3, 2), tuple(range(6)), tuple(range(3))
GPU_MAP_SEEDS, GPU_MAP_INTERLEAVED_SEEDS = tuple(range(6)), tuple(range(2))
CENTER = {3: (1.0, -1.0), 2: (1.0, 0.0)}


class _Generator:
    def __init__(self, seed, profile, dim_start, key=None):
        self.P = PROFILES[profile]
        self.rng = np.random.default_rng([seed, dim_start, sorted(PROFILES).index(profile)])
        self.seed, self.key, self.steps = seed, key, []
        slot = seed + (6 if dim_start == 2 else 0) + (0 if key is None else 1 + key)
        self.slot = slot
        self.form = {"create": (2 * slot + 5) % len(FORMS), "append": (2 * slot) % len(FORMS),
                     "crop": (2 * slot + len(FORMS) // 2) % len(FORMS)}
        for at, kind in enumerate(("thin", "remove", "filter")):  # (the map sequences: the old rotation after the new removals)
            self.form[kind] = (2 * slot + 3 + 5 * at) % len(FORMS)
        self.read_form = {kind: (3 * slot + at) % len(MAP_READS)
                          for at, kind in enumerate(("create", "append", "crop", "thin", "remove", "filter"))}
        self.new_turn = {kind: (slot + at) % 2 == 0
                         for at, kind in enumerate(("create", "append", "crop", "thin", "remove", "filter"))}
        self.last = "create"
        self.size = (3 * seed + (4 if dim_start == 2 else 0)) % len(self.P["n_sizes"])
        self.lives = 0
        self.model = None
        self.reads = self.masks = 0
        self.targets_done = set()
        self.borrowed = False

    def emit(self, op, **kw):
        step = {"op": op, **kw}
        if self.key is not None:
            step["h"] = self.key
        self.steps.append(step)
        return step

    def sub(self):
        return int(self.rng.integers(1, 1 << 30))

    def n(self):
        self.size = (self.size + 1) % len(self.P["n_sizes"])
        return self.P["n_sizes"][self.size]

    # -- the cloud
    def create(self, dim, m, first, borrowed=None):
        seed = self.sub()
        self.borrowed = bool(first and self.seed % 2 == 1) if borrowed is None else bool(borrowed)
        self.emit("create", dim=dim, m=m, seed=seed, borrowed=self.borrowed, trim=bool(first))
        self.model = Model(dim, make_cloud(dim, m, seed))
        self.lives += 1
        self.last = "create"

    def append(self, kind, clip=False):
        mo, lo_hi = self.model, self.P["near"]
        if mo.m == 0:
            k, shift = self.P["m_later"][self.seed % 3], (0.0, 0.0)
        elif lo_hi[0] <= mo.m < lo_hi[1] or (kind == "up" and mo.m < lo_hi[1]):   # across the threshold
            k, shift = lo_hi[1] - mo.m + mo.m // 12, (0.0, 0.0)
        elif kind in ("incremental", "up"):         # inside the box of the last build and below 1.5 x its size
            k, shift = max(mo.m // 8, 64), (0.0, 0.0)
        elif kind == "outside":             # beyond the box: the grid is rebuilt
            k, shift = max(mo.m // 8, 64), (1.5, -0.75)
        else:                               # more than half again of what the grid was built for
            k, shift = (mo.m * 3) // 5, (0.0, 0.0)
        k = min(k, max(self.P["m_max"] - mo.m, 64))
        seed = self.sub()
        pose = [0.02, -0.01, 0.005] if self.rng.random() < 0.4 else None
        if clip:  # (a map sequence's incremental append: surely inside the grid's box, so that the path can be predicted)
            step = self.emit("append", k=k, seed=seed, shift=shift, pose=pose, clip=True)
        else:
            step = self.emit("append", k=k, seed=seed, shift=shift, pose=pose)
        mo.append(appended_points(mo, step))
        self.last = "append"
        self.borrowed = False

    def crop(self, kind):
        mo, lo_hi = self.model, self.P["near"]
        c = CENTER[mo.dim]
        center = (c[0] + float(self.rng.integers(-8, 9)) / 32.0, c[1] + float(self.rng.integers(-8, 9)) / 32.0)
        d = np.sqrt(np.sort(np.sum((mo.cloud[:, :2] - np.array(center)) ** 2, axis=1)))
        if kind == "nothing":
            radius = "inf"
        elif kind == "everything":
            center, radius = (1.0e6, 1.0e6), 1.0
        else:
            keep = 0.88 if kind == "moving" else 0.5
            if lo_hi[1] <= mo.m < lo_hi[1] * 1.12:  # back across the threshold
                keep = min(keep, 0.85)
            radius = float(d[int(keep * (len(d) - 1))])
        self.emit("crop", center=[center[0], center[1]], radius=radius)
        mo.keep_rows(keep_mask(mo.cloud, center, INF if radius == "inf" else radius))
        self.last = "crop"

    def normals(self, wrong_k=False):
        mo = self.model
        update = 0 < mo.normals_m < mo.m
        k = mo.normals_k if update else NORMALS_K[(self.seed + self.lives) % 3]
        if wrong_k:
            self.emit("normals", k=k + 1, update=True, seed=self.sub())
            return
        self.emit("normals", k=k, update=update, seed=self.sub())
        mo.normals_m, mo.normals_k = mo.m, k

    # -- what follows
    def check(self, n=None):
        """the next form of the rotation after the last change of the cloud"""
        mo = self.model
        name = FORMS[self.form[self.last]]
        self.form[self.last] = (self.form[self.last] + 1) % len(FORMS)
        needs_normals = name.startswith(("normal", "evaluate_normal", "poison_normal", "poison_evaluate_normal"))
        if needs_normals and mo.stale:
            self.normals()
        r = {"half": "half", "inf": "inf"}.get(name.rsplit("_", 1)[-1])
        n = n or self.n()
        if name == "nn_search":
            self.emit("nn_search", n=self.P["nq"], seed=self.sub())
        elif name.startswith("estimate"):
            self.emit("estimate", n=n, seed=self.sub(), iters=3, r=r)
        elif name.startswith("normal"):
            self.emit("normal_estimate", n=n, seed=self.sub(), iters=3, r=r)
        elif name.startswith("evaluate"):
            self.emit("evaluate", kind="normal" if "normal" in name else "point", n=n, seed=self.sub(), r=r)
        elif name == "reserve":
            self.emit("reserve", capacity=int(mo.m * (0.5 if self.rng.random() < 0.3 else 1.7)))
        elif name == "set_nn_mode":
            mode = ("brute", "grid", "auto")[(self.seed + len(self.steps)) % 3]
            self.emit("set_nn_mode", mode=mode)
            mo.mode = mode
        else:  # a poisoned call, and the checked call that has to be right after it
            self.emit("poisoned", kind=name[len("poison_"):], n=self.P["n_poison"], seed=self.sub(), iters=2)
            self.emit("estimate" if "normal" not in name else "normal_estimate", n=self.n(), seed=self.sub(), iters=3,
                      r=None)

    def big_and_small(self):
        """a source above kGridCoopMaxN between two of at most 1 024 points: estimate, then its gate"""
        gate = "half" if (self.slot // 2) % 2 else None
        self.emit("estimate", n=1_024 if self.seed % 2 else 513, seed=self.sub(), iters=3, r=None)
        self.emit("estimate", n=self.P["n_big"], seed=self.sub(), iters=3, r=gate)
        self.emit("estimate", n=64 if self.seed % 2 else 1_024, seed=self.sub(), iters=3, r="half" if gate is None else None)

    def stale_episode(self):
        """normals, an append, a refused call, a crop on the stale cloud, an update with another k (refused), the update"""
        if self.model.stale:
            self.normals()
        self.append("incremental")
        self.emit("normal_estimate", n=self.n(), seed=self.sub(), iters=2, r=None if self.seed % 2 else "half")
        self.crop("moving")
        if self.seed % 2:
            self.emit("evaluate", kind="normal", n=self.n(), seed=self.sub(), r="inf")  # refused after the crop too
            self.normals(wrong_k=True)
        self.normals()
        self.emit("normal_estimate", n=self.n(), seed=self.sub(), iters=3, r="half" if self.seed % 2 else None)


def thin_size(cloud, share):
    """the voxel size whose restated mask keeps about `share` of `cloud`: bisected, since the 2-D outline and the 3-D room
    thin at quite different sizes"""
    lo, hi = 1e-4, 8.0
    for _ in range(22):
        mid = float(np.sqrt(lo * hi))
        lo, hi = (mid, hi) if thin_mask(cloud, mid).mean() > share else (lo, mid)
    return float(np.float32(np.sqrt(lo * hi)))


class _MapGenerator(_Generator):
    """the same generator with the four newer removals and the second rotation of forms, the reads through the grid"""

    # -- parameters from the model's cloud
    def thin_size(self, share):
        return thin_size(self.model.cloud, share)

    def kth_d2(self, k, rows=512):
        """the restated d2 to the k-th nearest target (itself included) of a seeded sample of rows"""
        c = self.model.cloud
        if len(c) <= rows:
            return lists_of(c, k)[1][:, k - 1]
        block = rows // 8  # (eight blocks spread over the cloud: its rows come wall by wall)
        firsts = (np.arange(8) * (len(c) - block)) // 7
        jitter = int(self.rng.integers(0, block))
        return np.concatenate([lists_of(c, k, max(int(f) - jitter, 0), block)[1][:, k - 1] for f in firsts])

    def filter_radius(self, need, share):
        """a radius that keeps about `share`: that quantile of the restated distance to the need-th neighbour"""
        return float(np.sqrt(np.quantile(self.kth_d2(need), share)))

    # -- the removals
    def removal(self, kind, how):
        """`how`: "moving" (keeps about 0.88: at least 1 / 1.5 of what the grid was built for), "rebuild" (about 0.5),
        "light" (a radius filter that keeps about 0.94: a grid stays a grid),
        "nothing", "everything", "handful" (a mask that keeps 3 to 12 targets)"""
        mo = self.model
        if kind in FILTERS and mo.m > self.P["quad_max"]:
            kind = "thin" if how in ("moving", "rebuild") else "remove"
        if kind == "stat_filter" and how not in ("moving", "nothing"):  # (the rule reaches no other share)
            kind = "radius_filter"
        if kind == "thin" and how in ("everything", "handful"):
            kind = "remove"
        share = {"moving": 0.88, "rebuild": 0.5, "light": 0.94}.get(how)
        if kind == "crop":
            self.crop(how)
            return
        if kind == "thin":
            step = self.emit("thin", v=1e-9 if how == "nothing" else self.thin_size(share))
        elif kind == "remove":
            entry, dtype = MASK_FORMS[(self.slot + self.masks) % 4]
            self.masks += 1
            share = {"nothing": 1.0, "everything": 0.0, "handful": 7.0 / max(mo.m, 1)}.get(how, share)
            while True:
                seed = self.sub()
                kept = int((make_mask(mo.m, share, seed, dtype) != 0).sum())
                if how != "handful" or 3 <= kept <= 12:
                    break
            step = self.emit("remove", share=share, seed=seed, entry=entry, dtype=dtype)
        elif kind == "radius_filter":
            if how == "everything":
                step = self.emit("radius_filter", radius=0.01, need=mo.m + 1)
            elif how == "nothing":
                step = self.emit("radius_filter", radius=0.0, need=1)
            else:
                need = 9 if how == "rebuild" else 5
                step = self.emit("radius_filter", radius=self.filter_radius(need, share), need=need)
        else:
            step = self.emit("stat_filter", k=8, ratio="inf" if how == "nothing" else 1.0)
        mask, _ = removal_mask(mo.cloud, step)
        if mask.sum() < len(mask):
            self.borrowed = False
        mo.keep_rows(mask)
        self.last = "filter" if kind in FILTERS else kind

    def crop(self, kind):
        super().crop(kind)
        self.borrowed = False

    # -- what follows
    def read(self, name=None):
        """the next form of the second rotation after the last change of the cloud (or the form `name`)"""
        mo, P = self.model, self.P
        if name is None:
            name = MAP_READS[self.read_form[self.last]]
            self.read_form[self.last] = (self.read_form[self.last] + 1) % len(MAP_READS)
        k = K_VALUES[(self.slot + self.reads) % len(K_VALUES)]
        n = P["q_sizes"][(2 * self.slot + self.reads) % len(P["q_sizes"])]
        self.reads += 1
        if name == "neighbours":
            if mo.m <= P["full_max"]:
                first, count = 0, None
            else:  # both ends and one in the middle
                count = min(SUB_ROWS, mo.m)
                first = (0, mo.m - count, (mo.m - count) // 2)[self.reads % 3]
            self.emit("neighbours", k=k, first=first, count=count)
        elif name in ("query", "query_pose"):
            self.emit("query", n=n, k=k, seed=self.sub(), pose=READ_POSE if name == "query_pose" else None)
        elif name.startswith("count"):
            radius = float(np.sqrt(np.median(self.kth_d2(8, 64))))
            self.emit("count_within", n=None if name == "count_targets" else n, radius=radius,
                      cap=5 if name == "count_cap" else None, seed=self.sub(),
                      pose=READ_POSE if name == "count" and self.reads % 2 else None)
        else:  # a poisoned read, and the checked call that has to be right after it
            if name == "poison_query":
                self.emit("poisoned", kind="query", n=READ_POISON_N, seed=self.sub(), iters=2, k=k)
            else:
                radius = float(np.sqrt(np.median(self.kth_d2(8, 64))))
                self.emit("poisoned", kind="count_within", n=READ_POISON_N, seed=self.sub(), iters=2, radius=radius, cap=None)
            self.emit("estimate", n=self.n(), seed=self.sub(), iters=3, r=None)

    def follow(self):
        """after a change of the cloud: the next form of the old rotation or the next two of the new one (the reads are
        cheap), alternately"""
        if self.model.m == 0:
            return
        new = self.new_turn[self.last]
        self.new_turn[self.last] = not new
        if new:
            # the counts around the targets themselves are quadratic in m to restate: once per generator after each kind of
            # change, at the first cloud small enough
            if self.last not in self.targets_done and self.model.m <= self.P["full_max"]:
                self.targets_done.add(self.last)
                self.read("count_targets")
            else:
                self.read()
            self.read()
        else:
            self.check()

    def noops(self, kinds):
        """on a borrowed cloud: removals that remove nothing (an all-ones mask, a huge ratio, a tiny voxel), each followed"""
        for kind in kinds:
            self.removal(kind, "nothing")
            self.follow()

    def stale_removal(self, kind):
        """normals, an append, a removal on the stale cloud, the refused normal call, the update, the normal estimate"""
        if self.model.stale:
            self.normals()
        self.append("incremental", clip=True)
        self.removal(kind, "moving")
        self.emit("normal_estimate", n=self.n(), seed=self.sub(), iters=2, r=None if self.seed % 2 else "half")
        self.normals()
        self.emit("normal_estimate", n=self.n(), seed=self.sub(), iters=3, r="half" if self.seed % 2 else None)

    def empty_removals(self):
        """every removal on the handle another removal has just emptied: nothing to remove, an empty map, statistics of +0.0
        -- with the grid unbuilt (m_full = 0) and the marks' scratch still sized for the old cloud"""
        assert self.model.m == 0
        self.emit("thin", v=0.05)
        self.emit("remove", share=1.0, seed=self.sub(), entry="host", dtype="bool")
        self.emit("remove", share=1.0, seed=self.sub(), entry="device", dtype="uint8")
        self.emit("radius_filter", radius=0.1, need=3)
        self.emit("stat_filter", k=8, ratio=1.0)
        self.emit("crop", center=list(CENTER[self.model.dim]), radius=1.0)
        self.last = "crop"

    def snapshot_query_snapshot(self):
        """a query of n_big points, its lanes forced into cell order, between two snapshot estimates of n_big points"""
        self.emit("estimate", n=self.P["n_big"], seed=self.sub(), iters=3, r=None)
        self.emit("query", n=self.P["n_big"], k=8, seed=self.sub(), pose=READ_POSE, order="cell")
        self.emit("estimate", n=self.P["n_big"], seed=self.sub(), iters=3, r=None)


def _map_first_life(g, dim, v, big_query):
    """create -> [no-op removals on a borrowed cloud] -> a chain of moves (removal, incremental append, removal; for the
    smaller clouds down across the threshold and back up) -> a rebuild -> a removal on stale normals -> the end: everything
    removed, a refused read, an append, a removal down to a handful and a list longer than the cloud (even v), or one more
    removal (odd v) -> close.  Every change of the cloud is followed by a form."""
    P = g.P
    big, by_filter = v % 3 == 0, v in (1, 5)
    # one life's filter starts well above the threshold and leaves a grid a grid (one more quadratic restatement: once)
    stays = v == 1 and dim == 3 and g.key is None
    m = P["m_big"] if big else (P["m_stay"] if stays else P["m_cross"][1 if by_filter else 0])
    g.create(dim, m, True, borrowed=bool(big and g.seed % 2))
    g.follow()
    if g.borrowed:
        g.noops(("remove", "thin"))
    if big:
        first, second = "thin", ("remove", "crop")[v // 3 % 2]
    else:
        first, second = (FILTERS[v // 3 % 2] if by_filter else "thin"), ("crop", "remove")[v % 2]
    g.removal(first, "light" if stays else "moving")
    g.follow()
    g.append("incremental" if big else "up", clip=True)
    g.follow()
    g.removal(second, "moving")
    g.follow()
    if big_query:
        g.snapshot_query_snapshot()
    g.removal({0: "remove", 1: "thin", 2: "remove", 3: "thin", 4: "crop", 5: "thin", 6: "crop"}[v], "rebuild")
    g.follow()
    g.stale_removal({0: "thin", 1: "stat_filter", 2: "radius_filter", 3: "remove", 4: "stat_filter", 5: "radius_filter",
                     6: "thin"}[v])
    g.follow()
    if v % 2 == 0:
        g.removal({0: "remove", 2: "radius_filter", 4: "crop", 6: "remove"}[v], "everything")
        refused = v // 2 % 3  # the read an empty handle refuses
        if refused == 0:
            g.emit("query", n=64, k=8, seed=g.sub(), pose=None)
        elif refused == 1:
            g.emit("neighbours", k=8, first=0, count=None)
        else:
            g.emit("count_within", n=64, radius=0.1, cap=None, seed=g.sub(), pose=None)
        g.empty_removals()
        g.append("grow")
        g.follow()
        g.removal("remove", "handful")
        g.emit("query", n=64, k=(32, 17)[v // 2 % 2], seed=g.sub(), pose=None)
    else:
        g.removal(("thin", "remove", "crop")[v // 2 % 3], "moving")
        g.follow()
    g.emit("close")


def _map_second_life(g, dim, v):
    """the handle that takes the first one's buffers from the pool: borrowed for an even v, with the no-op removals"""
    g.create(dim, g.P["m_second"][g.seed % 3], False, borrowed=v % 2 == 0)
    g.follow()
    if g.borrowed:
        g.noops(("remove", "stat_filter", "thin"))
    g.removal(("radius_filter", "thin", "stat_filter", "remove")[v % 4], "moving")
    g.follow()
    g.append("incremental", clip=True)
    g.follow()
    g.removal(("crop", "radius_filter", "remove", "thin")[v % 4], "rebuild")
    g.follow()
    g.emit("close")


def map_sequence(seed, profile="gpu", dim_start=3):
    """The steps of one random map sequence: like sequence(), with thin, remove (by mask), the two outlier filters,
    neighbours, query and count_within in the mix.  Deterministic: the same arguments give the same list."""
    g = _MapGenerator(seed, profile, dim_start)
    other = dim_start if seed % 2 == 0 else 5 - dim_start
    v = seed + (dim_start == 2)
    _map_first_life(g, dim_start, v, big_query=seed == 0 and dim_start == 3)
    _map_second_life(g, other, v)
    return g.steps


def map_interleaved(seed, profile="gpu"):
    """a 3-D and a 2-D map handle alive together, as interleaved()"""
    gens = []
    for key, dim in ((0, 3), (1, 2)):
        g = _MapGenerator(seed + 200, profile, dim, key=key)
        _map_first_life(g, dim, 2 * seed + key + 1, big_query=False)
        gens.append(g.steps)
    return _shuffled(gens, np.random.default_rng([seed, 78]), profile)


def _first_life(g, dim, m, v):
    """the handle a sequence starts with: changes of the cloud, each followed by the next form of its rotation"""
    g.create(dim, m, True)
    g.check()
    g.append(("incremental", "grow", "outside")[v % 3])
    if v % 2 == 0:
        g.big_and_small()
    g.check()
    g.crop(("moving", "rebuild", "nothing")[v % 3])
    g.check()
    if v % 2:
        g.stale_episode()
    elif v % 4 == 0:
        g.append("outside")
        g.check()
        g.crop("rebuild")
    else:
        g.crop("everything")
        g.append("grow")
        g.check()
        g.crop("moving")
    g.check()
    g.emit("close")


def _second_life(g, dim, m, v):
    """the handle that takes the first one's buffers from the pool"""
    g.create(dim, m, False)
    g.check()
    if v % 2:
        g.append("grow")
    else:
        g.crop("moving")
    g.check()
    g.emit("close")


def sequence(seed, profile="gpu", dim_start=3):
    """The steps of one random sequence: a handle of `dim_start` dimensions created after icp_trim_pool(), taken through
    appends, crops, normals and every kind of call, closed, and a second handle (of the other dimension for an odd
    seed) created from the pool.  Deterministic: the same arguments give the same list."""
    g = _Generator(seed, profile, dim_start)
    P = g.P
    other = dim_start if seed % 2 == 0 else 5 - dim_start
    v = seed + (dim_start == 2)
    _first_life(g, dim_start, P["m_create"][v % 4], v)
    _second_life(g, other, P["m_later"][seed % 3], v)
    return g.steps


def interleaved(seed, profile="gpu"):
    """A 3-D handle (key 0) and a 2-D handle (key 1) alive together: their steps alternate at random, each keeps its
    own order, and a free-function call (the scratch handle) is thrown in between."""
    P = PROFILES[profile]
    gens = []
    for key, dim in ((0, 3), (1, 2)):
        g = _Generator(seed + 100, profile, dim, key=key)
        _first_life(g, dim, P["m_create"][(seed + key + 1) % 4], seed + key + 1)
        gens.append(g.steps)
    return _shuffled(gens, np.random.default_rng([seed, 77]), profile)


def _shuffled(gens, rng, profile):
    """the two handles' steps alternating at random, each list in its own order, free-function calls thrown in"""
    out, at = [], [0, 0]
    while at[0] < len(gens[0]) or at[1] < len(gens[1]):
        left = [len(gens[k]) - at[k] for k in (0, 1)]
        k = int(rng.random() * (left[0] + left[1]) >= left[0])
        out.append(gens[k][at[k]])
        at[k] += 1
        if rng.random() < 0.2:
            out.append({"op": "free_update", "n": (1_000, 3, 65_537 if profile == "gpu" else 700)[len(out) % 3],
                        "seed": int(rng.integers(1, 1 << 30)), "pose": [0.02, 0.01, -0.003]})
    return out


# ------------------------------------------------------------ coverage, from the step lists and the model alone

def form_of(step, stale):
    """the row of the operation table a step exercises, with its gate where the row has both forms"""
    op, r = step["op"], step.get("r")
    gate = "" if r is None else ("_inf" if r == "inf" else "_finite")
    if op == "estimate":
        return "estimate" + gate
    if op == "normal_estimate":
        return "stale_refusal" if stale else "normal_estimate" + gate
    if op == "evaluate":
        return "stale_refusal" if stale and step["kind"] == "normal" else f"evaluate_{step['kind']}{gate}"
    if op == "normals":
        return "normals_update" if step["update"] else "normals_compute"
    if op == "poisoned":
        return "poisoned_" + step["kind"]
    if op == "query":
        return "query_pose" if step.get("pose") is not None else "query"
    if op == "count_within":
        return "count_targets" if step["n"] is None else ("count_cap" if step["cap"] is not None else "count")
    return op


def _append_moves(mo, m_full, step, k):
    """whether an append moves the grid's sorted records (append_grid in nn_grid.hip): True / False where the step decides
    it, None where it hangs on whether every point lies within half a cell of the box"""
    if mo.m == 0 or m_full == 0 or mo.m + k > 1.5 * m_full or tuple(step.get("shift", (0.0, 0.0))) != (0.0, 0.0):
        return False
    return True if step.get("clip") else None


def removal_moves(kept, m_full):
    """whether a removal that removed something moves the grid's sorted records (remove_marked_targets in crop.hip)"""
    return kept > 0 and m_full > 0 and not (kept < m_full / 1.5)


def trace(steps):
    """One record per step, computed by running the Model alone (no reference, no device): its number, its form,
    `after` -- the last change of the cloud in its handle's life ("create", "append", "crop"; for a create, that of the
    life closed before it) --, the target counts before and after, the source size, and whether the normals were stale."""
    models, last, out, m_full, removed = {}, {}, [], {}, {}
    for no, step in enumerate(steps):
        key, op = step.get("h", 0), step["op"]
        mo = models.get(key)
        rec = {"no": no, "h": key, "op": op, "after": last.get(key), "n": step.get("n") if op != "nn_search" else None}
        if op == "free_update":
            rec.update(form=op, n=None)
            out.append(rec)
            continue
        rec.update(m_before=mo.m if mo is not None else 0, stale=mo.stale if mo is not None else True,
                   dim_before=mo.dim if mo is not None else None, normals_m_before=mo.normals_m if mo is not None else 0)
        rec["form"] = form_of(step, rec["stale"])
        rec["removed_before"] = removed.get(key, 0)  # by the last removal, if no append came since
        if op in READS and rec["m_before"] == 0:
            rec["form"] = "read_refused"
        if op == "create":
            mo = models[key] = Model(step["dim"], make_cloud(step["dim"], step["m"], step["seed"], scale=step.get("scale", 1.0)))
            last[key], m_full[key], removed[key] = "create", mo.m, 0
            rec["borrowed"] = bool(step.get("borrowed"))
        elif op == "append":
            pts = appended_points(mo, step)
            rec["moved"] = _append_moves(mo, m_full.get(key, 0), step, len(pts))
            mo.append(pts)
            if rec["moved"] is False:
                m_full[key] = mo.m
            last[key], removed[key] = "append", 0
        elif op in REMOVALS:
            mask = removal_mask(mo.cloud, step)[0]
            kept = int(mask.sum())
            rec["moved"] = removal_moves(kept, m_full[key]) if kept < len(mask) else None  # (None: nothing removed)
            if rec["moved"] is False:
                m_full[key] = kept
            mo.keep_rows(mask)
            last[key], removed[key] = ("filter" if op in FILTERS else op), len(mask) - kept
        elif op == "normals":
            if step["update"] and mo.normals_m > 0 and mo.normals_k != step["k"]:
                rec["form"] = "normals_refused"
            else:
                mo.normals_m, mo.normals_k = mo.m, step["k"]
        elif op == "close":
            mo.alive = False
        rec.update(m=mo.m, dim=mo.dim)
        out.append(rec)
    return out
