"""One handle through every kind of call, in arbitrary order, on the GPU: the sequences of tests/handle_model.py
driven through Icp2d / Icp3d and held, step by step, to the references of the single-call tests.  What is held: a
handle's answer depends on the cloud and the normals it holds, never on how it got there -- appends, crops, thins,
removals by mask, outlier filters, the engine asked for, a reserve, earlier calls and reads, a poisoned call, the previous
owner of its pooled buffers.

A failure prints the seed, the step and the step list up to there; handle_model.run(GpuDevice(), steps[:k]) replays a
prefix.  tests/test_handle_model.py asserts, without a GPU, what these seeds cover and that the checker sees a wrong
device."""
import time

import numpy as np
import pytest

import handle_model as H
import icp_rust_amd as I
import oracle_ffi as O
from icp_rust_amd import _lib
from test_line_abi import lift

pytestmark = pytest.mark.gpu

KTINY_N, KTINY_M, KGRID, KCOOP = 1_024, 2_048, 8_192, 65_536  # kTinyMaxN, kTinyMaxM, kGridMinM, kGridCoopMaxN
KWIN_MIN_N = 4_096  # kWinMinN, and where gn_loop_applies starts: fewer pairs have neither a window nor the one-launch loop


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.set_threads(16)
    yield
    O.set_threads(1)


def _status(call):
    try:
        return _lib.OK, call()
    except I.IcpError as e:
        return e.status, None


class GpuDevice:
    """handle_model's device interface over Icp2d / Icp3d.  Source clouds go in as numpy arrays and as CUDA tensors
    in turn.  Where a counter shows which path served a call, it is asserted here: a sequence does not pass through a
    fallback.  Per estimate call (`log` keeps the figures):
      * single_launch_counters: one launch exactly where the call is ungated, n <= 1 024, m <= 2 048 and the grid is not
        forced; such a call moves no other counter;
      * icp_last_fold_order: a cell-sorted snapshot exactly beyond 65 536 sources on the grid engine;
      * gn_path_counters / gn_loop_counters: the full-key selection, the evaluation's last resort, never runs; below
        4 096 pairs no window is started and no loop launched, and a call that applied an update was served by the short
        pipeline; from 4 096 sources on an ungated call that applied an update was served by a window, the one-launch
        loop (which counts as windows started) or the short pipeline, and launched a loop or placed a bet.  Which of
        these, and whether a window misses or a bet holds, follows from the residuals' statistics and from how the
        handle's previous call (or its previous owner's) ended: no fixed figure can be asserted for them;
      * icp_nn_cert_counters: never moved by a call that takes no snapshot.
    Per change of the cloud:
      * a removal that removed something moves exactly one counter, of its own pair (crop_counters, thin_counters,
        remove_counters, outlier_counters); one that removed nothing moves none and leaves a borrowed tensor borrowed;
      * moved or rebuilt is PREDICTED from `m_full`, the number of targets the grid was last fully built for.  build_grid
        has five callers (icp_rust_amd/csrc): create_common (api.hip); append_common where append_grid did not move the
        records (api_ext.hip; counted as an append that rebuilt); remove_marked_targets where the records were not moved
        (crop.hip, behind all five removals; counted in the removal's "rebuilt" counter); and the two error paths of those
        that put the old cloud back, which a passing sequence never takes.  So m_full is m at create and after every step
        whose "rebuilt" counter moved; reserve, set_nn_mode, the normals, the searches, the estimates and the reads never
        reset it.  A removal moves the records exactly when kept > 0 and kept >= m_full / 1.5; an append exactly when
        m + k <= 1.5 * m_full and every point is within half a cell of the box of the last full build -- asserted where
        the points are inside that box (moved) or beyond it by more than half its largest extent, which no cell exceeds
        (rebuilt).  The counters name the path and the pair; they cannot name which scratch or which second buffer a
        launch used: that is held by the bytes that come back.
    Per read: query_counters moves by one, on the side query_order names (cell order beyond 65 536 points when forced or
    from 250 000 on, and always for the counts around the targets themselves); neighbours moves neither."""

    def __init__(self):
        self.icp = self.tensor = self.original = None
        self.calls = self.m_full = 0
        self.box = None
        self.borrowing = False
        self.changes = []  # (op, moved) per change of the cloud that moved a counter
        # (calls served per path; appends / crops as (records moved, grid rebuilt); gn_path_counters summed as they are)
        self.paths = {"single launch": 0, "general": 0, "snapshot order": 0, "appends": [0, 0], "crops": [0, 0],
                      "certificate searches": 0, "gn paths": [0] * 6, "loop": [0] * 3}
        self.log = []  # one record per estimate call that succeeded

    # -- life
    def create(self, dim, cloud, borrowed=False, trim=False):
        if trim:
            I.lib().icp_trim_pool()
        self.dim, self.mode = dim, "auto"
        cls = I.Icp3d if dim == 3 else I.Icp2d
        self.tensor = self.original = None
        if borrowed:  # the cloud is handed over as a CUDA tensor: borrowed until the first append or crop
            import torch

            self.original = cloud.copy()
            self.tensor = torch.from_numpy(cloud).cuda()
            self.icp = cls(self.tensor)
        else:
            self.icp = cls(cloud)
        self.borrowing = bool(borrowed)
        self._rebuilt(cloud)

    def _rebuilt(self, cloud=None):
        """the grid was fully built for the cloud as it is"""
        cloud = self.icp.read_targets() if cloud is None else cloud
        self.m_full = len(cloud)
        self.box = (cloud.min(axis=0), cloud.max(axis=0)) if len(cloud) else None

    def _still_borrows(self):
        """the handle reads the caller's tensor: a value written there shows in read_targets (and is put back)"""
        import torch

        was = float(self.original[0, 0])
        self.tensor[0, 0] = was + 1.0
        torch.cuda.synchronize()
        seen = self.icp.read_targets(0, 1)[0, 0]
        self.tensor[0, 0] = was
        torch.cuda.synchronize()
        return seen == was + 1.0

    def close(self):
        if self.icp is not None:
            self.icp.close()
        self.icp = self.tensor = None

    def _borrowed_bytes_unchanged(self):
        if self.tensor is not None:
            assert H.same_bits(self.tensor.cpu().numpy(), self.original), "the borrowed tensor was written"

    def _src(self, src):
        self.calls += 1
        if self.calls % 2:
            return src
        import torch

        return torch.from_numpy(src).cuda()

    def resolved(self):
        return I.lib().icp_get_nn_mode(self.icp._h)

    # -- the cloud
    def target_count(self):
        return self.icp.target_count

    def read_targets(self):
        return self.icp.read_targets()

    def append(self, points, T=None):
        before = self.icp.append_counters()
        m_old, k = self.icp.target_count, len(points)
        self.icp.append(points, T)
        after = self.icp.append_counters()
        assert sum(after) == sum(before) + 1, ("append counters", before, after)
        for j in (0, 1):
            self.paths["appends"][j] += after[j] - before[j]
        self._borrowed_bytes_unchanged()
        moved = after[0] == before[0] + 1
        what = ("append", m_old, k, "m_full", self.m_full, "moved", moved)
        if not (m_old > 0 and self.m_full > 0 and m_old + k <= 1.5 * self.m_full):
            assert not moved, what
        elif self.box is not None:
            world = H.moved(points, T) if T is not None else points
            lo, hi = self.box
            reach = 0.5 * float(np.max(hi - lo))
            if np.all(world >= lo) and np.all(world <= hi):
                assert moved, what + ("every point inside the box",)
            elif np.any(world < lo - reach) or np.any(world > hi + reach):
                assert not moved, what + ("a point far outside the box",)
        if not moved:
            self._rebuilt()
        self.borrowing = False
        self.changes.append(("append", moved))

    PAIRS = ("crop", "thin", "remove", "outlier")

    def _removal(self, pair, call):
        """one removal: its own pair of counters moves by one exactly when something was removed, on the side predicted
        from m_full; no other pair moves; a borrowed tensor is never written and stays borrowed when nothing was removed"""
        before = {p: getattr(self.icp, p + "_counters")() for p in self.PAIRS}
        m_old = self.icp.target_count
        out = call()
        removed = out[0]
        after = {p: getattr(self.icp, p + "_counters")() for p in self.PAIRS}
        delta = {p: (after[p][0] - before[p][0], after[p][1] - before[p][1]) for p in self.PAIRS}
        what = (pair, "m", m_old, "removed", removed, "m_full", self.m_full, delta)
        assert all(delta[p] == (0, 0) for p in self.PAIRS if p != pair), ("another pair of counters moved",) + what
        self._borrowed_bytes_unchanged()
        if removed == 0:
            assert delta[pair] == (0, 0), ("nothing removed, a counter moved",) + what
            assert self.icp.target_count == m_old
            if self.borrowing:
                assert self.icp._keep is self.tensor and self._still_borrows(), ("the handle stopped borrowing",) + what
            return out
        kept = m_old - removed
        predicted = H.removal_moves(kept, self.m_full)
        assert delta[pair] == ((1, 0) if predicted else (0, 1)), ("moved or rebuilt", "predicted moved", predicted) + what
        if pair == "crop":
            for j in (0, 1):
                self.paths["crops"][j] += delta[pair][j]
        if not predicted:
            self._rebuilt()
        if self.borrowing:
            assert self.icp._keep is None
        self.borrowing = False
        self.changes.append((pair, predicted))
        return out

    def crop(self, center, radius):
        return self._removal("crop", lambda: self.icp.crop(center, radius, return_index=True))

    def thin(self, v):
        return self._removal("thin", lambda: self.icp.thin(v, return_index=True))

    def remove(self, keep, entry):
        if entry == "device":
            import torch

            keep = torch.from_numpy(keep).cuda()
        return self._removal("remove", lambda: self.icp.remove(keep, return_index=True))

    def radius_filter(self, radius, need):
        return self._removal("outlier", lambda: self.icp.remove_radius_outliers(radius, need, return_index=True))

    def stat_filter(self, k, ratio):
        return self._removal("outlier", lambda: self.icp.remove_statistical_outliers(k, ratio, return_index=True,
                                                                                     return_stats=True))

    # -- the reads through the grid
    def _read(self, side, call):
        """query_counters moves by one on `side` (0: cell order, 1: the caller's; None: by nothing)"""
        before = self.icp.query_counters()
        rc, out = _status(call)
        after = self.icp.query_counters()
        want = [0, 0]
        if rc == _lib.OK and side is not None:
            want[side] = 1
        assert [after[0] - before[0], after[1] - before[1]] == want, ("query counters", before, after, side, rc)
        return rc, out

    @staticmethod
    def _host(a):
        """numpy whatever came back; the device entries hand the indices and counts over as int32 bits"""
        if isinstance(a, np.ndarray):
            return a
        a = a.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a

    def neighbours(self, k, first, count):
        rc, out = self._read(None, lambda: self.icp.neighbours(k, first, count))
        return (rc, None, None) if rc != _lib.OK else (rc,) + out

    def query(self, q, k, T=None, order=None):
        L = I.lib()
        if order is not None:
            _lib.check(L.icp_query_force_order(self.icp._h, 1 if order == "cell" else -1), "icp_query_force_order")
        try:
            cell = order == "cell" and len(q) > KCOOP or (order is None and len(q) >= 250_000)
            rc, out = self._read(0 if cell else 1, lambda: self.icp.query(self._src(q), k, T))
        finally:
            if order is not None:
                L.icp_query_force_order(self.icp._h, 0)
        return (rc, None, None) if rc != _lib.OK else (rc, self._host(out[0]), self._host(out[1]))

    def count_within(self, q, radius, cap=None, T=None):
        if q is None:
            rc, out = self._read(0, lambda: self.icp.count_within(None, radius, cap=cap))
        else:
            rc, out = self._read(0 if len(q) >= 250_000 else 1, lambda: self.icp.count_within(self._src(q), radius, T, cap=cap))
        return rc, (None if rc != _lib.OK else self._host(out))

    def reserve(self, capacity):
        if capacity > self.icp.target_count:
            self.borrowing = False  # (the cloud moves into storage of the handle's own)
        self.icp.reserve(capacity)

    def set_nn_mode(self, mode):
        _lib.check(I.lib().icp_set_nn_mode(self.icp._h, H.MODES[mode]), "icp_set_nn_mode")
        self.mode = mode

    def nn_search(self, q):
        return self.icp.nn_search(q)

    # -- point-to-point
    def last_fold_order(self, n, with_cells=False):
        return self.icp.last_fold_order(n, with_cells=with_cells)

    def _counters(self):
        return (self.icp.single_launch_counters()[0], I.nn_cert_counters(self.icp)[0], I.gn_path_counters(self.icp),
                I.gn_loop_counters(self.icp))

    def estimate(self, src, init, iters, r=None):
        n, m = len(src), self.icp.target_count
        tiny0, certs0, gn0, loop0 = self._counters()
        rc, out = _status(lambda: self.icp.estimate(self._src(src), init, iters, return_info=True,
                                                    max_correspondence_distance=r))
        if rc != _lib.OK:
            return rc, None, None, None, None
        tiny1, certs1, gn1, loop1 = self._counters()
        served, certs = tiny1 - tiny0, certs1 - certs0
        gn, loop = [b - a for a, b in zip(gn0, gn1)], [b - a for a, b in zip(loop0, loop1)]
        tried, missed, short, radix, spec_hit, spec_miss = gn
        T, idx, inner = out[:3]
        applied = int(np.sum(inner))
        pairs = n if r is None else int(np.max(out[3], initial=0))  # (the most pairs an inner loop of the call saw)
        what = dict(n=n, m=m, r=r, mode=self.mode, iters=iters, applied=applied, single_launch=served, gn=gn, loop=loop,
                    certs=certs)
        # one launch serves the ungated call of a small problem on a handle not forced onto the grid (gn_fast.hip)
        small = r is None and 1 <= n <= KTINY_N and 1 <= m <= KTINY_M and self.mode != "grid"
        assert served == (1 if small else 0), ("single-launch path", what)
        self.paths["single launch" if small else "general"] += 1
        # the sums fold in the order of a cell-sorted snapshot exactly beyond kGridCoopMaxN points on the grid engine
        identity = np.array_equal(self.icp.last_fold_order(n), np.arange(n))
        snapshot = n > KCOOP and self.resolved() == I.NN_GRID
        assert identity == (not snapshot), ("fold order", identity, what)
        self.paths["snapshot order"] += int(snapshot)
        what["snapshot"] = snapshot
        if small:  # the whole call was that launch
            assert not any(gn) and not any(loop) and certs == 0, ("a single-launch call moved another counter", what)
        else:
            assert radix == 0, ("the full-key selection ran", what)
            if pairs < KWIN_MIN_N:
                assert tried == 0 and missed == 0 and not any(loop), ("a window or a loop below 4 096 pairs", what)
                if applied:
                    assert short >= 1, ("an update without an evaluation of the short pipeline", what)
            elif r is None:
                if applied:
                    assert tried + short >= 1, ("an update without an evaluation", what)
                # an outer iteration runs its inner loop as ONE launch or, after a loop of exactly one update (this
                # call's, or the one the handle's previous call ended on), bets on the next pose (icp_estimate_device)
                if iters >= 2:
                    assert loop[0] + spec_hit + spec_miss >= 1, ("neither a loop launch nor a bet", what)
        if not snapshot:
            assert certs == 0, ("certificates without a snapshot", what)
        self.paths["certificate searches"] += certs
        self.paths["gn paths"] = [a + b for a, b in zip(self.paths["gn paths"], gn)]
        self.paths["loop"] = [a + b for a, b in zip(self.paths["loop"], loop)]
        self.log.append(what)
        return rc, T.as_array(), idx, inner, (out[3] if r is not None else None)

    def evaluate(self, kind, src, T, r):
        f = self.icp.evaluate if kind == "point" else (
            self.icp.evaluate_point_to_plane if self.dim == 3 else self.icp.evaluate_point_to_line)
        rc, out = _status(lambda: f(self._src(src), T, r, return_indices=True))
        if rc != _lib.OK:
            return rc, len(src), 0, None, None
        q, idx = out
        return rc, q.n, q.inliers, q.as_array(), idx

    # -- normals and the normal residual
    def normals(self, k, update):
        if self.dim == 3:
            f = self.icp.update_normals if update else self.icp.compute_normals
        else:
            f = self.icp.update_line_normals if update else self.icp.compute_line_normals
        return _status(lambda: f(k))[0]

    def read_normals(self):
        rc, out = _status(self.icp.read_normals if self.dim == 3 else self.icp.read_line_normals)
        return rc, (out if self.dim == 3 or out is None else lift(out))

    def estimate_normal(self, src, init, iters, r=None):
        f = self.icp.estimate_point_to_plane if self.dim == 3 else self.icp.estimate_point_to_line
        rc, out = _status(lambda: f(self._src(src), init, iters, return_info=True, max_correspondence_distance=r))
        if rc != _lib.OK:
            return rc, None, None, None, None
        T, idx, inner = out[:3]
        return rc, T.as_array(), idx, inner, (out[3] if r is not None else None)

    def free_update(self, T, a, b):
        return I.weighted_gauss_newton_update(T, a, b)


def run(steps, seed=None, on_step=None):
    """handle_model.run on fresh GpuDevices (one per handle key); whatever happens, the handles are closed"""
    devices = {key: GpuDevice() for key in sorted({s.get("h", 0) for s in steps})}
    t0 = time.perf_counter()
    try:
        H.run(devices if len(devices) > 1 else devices[0], steps, seed=seed, on_step=on_step)
    finally:
        for d in devices.values():
            d.close()
    print(f"{len(steps)} steps in {time.perf_counter() - t0:.1f} s; paths {[d.paths for d in devices.values()]}")
    return devices


# ------------------------------------------------------------------ random sequences

@pytest.mark.parametrize("seed", H.GPU_SEEDS)
@pytest.mark.parametrize("dim_start", H.GPU_DIMS)
def test_random_sequences(dim_start, seed):
    """The first handle is created after icp_trim_pool(), the second takes its buffers from the pool (of the other
    dimension for an odd seed); for an odd seed the first cloud is a borrowed CUDA tensor, whose bytes must be
    unchanged after the first append or crop."""
    steps = H.sequence(seed, "gpu", dim_start)
    creates = [s for s in steps if s["op"] == "create"]
    assert creates[0]["trim"] and not any(s["trim"] for s in creates[1:])
    assert creates[0]["borrowed"] == bool(seed % 2)
    run(steps, seed=seed)


@pytest.mark.parametrize("seed", H.GPU_INTERLEAVED_SEEDS)
def test_two_handles_interleaved(seed):
    """a 3-D and a 2-D handle alive together, their steps alternating at random, each held to its own model; the free
    function weighted_gauss_newton_update (the scratch handle) in between, against the oracle's tree-order update"""
    steps = H.interleaved(seed, "gpu")
    assert {s["op"] for s in steps} >= {"free_update", "create", "append", "crop"}
    run(steps, seed=seed)


@pytest.mark.parametrize("seed", H.GPU_MAP_SEEDS)
@pytest.mark.parametrize("dim_start", H.GPU_DIMS)
def test_random_map_sequences(dim_start, seed):
    """the map sequences: append, crop, thin, remove by mask (host and device entry, bool and uint8) and the two outlier
    filters in one life, each change followed by a form of the old rotation or by reads through the grid (neighbours,
    query, count_within).  GpuDevice asserts the counters of every removal, append and read."""
    steps = H.map_sequence(seed, "gpu", dim_start)
    assert {s["op"] for s in steps} >= {"thin", "remove", "neighbours", "query", "count_within", "append"}
    run(steps, seed=seed)


@pytest.mark.parametrize("seed", H.GPU_MAP_INTERLEAVED_SEEDS)
def test_two_map_handles_interleaved(seed):
    """a 3-D and a 2-D map handle alive together: the marks and counts live in each handle's grid, the query workspace
    is one per device and shared by both"""
    steps = H.map_interleaved(seed, "gpu")
    ops = {s["op"] for s in steps}
    assert ops >= {"free_update", "thin", "remove", "query", "count_within"} and ops & set(H.FILTERS)
    run(steps, seed=seed)


# ------------------------------------------------------------------ scripted sequences: one transition each

def _checks(sub, n=513, normal=True):
    """search, estimate, and (with current normals) the normal estimate and its quality"""
    out = [{"op": "nn_search", "n": 1_500, "seed": sub + 1}, {"op": "estimate", "n": n, "seed": sub + 2, "iters": 3, "r": None}]
    if normal:
        out += [{"op": "normal_estimate", "n": n, "seed": sub + 3, "iters": 3, "r": None},
                {"op": "evaluate", "kind": "normal", "n": n, "seed": sub + 4, "r": "half"}]
    return out


def test_sweep_to_grid_to_sweep():
    """7 000 targets (the sweep), + 2 000 (the grid), cropped back below 8 192 (the sweep again): search, estimate, the
    plane estimate and the plane quality at each stage"""
    steps = ([{"op": "create", "dim": 3, "m": 7_000, "seed": 11, "trim": True}, {"op": "normals", "k": 8, "update": False, "seed": 1}]
             + _checks(100)
             + [{"op": "append", "k": 2_000, "seed": 12, "shift": (0.0, 0.0), "pose": None},
                {"op": "normals", "k": 8, "update": True, "seed": 2}] + _checks(200)
             + [{"op": "crop", "center": [1.0, -1.0], "radius": 3.3}] + _checks(300))
    engines = {}
    device = GpuDevice()

    def on_step(no, step, models):
        engines[no] = (models[0].m, device.resolved())

    try:
        H.run(device, steps, on_step=on_step)
    finally:
        device.close()
    stages = [engines[1], engines[7], engines[12]]
    print("targets and engine per stage", stages)
    assert stages[0] == (7_000, I.NN_BRUTE) and stages[1] == (9_000, I.NN_GRID)
    assert 4_000 < stages[2][0] < KGRID and stages[2][1] == I.NN_BRUTE


def test_tiny_to_snapshot_to_tiny():
    """One 3-D handle: 1 000 source points against 2 000 targets (one launch), 70 000 against the grown cloud (the grid's
    cell-sorted snapshot), then 1 024 (one launch again) and 1 025 (the general path) against the cloud cropped back;
    estimate and its finite gate at each.  GpuDevice.estimate asserts the path of every call."""
    def both(n, sub):
        return [{"op": "estimate", "n": n, "seed": sub, "iters": 3, "r": None},
                {"op": "estimate", "n": n, "seed": sub + 1, "iters": 3, "r": "half"}]

    steps = ([{"op": "create", "dim": 3, "m": 2_000, "seed": 21, "trim": True}] + both(1_000, 30)
             + [{"op": "append", "k": 7_000, "seed": 22, "shift": (0.0, 0.0), "pose": None}] + both(70_000, 40)
             + [{"op": "crop", "center": [1.0, -1.0], "radius": 2.0}] + both(1_024, 50) + both(1_025, 60))
    t = H.trace(steps)
    assert t[3]["m"] == 9_000 and 500 < t[6]["m"] <= KTINY_M
    d = run(steps)[0]
    assert d.paths["single launch"] == 2 and d.paths["snapshot order"] == 2 and d.paths["general"] == 6
    for c in d.log:
        print(c)
    big = [c for c in d.log if c["snapshot"]]
    assert [c["r"] is None for c in big] == [True, False]
    # the snapshot calls are the only ones with 4 096 pairs or more: theirs are all the windows, and they started some
    assert all(c["gn"][0] == 0 and not any(c["loop"]) for c in d.log if not c["snapshot"])
    assert all(c["applied"] >= 1 and c["gn"][0] >= 1 for c in big), big


@pytest.mark.parametrize("dim", [3, 2])
def test_a_normals_life_cycle(dim):
    """compute -> append -> a refused call -> crop (the stale rows stay stale) -> an update with another k (refused) ->
    update -> the normal estimate, ungated and gated, and its quality; plane normals on a 3-D handle, line normals on a
    2-D one"""
    c = list(H.CENTER[dim])
    steps = [{"op": "create", "dim": dim, "m": 6_000, "seed": 31, "trim": True},
             {"op": "normals", "k": 8, "update": False, "seed": 1},
             {"op": "normal_estimate", "n": 1_025, "seed": 32, "iters": 3, "r": None},
             {"op": "append", "k": 1_500, "seed": 33, "shift": (0.0, 0.0), "pose": [0.02, -0.01, 0.005]},
             {"op": "normal_estimate", "n": 513, "seed": 34, "iters": 2, "r": None},
             {"op": "evaluate", "kind": "normal", "n": 513, "seed": 35, "r": "inf"},
             {"op": "crop", "center": c, "radius": 2.9 if dim == 3 else 2.6},
             {"op": "normal_estimate", "n": 513, "seed": 36, "iters": 2, "r": "half"},
             {"op": "normals", "k": 9, "update": True, "seed": 2},
             {"op": "normals", "k": 8, "update": True, "seed": 3},
             {"op": "normal_estimate", "n": 1_025, "seed": 37, "iters": 3, "r": None},
             {"op": "normal_estimate", "n": 1_025, "seed": 38, "iters": 3, "r": "half"},
             {"op": "evaluate", "kind": "normal", "n": 5_000, "seed": 39, "r": "half"},
             {"op": "evaluate", "kind": "normal", "n": 64, "seed": 40, "r": "inf"}]
    t = H.trace(steps)
    assert [r["form"] for r in t].count("stale_refusal") == 3 and t[8]["form"] == "normals_refused"
    crop = t[6]
    assert 0 < crop["normals_m_before"] < crop["m_before"] and 0 < crop["m"] < crop["m_before"]  # stale, and both parts cut
    run(steps)


def test_a_pool_round():
    """A 2-D handle with line normals and a gated line call is closed; a 3-D handle with MORE targets takes the pooled
    buffers and runs compute_normals, a gated plane call and a crop; it is closed, and a 2-D handle follows.  After each
    create read_normals is refused until normals are computed (handle_model checks the state after every create)."""
    steps = [{"op": "create", "dim": 2, "m": 3_000, "seed": 41, "trim": True},
             {"op": "normals", "k": 8, "update": False, "seed": 1},
             {"op": "normal_estimate", "n": 1_025, "seed": 42, "iters": 3, "r": "half"},
             {"op": "close"},
             {"op": "create", "dim": 3, "m": 9_000, "seed": 43},
             {"op": "normal_estimate", "n": 64, "seed": 44, "iters": 1, "r": None},
             {"op": "normals", "k": 10, "update": False, "seed": 2},
             {"op": "normal_estimate", "n": 1_025, "seed": 45, "iters": 3, "r": "half"},
             {"op": "crop", "center": [1.0, -1.0], "radius": 3.0},
             {"op": "normal_estimate", "n": 513, "seed": 46, "iters": 3, "r": None},
             {"op": "close"},
             {"op": "create", "dim": 2, "m": 5_000, "seed": 47},
             {"op": "evaluate", "kind": "normal", "n": 64, "seed": 48, "r": "inf"},
             {"op": "estimate", "n": 1_024, "seed": 49, "iters": 3, "r": None},
             {"op": "normals", "k": 6, "update": False, "seed": 3},
             {"op": "normal_estimate", "n": 513, "seed": 50, "iters": 3, "r": None},
             {"op": "evaluate", "kind": "normal", "n": 513, "seed": 51, "r": "half"}]
    t = H.trace(steps)
    assert [r["form"] for r in t].count("stale_refusal") == 2 and t[4]["m"] > t[0]["m"]
    run(steps)


def test_both_append_paths_and_both_crop_paths_in_one_life():
    """an append inside the grid's box and below 1.5 x its built size (the records move), one beyond the box (rebuilt), a
    crop that keeps more than 1 / 1.5 of the built size (the records move) and one that keeps less (rebuilt):
    append_counters() / crop_counters() confirm which path served each, and search and estimate follow every one"""
    def after(sub):
        return [{"op": "nn_search", "n": 1_500, "seed": sub}, {"op": "estimate", "n": 5_000, "seed": sub + 1, "iters": 3, "r": None}]

    steps = ([{"op": "create", "dim": 3, "m": 24_000, "seed": 61, "trim": True}]
             + [{"op": "append", "k": 3_000, "seed": 62, "shift": (0.0, 0.0), "pose": None}] + after(70)
             + [{"op": "append", "k": 3_000, "seed": 63, "shift": (1.5, -0.75), "pose": None}] + after(80)
             + [{"op": "crop", "center": [1.0, -1.0], "radius": 4.2}] + after(90)
             + [{"op": "crop", "center": [1.0, -1.0], "radius": 2.4}] + after(100))
    t = H.trace(steps)
    assert t[7]["m"] > t[7]["m_before"] / 1.5 and t[7]["m"] < t[7]["m_before"] and KGRID < t[10]["m"] < 30_000 / 1.5
    seen = {}
    device = GpuDevice()

    def on_step(no, step, models):
        if step["op"] in ("append", "crop"):
            seen[no] = (device.icp.append_counters(), device.icp.crop_counters())

    try:
        H.run(device, steps, on_step=on_step)
    finally:
        device.close()
    print("counters after each change of the cloud", seen)
    assert seen[1] == ((1, 0), (0, 0)) and seen[4] == ((1, 1), (0, 0))
    assert seen[7] == ((1, 1), (1, 0)) and seen[10] == ((1, 1), (1, 1))


def test_four_moves_the_rebuild_m_full_forces_a_filter_back_to_the_sweep_and_a_cell_ordered_query():
    """One 3-D life.  24 000 targets; a thin, an incremental append and two removals by mask each move the grid's records
    (m_full stays 24 000); a third mask keeps 85 % -- more than 1 / 1.5 of the cloud it is applied to, less than
    24 000 / 1.5 -- and so rebuilds; a fourth takes the cloud to about 8 400 (still the grid); a query of 70 000 points
    forced into cell order sits between two snapshot estimates of 70 000 points; the statistical filter takes the handle
    back below 8 192 (the sweep: build_target_soa / build_target_screen), and an estimate and a query follow."""
    mask = dict(op="remove", entry="host", dtype="bool")
    pose = [0.03, -0.02, 0.01]
    steps = [{"op": "create", "dim": 3, "m": 24_000, "seed": 81, "trim": True},
             {"op": "thin", "v": H.thin_size(H.make_cloud(3, 24_000, 81), 0.88)},
             {"op": "nn_search", "n": 1_500, "seed": 82},
             {"op": "append", "k": 2_600, "seed": 83, "shift": (0.0, 0.0), "pose": None, "clip": True},
             {"op": "query", "n": 2_000, "k": 16, "seed": 84, "pose": None},
             dict(mask, share=0.88, seed=85),
             {"op": "estimate", "n": 5_000, "seed": 86, "iters": 3, "r": None},
             dict(mask, share=0.88, seed=87, entry="device", dtype="uint8"),
             {"op": "count_within", "n": 513, "radius": 0.05, "cap": 5, "seed": 88, "pose": pose},
             dict(mask, share=0.85, seed=89, dtype="uint8"),
             {"op": "neighbours", "k": 17, "first": 7_000, "count": 1_024},
             dict(mask, share=0.54, seed=90, entry="device"),
             {"op": "estimate", "n": 70_000, "seed": 91, "iters": 3, "r": None},
             {"op": "query", "n": 70_000, "k": 8, "seed": 92, "pose": pose, "order": "cell"},
             {"op": "estimate", "n": 70_000, "seed": 93, "iters": 3, "r": None},
             {"op": "stat_filter", "k": 8, "ratio": 1.0},
             {"op": "estimate", "n": 513, "seed": 94, "iters": 3, "r": None},
             {"op": "query", "n": 65, "k": 32, "seed": 95, "pose": pose}]
    t = H.trace(steps)
    assert [t[k]["moved"] for k in (1, 3, 5, 7, 9, 11, 15)] == [True, True, True, True, False, False, True]
    forced = t[9]
    assert forced["m"] >= forced["m_before"] / 1.5 and forced["m"] < 24_000 / 1.5  # m_full, not the cloud it cut
    assert KGRID <= t[11]["m"] < 9_000 and 0 < t[15]["m"] < KGRID
    seen, engines = {}, {}
    device = GpuDevice()

    def on_step(no, step, models):
        engines[no] = device.resolved()
        if step["op"] in H.REMOVALS + ("append",):
            seen[no] = (device.icp.append_counters(), device.icp.thin_counters(), device.icp.remove_counters(),
                        device.icp.outlier_counters(), device.icp.crop_counters())

    try:
        H.run(device, steps, on_step=on_step)
        queries = device.icp.query_counters()
    finally:
        device.close()
    print("counters after each change of the cloud", seen, "query counters (cell order, caller's order)", queries)
    # in cell order: the forced query of 70 000; in the caller's: the queries of 2 000 and 65, the counts of 513, and the
    # 70 000 again, forced the other way
    assert queries == (1, 4)
    assert seen[1] == ((0, 0), (1, 0), (0, 0), (0, 0), (0, 0)) and seen[3] == ((1, 0), (1, 0), (0, 0), (0, 0), (0, 0))
    assert seen[5][2] == (1, 0) and seen[7][2] == (2, 0) and seen[9][2] == (2, 1) and seen[11][2] == (2, 2)
    assert seen[15] == ((1, 0), (1, 0), (2, 2), (1, 0), (0, 0))
    assert engines[14] == I.NN_GRID and engines[15] == engines[17] == I.NN_BRUTE
    snapshots = [c for c in device.log if c["snapshot"]]
    assert [c["n"] for c in snapshots] == [70_000, 70_000]  # the estimates on both sides of the cell-ordered query


def restated_search_plan(cloud, src, iters):
    """Which kernel each search of an ungated estimate from the identity takes on a snapshot of `src`, for a handle whose
    grid was built on `cloud`: the poses from the oracle one iteration at a time, the fixed-point exit of
    icp_estimate_device (an iteration that applies nothing and leaves the pose goes straight to the last one), and
    test_gpu_nn_blind._cert_plan's restatement of launch_nn_grid ("cert": a search that checked certificates)."""
    from test_gpu_nn_blind import _cert_plan

    dim, n = cloud.shape[1], len(src)
    blocks, threads = I.reduce_geometry(n)
    poses, k = [I.Transform()], 1
    while k < iters:
        rc, T, _, inner = O.icp_estimate(dim, cloud, src, O.transform_identity(), k, use_kdtree=True, sum_mode=1,
                                         reduce_blocks=blocks, reduce_threads=threads)
        assert rc == O.OK
        T = I.Transform.from_pose(I.Pose(*[float(x) for x in T.as_array()]))
        if inner[-1] == 0 and k + 1 < iters and H.same_bits(T.as_array(), poses[-1].as_array()):
            poses.append(T)  # the last iteration's search, at the same pose
            break
        poses.append(T)
        k += 1
    return _cert_plan(cloud, poses)


def test_certified_searches_on_a_pooled_handle():
    """The certificates of a snapshot (`qsort.d_cert_lists`, previous matches, decay) through a handle that has had
    another owner and other calls.  A search checks certificates only as the third of one snapshot whose last two steps
    were at most a hundredth of a cell: three iterations from 3 cm off never get there (the random sequences), a room in
    millimetres registered for ten iterations does -- its last updates are microns.  A 2-D handle takes a snapshot and is
    closed; a 3-D handle takes its buffers, runs a small call, the long one (certificates asserted from the restated
    plan), a small one, a second long one on another scan; every call equals the oracle in the device's order."""
    long_call = {"op": "estimate", "n": 70_000, "iters": 10, "r": None, "sigma": 4.0, "pose": [30.0, -20.0, 0.01]}
    steps = [{"op": "create", "dim": 2, "m": 9_000, "seed": 71, "trim": True},
             {"op": "estimate", "n": 70_000, "seed": 72, "iters": 3, "r": None},
             {"op": "close"},
             {"op": "create", "dim": 3, "m": 9_000, "seed": 43, "scale": 1000.0},
             {"op": "estimate", "n": 513, "seed": 73, "iters": 3, "r": None, "sigma": 4.0, "pose": [30.0, -20.0, 0.01]},
             dict(long_call, seed=101),
             {"op": "estimate", "n": 1_024, "seed": 74, "iters": 3, "r": None, "sigma": 4.0, "pose": [30.0, -20.0, 0.01]},
             dict(long_call, seed=102)]
    cloud = H.make_cloud(3, 9_000, 43, scale=1000.0)
    plans = [restated_search_plan(cloud, H.make_scan(cloud, 70_000, seed, 4.0, [30.0, -20.0, 0.01]), 10) for seed in (101, 102)]
    print(plans)
    assert all(p[0] == "seeded" and "leave" in p and "cert" in p for p in plans)
    d = run(steps)[0]
    for c in d.log:
        print(c)
    first_owner, small_a, long_a, small_b, long_b = d.log
    assert first_owner["snapshot"] and first_owner["certs"] == 0  # (three iterations: the steps are too long)
    for c, plan in ((long_a, plans[0]), (long_b, plans[1])):
        assert c["snapshot"] and c["applied"] >= 3
        assert c["certs"] >= 1, ("no search checked certificates", plan, c)
        assert c["gn"][0] >= 1, ("no window and no loop", c)
    assert small_a["certs"] == small_b["certs"] == 0
