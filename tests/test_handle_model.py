"""The model, the generator and the checker of the sequence tests (tests/handle_model.py), without a GPU: the generator
is deterministic; over the exact seeds tests/test_gpu_sequences.py runs, the coverage conditions hold; the checker
passes a stand-in built from the references themselves and catches five sabotaged ones at the first step where each
fault can be seen.  The same again for the map sequences (thin, remove by mask, the two outlier filters, neighbours,
query, count_within): the older lists are pinned by digest, the map sequences have coverage conditions of their own, the
stand-in passes four reduced ones and an interleaved one, and five more sabotaged stand-ins are caught.  This is the
only place faults are injected -- into a numpy stand-in, never into the library."""
import collections

import numpy as np
import pytest

import handle_model as H
import oracle_ffi as O

KGRID, KCOOP, KTINY_N = 8_192, 65_536, 1_024  # kGridMinM, kGridCoopMaxN, kTinyMaxN of icp_rust_amd/csrc


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.set_threads(16)
    yield
    O.set_threads(1)


def gpu_lists():
    return ([H.sequence(s, "gpu", d) for d in H.GPU_DIMS for s in H.GPU_SEEDS] +
            [H.interleaved(s, "gpu") for s in H.GPU_INTERLEAVED_SEEDS])


@pytest.fixture(scope="module")
def traces():
    return [H.trace(steps) for steps in gpu_lists()]


# ------------------------------------------------------------------ the generator

def test_the_same_seed_gives_the_same_list_and_another_seed_another():
    for profile in ("gpu", "cpu"):
        assert H.sequence(3, profile, 2) == H.sequence(3, profile, 2)
        assert H.interleaved(1, profile) == H.interleaved(1, profile)
        assert H.sequence(3, profile, 2) != H.sequence(4, profile, 2)
        assert H.sequence(3, profile, 2) != H.sequence(3, profile, 3)
    # plain data: the list survives being printed as a literal and read back
    steps = H.sequence(5, "gpu", 3)
    assert eval(repr(steps)) == steps


def test_sizes_sit_at_the_thresholds(traces):
    ms = {r["m"] for t in traces for r in t if r["op"] in ("create", "append", "crop")}
    assert any(0 < m < 2_048 for m in ms) and any(2_048 < m < KGRID for m in ms)
    assert any(KGRID <= m < 9_200 for m in ms) and any(7_000 <= m < KGRID for m in ms)
    assert any(20_000 <= m <= 30_000 for m in ms) and max(ms) <= 30_000
    ns = {r["n"] for t in traces for r in t if r.get("n")}
    assert {1, 2, 63, 64, 65, 511, 512, 513, 1_024, 1_025, 5_000, 70_000} <= ns
    # the one size above kGridCoopMaxN: estimate and its gate only
    assert {r["form"] for t in traces for r in t if (r.get("n") or 0) > KCOOP} == {"estimate", "estimate_finite"}
    crops = [r for t in traces for r in t if r["op"] == "crop"]
    assert any(r["m"] == r["m_before"] for r in crops)                         # one removes nothing
    assert any(r["m"] == 0 for r in crops)                                     # one removes everything ...
    for t in traces:
        for a, b in zip(t, t[1:]):
            if a["op"] == "crop" and a["m"] == 0:                              # ... and is followed by an append
                nxt = next(r for r in t[a["no"] + 1:] if r["h"] == a["h"])
                assert nxt["op"] == "append"
    assert any(r["m"] > r["m_before"] / 1.5 and r["m"] < r["m_before"] for r in crops)
    assert any(0 < r["m"] < r["m_before"] / 1.5 for r in crops)
    appends = [s for steps in gpu_lists() for s in steps if s["op"] == "append"]
    assert any(s["shift"] != (0.0, 0.0) for s in appends) and any(s["shift"] == (0.0, 0.0) for s in appends)
    assert any(s["pose"] is not None for s in appends) and any(s["pose"] is None for s in appends)


# the rows of the operation table, as the forms handle_model.form_of names them
ROWS = {
    "nn_search": ["nn_search"],
    "estimate": ["estimate"],
    "gated estimate": ["estimate_finite", "estimate_inf"],
    "compute normals": ["normals_compute"],
    "update normals": ["normals_update"],
    "normal estimate": ["normal_estimate", "normal_estimate_finite", "normal_estimate_inf"],
    "evaluate": ["evaluate_point_inf", "evaluate_point_finite"],
    "evaluate normal": ["evaluate_normal_inf", "evaluate_normal_finite"],
    "append": ["append"], "crop": ["crop"], "reserve": ["reserve"], "set_nn_mode": ["set_nn_mode"],
    "poisoned estimate": ["poisoned_estimate", "poisoned_gated"],
    "poisoned normal estimate": ["poisoned_normal"],
    "poisoned quality": ["poisoned_evaluate", "poisoned_evaluate_normal"],
    "close and create": ["close", "create"],
}


def test_every_operation_occurs_five_times_and_every_form_after_an_append_and_after_a_crop(traces):
    total, after = collections.Counter(), collections.defaultdict(set)
    for t in traces:
        for r in t:
            total[r["form"]] += 1
            after[r["form"]].add(r["after"])
    for row, forms in ROWS.items():
        assert sum(total[f] for f in forms) >= 5, (row, {f: total[f] for f in forms})
        for f in forms:
            if f in ("append", "crop", "create"):
                # an append after a crop, a crop after an append; a create follows a close, which is held to both
                want = {"append": {"crop"}, "crop": {"append"}, "create": set()}[f]
            else:
                want = {"append", "crop"}
            assert want <= after[f], (row, f, after[f])
    print({f: total[f] for forms in ROWS.values() for f in forms}, "steps", sum(len(t) for t in traces))


def by_handle(t):
    out = collections.defaultdict(list)
    for r in t:
        if r["form"] != "free_update":
            out[r["h"]].append(r)
    return out.values()


def test_every_transition_occurs_twice(traces):
    c = collections.Counter()
    for t in traces:
        for recs in by_handle(t):
            sources = []
            for r, nxt in zip(recs, recs[1:] + [None]):
                if r["op"] == "append" and r["m_before"] < KGRID <= r["m"]:
                    c["up"] += 1
                if r["op"] == "crop" and r["m_before"] >= KGRID > r["m"] > 0:
                    c["down"] += 1
                if r["form"] == "stale_refusal":
                    c["stale refusal"] += 1
                if r["form"] == "normals_refused":  # an update with another k: refused, and nothing changes
                    c["update with another k"] += 1
                if r["op"] == "crop" and 0 < r["normals_m_before"] < r["m_before"]:
                    c["crop on stale normals"] += 1
                if r["op"] == "create" and r["dim_before"] not in (None, r["dim"]):
                    c["dimension change"] += 1
                if r["op"] == "poisoned" and nxt is not None and nxt["op"] in ("estimate", "normal_estimate"):
                    c["poisoned then checked"] += 1
                if r["op"] in ("create", "close"):
                    sources = []
                if r.get("n"):
                    if sources and sources[-1] > KCOOP and r["n"] <= KTINY_N:
                        c["small after big"] += 1
                    if sources and sources[-1] <= KTINY_N and r["n"] > KCOOP:
                        c["big after small"] += 1
                    sources.append(r["n"])
    print(dict(c))
    for what in ("up", "down", "small after big", "big after small", "stale refusal", "update with another k", "crop on stale normals",
                 "dimension change", "poisoned then checked"):
        assert c[what] >= 2, (what, dict(c))


# ------------------------------------------------------------------ the checker and a right device

CPU_RUNS = [(3, 0), (2, 1), (3, 2), (2, 3)]


@pytest.mark.parametrize("dim,seed", CPU_RUNS)
def test_the_stand_in_built_from_the_references_passes(dim, seed):
    steps = H.sequence(seed, "cpu", dim)
    t = H.trace(steps)
    assert max(r["m"] for r in t) <= 3_000 and max(r.get("n") or 0 for r in t) <= 1_200
    H.run(H.ReferenceDevice(), steps, seed=seed)


def test_two_stand_ins_interleaved_pass():
    steps = H.interleaved(0, "cpu")
    assert {s.get("h") for s in steps} == {0, 1, None}
    H.run({0: H.ReferenceDevice(), 1: H.ReferenceDevice()}, steps, seed=0)


def test_a_failure_names_the_seed_the_step_and_the_prefix_and_the_prefix_replays():
    steps = H.sequence(0, "cpu", 3)

    class Forgetful(H.ReferenceDevice):
        def target_count(self):
            return self.model.m - (1 if self.model.m > 1_400 else 0)

    with pytest.raises(H.SequenceFailure) as e:
        H.run(Forgetful(), steps, seed=0)
    f = e.value
    assert f.seed == 0 and f.prefix == steps[:f.step + 1] and "target_count" in f.what
    assert f"seed 0, step {f.step}" in str(f) and "steps = [" in str(f)
    literal = str(f).split("steps = ", 1)[1]
    assert eval(literal) == f.prefix  # the list in the message is a Python literal
    H.run(Forgetful(), steps[:f.step], seed=0)  # the prefix before the failing step passes
    with pytest.raises(H.SequenceFailure) as again:
        H.run(Forgetful(), f.prefix, seed=0)
    assert again.value.step == f.step


# ------------------------------------------------------------------ the checker and five wrong devices

class CropKeepsTheFirstNormals(H.Model):
    def carried(self, mask):
        return self.normals[:int(mask.sum())]


class NormalsOfTheFirstRows(H.ReferenceDevice):
    model_cls = CropKeepsTheFirstNormals


class AppendUnseenBySearch(H.ReferenceDevice):
    def searched_cloud(self):
        return self.model.cloud[:self.model.m - self.last_block]

    def crop(self, center, radius):
        self.last_block = 0
        return super().crop(center, radius)


class CreateInheritsNormals(H.ReferenceDevice):
    def new_model(self, dim, cloud):
        new, old = H.Model(dim, cloud), self.model
        if old is not None and not old.stale:
            new.normals, new.normals_m, new.normals_k = np.resize(old.normals, (new.m, 3)), new.m, old.normals_k
        return new


class GateFoldsInIndexOrder(H.ReferenceDevice):
    def gated_fold(self, perm):
        return np.sort(perm)


class RepeatsIndicesAfterPoison(H.ReferenceDevice):
    def indices(self, idx):
        if self.after_poison and self.prev_idx is not None:
            idx = np.resize(self.prev_idx, len(idx))
        return super().indices(idx)


def first(t, pred):
    return next(r["no"] for r in t if pred(r))


def failing_step(device, steps):
    with pytest.raises(H.SequenceFailure) as e:
        H.run(device, steps)
    print(e.value.step, e.value.what[:200])
    return e.value.step


def scan_for(pred, what, make=H.sequence):
    """the first reduced sequence whose trace has a step for the fault to show at"""
    for dim, seed in CPU_RUNS + [(d, s) for s in range(4, 12) for d in (3, 2)]:
        steps = make(seed, "cpu", dim)
        t = H.trace(steps)
        if any(pred(r, t) for r in t):
            return steps, t, first(t, lambda r: pred(r, t))
    raise AssertionError(f"no reduced sequence shows {what}")


def test_a_crop_that_keeps_the_normals_of_the_first_rows_is_caught_at_that_crop():
    # seen where the normals are current (read back right after the crop) and a row in front of a kept one goes
    steps, t, want = scan_for(lambda r, t: r["op"] == "crop" and not r["stale"] and 0 < r["m"] < r["m_before"], "it")
    assert failing_step(NormalsOfTheFirstRows(), steps) == want


def test_an_append_the_next_search_does_not_see_is_caught_at_that_search():
    steps, t, want = scan_for(lambda r, t: r["form"] == "nn_search" and t[r["no"] - 1]["op"] == "append", "it")
    assert failing_step(AppendUnseenBySearch(), steps) == want


def test_a_created_handle_that_inherits_normals_is_caught_at_the_create():
    def pred(r, t):
        return r["op"] == "create" and r["no"] > 0 and not t[r["no"] - 1]["stale"] and t[r["no"] - 1]["op"] == "close"

    steps, t, want = scan_for(pred, "a handle closed with current normals")
    assert failing_step(CreateInheritsNormals(), steps) == want


def test_a_gate_that_folds_in_index_order_is_caught_at_the_first_gated_estimate_with_a_fold_order_of_its_own():
    steps, t, want = scan_for(lambda r, t: r["form"] in ("estimate_finite", "estimate_inf") and r["n"] >= 63, "it")
    n = t[want]["n"]

    def perm_of(k):
        """a cell-sorted order for the sources of that step, the caller's order for every other size"""
        cell = ((np.arange(k) * 7919) % 13).astype(np.uint32) if k == n else np.zeros(k, dtype=np.uint32)
        perm = np.argsort(cell, kind="stable").astype(np.int64)
        return perm, cell[perm]

    assert not np.array_equal(perm_of(n)[0], np.arange(n))
    H.run(H.ReferenceDevice(perm_of), steps)  # a right device with that fold order passes
    assert failing_step(GateFoldsInIndexOrder(perm_of), steps) == want


def test_a_call_that_repeats_the_indices_from_before_a_poisoned_call_is_caught_right_after_it():
    def pred(r, t):
        seen = any(p["op"] in ("estimate", "normal_estimate", "evaluate") and p["form"] != "stale_refusal" for p in t[:r["no"]])
        return r["op"] == "poisoned" and r["form"] != "poisoned_gated" and seen

    steps, t, poisoned = scan_for(pred, "a poisoned call behind a call that returned indices")
    assert t[poisoned + 1]["op"] in ("estimate", "normal_estimate")
    assert failing_step(RepeatsIndicesAfterPoison(), steps) == poisoned + 1


# ------------------------------------------------------------------ the old lists are the old lists

# sha256(repr(steps))[:16] of every list the older tests run, computed before the generator learnt the map sequences
DIGESTS = {
    ("sequence", 0, "gpu", 3): "ed6c41e1772c4abf", ("sequence", 1, "gpu", 3): "3b3dab612db389cb",
    ("sequence", 2, "gpu", 3): "98e24e4f2c810de1", ("sequence", 3, "gpu", 3): "8967759b624e1e52",
    ("sequence", 4, "gpu", 3): "761c0640ef8bad44", ("sequence", 5, "gpu", 3): "4c990a545074b27a",
    ("sequence", 0, "gpu", 2): "c8dd8b17aeb03984", ("sequence", 1, "gpu", 2): "37f9031b0eec73a3",
    ("sequence", 2, "gpu", 2): "2315614c45455931", ("sequence", 3, "gpu", 2): "e0192c71a54799b0",
    ("sequence", 4, "gpu", 2): "b37b64d8bc89d4f9", ("sequence", 5, "gpu", 2): "ef30634d5abce910",
    ("interleaved", 0, "gpu"): "0f07248829a21f32", ("interleaved", 1, "gpu"): "288f4ba5a5911670",
    ("interleaved", 2, "gpu"): "dd94512dc581009b",
    ("sequence", 0, "cpu", 3): "1cf4435dadc02b52", ("sequence", 1, "cpu", 2): "886675d9828377b2",
    ("sequence", 2, "cpu", 3): "179aa15fd9f6bdab", ("sequence", 3, "cpu", 2): "d6172159173309e0",
    ("interleaved", 0, "cpu"): "976305a5d077d3e5",
}


def test_sequence_and_interleaved_return_the_lists_they_returned_before_the_map_sequences():
    import hashlib

    wanted = ({("sequence", s, "gpu", d) for d in H.GPU_DIMS for s in H.GPU_SEEDS}
              | {("interleaved", s, "gpu") for s in H.GPU_INTERLEAVED_SEEDS}
              | {("sequence", s, "cpu", d) for d, s in CPU_RUNS} | {("interleaved", 0, "cpu")})
    assert wanted == set(DIGESTS)
    for key, want in DIGESTS.items():
        steps = H.sequence(key[1], key[2], key[3]) if key[0] == "sequence" else H.interleaved(key[1], key[2])
        assert hashlib.sha256(repr(steps).encode()).hexdigest()[:16] == want, key


# ------------------------------------------------------------------ the map sequences: coverage

NEW_OPS = ("thin", "remove", "radius_filter", "stat_filter", "neighbours", "query", "count_within")
READ_FORMS = ("neighbours", "query", "query_pose", "count", "count_cap", "count_targets")
CHANGES = ("create", "append") + H.REMOVALS
AFTER_REMOVAL = ("crop", "thin", "remove", "filter")


def map_lists():
    return ([H.map_sequence(s, "gpu", d) for d in H.GPU_DIMS for s in H.GPU_MAP_SEEDS] +
            [H.map_interleaved(s, "gpu") for s in H.GPU_MAP_INTERLEAVED_SEEDS])


@pytest.fixture(scope="module")
def map_traces():
    """(steps, trace) of every map sequence tests/test_gpu_sequences.py runs"""
    return [(steps, H.trace(steps)) for steps in map_lists()]


def handles(steps, t):
    """per handle of a list: its (step, record) pairs in order"""
    out = collections.defaultdict(list)
    for s, r in zip(steps, t):
        if r["form"] != "free_update":
            out[r["h"]].append((s, r))
    return list(out.values())


def test_map_sequences_are_deterministic_plain_data():
    assert H.map_sequence(2, "cpu", 3) == H.map_sequence(2, "cpu", 3)
    assert H.map_sequence(2, "cpu", 3) != H.map_sequence(2, "cpu", 2)
    assert H.map_interleaved(1, "cpu") == H.map_interleaved(1, "cpu")
    steps = H.map_sequence(1, "cpu", 2)
    assert eval(repr(steps)) == steps


def test_every_new_operation_occurs_five_times_and_every_read_form_after_every_kind_of_change(map_traces):
    total, after = collections.Counter(), collections.defaultdict(set)
    for steps, t in map_traces:
        for r in t:
            total[r["op"]] += 1
            after[r["form"]].add(r["after"])
    print(dict(total), {f: sorted(after[f]) for f in READ_FORMS})
    for op in NEW_OPS:
        assert total[op] >= 5, (op, total[op])
    for f in READ_FORMS:
        assert {"append", "crop", "thin", "remove", "filter"} <= after[f], (f, after[f])
    assert total["append"] >= 5 and total["crop"] >= 5
    for f in ("poisoned_query", "poisoned_count_within"):
        assert after[f], f


def test_list_lengths_query_sizes_and_where_the_quadratic_restatements_stop(map_traces):
    ks, sizes, padded, big = set(), set(), 0, []
    for steps, t in map_traces:
        for s, r in zip(steps, t):
            if r["op"] in ("neighbours", "query"):
                ks.add(s["k"])
                if s["k"] > r["m_before"] > 0 and r["after"] in AFTER_REMOVAL:
                    assert r["m_before"] <= 12
                    padded += 1
            if r["op"] in ("query", "count_within") and s["n"] is not None:
                sizes.add(s["n"])
            # the filters up to 12 000 targets only; the full-range lists and the counts around the targets themselves up to
            # the profile's lower limit
            if r["op"] in H.FILTERS:
                assert r["m_before"] <= H.QUADRATIC_MAX_M, (s, r["m_before"])
            if (r["op"] == "neighbours" and s["count"] is None) or r["form"] == "count_targets":
                assert r["m_before"] <= H.PROFILES["gpu"]["full_max"] <= H.QUADRATIC_MAX_M, (s, r["m_before"])
            if r["op"] == "neighbours" and s["count"] is not None:
                assert s["count"] == H.SUB_ROWS <= 1_024 and s["first"] + s["count"] <= r["m_before"]
                big.append((s["first"], s["first"] + s["count"] == r["m_before"]))
            if r["op"] in ("thin", "remove") and r["m_before"] >= 20_000:
                big.append(r["op"])
    assert {1, 8, 16, 17, 32} <= ks and padded >= 1
    assert {1, 63, 64, 65, 2_000} <= sizes
    assert "thin" in big and "remove" in big  # thin and remove at 20-30 k
    ranges = [b for b in big if isinstance(b, tuple)]
    assert any(f == 0 for f, _ in ranges) and any(end for _, end in ranges) and any(f > 0 and not end for f, end in ranges)
    filters = [r for steps, t in map_traces for r in t if r["op"] in H.FILTERS]
    assert any(r["m_before"] >= KGRID for r in filters) and any(0 < r["m_before"] < KGRID for r in filters)
    # ... and one on a grid well above the threshold that removes something and leaves a grid
    assert any(r["m_before"] >= 9_000 and KGRID <= r["m"] < r["m_before"] for r in filters)


def test_every_map_transition_occurs_twice(map_traces):
    c = collections.Counter()
    for steps, t in map_traces:
        for pairs in handles(steps, t):
            recs = [r for _, r in pairs]
            # the changes of the cloud, each with whether a read or an estimate came before the next change
            changes = []
            for s, r in pairs:
                if r["op"] in CHANGES:
                    changes.append([s, r, False])
                elif changes and r["op"] in H.READS + ("nn_search", "estimate", "normal_estimate", "evaluate"):
                    changes[-1][2] = True
            for a, b, d in zip(changes, changes[1:], changes[2:]):
                if (a[1]["op"] in H.REMOVALS and a[1]["moved"] is True and b[1]["op"] == "append" and b[1]["moved"] is True
                        and d[1]["op"] in H.REMOVALS and d[1]["moved"] is True and a[2] and b[2] and d[2]):
                    c["moved removal, incremental append, moved removal"] += 1
            borrowed = False
            for at, (s, r) in enumerate(pairs):
                nxt = recs[at + 1:at + 4]
                op = r["op"]
                if op == "create":
                    borrowed = r["borrowed"]
                    if r["dim_before"] not in (None, r["dim"]) and recs[at - 1]["op"] == "close" and \
                            recs[at - 1]["after"] in AFTER_REMOVAL:
                        c["close after a removal, create of the other dimension"] += 1
                if op in H.REMOVALS and op != "crop" and 0 < r["normals_m_before"] < r["m_before"] and len(nxt) == 3 and \
                        nxt[0]["form"] == "stale_refusal" and nxt[1]["form"] == "normals_update" and \
                        nxt[2]["form"].startswith("normal_estimate"):
                    c[op + " on stale normals"] += 1
                if op in H.REMOVALS and r["m_before"] >= KGRID > r["m"] > 0:
                    c["down by " + ("a filter" if op in H.FILTERS else op)] += 1
                if op == "append" and r["m_before"] < KGRID <= r["m"]:
                    c["up by an append"] += 1
                if op in H.REMOVALS and borrowed and r["m"] == r["m_before"] > 0:
                    what = {"remove": "all-ones mask", "stat_filter": "huge ratio", "thin": "tiny voxel"}.get(op)
                    assert op != "remove" or s["share"] == 1.0
                    assert op != "stat_filter" or s["ratio"] == "inf"
                    c[f"nothing removed on a borrowed cloud: {what}"] += 1
                if op in H.REMOVALS and r["m"] == 0 < r["m_before"] and len(nxt) >= 2 and nxt[0]["form"] == "read_refused":
                    # (the removals on the emptied handle come in between)
                    rest = [x for x in recs[at + 2:] if not (x["op"] in H.REMOVALS and x["m_before"] == 0)]
                    if rest and rest[0]["op"] == "append":
                        c["everything removed, a refused read, an append"] += 1
                if op in H.REMOVALS and r["m_before"] == 0:
                    assert r["m"] == 0 and r["after"] in AFTER_REMOVAL
                    c["on an empty handle: " + (op if op != "remove" else f"remove {s['entry']}")] += 1
                if op == "remove":
                    c[f"mask {s['entry']} {s['dtype']}"] += 1
                    if s["dtype"] == "uint8" and 0 < s["share"] and r["m_before"]:
                        assert H.make_mask(r["m_before"], s["share"], s["seed"], "uint8").max() > 1
                if op == "append" or (op in H.REMOVALS and r["m"] < r["m_before"]):
                    borrowed = False
    print(dict(c))
    wanted = (["moved removal, incremental append, moved removal", "close after a removal, create of the other dimension",
               "down by thin", "down by a filter", "up by an append", "everything removed, a refused read, an append"]
              + [k + " on stale normals" for k in ("thin", "remove", "radius_filter", "stat_filter")]
              + [f"nothing removed on a borrowed cloud: {w}" for w in ("all-ones mask", "huge ratio", "tiny voxel")]
              + [f"mask {e} {d}" for e in ("host", "device") for d in ("bool", "uint8")]
              + ["on an empty handle: " + k for k in ("thin", "remove host", "remove device", "radius_filter", "stat_filter",
                                                      "crop")])
    for what in wanted:
        assert c[what] >= 2, (what, dict(c))


def test_one_cell_ordered_query_sits_between_two_snapshot_estimates(map_traces):
    found = 0
    for steps, t in map_traces:
        for pairs in handles(steps, t):
            for at, (s, r) in enumerate(pairs):
                if s.get("order") == "cell":
                    before, after = pairs[at - 1], pairs[at + 1]
                    assert s["op"] == "query" and s["n"] == 70_000 and r["m_before"] >= KGRID
                    for ps, pr in (before, after):  # beyond kGridCoopMaxN on the grid engine: a cell-sorted snapshot
                        assert ps["op"] == "estimate" and ps["n"] == 70_000 > KCOOP and pr["m_before"] == r["m_before"]
                    found += 1
    assert found == 1


# ------------------------------------------------------------------ the map checker and a right device

CPU_MAP_RUNS = [(3, 0), (2, 0), (3, 2), (2, 4)]


@pytest.mark.parametrize("dim,seed", CPU_MAP_RUNS)
def test_the_stand_in_passes_the_reduced_map_sequences(dim, seed):
    steps = H.map_sequence(seed, "cpu", dim)
    t = H.trace(steps)
    assert max(r["m"] for r in t) <= 3_000 and max(r.get("n") or 0 for r in t) <= 1_200
    assert {r["op"] for r in t} >= {"thin", "remove", "neighbours", "query", "count_within"}
    if (dim, seed) in ((3, 0), (3, 2)):  # these pass through every removal on an emptied handle
        assert {r["op"] for r in t if r["op"] in H.REMOVALS and r["m_before"] == 0} == set(H.REMOVALS)
    H.run(H.ReferenceDevice(), steps, seed=seed)


def test_two_stand_ins_pass_the_reduced_interleaved_map_sequence():
    steps = H.map_interleaved(0, "cpu")
    assert {s.get("h") for s in steps} == {0, 1, None}
    H.run({0: H.ReferenceDevice(), 1: H.ReferenceDevice()}, steps, seed=0)


# ------------------------------------------------------------------ the map checker and five more wrong devices

class ThinKeepsTheLastOfAVoxel(H.ReferenceDevice):
    def thin_keep(self, cloud, v):
        return np.ascontiguousarray(H.thin_mask(cloud[::-1], v)[::-1])


class AllKeptNormalsCurrent(H.Model):
    def current(self, mask):
        return int(mask.sum()) if 0 < self.normals_m < self.m else super().current(mask)


class StaleRemovalReportsCurrentNormals(H.ReferenceDevice):
    model_cls = AllKeptNormalsCurrent


class ReadsSearchTheCloudBeforeTheRemoval(H.ReferenceDevice):
    def searched_cloud(self):
        return self.model.cloud if self.cloud_before is None else self.cloud_before


class RadiusFilterDoesNotCountTheTarget(H.ReferenceDevice):
    def radius_keep(self, cloud, radius, need):
        return H.radius_keep(cloud, radius, need + 1)


class NewIndexNumbersTheOldRows(H.ReferenceDevice):
    def index_of(self, mask):
        return np.where(mask, np.arange(len(mask)), H.GONE).astype(np.uint32)


def scan_map_for(pred, what):
    return scan_for(pred, what, make=H.map_sequence)


def test_a_thin_that_keeps_the_last_point_of_a_voxel_is_caught_at_that_thin():
    steps, t, want = scan_map_for(lambda r, t: r["op"] == "thin" and r["m"] < r["m_before"], "a thin that removes")
    assert failing_step(ThinKeepsTheLastOfAVoxel(), steps) == want


def test_a_removal_on_stale_normals_that_reports_them_current_is_caught_at_that_removal():
    def pred(r, t):
        return r["op"] in H.REMOVALS and 0 < r["normals_m_before"] < r["m_before"] and r["m"] > 0

    steps, t, want = scan_map_for(pred, "a removal on stale normals")
    assert failing_step(StaleRemovalReportsCurrentNormals(), steps) == want


def test_a_read_of_the_cloud_from_before_the_last_removal_is_caught_at_that_read():
    reads = READ_FORMS + ("nn_search", "read_refused", "poisoned_query", "poisoned_count_within")
    steps, t, want = scan_map_for(lambda r, t: r["form"] in reads and r["removed_before"] > 0, "a read after a removal")
    assert failing_step(ReadsSearchTheCloudBeforeTheRemoval(), steps) == want


def test_a_radius_filter_that_does_not_count_the_target_itself_is_caught_at_that_filter():
    steps, t, want = scan_map_for(lambda r, t: r["op"] == "radius_filter" and r["m"] > 0, "a radius filter that keeps some")
    assert failing_step(RadiusFilterDoesNotCountTheTarget(), steps) == want


def test_a_new_index_that_numbers_the_old_rows_is_caught_at_the_first_removal_that_removes():
    steps, t, want = scan_map_for(lambda r, t: r["op"] in H.REMOVALS and 0 < r["m"] < r["m_before"], "a removal")
    assert failing_step(NewIndexNumbersTheOldRows(), steps) == want
