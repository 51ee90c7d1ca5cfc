"""The model, the generator and the checker of the sequence tests (tests/handle_model.py), without a GPU: the generator
is deterministic; over the exact seeds tests/test_gpu_sequences.py runs, the coverage conditions hold; the checker
passes a stand-in built from the references themselves and catches five sabotaged ones at the first step where each
fault can be seen.  This is the only place faults are injected -- into a numpy stand-in, never into the library."""
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


def scan_for(pred, what):
    """the first reduced sequence whose trace has a step for the fault to show at"""
    for dim, seed in CPU_RUNS + [(d, s) for s in range(4, 12) for d in (3, 2)]:
        steps = H.sequence(seed, "cpu", dim)
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
