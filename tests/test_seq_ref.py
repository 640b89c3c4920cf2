"""The unified CPU references (tests/seq_ref.py) against a recording, and against each other with every feature on.

tests/golden/seq_ref_digests.json was recorded once from the per-layer loops that the eight `*_ref.py` modules held
before they became delegations to seq_ref: for every layer, a SHA-256 over what its `per_pod` returns (and over what
its observation hook collects) on the layer's generator at seeds 0..19, on the special cases named in `cases`, and
on the inputs of the layer's hand-worked tests. `record` recomputes it through today's modules. A digest that differs
means that seq_ref changed what a layer computes: seq_ref is what gets fixed, the file is never recorded again.
"""
from __future__ import annotations

import copy
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import balanced_ref as BR
import classes_ref as KR
import podaffinity_ref as PA
import prefs_ref as PR
import resource_score_ref as RS
import soft_spread_ref as SR
import spread_ref as S
import spread_score_ref as X
import test_balanced
import test_classes
import test_podaffinity
import test_prefs
import test_resource_score
import test_soft_spread
import test_spread
import test_spread_score

GOLDEN = Path(__file__).resolve().parent / "golden" / "seq_ref_digests.json"
LAYERS = ("resource_score_ref", "spread_ref", "spread_score_ref", "classes_ref", "prefs_ref", "soft_spread_ref",
          "balanced_ref", "podaffinity_ref")
SEEDS = range(20)
MAX_N, MAX_P = 700, 300   # the generators' sizes in the recording


def digest(out, hook=None) -> str:
    """SHA-256 over dtype, shape and little-endian contiguous bytes of every array, then over repr(hook)."""
    h = hashlib.sha256()
    for a in out:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.astype(a.dtype.newbyteorder("<")).tobytes())
    if hook is not None:
        h.update(repr(hook).encode())
    return h.hexdigest()


def state_hook(st):
    return sorted(st.stats.items()), st.present.tolist(), st.repel.tolist()


def hand_calls(mod, *tests):
    """The inputs (without the oracle) that the layer's hand-worked tests feed its references: the tests run, with
    their own assertions, while mod.serial and mod.per_pod note what they are called with."""
    calls, orig = [], {name: getattr(mod, name) for name in ("serial", "per_pod") if hasattr(mod, name)}

    def spy(f):
        def wrapped(O, *a, **kw):
            calls.append(copy.deepcopy((a, kw)))
            return f(O, *a, **kw)
        return wrapped

    for name, f in orig.items():
        setattr(mod, name, spy(f))
    try:
        for t in tests:
            t()
    finally:
        for name, f in orig.items():
            setattr(mod, name, f)
    return calls


def replay(mod, O, calls):
    """(label, digest) of mod.per_pod on the recorded inputs; a `trace` list and a State are hashed after the call."""
    for k, (a, kw) in enumerate(calls):
        kw = {key: v for key, v in kw.items() if key != "moved"}
        if "trace" in kw:
            kw["trace"] = []
        st = next((x for x in a if isinstance(x, PA.State)), None)
        out = mod.per_pod(O, *a, **kw)
        yield f"hand/{k}", digest(out, state_hook(st) if st is not None else kw.get("trace"))


def resource_score_draws(O):
    """The cases of test_resource_score.py::test_the_two_references_agree."""
    rng = np.random.default_rng(20266)
    for case in range(150):
        c = RS.sweep_case(O, rng, case, (0, 1, 2, 5, 9, 14))
        c["p"] = min(c["p"], 40)
        for k in ("pd", "pt"):
            c[k] = c[k][: c["p"]]
        c["req"] = c["req"][:, : c["p"]]
        if case % 4 == 0 and c["n"]:
            f = RS.SCORE_MAX // (int(max(c["alloc"].max(initial=1), c["used"].max(initial=1), 1)) + 1)
            c["alloc"] = c["alloc"] * f + (c["alloc"] > 0)
            c["used"], c["req"] = c["used"] * f, c["req"] * f
        if case % 7 == 0 and c["n"]:
            c["used"][:, 0] = np.maximum(c["used"][:, 0], 1)
            c["alloc"][:, 0] = c["used"][:, 0] - 1
        yield case, c


def cases(layer, O):
    """(label, digest) for every recorded case of the layer, in the file's order. The calls are the ones the layer's
    CPU test makes (its helpers are imported), with `per_pod`."""
    if layer == "resource_score_ref":
        for case, c in resource_score_draws(O):
            yield f"agree/{case}", digest(test_resource_score.run(RS.per_pod, O, c))
        yield from replay(RS, O, hand_calls(RS, lambda: test_resource_score.test_hand_worked_placements(O)))
    elif layer == "spread_ref":
        for seed in SEEDS:
            c = S.gen_case(seed, MAX_N, MAX_P)
            cols, eff, res, sp = test_spread.sweep_inputs(c)
            yield f"seed/{seed}", digest(S.per_pod(O, *cols, test_classes.case_plugins(O, c), eff, *res, *sp))
        yield from replay(S, O, hand_calls(S, lambda: test_spread.test_three_zones_max_skew_one(O),
                                           lambda: test_spread.test_a_full_zone_pins_the_minimum(O),
                                           lambda: test_spread.test_a_node_without_a_zone(O)))
    elif layer == "spread_score_ref":
        for seed in SEEDS:
            c = X.gen_case(seed, MAX_N, MAX_P)
            cols, eff, res, sp = test_spread_score.case_args(c)
            yield f"seed/{seed}", digest(X.per_pod(O, *cols, test_spread_score.case_plugins(O, c), eff, *res, *sp,
                                                   c["score_mode"], c["rs_weight"], c["rw"]))
        yield from replay(X, O, hand_calls(X, lambda: test_spread_score.test_the_skew_bars_the_best_scored_node(O),
                                           lambda: test_spread_score.test_the_score_decides_among_the_allowed_zones(O)))
    elif layer == "classes_ref":
        for seed in SEEDS:
            c = KR.gen_case(seed, MAX_N, MAX_P)
            cols, eff, res, sp, sc = test_classes.case_args(c)
            yield f"seed/{seed}", digest(KR.per_pod(O, *cols, test_classes.case_plugins(O, c), eff, *res, *sp, *sc,
                                                    c["bits"], c["C"], c["pod_class"]))
    elif layer == "prefs_ref":
        for seed in SEEDS:
            trace = []
            out = test_prefs.run(PR.per_pod, O, PR.gen_case(seed, MAX_N, MAX_P), trace=trace)
            yield f"seed/{seed}", digest(out, trace)
        none, zero = np.full(3, -1, np.int32), np.zeros(3, np.int32)
        yield from replay(PR, O, hand_calls(
            PR, lambda: test_prefs.test_hand_worked_fill_up(O, PR.per_pod),
            lambda: test_prefs.test_hand_worked_taints_and_truncation(O, PR.per_pod),
            # test_pods_without_a_preference_still_carry_the_taint_term's two calls
            lambda: test_prefs.tiny(O, 2, 3, [2, 2], w_aff=5, w_taint=7, cls=none, ref=PR.per_pod),
            lambda: test_prefs.tiny(O, 2, 3, [2, 2], w_aff=5, w_taint=7, cls=zero, ref=PR.per_pod)))
    elif layer == "soft_spread_ref":
        for seed in SEEDS:
            trace = []
            out = test_soft_spread.run(SR.per_pod, O, SR.gen_case(seed, MAX_N, MAX_P), trace=trace)
            yield f"seed/{seed}", digest(out, trace)
        yield from replay(SR, O, hand_calls(
            SR, lambda: test_soft_spread.test_hand_worked_two_zones(O, SR.per_pod),
            lambda: test_soft_spread.test_hand_worked_skew_and_ignored_nodes(O, SR.per_pod)))
    elif layer == "balanced_ref":
        for seed in SEEDS:
            yield f"seed/{seed}", digest(test_balanced.run(BR.per_pod, O, BR.gen_case(seed, MAX_N, MAX_P)))
    elif layer == "podaffinity_ref":
        for case in range(len(test_podaffinity.GPU_CASES)):  # test_the_gpu_cases_reach_every_rule's
            out, st = test_podaffinity.ref_case(O, test_podaffinity.gpu_case(case))
            yield f"gpu_case/{case}", digest(out, state_hook(st))
        for seed in SEEDS:
            out, st = test_podaffinity.ref_case(O, test_podaffinity.gpu_case(seed % 10, seed))
            yield f"seed/{seed}", digest(out, state_hook(st))
        T = test_podaffinity
        yield from replay(PA, O, hand_calls(PA, *(lambda t=t: t(O) for t in (
            T.test_one_replica_per_node, T.test_one_replica_per_zone,
            T.test_symmetric_repulsion_of_a_pod_without_anti_affinity, T.test_a_self_affine_series_opens_exactly_one_zone,
            T.test_a_follower_has_no_first_pod_exception, T.test_a_zone_term_fails_on_a_node_without_a_zone,
            T.test_a_pod_without_a_profile_is_untouched, T.test_hostname_and_zone_terms_together,
            T.test_derived_words_follow_a_new_zone_column))))


def record(O, layers=LAYERS) -> dict:
    return {layer: [{"case": label, "sha256": d} for label, d in cases(layer, O)] for layer in layers}


def test_the_recording_names_every_layer():
    assert tuple(json.loads(GOLDEN.read_text())) == LAYERS


@pytest.mark.parametrize("layer", LAYERS)
def test_the_layer_computes_what_was_recorded(oracle, layer):
    want = json.loads(GOLDEN.read_text())[layer]
    got = record(oracle, [layer])[layer]
    assert len(want) >= len(SEEDS) and [e["case"] for e in got] == [e["case"] for e in want]
    differ = [g["case"] for g, w in zip(got, want) if g != w]
    assert not differ, f"{layer}: {differ}"


def test_serial_equals_per_pod_with_every_feature_on(oracle):
    """The superset, which only balanced_ref's pair reached before: every term of the total at once, with both traces."""
    import seq_ref
    soft_scored = 0
    for seed in SEEDS:
        c = BR.gen_case(seed, max_n=65, max_p=80)
        ta, tb, sa, sb = [], [], [], []
        a = test_balanced.run(seq_ref.serial, oracle, c, prefs_trace=ta, soft_trace=sa)
        b = test_balanced.run(seq_ref.per_pod, oracle, c, prefs_trace=tb, soft_trace=sb)
        test_classes.same(a, b, f"seed {seed}")
        assert [x.dtype for x in a] == [x.dtype for x in b] and [x.shape for x in a] == [x.shape for x in b]
        assert ta == tb and sa == sb, f"seed {seed}: a trace differs"
        soft_scored += len(sa)
    assert soft_scored > 100
