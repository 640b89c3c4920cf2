"""Which refusal wins, and its exact text, for the twelve grouped sequential-commit entry points
(msh_schedule_sequential_{spread, spread_scored, classes, prefs, soft, balanced} and their _device forms).

Every case puts a fresh ctx in one state, makes one call on the host entry point (numpy arrays) and one on the device
entry point (torch tensors), and asserts the error code and the whole message. Nothing here launches a kernel:
every call is refused on the host, and node_pod_counts(), node_resources() and spread_counts() read the same after
it. States in which two refusals apply pin their order. The delegation cases (a weight of 0, no soft group, no
classes) pin the entry name a message carries: refuse_random's text has it.

Not reachable through the Python API, so not covered: a negative p, a pod count above 2^24 and a null pointer on the
host entry points (the device entry points cover all three), and a null pod_group on a host spread call."""
from __future__ import annotations

import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORMS = ("spread", "spread_scored", "classes", "prefs", "soft", "balanced")
SPREAD, CLASSED, KEYED, SOFT = FORMS[:2], FORMS[2:], FORMS[3:], FORMS[4:]
N, P, NRES, G, C = 8, 3, 2, 2, 3
B24, B55, B62 = 1 << 24, 1 << 55, 1 << 62
INVALID, STATE, UNSUPPORTED = "MSH_ERR_INVALID", "MSH_ERR_STATE", "MSH_ERR_UNSUPPORTED"


def entry(form, dev):
    return f"msh_schedule_sequential_{form}" + ("_device" if dev else "")


# -- the messages, written out --
NEG = (INVALID, "negative argument")
NRES_RANGE = (INVALID, "nres outside [0, MSH_MAX_RESOURCES]")
NULL_DEV = (INVALID, "null device pointer")
GENERIC = (UNSUPPORTED, "score-column plugins run on the batch entry points only")
NO_NODES = (STATE, "msh_upload_nodes has not been called")
NO_ZONES = (STATE, "msh_upload_node_zones has not been called")
NO_BITS = (STATE, "msh_upload_node_class_bits has not been called")
NO_RES = (STATE, "msh_upload_node_resources has not been called")
NEITHER = (STATE, "pod classes with neither msh_upload_node_class_prefs nor msh_upload_node_class_bits")
PODS = (UNSUPPORTED, "a soft-spread call takes at most MSH_SPREAD_SOFT_MAX = 2^24 pods")


def soft_groups(name, k):
    return (UNSUPPORTED, f"{name}: the ctx holds {k} SCHEDULE_ANYWAY spread group(s) (msh_set_spread_group_modes); a "
                         "call with pod groups must be msh_schedule_sequential_soft")


def random_tb(name):
    return (UNSUPPORTED, f"{name}: MSH_TIEBREAK_RANDOM is not implemented for this entry point "
                         "(msh_set_tiebreak(ctx, MSH_TIEBREAK_FIRST, 0, 0) restores the first maximum)")


def spread_with_score(name):
    return (UNSUPPORTED, f"{name}: a resource score (msh_set_resource_score) together with topology spread is not "
                         "implemented (MSH_RESOURCE_SCORE_NONE restores the unscored form)")


def two_resources(t):
    return (STATE, f"the balanced score needs a resource table with at least two resources, the table has {t}")


def all_requests(t, k):
    return (STATE, f"the balanced score needs the requests of all {t} resources of the table, the call has {k}")


def table_nres(k, t):
    return (INVALID, f"requests for {k} resources against a table of {t}")


def setting_nres(r, k):
    return (STATE, f"msh_set_resource_score was given {r} resources, the call has {k}")


def table_limit(form_name, lim, nres):
    return (UNSUPPORTED, f"the {form_name} form keeps the node state in registers: at most {lim} nodes per device with "
                         f"{nres} resource" + ("" if nres == 1 else "s"))


def amount(v, who="a resource score"):
    return (UNSUPPORTED, f"{who} needs every amount of the table within MSH_RESOURCE_SCORE_MAX = 2^55; an upload or "
                         f"patch wrote {v}")


def unequal_c(a, b):
    return (STATE, f"the class masks were uploaded for C = {a}, the preference values for C = {b}")


def key_sum(what, w):
    return (UNSUPPORTED, f"the weights of {what} sum to {w}: the packed key holds 100 x 655 at most")


KEY1 = "the resource score and the two preference scores"
KEY2 = "the resource score, the two preference scores and the spread score"
KEY3 = "the resource score, the two preference scores, the spread score and the balanced score"


def count_bound(b):
    return (UNSUPPORTED, f"a spread count may have reached {b}, above MSH_SPREAD_SOFT_MAX = 2^24 "
                         "(msh_reset_spread_counts zeroes them)")


def skew_bound(g, s):
    return (UNSUPPORTED, f"SCHEDULE_ANYWAY group {g} has max_skew {s}, above MSH_SPREAD_SOFT_MAX = 2^24")


def group_range(j, v, g):
    return (INVALID, f"pod {j}: group {v} outside [-1, G) with G = {g}")


def class_range(j, v, c):
    return (INVALID, f"pod {j}: class {v} outside [-1, C) with C = {c}")


def request_range(j):
    return (INVALID, f"request outside [0, 2^62] at pod {j}")


def request_55(j, who="a resource score"):
    return (INVALID, f"{who} needs every request within MSH_RESOURCE_SCORE_MAX = 2^55: pod {j}")


class Case:
    """One ctx state and one call. prepare(ctx, form) changes the good state (good()) and may return call arguments
    that replace the good call's; want(form, dev, ctx) is (code name, message), or None where the form, or the host
    or device side of it, cannot reach the refusal."""

    def __init__(self, name, want, prepare=None, forms=FORMS, nodes=N, nres_table=NRES, score=False, amount_value=1000,
                 **call):
        self.name, self.want, self.prepare, self.forms = name, want, prepare, forms
        # nodes: a count, or the name of the form whose table limit plus one it is ("": the case's own form);
        # score: a resource score (LEAST, weight 1) set before anything else
        self.nodes, self.nres_table, self.score, self.amount_value, self.call = nodes, nres_table, score, amount_value, call


def good(ctx, form, n, nres_table, amount_value=1000):
    """A ctx on which `form`'s entry points run their own kernel form: nodes, zones, G groups, a resource table, the
    class columns for the class forms, nonzero preference weights from _prefs on, a SCHEDULE_ANYWAY group from _soft
    on and a balanced weight for _balanced. n = 0: no upload_nodes, and none of the columns that need one."""
    ctx.set_spread_groups([1] * G)
    if form in KEYED:
        ctx.set_preference_weights(1, 1)
    if form in SOFT:
        ctx.set_spread_group_modes([0, 1])
        ctx.set_spread_score_weight(1)
    if form == "balanced":
        ctx.set_balanced_score(1)
    if n == 0:
        return
    ctx.upload_nodes(np.ones(n, np.uint8), np.arange(n) % 3)  # every node unschedulable: nothing could be placed
    ctx.upload_node_zones(np.arange(n) % 2)
    if nres_table:
        ctx.upload_node_resources(np.full((nres_table, n), amount_value, np.int64))
    if form in CLASSED:
        ctx.upload_node_class_bits(C, np.full(n, (1 << C) - 1, np.uint64))
    if form in KEYED:
        ctx.upload_node_class_prefs(C, np.ones((C, n), np.uint16), np.ones((C, n), np.uint16))


def scored(ctx, weight=1, rw=(1, 1)):
    ctx.set_resource_score("least", weight, list(rw))


def limit_of(ctx, form, nres):
    return getattr(ctx, f"seq_{form}_max_nodes")(nres)


LIMIT_NAME = {"spread": "topology-spread", "spread_scored": "topology-spread", "classes": "class-mask",
              "prefs": "preference", "soft": "soft-spread", "balanced": "balanced-allocation"}
SCORED_LIMIT_NAME = dict(LIMIT_NAME, spread_scored="scored topology-spread", classes="scored class-mask")


# -- prepare functions: each returns the call arguments it replaces (or None) --
def p_soft_and_random(ctx, form):
    ctx.set_spread_group_modes([0, 1])
    ctx.set_tiebreak("random", 1, 0)


def p_random(ctx, form):
    ctx.set_tiebreak("random", 1, 0)


def p_generic_no_zones(ctx, form):
    msh = importlib.import_module("mini-kube-scheduler_amd")
    ctx.set_plugins([msh.NODE_UNSCHEDULABLE], [msh.NODE_NUMBER],
                    [msh.ScorePluginConfig(msh.NODE_NUMBER), msh.ScorePluginConfig(msh.SCORE_COLUMNS[0])])
    ctx.clear_node_zones()


def p_score_no_zones(ctx, form):
    scored(ctx)
    ctx.clear_node_zones()


def p_no_zones(ctx, form):
    ctx.clear_node_zones()


def p_no_bits(ctx, form):
    ctx.clear_node_class_bits()


def p_no_res(ctx, form):
    ctx.clear_node_resources()


def p_no_res_scored(ctx, form):
    scored(ctx)
    ctx.clear_node_resources()
    return {"req": None}


def p_setting_one(ctx, form):
    scored(ctx, rw=(1,))


def p_neither(ctx, form):
    ctx.clear_node_class_bits()
    ctx.clear_node_class_prefs()


def p_unequal_c(ctx, form):
    ctx.upload_node_class_prefs(2, np.ones((2, N), np.uint16), None)
    scored(ctx, 500)
    ctx.set_preference_weights(100, 100)  # the key sum overflows too: the columns come first
    return {"cls": np.array([0, 1, -1], np.int32)}


def p_key1(ctx, form):
    scored(ctx, 500)
    ctx.set_preference_weights(100, 100)
    ctx.set_spread_score_weight(100)  # the longer sums overflow too: the shortest comes first
    if form == "balanced":
        ctx.set_balanced_score(100)


def p_key2(ctx, form):
    scored(ctx, 400)
    ctx.set_preference_weights(100, 100)
    ctx.set_spread_score_weight(100)
    if form == "balanced":
        ctx.set_balanced_score(100)


def p_key3(ctx, form):
    scored(ctx, 300)
    ctx.set_preference_weights(100, 100)
    ctx.set_spread_score_weight(100)
    ctx.set_balanced_score(100)


def p_count_and_skew(ctx, form):
    ctx.set_spread_groups([1, B24 + 1])  # the same G: the modes stay
    ctx.patch_spread_counts([0], [0], [B24 + 1])


def p_skew(ctx, form):
    ctx.set_spread_groups([1, B24 + 1])


def p_class_range(ctx, form):
    """_classes bounds pod_class by the mask column's C, the forms above it by the preference column's when there is
    one: here C = 2 with no mask column."""
    if form == "classes":
        return {"cls": np.array([0, 3, -1], np.int32), "req": np.array([[1, 1, -1], [1, 1, 1]], np.int64)}
    ctx.clear_node_class_bits()
    ctx.upload_node_class_prefs(2, np.ones((2, N), np.uint16), None)
    return {"cls": np.array([0, 2, -1], np.int32), "req": np.array([[1, 1, -1], [1, 1, 1]], np.int64)}


def p_request_range(ctx, form):
    if form != "spread":
        scored(ctx)  # 2^62 + 1 is above 2^55 too: the 2^62 bound comes first
    return {"req": np.array([[1, B62 + 1, 1], [1, 1, -1]], np.int64)}


def p_request_55_scored(ctx, form):
    scored(ctx)
    return {"req": np.array([[1, 1, 1], [1, 1, B55 + 1]], np.int64)}


def p_balanced_zero(ctx, form):
    ctx.set_balanced_score(0)
    ctx.set_tiebreak("random", 1, 0)


def p_no_soft_group(ctx, form):
    ctx.set_spread_group_modes([0, 0])
    ctx.set_balanced_score(0)
    ctx.set_tiebreak("random", 1, 0)


def p_zero_weights(ctx, form):
    ctx.set_spread_group_modes([0, 0])
    ctx.set_balanced_score(0)
    ctx.set_preference_weights(0, 0)
    ctx.set_tiebreak("random", 1, 0)


def p_zero_weights_no_classes(ctx, form):
    p_zero_weights(ctx, form)
    return {"cls": None}


def p_zero_weights_no_bits(ctx, form):
    p_zero_weights(ctx, form)
    ctx.set_tiebreak("first")
    ctx.clear_node_class_bits()


def p_no_classes(ctx, form):
    return {"cls": None}


def want_limit(names):
    return lambda f, dev, ctx: table_limit(names[f], limit_of(ctx, f, NRES), NRES)


def lower_name(f, dev, host_name, dev_name):
    return random_tb(entry(dev_name if dev else host_name, dev))


CASES = [
    Case("negative argument before no nodes", lambda f, dev, ctx: NEG, nodes=0, neg=True),
    Case("no nodes", lambda f, dev, ctx: NO_NODES, nodes=0),
    Case("null pointer before a negative limit", lambda f, dev, ctx: NULL_DEV if dev else None, pd=None, mppn=-1),
    Case("null requests", lambda f, dev, ctx: NULL_DEV if dev else None, null_req=True),
    Case("null group on a spread form", lambda f, dev, ctx: NULL_DEV if dev else None, forms=SPREAD, grp=None),
    Case("nres out of range", lambda f, dev, ctx: NRES_RANGE, req=np.ones((5, P), np.int64)),
    Case("soft group on a non-soft entry before the random tie-break",
         lambda f, dev, ctx: random_tb(entry(f, dev)) if f in SOFT else soft_groups(entry(f, dev), 1), p_soft_and_random),
    Case("random tie-break", lambda f, dev, ctx: random_tb(entry(f, dev)), p_random),
    Case("generic flag before missing zones", lambda f, dev, ctx: GENERIC, p_generic_no_zones),
    Case("resource score on _spread before missing zones",
         lambda f, dev, ctx: spread_with_score(entry(f, dev)) if f == "spread" else NO_ZONES, p_score_no_zones),
    Case("no zones", lambda f, dev, ctx: NO_ZONES, p_no_zones),
    Case("no class column", lambda f, dev, ctx: NO_BITS, p_no_bits, forms=("classes",)),
    Case("no resource table", lambda f, dev, ctx: NO_RES, p_no_res),
    Case("no resource table, a score and no requests",
         lambda f, dev, ctx: spread_with_score(entry(f, dev)) if f == "spread" else NO_RES, p_no_res_scored),
    Case("balanced with one resource", lambda f, dev, ctx: two_resources(1), forms=("balanced",), nres_table=1,
         req=np.ones((1, P), np.int64)),
    Case("requests against a larger table",
         lambda f, dev, ctx: all_requests(3, 2) if f == "balanced" else table_nres(2, 3), nres_table=3),
    Case("table mismatch before setting mismatch",
         lambda f, dev, ctx: (spread_with_score(entry(f, dev)) if f == "spread" else
                              all_requests(3, 2) if f == "balanced" else table_nres(2, 3)), p_setting_one, nres_table=3),
    Case("setting mismatch",
         lambda f, dev, ctx: spread_with_score(entry(f, dev)) if f == "spread" else setting_nres(1, 2), p_setting_one),
    Case("table limit before an amount above 2^55", want_limit(SCORED_LIMIT_NAME), forms=FORMS[1:], nodes="",
         score=True, amount_value=B55 + 1),
    Case("table limit, unscored", want_limit(LIMIT_NAME), forms=FORMS[:3], nodes=""),
    Case("amount above 2^55", lambda f, dev, ctx: amount(B55 + 1), forms=FORMS[1:], score=True,
         amount_value=B55 + 1),
    Case("balanced amount above 2^55", lambda f, dev, ctx: amount(B55 + 1, "the balanced score"), forms=("balanced",),
         amount_value=B55 + 1),
    Case("classes with neither column", lambda f, dev, ctx: NEITHER, p_neither, forms=KEYED),
    Case("unequal C before the key sum", lambda f, dev, ctx: unequal_c(3, 2), p_unequal_c, forms=KEYED),
    Case("key sum, preferences", lambda f, dev, ctx: key_sum(KEY1, 700), p_key1, forms=KEYED),
    Case("key sum, spread", lambda f, dev, ctx: key_sum(KEY2, 700), p_key2, forms=SOFT),
    Case("key sum, balanced", lambda f, dev, ctx: key_sum(KEY3, 700), p_key3, forms=("balanced",)),
    Case("count bound before skew bound", lambda f, dev, ctx: count_bound(B24 + 1), p_count_and_skew, forms=SOFT),
    Case("pod bound before skew bound", lambda f, dev, ctx: PODS if dev else skew_bound(1, B24 + 1), p_skew, forms=SOFT,
         p=B24 + 1),
    Case("skew bound", lambda f, dev, ctx: skew_bound(1, B24 + 1), p_skew, forms=SOFT),
    Case("group before class and request", lambda f, dev, ctx: None if dev else group_range(1, 2, 2),
         grp=np.array([0, 2, -1], np.int32), cls=np.array([0, 3, -1], np.int32),
         req=np.array([[1, 1, -1], [1, 1, 1]], np.int64)),
    Case("class before request",
         lambda f, dev, ctx: None if dev else class_range(1, 3, 3) if f == "classes" else class_range(1, 2, 2),
         p_class_range, forms=CLASSED),
    Case("request outside 2^62 before 2^55", lambda f, dev, ctx: None if dev or f == "spread" else request_range(1),
         p_request_range),
    Case("request outside 2^62", lambda f, dev, ctx: None if dev else request_range(1), forms=("spread",),
         req=np.array([[1, B62 + 1, 1], [1, 1, -1]], np.int64)),
    Case("request above 2^55 with a score (balanced: the score's message first)",
         lambda f, dev, ctx: None if dev else request_55(2), p_request_55_scored, forms=FORMS[1:]),
    Case("balanced request above 2^55", lambda f, dev, ctx: None if dev else request_55(2, "the balanced score"),
         forms=("balanced",), req=np.array([[1, 1, 1], [1, 1, B55 + 1]], np.int64)),
    # -- delegation: the entry name in the message, and the lower form's refusals --
    Case("_balanced with weight 0 is _soft", lambda f, dev, ctx: lower_name(f, dev, "soft", "soft"), p_balanced_zero,
         forms=("balanced",)),
    Case("_soft without a soft group is _prefs", lambda f, dev, ctx: lower_name(f, dev, "prefs", "prefs"),
         p_no_soft_group, forms=SOFT),
    # the asymmetry: the host _prefs delegates to the public _classes, the device one passes its own name down
    Case("_prefs with zero weights is _classes", lambda f, dev, ctx: lower_name(f, dev, "classes", "prefs"),
         p_zero_weights, forms=KEYED),
    Case("_prefs with zero weights and no classes is _spread_scored under the same name",
         lambda f, dev, ctx: lower_name(f, dev, "classes", "prefs"), p_zero_weights_no_classes, forms=KEYED),
    Case("_prefs with zero weights needs the class column", lambda f, dev, ctx: NO_BITS, p_zero_weights_no_bits,
         forms=KEYED),
    Case("_classes without classes keeps its name", lambda f, dev, ctx: random_tb(entry(f, dev)), p_random,
         forms=("classes",), cls=None),
    Case("_classes without classes has _spread_scored's table limit",
         lambda f, dev, ctx: table_limit("scored topology-spread", limit_of(ctx, "spread_scored", NRES), NRES),
         p_no_classes, forms=("classes",), nodes="spread_scored", score=True),
    Case("_classes without classes has _spread's table limit, unscored",
         lambda f, dev, ctx: table_limit("topology-spread", limit_of(ctx, "spread", NRES), NRES), p_no_classes,
         forms=("classes",), nodes="spread"),
]


@pytest.fixture(scope="module")
def dev_bufs():
    """Device columns and outputs of P entries: refused calls never read or write them."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    z = lambda dt, *shape: torch.zeros(*shape, dtype=dt, device=dev)
    return {"pd": z(torch.int8, P), "pt": z(torch.uint8, P), "grp": z(torch.int32, P), "cls": z(torch.int32, P),
            "req": z(torch.int64, 5, P), "idx": z(torch.int32, P), "score": z(torch.int64, P), "status": z(torch.int32, P)}


def snapshot(ctx):
    res = ctx.node_resources()
    return (ctx.node_pod_counts() if ctx.n_nodes else None, None if res is None else np.stack(res), ctx.spread_counts())


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def host_call(ctx, form, a):
    fn = getattr(ctx, f"schedule_sequential_{form}")
    cols = (a["pd"], a["pt"], a["grp"]) if form in SPREAD else (a["pd"], a["pt"], a["grp"], a["cls"])
    return fn(*cols, a["req"], a["mppn"])


def device_call(ctx, form, a, bufs):
    fn = getattr(ctx, f"schedule_sequential_{form}_device")
    at = lambda k: 0 if a[k] is None else bufs[k].data_ptr()
    cols = (at("pd"), at("pt"), at("grp")) if form in SPREAD else (at("pd"), at("pt"), at("grp"), at("cls"))
    nres = 0 if a["req"] is None else a["req"].shape[0]
    d_req = 0 if a["req"] is None or a["null_req"] else bufs["req"].data_ptr()
    return fn(a["p"], *cols, nres, d_req, a["mppn"], bufs["idx"].data_ptr(), bufs["score"].data_ptr(),
              bufs["status"].data_ptr(), 0)


@pytest.mark.parametrize("case,form", [pytest.param(c, f, id=f"{c.name.replace(' ', '-')}-{f}") for c in CASES for f in c.forms])
def test_refusal(msh, dev_bufs, case, form):
    E = msh._native
    with msh.DeviceContext(0) as ctx:
        if case.score:
            scored(ctx)
        n = case.nodes if isinstance(case.nodes, int) else limit_of(ctx, case.nodes or form, NRES) + 1
        good(ctx, form, n, case.nres_table, case.amount_value)
        a = {"p": P, "pd": np.zeros(P, np.int8), "pt": np.zeros(P, np.uint8), "grp": np.array([0, 1, -1], np.int32),
             "cls": np.array([0, 2, -1], np.int32), "req": np.ones((NRES, P), np.int64), "mppn": 0, "null_req": False,
             "neg": False}
        a.update(case.call)
        a.update((case.prepare(ctx, form) if case.prepare else None) or {})
        before = snapshot(ctx)
        for dev in (False, True):
            want = case.want(form, dev, ctx)
            if want is None:
                continue
            b = dict(a)
            if a["neg"]:  # a negative p has no host form through the Python API: a negative limit there
                b["p" if dev else "mppn"] = -1
            with pytest.raises(msh.MshError) as ei:
                device_call(ctx, form, b, dev_bufs) if dev else host_call(ctx, form, b)
            code = getattr(E, want[0])
            assert ei.value.code == code, f"{entry(form, dev)}: {ei.value}"
            assert str(ei.value) == f"{E.ERR_NAMES.get(code, code)}: {want[1]}", entry(form, dev)
            assert same(before, snapshot(ctx)), f"{entry(form, dev)}: the refused call changed the ctx"
