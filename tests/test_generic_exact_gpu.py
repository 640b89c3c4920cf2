"""generic_kernel's exact quotients through schedule_batch: the cases of tests/generic_exact.py (quotient boundaries of
DEFAULT, REVERSE and MIN-MAX columns for the divisors 1, 3, 7, 100, 2^31 - 1, 2^31 and a MIN-MAX span of 2^32 - 1, in
32-bit, double and uint64_t keys, the last by weight and forced; negative raws down to -2^31; feasible maxima of 0 and
below, where DEFAULT takes its own reciprocal, 0.01 biased; a table past an LDS tile), each step of each case against
the oracle. tests/test_generic_exact.py shows on the CPU that every listed quotient decides some pod's output."""
from __future__ import annotations

import numpy as np
import pytest

import generic_exact as GE

pytestmark = pytest.mark.gpu

CASES = GE.cases()


@pytest.fixture(scope="module")
def ctxs(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    made = {"auto": msh.DeviceContext(0), "u64": msh.DeviceContext(0, {"gen_keys": "u64"})}
    yield made
    for c in made.values():
        c.close()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_quotient_boundaries_decide_the_winner(msh, oracle, ctxs, c):
    """One step per listed node, the nodes before it cordoned with msh_patch_nodes: node, score and status of all 130
    pods equal the oracle's, and the oracle's equal the Python restatement that the CPU mutant test perturbs (the pod
    that does not tolerate the taint takes the head node at the total all nodes share). Up to 0.4 s per case."""
    ctx = ctxs[c["keys"]]
    pl = GE.plugin_list(c)
    ps = oracle.PluginSet(filters=["NodeUnschedulable"], prescore=[], score=[nm for nm, _, _ in pl],
                          weights=[w for _, w, _ in pl], normalize=[m for _, _, m in pl])
    ctx.set_plugins(ps.filters, ps.prescore, [msh.ScorePluginConfig(nm, w, msh.Normalize(m)) for nm, w, m in pl])
    cols = GE.columns(c)
    nd = np.zeros(c["n"], np.int8)
    pd, pt = GE.pods()
    ctx.upload_nodes(GE.unsched_at(c, 0), nd)
    for k in range(4):
        ctx.upload_score_column(f"ScoreColumn{k}", cols[k])
    for t in range(c["L"]):
        u = GE.unsched_at(c, t)
        if t:
            at = np.array([c["pad"] + t - 1], np.int32)
            ctx.patch_nodes(at, u[at], nd[at])
        got = ctx.schedule_batch(pd, pt)
        want = oracle.c_schedule_batch(u, nd, pd, pt, ps, cols=cols)
        for g, w, what in zip(got, want[:3], ("node", "score", "status")):
            bad = np.flatnonzero(np.asarray(g) != np.asarray(w))
            assert len(bad) == 0, (f"{c['name']} step {t} (head raw {c['raws'][c['pad'] + t]}): {what} of pod {bad[0]} "
                                   f"(tolerates {pt[bad[0]]}) is {g[bad[0]]}, the oracle's {w[bad[0]]}")
        for tol in (False, True):
            j = int(np.flatnonzero(pt == tol)[0])
            assert (int(want[0][j]), int(want[1][j])) == GE.outcome(c, t, tol), (c["name"], t, tol)
