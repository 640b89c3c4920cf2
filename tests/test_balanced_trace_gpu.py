"""A seeded 60-step call trace over the state a context carries for the balanced-allocation score, in the manner of
tests/test_spread_score_trace_gpu.py: msh_schedule_sequential_balanced and msh_set_balanced_score interleaved with the
soft, preference and fit calls, the other setters and the writers, in an order drawn from a seed, against
tests/balanced_ref.py. After every step every output and every read-back (pod counts, the resource table, the spread
counts, the class and preference columns, the group modes, the weights, the score setting) is compared with the state
the reference carries."""
from __future__ import annotations

import numpy as np
import pytest

import balanced_ref as BR
import classes_ref as KR
import prefs_ref as PR
from test_balanced_gpu import BMirror, uneven
from test_classes_gpu import rand_case, refused
from test_prefs_gpu import PMirror
from test_soft_spread_gpu import SMirror

pytestmark = pytest.mark.gpu

STEPS = 60
OPS = ("balanced", "balanced", "balanced", "balanced", "balanced", "balanced_nores", "set_balanced", "set_balanced",
       "soft", "prefs", "fit", "set_score", "set_weights", "set_modes", "reset_counts", "patch_cnt", "reset_cnt",
       "patch_res", "patch_cap", "upload_nodes")
C = 6


def fresh(ctx, msh, oracle, rng, ps, n, mode, weight, rw, w, modes, ws, wb):
    u, nd, _, _ = rand_case(rng, n, 0, p_unsched=0.15)
    alloc, used, _ = uneven(rng, 2, n, 0)
    bits, _ = KR.gen_bits(rng, n, C)
    A, T = PR.gen_prefs(rng, n, C)
    return BMirror(ctx, msh, oracle, ps, u, nd, rng.integers(-1, 4, n), rng.choice([1, 2, 3], len(modes)), alloc, used,
                   rng.integers(1, 6, n), mode, weight, rw, bits, C, A=A, T=T, PC=C, w=w, modes=modes, ws=ws, wb=wb)


def test_sixty_step_trace(msh, oracle):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    E = msh._native
    rng = np.random.default_rng(7171)
    ops = [OPS[k] for k in np.random.default_rng(7174).integers(0, len(OPS), STEPS)]  # drawn apart from the inputs
    assert {"balanced", "balanced_nores", "set_balanced", "soft", "prefs", "fit", "set_score", "patch_res"} <= set(ops)
    ps = oracle.PluginSet(weights=[2], normalize=[1])
    n = 150
    log = []
    with msh.DeviceContext(0) as ctx:
        m = fresh(ctx, msh, oracle, rng, ps, n, BR.LEAST, 1, [1, 1], (3, 2), [0, 1, 0], 4, 1)
        for step in range(STEPS):
            op = ops[step]
            what = f"step {step}: {op}, mode {m.mode}, w_balanced {m.wb} (trace so far: {log[-6:]})"
            log.append(op)
            G = len(m.skew)
            p = int(rng.integers(1, 90))
            _, _, pd, pt = rand_case(rng, 1, p)
            _, _, req = uneven(rng, 2, 1, p)
            grp = rng.integers(-1, G, p).astype(np.int32)
            cls = rng.integers(-1, C, p).astype(np.int32)
            if op == "balanced":
                m.call(pd, pt, grp, cls, req, what=what)
                continue
            if op == "balanced_nores":  # nres = 0 against the table: refused with a weight, _soft's answer without
                code = E.MSH_ERR_STATE if (m.wb or m.mode != BR.NONE) else None
                if code is None:
                    w = SMirror.expect(m, pd, pt, grp, cls, None)
                    m.compare(ctx.schedule_sequential_balanced(pd, pt, grp, cls, None), w, what)
                    m.commit(w, False)
                else:
                    refused(msh, code, ctx.schedule_sequential_balanced, pd, pt, grp, cls, None)
            elif op == "set_balanced":  # policy: the state stays
                m.balanced_weight(int(rng.choice([0, 1, 2, 100])))
            elif op == "soft":  # reads no balanced weight
                w = SMirror.expect(m, pd, pt, grp, cls, req)
                m.compare(ctx.schedule_sequential_soft(pd, pt, grp, cls, req), w, what)
                m.commit(w)
            elif op == "prefs":  # without groups: the ctx holds a soft group
                w = PMirror.expect(m, pd, pt, None, cls, req)
                m.compare(ctx.schedule_sequential_prefs(pd, pt, None, cls, req), w, what)
                m.commit(w)
            elif op == "fit":  # scored or not as the ctx is set; no classes, no preferences, no balanced term
                w = KR.per_pod(oracle, m.u, m.nd, pd, pt, ps, m.eff(0), m.alloc, m.used, req, m.zone, np.full(p, -1), m.skew,
                               m.mode, m.weight, m.rw, None, 0, None, m.counts, m.cnt)
                m.compare(ctx.schedule_sequential_fit(pd, pt, req), w, what)
                m.commit(w)
            elif op == "set_score":
                mode = int(rng.integers(0, 3))
                m.score(mode, int(rng.choice([1, 3, 400])), [int(x) for x in rng.choice([1, 7, 100], 2)])
            elif op == "set_weights":
                m.weights(int(rng.integers(0, 20)), int(rng.integers(0, 20)))
                m.spread_weight(int(rng.integers(0, 20)))
            elif op == "set_modes":
                m.set_modes(rng.integers(0, 2, G))
                if not m.modes.any():
                    m.set_modes([1] + [0] * (G - 1))  # the prefs step counts on a soft group
            elif op == "reset_counts":
                ctx.reset_node_pod_counts()
                m.counts = np.zeros(n, np.int32)
            elif op == "patch_cnt":
                cells = rng.permutation(G * 4)[:3]
                gi, zi, val = cells // 4, cells % 4, rng.integers(0, 4, len(cells))
                ctx.patch_spread_counts(gi, zi, val)
                m.cnt[gi, zi] = val
            elif op == "reset_cnt":
                ctx.reset_spread_counts()
                m.cnt[:] = 0
            elif op == "patch_res":  # used, and alloc sometimes below it or 0
                i = rng.permutation(n)[:3].astype(np.int32)
                m.alloc, m.used = m.alloc.copy(), m.used.copy()
                m.used[:, i] = rng.integers(0, 90, (2, 3))
                m.alloc[:, i] = rng.integers(0, 3, (2, 3)) * rng.integers(20, 400, (2, 3))
                ctx.patch_node_resources(i, alloc=m.alloc[:, i], used=m.used[:, i])
            elif op == "patch_cap":
                i = rng.permutation(n)[:3].astype(np.int32)
                m.cap[i] = rng.integers(0, 8, 3)
                ctx.patch_node_capacity(i, m.cap[i])
            elif op == "upload_nodes":  # drops the columns and the table, zeroes every count, keeps the settings
                ctx.upload_nodes(m.u, m.nd)
                assert ctx.node_resources() is None and ctx.balanced_score() == m.wb, what
                m = fresh(ctx, msh, oracle, rng, ps, n, m.mode, m.weight, m.rw, m.w, m.modes, m.ws, m.wb)
            m.verify(what)
            mode, weight, rw = ctx.resource_score()
            assert mode == m.mode and (mode == BR.NONE or (weight, rw) == (m.weight, list(m.rw))), what
