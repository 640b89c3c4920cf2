"""A seeded 60-step call trace over the state a context carries for topology spread together with a resource score,
modelled on tests/test_spread_trace_gpu.py: msh_schedule_sequential_spread_scored interleaved with the setters, the
writers and the other three sequential entry points (_spread, _fit, the plain call), in an order drawn from a seed,
against tests/spread_score_ref.py. After every step every output and every read-back (pod counts, the resource
table, the zone column, the groups, the spread counts, the score setting) is compared with the state the reference
carries."""
from __future__ import annotations

import numpy as np
import pytest

import spread_ref as S
import spread_score_ref as X
from test_spread_score_gpu import Mirror, rand_amounts, rand_case, refused

pytestmark = pytest.mark.gpu

STEPS = 60
OPS = ("scored", "scored", "scored", "scored", "scored_nores", "spread", "fit", "plain", "set_score", "set_score",
       "reset_counts", "patch_cnt", "reset_cnt", "skews", "groups", "zones", "patch_cap", "patch_res", "patch_nodes",
       "upload_nodes")


def fresh(ctx, msh, oracle, rng, ps, n, mode, weight, rw):
    u, nd, _, _ = rand_case(rng, n, 0, p_unsched=0.15)
    G = int(rng.integers(1, 5))
    alloc, used, _ = rand_amounts(rng, 2, n, 0)
    return Mirror(ctx, msh, oracle, ps, u, nd, rng.integers(-1, 4, n), rng.choice([1, 2, 3], G), alloc // 4, used // 4,
                  rng.integers(1, 6, n), mode, weight, rw)


def test_sixty_step_trace(msh, oracle):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    E = msh._native
    rng = np.random.default_rng(6161)
    ops = [OPS[k] for k in np.random.default_rng(6164).integers(0, len(OPS), STEPS)]  # drawn apart from the inputs
    assert {"scored", "scored_nores", "spread", "fit", "plain", "set_score", "patch_res", "patch_cnt"} <= set(ops)
    ps = oracle.PluginSet(weights=[2], normalize=[1])
    n = 150
    log = []
    with msh.DeviceContext(0) as ctx:
        m = fresh(ctx, msh, oracle, rng, ps, n, X.LEAST, 1, [1, 1])
        for step in range(STEPS):
            op = ops[step]
            what = f"step {step}: {op}, mode {m.mode} (trace so far: {log[-6:]})"
            log.append(op)
            G = len(m.skew)
            p = int(rng.integers(1, 90))
            _, _, pd, pt = rand_case(rng, 1, p)
            req = rng.integers(0, 4, (2, p)).astype(np.int64)
            grp = rng.integers(-1, G, p)
            if op == "scored":
                m.scored(pd, pt, grp, req, what=what)
                continue
            if op == "scored_nores":  # nres = 0: the spread call's with mode NONE, refused with a score set
                if m.mode == X.NONE:
                    m.scored(pd, pt, grp, None, scalar=int(rng.choice([0, 4])), what=what)
                    continue
                refused(msh, E.MSH_ERR_STATE, ctx.schedule_sequential_spread_scored, pd, pt, grp, None)
            elif op == "spread":  # the old entry point: refuses a scored ctx, equals the new one otherwise
                if m.mode == X.NONE:
                    w = m.expect(pd, pt, grp, req)
                    m.compare(ctx.schedule_sequential_spread(pd, pt, grp, req), w, what)
                    m.commit(w)
                else:
                    refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_spread, pd, pt, grp, req)
            elif op == "fit":  # scored or not as the ctx is set; commits counts and used, never the spread counts
                w = m.expect(pd, pt, np.full(p, -1), req)
                m.compare(ctx.schedule_sequential_fit(pd, pt, req), w, what)
                m.commit(w)
            elif op == "plain":  # ignores the table, the setting, zones and groups
                w = m.expect(pd, pt, np.full(p, -1), None, mode=X.NONE)
                m.compare(ctx.schedule_sequential(pd, pt, 0), w, what)
                m.commit(w, False)
            elif op == "set_score":  # policy: the state stays
                mode = int(rng.integers(0, 3))
                m.score(mode, int(rng.choice([1, 3, 2**32])), [int(x) for x in rng.choice([0, 1, 7, 100], 2)] if
                        rng.random() < 0.5 else [1, 1])
                if not any(m.rw):
                    m.score(mode, m.weight, [1, 0])
            elif op == "reset_counts":
                ctx.reset_node_pod_counts()
                m.counts = np.zeros(n, np.int32)
            elif op == "patch_cnt":
                k = int(rng.integers(1, 5))
                cells = rng.permutation(G * 4)[:k]
                gi, zi, val = cells // 4, cells % 4, rng.integers(0, 4, len(cells))
                ctx.patch_spread_counts(gi, zi, val)
                m.cnt[gi, zi] = val
            elif op == "reset_cnt":
                ctx.reset_spread_counts()
                m.cnt[:] = 0
            elif op == "skews":  # the same G: the counts stay
                m.skew = rng.choice([1, 2, 5], G).astype(np.int32)
                ctx.set_spread_groups(m.skew)
            elif op == "groups":  # another G: the counts are zeroed
                G2 = G % 4 + 1
                m.skew = rng.choice([1, 2], G2).astype(np.int32)
                ctx.set_spread_groups(m.skew)
                m.cnt = np.zeros((G2, S.MAX_ZONES), np.int32)
            elif op == "zones":
                m.zone = rng.integers(-1, 5, n).astype(np.int32)
                ctx.upload_node_zones(m.zone)
                m.cnt[:] = 0
            elif op == "patch_cap":
                i = rng.permutation(n)[:3].astype(np.int32)
                m.cap[i] = rng.integers(0, 8, 3)
                ctx.patch_node_capacity(i, m.cap[i])
            elif op == "patch_res":  # used, and alloc sometimes below it
                i = rng.permutation(n)[:3].astype(np.int32)
                m.alloc, m.used = m.alloc.copy(), m.used.copy()
                m.used[:, i] = rng.integers(0, 9, (2, 3))
                m.alloc[:, i] = rng.integers(0, 40, (2, 3))
                ctx.patch_node_resources(i, alloc=m.alloc[:, i], used=m.used[:, i])
            elif op == "patch_nodes":
                i = rng.permutation(n)[:5].astype(np.int32)
                m.u = m.u.copy()
                m.u[i] ^= 1
                ctx.patch_nodes(i, m.u[i], m.nd[i])
            elif op == "upload_nodes":  # drops the columns and the table, zeroes every count, keeps groups and setting
                ctx.upload_nodes(m.u, m.nd)
                assert ctx.node_zones() is None and ctx.node_resources() is None and not ctx.spread_counts().any(), what
                assert np.array_equal(ctx.spread_groups(), m.skew), what
                m = fresh(ctx, msh, oracle, rng, ps, n, m.mode, m.weight, m.rw)
            m.verify(what)
            assert np.array_equal(ctx.node_zones(), m.zone) and np.array_equal(ctx.spread_groups(), m.skew), what
            assert np.array_equal(ctx.node_capacity(), m.cap), what
            mode, weight, rw = ctx.resource_score()
            assert mode == m.mode and (mode == X.NONE or (weight, rw) == (m.weight, list(m.rw))), what
