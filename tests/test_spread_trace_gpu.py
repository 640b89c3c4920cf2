"""A seeded 60-step call trace over the state a context carries for pod topology spread, in the spirit of
tests/test_ctx_trace_gpu.py: spread calls, _fit calls, plain sequential calls, resets and every writer, in an order
drawn from a seed, against tests/spread_ref.py. After every step every read-back (pod counts, the resource table,
the zone column, the groups and the spread counts) is compared with the state the reference carries."""
from __future__ import annotations

import numpy as np
import pytest

import spread_ref as S
from test_spread_gpu import Mirror, rand_case

pytestmark = pytest.mark.gpu

STEPS = 60
OPS = ("spread", "spread", "spread", "spread_nores", "fit", "plain", "reset_counts", "patch_cnt", "reset_cnt",
       "skews", "groups", "zones", "patch_cap", "patch_used", "patch_nodes", "upload_nodes")


def fresh(ctx, msh, oracle, rng, ps, n):
    u, nd, _, _ = rand_case(rng, n, 0, p_unsched=0.15)
    G = int(rng.integers(1, 5))
    return Mirror(ctx, msh, oracle, ps, u, nd, rng.integers(-1, 4, n), rng.choice([1, 2, 3], G),
                  rng.integers(4, 12, (2, n)).astype(np.int64), rng.integers(1, 6, n))


def test_sixty_step_trace(msh, oracle):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    rng = np.random.default_rng(6060)
    ps = oracle.PluginSet(weights=[2], normalize=[1])
    n = 150
    log = []
    with msh.DeviceContext(0) as ctx:
        m = fresh(ctx, msh, oracle, rng, ps, n)
        for step in range(STEPS):
            op = OPS[int(rng.integers(0, len(OPS)))]
            what = f"step {step}: {op} (trace so far: {log[-6:]})"
            log.append(op)
            G = len(m.skew)
            p = int(rng.integers(1, 90))
            _, _, pd, pt = rand_case(rng, 1, p)
            req = rng.integers(0, 3, (2, p)).astype(np.int64)
            if op == "spread":
                m.spread(pd, pt, rng.integers(-1, G, p), req, what=what)
                continue
            if op == "spread_nores":
                m.spread(pd, pt, rng.integers(-1, G, p), None, scalar=int(rng.choice([0, 4])), what=what)
                continue
            if op in ("fit", "plain"):  # commit counts (and used), never the spread counts
                a, us, rq = (m.alloc, m.used, req) if op == "fit" else S.no_res(n, p)
                w = S.per_pod(oracle, m.u, m.nd, pd, pt, ps, m.eff(), a, us, rq, m.zone, np.full(p, -1), m.skew,
                              m.counts, m.cnt)
                got = ctx.schedule_sequential_fit(pd, pt, req) if op == "fit" else ctx.schedule_sequential(pd, pt, 0)
                assert all(np.array_equal(x, y) for x, y in zip(got, w[:3])), what
                m.commit(w, op == "fit")
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
            elif op == "patch_used":
                i = rng.permutation(n)[:3].astype(np.int32)
                m.used[:, i] = rng.integers(0, 5, (2, 3))
                ctx.patch_node_resources(i, used=m.used[:, i])
            elif op == "patch_nodes":
                i = rng.permutation(n)[:5].astype(np.int32)
                m.u = m.u.copy()
                m.u[i] ^= 1
                ctx.patch_nodes(i, m.u[i], m.nd[i])
            elif op == "upload_nodes":  # drops the columns and the table, zeroes every count, keeps the groups
                ctx.upload_nodes(m.u, m.nd)
                assert ctx.node_zones() is None and ctx.node_resources() is None and not ctx.spread_counts().any(), what
                assert np.array_equal(ctx.spread_groups(), m.skew), what
                m = fresh(ctx, msh, oracle, rng, ps, n)
            m.verify(what)
            assert np.array_equal(ctx.node_zones(), m.zone) and np.array_equal(ctx.spread_groups(), m.skew), what
            assert np.array_equal(ctx.node_capacity(), m.cap), what
    assert {"spread", "fit", "plain"} <= set(log)
