"""A seeded 60-step call trace over the state a context carries for the required inter-pod affinity filter, in the
manner of tests/test_balanced_trace_gpu.py: msh_schedule_sequential_podaffinity interleaved with _balanced and _prefs,
the term, profile and state writers, upload_nodes onto tables of other sizes, the zone upload, and the count and
resource patches, in an order drawn from a seed, against tests/podaffinity_ref.py. After every step every output and
every read-back (pod counts, the resource table, the spread counts, the class and preference columns, the weights, the
terms, the profiles and the two state words of every node) is compared with the state the reference carries."""
from __future__ import annotations

import numpy as np
import pytest

import classes_ref as KR
import podaffinity_ref as PA
import prefs_ref as PR
from test_balanced_gpu import BMirror, uneven
from test_classes_gpu import rand_case
from test_podaffinity_gpu import AMirror
from test_prefs_gpu import PMirror

pytestmark = pytest.mark.gpu

STEPS = 60
OPS = ("podaff", "podaff", "podaff", "podaff", "podaff", "podaff", "podaff_null", "balanced", "prefs", "set_terms",
       "set_profiles", "set_profiles", "upload_state", "patch_state", "patch_state", "upload_nodes", "upload_nodes",
       "upload_zones", "reset_counts", "patch_cnt", "patch_res", "patch_cap", "set_balanced")
NEW_OPS = {"podaff", "podaff_null", "set_terms", "set_profiles", "upload_state", "patch_state", "upload_nodes",
           "upload_zones"}
OPS_SEED = 7272
SIZES = (90, 150, 300, 1100)  # 1, 4 and 16 waves; 1,100 nodes pad to a larger table than the others: the state grows
C = 6


def rand_terms(rng):
    T = int(rng.integers(1, 6))
    topo = [int(x) for x in rng.integers(0, 2, T)]
    return topo


def rand_profiles(rng, T):
    """Three to eight profiles over T terms: sparse match and anti words, an affinity term for every third."""
    Q = int(rng.integers(3, 9))
    one = lambda: int(1 << int(rng.integers(0, T))) if rng.random() < 0.7 else 0  # noqa: E731
    match = [one() | one() for _ in range(Q)]
    anti = [one() if rng.random() < 0.5 else 0 for _ in range(Q)]
    aff = [int(rng.integers(0, T)) if q % 3 == 2 else -1 for q in range(Q)]
    return match, anti, aff


def fresh(ctx, msh, oracle, rng, ps, n, old, topo, prof):
    """A new table of n nodes with every column; the settings are old's (None: the first table)."""
    u, nd, _, _ = rand_case(rng, n, 0, p_unsched=0.15)
    alloc, used, _ = uneven(rng, 2, n, 0)
    bits, _ = KR.gen_bits(rng, n, C)
    A, T = PR.gen_prefs(rng, n, C)
    mode, weight, rw, w, ws, wb = (PA.LEAST, 1, [1, 1], (3, 2), 4, 1) if old is None else \
        (old.mode, old.weight, old.rw, old.w, old.ws, old.wb)
    zone = rng.integers(-1, 4, n)
    return AMirror(ctx, msh, oracle, ps, u, nd, zone, [1, 2, 2], alloc, used, rng.integers(1, 6, n), mode, weight, rw, bits,
                   C, A=A, T=T, PC=C, w=w, modes=[0, 1, 0], ws=ws, wb=wb, topo=topo, prof=prof)


def test_the_drawn_ops_hold_every_new_one():
    ops = {OPS[k] for k in np.random.default_rng(OPS_SEED).integers(0, len(OPS), STEPS)}
    assert NEW_OPS | {"balanced", "prefs", "reset_counts", "patch_res"} <= ops, sorted(set(OPS) - ops)


def test_sixty_step_trace(msh, oracle):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    rng = np.random.default_rng(7271)
    ops = [OPS[k] for k in np.random.default_rng(OPS_SEED).integers(0, len(OPS), STEPS)]  # drawn apart from the inputs
    assert NEW_OPS | {"balanced", "prefs", "reset_counts", "patch_res"} <= set(ops)
    ps = oracle.PluginSet(weights=[2], normalize=[1])
    log = []
    with msh.DeviceContext(0) as ctx:
        topo = [PA.HOSTNAME, PA.ZONE]
        m = fresh(ctx, msh, oracle, rng, ps, SIZES[1], None, topo, rand_profiles(rng, 2))
        for step in range(STEPS):
            op = ops[step]
            n, T, Q = len(m.u), len(m.st.topo), len(m.st.match)
            what = f"step {step}: {op}, n {n}, T {T}, Q {Q}, w_balanced {m.wb} (trace so far: {log[-6:]})"
            log.append(op)
            p = int(rng.integers(1, 90))
            _, _, pd, pt = rand_case(rng, 1, p)
            _, _, req = uneven(rng, 2, 1, p)
            grp = rng.integers(-1, len(m.skew), p).astype(np.int32)
            cls = rng.integers(-1, C, p).astype(np.int32)
            prf = rng.integers(-1, Q, p).astype(np.int32)
            if op == "podaff":
                m.call_pa(pd, pt, grp, cls, prf, req, what=what)
                continue
            if op == "podaff_null":  # no profile column: _balanced, the state untouched
                w = BMirror.expect(m, pd, pt, grp, cls, req)
                m.compare(ctx.schedule_sequential_podaffinity(pd, pt, grp, cls, None, req), w, what)
                m.commit(w)
            elif op == "balanced":  # reads no term, profile or state
                w = BMirror.expect(m, pd, pt, grp, cls, req)
                m.compare(ctx.schedule_sequential_balanced(pd, pt, grp, cls, req), w, what)
                m.commit(w)
            elif op == "prefs":  # without groups: the ctx holds a soft group
                w = PMirror.expect(m, pd, pt, None, cls, req)
                m.compare(ctx.schedule_sequential_prefs(pd, pt, None, cls, req), w, what)
                m.commit(w)
            elif op == "set_terms":  # drops the profiles and zeroes the state
                topo = rand_terms(rng)
                m.terms(topo, rand_profiles(rng, len(topo)))
            elif op == "set_profiles":  # keeps the state
                m.profiles(rand_profiles(rng, T))
            elif op == "upload_state":
                pr = (rng.integers(0, 1 << T, n) * (rng.random(n) < 0.3)).astype(np.uint32)
                rp = (rng.integers(0, 1 << T, n) * (rng.random(n) < 0.3)).astype(np.uint32)
                which = int(rng.integers(0, 3))  # both, present alone (repel: zeros), neither
                ctx.upload_pod_affinity_state(pr if which < 2 else None, rp if which == 0 else None)
                m.st.present[:] = pr if which < 2 else 0
                m.st.repel[:] = rp if which == 0 else 0
            elif op == "patch_state":
                i = rng.permutation(n)[:4].astype(np.int32)
                pr, rp = rng.integers(0, 1 << T, 4).astype(np.uint32), rng.integers(0, 1 << T, 4).astype(np.uint32)
                ctx.patch_pod_affinity_state(i, pr, rp)
                m.st.present[i], m.st.repel[i] = pr, rp
            elif op == "upload_nodes":  # another table size: the state is zeroed, the terms and profiles stay
                n2 = int(rng.choice([s for s in SIZES if s != n]))
                u2, nd2, _, _ = rand_case(rng, n2, 0)
                ctx.upload_nodes(u2, nd2)
                assert np.array_equal(ctx.pod_affinity_terms(), m.st.topo), what
                assert [list(x) for x in ctx.pod_profiles()] == [m.st.match, m.st.anti, m.st.aff], what
                pr, rp = ctx.pod_affinity_state()
                assert len(pr) == n2 and not pr.any() and not rp.any(), what
                m = fresh(ctx, msh, oracle, rng, ps, n2, m, m.st.topo, (m.st.match, m.st.anti, m.st.aff))
            elif op == "upload_zones":  # the derived words follow the new column; the spread counts are zeroed
                m.zone = rng.integers(-1, 5, n).astype(np.int32)
                ctx.upload_node_zones(m.zone)
                m.cnt[:] = 0
            elif op == "reset_counts":
                ctx.reset_node_pod_counts()
                m.counts = np.zeros(n, np.int32)
            elif op == "patch_cnt":
                cells = rng.permutation(len(m.skew) * 4)[:3]
                gi, zi, val = cells // 4, cells % 4, rng.integers(0, 4, len(cells))
                ctx.patch_spread_counts(gi, zi, val)
                m.cnt[gi, zi] = val
            elif op == "patch_res":
                i = rng.permutation(n)[:3].astype(np.int32)
                m.alloc, m.used = m.alloc.copy(), m.used.copy()
                m.used[:, i] = rng.integers(0, 90, (2, 3))
                m.alloc[:, i] = rng.integers(0, 3, (2, 3)) * rng.integers(20, 400, (2, 3))
                ctx.patch_node_resources(i, alloc=m.alloc[:, i], used=m.used[:, i])
            elif op == "patch_cap":
                i = rng.permutation(n)[:3].astype(np.int32)
                m.cap[i] = rng.integers(0, 8, 3)
                ctx.patch_node_capacity(i, m.cap[i])
            elif op == "set_balanced":
                m.balanced_weight(int(rng.choice([0, 1, 2])))
            m.verify(what)
