"""The frame that seq_fit_kernel, seq_score_kernel and seq_spread_kernel share (csrc/msh_seq_frame.h), run through
each of its policies over the same inputs, bit-exact against the CPU references (resource_fit_ref,
resource_score_ref, spread_ref): idx, score, status, node_pod_counts(), used and spread_counts().

What the frame owns and what goes wrong there shows at these shapes, so they are the cases:
 * tables one node below, at and one above 64 x NPL and 256 x NPL nodes (the 1 / 4 / 16-wave instances), for the
   NPL of the two-resource and of the four-resource instance of each family, and a table of 45 nodes whose last
   plane word is partly padding. The last node alone carries digit 7, so the pods of digit 7 land in the last
   thread that holds a node;
 * calls of 1, 64, 65 and 129 pods, one after the other on carried state: one block, the block boundary and the
   clamped tail of the pod loads;
 * before them a plain sequential call in 64-pod blocks, which leaves counts in the count replicas: the first
   call folds them;
 * with and without a capacity column; a plugin list that needs the first feasible non-match (MINMAX) and one that
   does not (DEFAULT), LEAST and MOST; no score buffer in the device form;
 * for spread, few groups, so that a placed grouped pod directly precedes a pod of its group (the step that needs
   the second barrier)."""
from __future__ import annotations

import numpy as np
import pytest

import node_capacity_ref as CR
import resource_fit_ref as R
import resource_score_ref as RS
import spread_ref as S

pytestmark = pytest.mark.gpu

FAMILIES = ("fit", "least", "most", "spread")
POD_CALLS = (1, 64, 65, 129)
SKEW = [1, 2]
SCORE_WEIGHT = 2


@pytest.fixture(scope="module")
def ctx(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    c = msh.DeviceContext(0, {"seq_split": "blocks"})
    yield c
    c.set_resource_score("none")
    c.close()


def limit(ctx, family, nres):
    if family == "spread":
        return ctx.seq_spread_max_nodes(nres)
    return ctx.seq_fit_max_nodes(nres, scored=family != "fit")


def table_sizes(ctx, family, nres):
    npl = limit(ctx, family, nres) // 1024
    return [45] + [w * 64 * npl + d for w in (1, 4) for d in (-1, 0, 1)]


def inputs(seed, n, nres):
    """One table and one batch for every family: scarce amounts and capacities, and node n - 1 the only match of
    digit 7, open to every pod."""
    rng = np.random.default_rng(seed)
    p = sum(POD_CALLS)
    u = (rng.random(n) < 0.3).astype(np.uint8)
    nd = rng.integers(-1, 7, n).astype(np.int8)
    pd = rng.integers(-1, 8, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    alloc = (rng.integers(0, 9, (nres, n)) * 2**33).astype(np.int64)
    req = (rng.integers(0, 4, (nres, p)) * 2**33).astype(np.int64)
    cap = rng.integers(0, 4, n)
    zone = rng.integers(-1, 3, n)
    grp = rng.integers(-1, len(SKEW), p).astype(np.int32)
    u[-1], nd[-1], cap[-1], zone[-1] = 0, 7, p, 1
    alloc[:, -1] = 2**33 * 4 * p
    return u, nd, pd, pt, alloc, req, cap, zone, grp


class Table:
    """The device's table and the state the references carry for it."""

    def __init__(self, ctx, msh, O, family, ps, u, nd, alloc, zone, with_cap, cap):
        self.ctx, self.O, self.family, self.ps, self.u, self.nd = ctx, O, family, ps, u, nd
        n = len(u)
        ctx.set_plugins(ps.filters, ps.prescore, [msh.ScorePluginConfig(s, w, msh.Normalize(m))
                                                  for s, w, m in zip(ps.score, ps.weights, ps.normalize)])
        ctx.set_tiebreak("first")
        ctx.set_resource_score("none")
        ctx.upload_nodes(u, nd)  # zeroes the counts, drops the columns and the table
        self.alloc, self.used = alloc, np.zeros_like(alloc)
        if alloc.shape[0]:
            ctx.upload_node_resources(alloc)
        self.zone, self.cnt = zone, np.zeros((len(SKEW), S.MAX_ZONES), np.int32)
        if family == "spread":
            ctx.set_spread_groups(SKEW)
            ctx.upload_node_zones(zone)
        self.rw = [1] * alloc.shape[0]
        self.counts = np.zeros(n, np.int32)
        self.eff = S.no_limit(n)
        self.with_cap, self.cap = with_cap, cap

    def plain(self, pd, pt):
        """A plain sequential call in pod blocks (no column yet): counts only, left in the count replicas."""
        n, p = len(self.u), len(pd)
        a, us, rq = S.no_res(n, p)
        want = S.per_pod(self.O, self.u, self.nd, pd, pt, self.ps, self.eff, a, us, rq, self.zone,
                         np.full(p, -1, np.int32), SKEW, self.counts, self.cnt)
        got = self.ctx.schedule_sequential(pd, pt, 0)
        assert all(np.array_equal(g, w) for g, w in zip(got, want[:3])), "plain call"
        self.counts = want[3]
        if self.with_cap:
            self.ctx.upload_node_capacity(self.cap)
            self.eff = CR.effective(self.cap, 0)
        if self.family in ("least", "most"):
            self.ctx.set_resource_score(self.family, SCORE_WEIGHT, self.rw)

    def expect(self, pd, pt, req, grp):
        """(idx, score, status) of the family's reference; the carried state moves on."""
        args = (self.O, self.u, self.nd, pd, pt, self.ps, self.eff)
        if self.family == "fit":
            *out, self.counts, self.used = R.per_pod(*args, self.alloc, self.used, req, self.counts)
        elif self.family == "spread":
            a, us, rq = (self.alloc, self.used, req) if self.alloc.shape[0] else S.no_res(len(self.u), len(pd))
            *out, self.counts, us, self.cnt = S.per_pod(*args, a, us, rq, self.zone, grp, SKEW, self.counts, self.cnt)
            if self.alloc.shape[0]:
                self.used = us
        else:
            mode = RS.LEAST if self.family == "least" else RS.MOST
            *out, self.counts, self.used = RS.per_pod(*args, self.alloc, self.used, req, mode, SCORE_WEIGHT, self.rw,
                                                      self.counts)
        return out

    def call(self, pd, pt, req, grp):
        if self.family == "spread":
            return self.ctx.schedule_sequential_spread(pd, pt, grp, req if self.alloc.shape[0] else None, 0)
        return self.ctx.schedule_sequential_fit(pd, pt, req, 0)

    def verify(self, what):
        assert np.array_equal(self.ctx.node_pod_counts(), self.counts), f"{what}: counts"
        if self.alloc.shape[0]:
            a, b = self.ctx.node_resources()
            assert np.array_equal(a, self.alloc), f"{what}: alloc moved"
            assert np.array_equal(b, self.used), f"{what}: used differs at {np.argwhere(b != self.used)[:5].tolist()}"
        if self.family == "spread":
            assert np.array_equal(self.ctx.spread_counts(), self.cnt), f"{what}: spread counts"


def nres_of(family):
    return (2, 0, 3) if family == "spread" else (2, 3)


CASES = [(f, nres) for f in FAMILIES for nres in nres_of(f)]


@pytest.mark.parametrize("kx,with_cap", [(False, False), (True, True)], ids=["DEFAULT, no column", "MINMAX, column"])
@pytest.mark.parametrize("family,nres", CASES)
def test_frame_through_every_policy(msh, oracle, ctx, family, nres, kx, with_cap):
    ps = oracle.PluginSet(weights=[3], normalize=[3 if kx else 1])
    for n in table_sizes(ctx, family, nres):
        u, nd, pd, pt, alloc, req, cap, zone, grp = inputs(n + nres, n, nres)
        t = Table(ctx, msh, oracle, family, ps, u, nd, alloc, zone, with_cap, cap)
        rng = np.random.default_rng(n)
        t.plain(rng.integers(-1, 7, 70).astype(np.int8), (rng.random(70) < 0.4).astype(np.uint8))
        lo, hit_last, chained = 0, False, False
        for p in POD_CALLS:
            sl = slice(lo, lo + p)
            what = f"{family} nres={nres} n={n} pods {lo}..{lo + p}"
            want = t.expect(pd[sl], pt[sl], req[:, sl], grp[sl])
            got = t.call(pd[sl], pt[sl], req[:, sl], grp[sl])
            for g, w, name in zip(got, want, ("idx", "score", "status")):
                assert np.array_equal(g, w), f"{what}: {name} differs at {np.flatnonzero(np.asarray(g) != np.asarray(w))[:5]}"
            t.verify(what)
            hit_last |= bool((want[0] == n - 1).any())
            g, placed = grp[sl], want[2] == R.PLACED
            chained |= bool(((g[:-1] >= 0) & (g[:-1] == g[1:]) & placed[:-1]).any())
            lo += p
        assert hit_last, f"{family} nres={nres} n={n}: no pod reached the last node"
        assert family != "spread" or chained, "no placed grouped pod directly before a pod of its group"


@pytest.mark.parametrize("family", FAMILIES)
def test_device_form_without_a_score_buffer(msh, oracle, ctx, family):
    """out_score is optional: a null pointer changes nothing else. The 4-wave instance, 129 pods."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    nres = 2
    n = limit(ctx, family, nres) // 4
    u, nd, pd, pt, alloc, req, cap, zone, grp = inputs(7, n, nres)
    p = 129
    pd, pt, req, grp = pd[:p], pt[:p], np.ascontiguousarray(req[:, :p]), grp[:p]
    t = Table(ctx, msh, oracle, family, oracle.PluginSet(weights=[3], normalize=[3]), u, nd, alloc, zone, True, cap)
    t.plain(pd[:70], pt[:70])
    want = t.expect(pd, pt, req, grp)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pd, pt, grp, req)]
    idx = torch.full((p,), -7, dtype=torch.int32, device=dev)
    status = torch.full((p,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if family == "spread":
        ctx.schedule_sequential_spread_device(p, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nres,
                                              d[3].data_ptr(), 0, idx.data_ptr(), 0, status.data_ptr(), 0)
    else:
        ctx.schedule_sequential_fit_device(p, d[0].data_ptr(), d[1].data_ptr(), nres, d[3].data_ptr(), 0,
                                           idx.data_ptr(), 0, status.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(status.cpu().numpy(), want[2])
    t.verify(f"{family} without a score buffer")
