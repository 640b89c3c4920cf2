"""Soft topology spread (whenUnsatisfiable: ScheduleAnyway) in sequential-commit mode on the GPU
(msh_schedule_sequential_soft and friends; csrc/msh_seq_soft.hip).

Every comparison is bit-exact on idx, score, status, node_pod_counts(), the `used` half of node_resources(),
spread_counts(), the class and preference columns, the group modes and the weights. The expected values come from
tests/soft_spread_ref.py: the plain serial loop for tiny shapes, the numpy per-pod loop otherwise
(tests/test_soft_spread.py shows on the CPU that the two agree, and that no count below 2^20 is rounded differently
by a fused multiply-add, so there is no such case here). The kernel holds NPL nodes per thread on 1, 4 or 16 waves;
the limits are read from msh_seq_soft_max_nodes."""
from __future__ import annotations

import numpy as np
import pytest

import classes_ref as KR
import prefs_ref as PR
import soft_spread_ref as SR
import spread_ref as S
from test_classes import case_plugins
from test_classes_gpu import device_call, mask_bits, rand_amounts, rand_case, refused
from test_prefs_gpu import PMirror
from test_soft_spread import SWEEP_SEEDS

pytestmark = pytest.mark.gpu
NONE, LEAST, MOST = SR.NONE, SR.LEAST, SR.MOST


@pytest.fixture(scope="module")
def ctx(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    c = msh.DeviceContext(0)
    yield c
    c.close()


class SMirror(PMirror):
    """PMirror with the group modes and the spread weight."""

    def __init__(self, ctx, msh, O, ps, u, nd, *a, modes=None, ws=1, **kw):
        kw.setdefault("w", (0, 0))
        super().__init__(ctx, msh, O, ps, u, nd, *a, **kw)
        self.set_modes(np.zeros(len(self.skew), np.uint8) if modes is None else modes)
        self.spread_weight(ws)

    def set_modes(self, modes):
        self.modes = np.array(modes, np.uint8)
        self.ctx.set_spread_group_modes(self.modes)

    def spread_weight(self, ws):
        self.ws = ws
        self.ctx.set_spread_score_weight(ws)

    def expect(self, pd, pt, grp, cls, req=None, scalar=0):
        n, p = len(self.u), len(pd)
        ref = SR.serial if n * p <= 2 * 10**4 else SR.per_pod
        if req is None:
            a, us, rq = S.no_res(n, p)
        else:
            a, us, rq = self.alloc, self.used, np.asarray(req, np.int64)
        return ref(self.O, self.u, self.nd, pd, pt, self.ps, self.eff(scalar), a, us, rq, self.zone, grp, self.skew,
                   self.mode, self.weight, self.rw, self.bits, self.PC or self.C, cls, self.A, self.T, *self.w,
                   self.modes, self.ws, self.counts, self.cnt)

    def call(self, pd, pt, grp, cls, req=None, scalar=0, what=""):
        got = self.ctx.schedule_sequential_soft(pd, pt, grp, cls, req, scalar)
        want = self.expect(pd, pt, grp, cls, req, scalar)
        self.compare(got, want, what)
        self.commit(want, req is not None)
        self.verify(what)
        return want

    def verify(self, what=""):
        super().verify(what)
        assert np.array_equal(self.ctx.spread_group_modes(), self.modes), f"{what}: group modes"
        assert self.ctx.spread_score_weight() == self.ws, f"{what}: spread weight"


def lim_npl(ctx, nres):
    lim = ctx.seq_soft_max_nodes(nres)
    return lim, lim // 1024


def plain(ctx, msh, oracle, zone, skew, modes, cap=None, ws=1, **kw):
    """Schedulable nodes without digits (NodeNumber scores 0 everywhere), no classes."""
    n = len(zone)
    return SMirror(ctx, msh, oracle, oracle.PluginSet(), np.zeros(n, np.uint8), np.full(n, -1, np.int8), zone, skew,
                   cap=cap, modes=modes, ws=ws, **kw)


def pods(p, g=0):
    return np.zeros(p, np.int8), np.ones(p, np.uint8), np.full(p, g, np.int32)


@pytest.mark.parametrize("nres,mode", [(0, NONE)] + [(r, m) for r in (1, 2, 3, 4) for m in (NONE, LEAST, MOST)])
def test_instance_thresholds(msh, oracle, ctx, nres, mode):
    """n = 1, 5, 65, at each wave threshold of the instance and one past it, and the limit, with pods of hard groups,
    of soft groups and of none mixed; one node past the limit is refused with the limit in the message. Sizes past a
    threshold are no multiple of NPL or 32."""
    rng = np.random.default_rng(2000 + 100 * mode + nres)
    lim, npl = lim_npl(ctx, nres)
    assert lim == ctx.seq_prefs_max_nodes(nres) == (4096 if nres <= 2 else 2048)
    ps = oracle.PluginSet(weights=[3], normalize=[(2, 0, 3, 1, 2)[nres]])
    for t, n in enumerate((1, 5, 65, lim // 16, lim // 16 + 1, lim // 4, lim // 4 + 1, lim)):
        p = int(rng.integers(200, 300)) | 1
        u, nd, pd, pt = rand_case(rng, n, p)
        C = int(rng.choice([3, 17, 64]))
        bits, _ = KR.gen_bits(rng, n, C)
        A, T = PR.gen_prefs(rng, n, C)
        cls = rng.integers(-1, C, p).astype(np.int32)
        zone = rng.integers(-1, (8, 64)[t % 2], n)
        grp = rng.integers(-1, 16, p)
        modes = rng.integers(0, 2, 16).astype(np.uint8)
        modes[:2] = (0, 1)
        alloc = used = req = None
        if nres:
            alloc, used, req = rand_amounts(rng, nres, n, p, int(rng.choice([1, 2**33])))
        cap = rng.integers(0, 4, n) if n < 300 else rng.integers(1, 4, n) * (rng.random(n) < 0.4 * p / n)
        m = SMirror(ctx, msh, oracle, ps, u, nd, zone, rng.choice([1, 2, 3], 16), alloc, used, cap, mode,
                    int(rng.choice([1, 7])), rng.integers(1, 101, nres), bits if t % 3 else None, C if t % 3 else 0,
                    A=A, T=T, PC=C, w=(int(rng.integers(0, 101)), int(rng.integers(0, 101))) if t % 4 else (0, 0),
                    modes=modes, ws=int(rng.integers(1, 101)))
        m.call(pd, pt, grp, cls, req, what=f"mode={mode} nres={nres} n={n} p={p}")
    n = lim + 1
    m = SMirror(ctx, msh, oracle, ps, np.zeros(n, np.uint8), np.zeros(n, np.int8), np.zeros(n, np.int32), [1],
                np.ones((nres, n), np.int64) if nres else None, mode=mode, modes=[1])
    msg = refused(msh, msh._native.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_soft, np.zeros(3, np.int8),
                  np.zeros(3, np.uint8), np.zeros(3, np.int32), None, np.ones((nres, 3), np.int64) if nres else None)
    assert f"{lim:,} nodes".replace(",", "") in msg.replace(",", "")
    m.verify("past the limit")


@pytest.mark.parametrize("zones", ["64 in use", "one", "none", "zoned nodes infeasible"])
def test_zones(msh, oracle, ctx, zones):
    """Lane 63 live; a single zone (every ns 100); every node without a zone (Zs empty, ns 0); and the zoned nodes all
    outside the pod's class, so that Zs is empty while F is not."""
    rng = np.random.default_rng(3000)
    n, p = 700, 300
    bits = None
    if zones == "64 in use":
        zone = rng.permutation(np.arange(n) % 64)
    elif zones == "one":
        zone = np.where(rng.random(n) < 0.8, 17, -1)
    elif zones == "none":
        zone = np.full(n, -1)
    else:
        zone = np.where(rng.random(n) < 0.7, rng.integers(0, 5, n), -1)
        bits = mask_bits({0: zone < 0, 1: np.ones(n, bool)})
    u, nd, pd, pt = rand_case(rng, n, p)
    grp = rng.integers(-1, 3, p).astype(np.int32)
    cls = None if bits is None else rng.integers(-1, 2, p).astype(np.int32)
    m = SMirror(ctx, msh, oracle, oracle.PluginSet(weights=[1], normalize=[1]), u, nd, zone, [1, 2, 1], None, None,
                rng.integers(0, 3, n), bits=bits, C=2 if bits is not None else 0, modes=[1, 1, 0], ws=9)
    want = m.call(pd, pt, grp, cls, what=zones)
    soft = (grp >= 0) & (grp < 2) & (want[2] == SR.PLACED)
    if zones == "64 in use":
        assert m.cnt[:2, 63].sum() > 0
    if zones == "none":
        assert soft.sum() > 50 and (want[2][grp == 2] == SR.FIT_ERROR).all() and not m.cnt.any()
    if zones == "zoned nodes infeasible":
        assert (zone[want[0][soft & (cls == 0)]] < 0).all() and (soft & (cls == 0)).sum() > 20


@pytest.mark.parametrize("waves", [4, 16])
def test_phase_skipping_keeps_the_slots_in_step(msh, oracle, ctx, waves):
    """Consecutive pods alternate between running the shared phase for the preferences only (a preferring class, no
    soft group), for the spread only, for both and for neither, in runs of 1, 2 and 3: the slots advance only with the
    pods that use them, and a slot's Zs dwords are zero again when it comes round."""
    lim, npl = lim_npl(ctx, 1)
    n = lim // 4 if waves == 4 else lim - 3
    rng = np.random.default_rng(3100 + waves)
    A = np.zeros((2, n), np.uint16)
    T = np.zeros((2, n), np.uint16)
    A[0], T[0] = rng.integers(0, 101, n), rng.integers(0, 3, n)
    # (class, group): class 0 prefers, class 1 has no raw value; group 0 is soft, group 1 hard
    kinds = {"prefs": (0, 1), "soft": (1, 0), "both": (0, 0), "neither": (-1, -1), "hard": (1, 1)}
    pat = ["prefs", "soft", "both", "neither", "soft", "soft", "prefs", "prefs", "neither", "both", "both", "both",
           "hard", "soft", "neither", "neither", "both", "prefs", "soft", "hard", "hard", "soft", "soft", "soft"]
    cls = np.array([kinds[k][0] for k in pat] * 9, np.int32)
    grp = np.array([kinds[k][1] for k in pat] * 9, np.int32)
    p = len(cls)
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 1, n, p)
    cap = (rng.random(n) < 0.1).astype(np.int64)
    zone = np.where(rng.random(n) < 0.9, rng.integers(0, 64, n), -1)
    m = SMirror(ctx, msh, oracle, oracle.PluginSet(weights=[1], normalize=[3]), u, nd, zone, [2, 3], alloc, used, cap,
                MOST, bits=mask_bits({0: rng.random(n) < 0.7, 1: rng.random(n) < 0.5}), C=2, A=A, T=T, PC=2, w=(5, 11),
                modes=[1, 0], ws=13)
    m.call(pd, pt, grp, cls, req, what="alternating")


def test_commit_guard(msh, oracle, ctx):
    """A soft pod lands on a node without a zone, then pods of the same group follow: no count moves for the first,
    and the followers see the counts unchanged."""
    n = 300
    zone = np.full(n, -1)
    zone[[10, 200]] = (3, 60)
    cap = np.zeros(n, np.int64)
    cap[[5, 299]] = 1  # at first only two nodes without a zone take a pod
    m = plain(ctx, msh, oracle, zone, [1], [1], cap, ws=10)
    first = m.call(*pods(1), None, what="lands on a node without a zone")
    assert first[0][0] == 5 and first[1][0] == 0 and not m.cnt.any()
    ctx.patch_node_capacity([10, 200], [1, 1])
    m.cap = m.cap.copy()
    m.cap[[10, 200]] = 1
    want = m.call(*pods(3), None, what="followers")
    assert want[0].tolist() == [10, 200, 299] and want[1].tolist() == [1000, 1000, 0]
    assert m.cnt[0, 3] == 1 and m.cnt[0, 60] == 1 and m.cnt.sum() == 2


def test_state_across_calls(msh, oracle, ctx):
    """Two calls on one ctx with patch_spread_counts between them; the modes change between calls with the same G; a
    change of G resets the modes."""
    rng = np.random.default_rng(3200)
    n, p = 500, 120
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    zone = rng.integers(-1, 6, n)
    grp = rng.integers(-1, 4, p).astype(np.int32)
    m = SMirror(ctx, msh, oracle, oracle.PluginSet(weights=[2], normalize=[2]), u, nd, zone, [1, 2, 3, 1], alloc, used,
                np.full(n, 2), LEAST, 3, [1, 2], modes=[1, 0, 1, 0], ws=40)
    m.call(pd, pt, grp, None, req, what="first")
    g, z, v = [0, 0, 2, 1], [0, 3, 5, 1], [7, 0, 1000, 2]
    ctx.patch_spread_counts(g, z, v)
    m.cnt[g, z] = v
    m.call(pd, pt, grp, None, req, what="after the patch")
    ctx.set_spread_groups([2, 2, 2, 2])  # the same G: the modes stay
    m.skew = np.array([2, 2, 2, 2], np.int32)
    m.verify("same G")
    m.set_modes([0, 1, 1, 1])
    m.call(pd, pt, grp, None, req, what="other modes")
    ctx.set_spread_groups([1, 1, 1])  # another G: modes and counts reset
    m.skew, m.modes, m.cnt = np.array([1, 1, 1], np.int32), np.zeros(3, np.uint8), np.zeros((3, S.MAX_ZONES), np.int32)
    m.verify("another G")
    refused(msh, msh._native.MSH_ERR_INVALID, ctx.set_spread_group_modes, [1, 1, 1, 1])
    refused(msh, msh._native.MSH_ERR_INVALID, ctx.set_spread_group_modes, [0, 2, 0])
    for bad in (-1, 101):
        refused(msh, msh._native.MSH_ERR_INVALID, ctx.set_spread_score_weight, bad)
    m.verify("after the refused setters")


def test_equivalences(msh, oracle, ctx):
    """No soft group: _soft is _prefs, output for output, whatever w_spread is. With soft groups and w_spread 0 the
    call equals the reference, which is not _prefs: the filter is lifted."""
    rng = np.random.default_rng(3300)
    n, p = 500, 150
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    zone, grp = rng.integers(-1, 4, n), rng.integers(-1, 3, p).astype(np.int32)
    bits, _ = KR.gen_bits(rng, n, 5)
    A, T = PR.gen_prefs(rng, n, 5)
    cls = rng.integers(-1, 5, p).astype(np.int32)
    ps = oracle.PluginSet(weights=[2], normalize=[2])
    args = (zone, [1, 2, 1], alloc, used, np.full(n, 2), LEAST, 3, [1, 2], bits, 5)
    outs = []
    for w in ((13, 7), (0, 0)):
        m = SMirror(ctx, msh, oracle, ps, u, nd, *args, A=A, T=T, PC=5, w=w, ws=100)
        a = m.call(pd, pt, grp, cls, req, what=f"no soft group, w={w}")
        m2 = PMirror(ctx, msh, oracle, ps, u, nd, *args, A=A, T=T, PC=5, w=w)
        b = m2.call(pd, pt, grp, cls, req, what="_prefs")
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        outs.append(b)
    m = SMirror(ctx, msh, oracle, ps, u, nd, *args, A=A, T=T, PC=5, w=(13, 7), modes=[1, 1, 0], ws=0)
    c = m.call(pd, pt, grp, cls, req, what="soft groups, w_spread 0")
    assert not np.array_equal(c[0], outs[0][0])  # not _prefs: the filter is lifted


def test_refusals_change_nothing(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(3400)
    n, p = 200, 30
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    bits, _ = KR.gen_bits(rng, n, 4)
    A, T = PR.gen_prefs(rng, n, 4)
    zone = rng.integers(-1, 4, n)
    grp = rng.integers(-1, 2, p).astype(np.int32)
    cls = rng.integers(-1, 4, p).astype(np.int32)
    m = SMirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1, 2], alloc, used, None, LEAST, 1, [1, 1], bits, 4,
                A=A, T=T, PC=4, w=(2, 3), modes=[0, 1], ws=5)
    m.call(pd, pt, grp, cls, req, what="before")
    # the four existing calls that take pod_group, on a ctx with a soft group
    for name, call in (("spread", lambda: ctx.schedule_sequential_spread(pd, pt, grp, req)),
                       ("spread_scored", lambda: ctx.schedule_sequential_spread_scored(pd, pt, grp, req)),
                       ("classes", lambda: ctx.schedule_sequential_classes(pd, pt, grp, cls, req)),
                       ("prefs", lambda: ctx.schedule_sequential_prefs(pd, pt, grp, cls, req))):
        assert "msh_schedule_sequential_soft" in refused(msh, E.MSH_ERR_UNSUPPORTED, call), name
    m.verify("after the four refusals")
    # without pod groups they run as before
    got = ctx.schedule_sequential_prefs(pd, pt, None, cls, req)
    want = PMirror.expect(m, pd, pt, None, cls, req)
    m.compare(got, want, "_prefs without groups")
    m.commit(want)
    # _prefs' refusals come first: groups without zones, before the key
    m.score(LEAST, 646, [1, 1])
    ctx.clear_node_zones()
    refused(msh, E.MSH_ERR_STATE, ctx.schedule_sequential_soft, pd, pt, grp, cls, req)
    ctx.upload_node_zones(m.zone)
    m.cnt[:] = 0
    # the key's sum: 646 + 2 + 3 + 5 = 656
    assert "656" in refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_soft, pd, pt, grp, cls, req)
    m.score(LEAST, 645, [1, 1])
    m.call(pd, pt, grp, cls, req, what="655 fits")
    m.score(LEAST, 1, [1, 1])
    # MSH_SPREAD_SOFT_MAX through a patched count (a hard group's too: the bound is one number) and through a skew
    ctx.patch_spread_counts([0], [9], [E.SPREAD_SOFT_MAX + 1])
    m.cnt[0, 9] = E.SPREAD_SOFT_MAX + 1
    assert "2^24" in refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_soft, pd, pt, grp, cls, req)
    m.verify("after the count refusal")
    ctx.patch_spread_counts([0, 1], [9, 9], [0, E.SPREAD_SOFT_MAX])
    m.cnt[0, 9], m.cnt[1, 9] = 0, E.SPREAD_SOFT_MAX
    m.call(pd[:5], pt[:5], grp[:5], cls[:5], req[:, :5], what="a count of 2^24 is taken")
    ctx.patch_spread_counts([1], [9], [0])
    m.cnt[1, 9] = 0
    ctx.set_spread_groups([1, E.SPREAD_SOFT_MAX + 1])
    m.skew = np.array([1, E.SPREAD_SOFT_MAX + 1], np.int32)
    assert "max_skew" in refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_soft, pd, pt, grp, cls, req)
    m.verify("after the skew refusal")
    m.set_modes([1, 0])  # the large skew on a hard group is no obstacle
    m.call(pd, pt, grp, cls, req, what="a hard group's skew is not bounded")
    ctx.set_spread_groups([1, E.SPREAD_SOFT_MAX])
    m.skew = np.array([1, E.SPREAD_SOFT_MAX], np.int32)
    m.set_modes([0, 1])
    m.call(pd, pt, grp, cls, req, what="a soft group's skew of 2^24 is taken")


def test_device_form(msh, oracle, ctx):
    """The device form agrees with the host form's reference: group and class values out of range are pods without
    one; two streams, one after the other on the same counts."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3500)
    n, p, C = 300, 250, 5
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 1, n, p)
    bits, _ = KR.gen_bits(rng, n, C)
    A, T = PR.gen_prefs(rng, n, C)
    cls = rng.choice(np.array([-1, -7, C, 0, 1, 2, 3, 4], np.int32), p)
    grp = rng.choice(np.array([-1, -9, 3, S.INT32_MAX, 0, 1, 2], np.int32), p)
    m = SMirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, rng.integers(-1, 7, n), [1, 1, 2], alloc, used, np.full(n, 3),
                LEAST, bits=bits, C=C, A=A, T=T, PC=C, w=(20, 30), modes=[1, 0, 1], ws=50)
    for k in range(2):
        want = m.expect(pd, pt, grp, cls, req)
        got = device_call(torch, ctx.schedule_sequential_soft_device, pd, pt, grp, cls, req,
                          torch.cuda.Stream(torch.device("cuda:0")))
        m.compare(got, want, f"stream {k}")
        m.commit(want)
        m.verify(f"stream {k}")


SWEEP_CHUNKS = [list(SWEEP_SEEDS)[k:k + 15] for k in range(0, len(SWEEP_SEEDS), 15)]


@pytest.mark.parametrize("seeds", SWEEP_CHUNKS, ids=lambda s: f"{s[0]}-{s[-1]}")
def test_random_sweep(msh, oracle, ctx, seeds):
    torch = pytest.importorskip("torch")
    st = torch.cuda.Stream(torch.device("cuda:0"))
    for seed in seeds:
        c = SR.gen_case(seed)
        made = []
        for form in ("host", "device"):
            m = SMirror(ctx, msh, oracle, case_plugins(oracle, c), c["unsched"], c["node_digit"], c["zone"], c["max_skew"],
                        c["alloc"], None, c["cap"], c["score_mode"], c["rs_weight"], c["rw"], c["bits"],
                        c["C"] if c["bits"] is not None else 0, A=c["A"], T=c["T"], PC=c["C"],
                        w=(c["w_aff"], c["w_taint"]), modes=c["modes"], ws=c["w_spread"])
            args = (c["pod_digit"], c["pod_tol"], c["group"], c["pod_class"], c["req"])
            if form == "host":
                made.append(m.call(*args, what=f"seed {seed}"))
            else:
                got = device_call(torch, ctx.schedule_sequential_soft_device, *args, st)
                m.compare(got, made[0], f"seed {seed}, device form")
                m.commit(made[0])
                m.verify(f"seed {seed}, device form")
