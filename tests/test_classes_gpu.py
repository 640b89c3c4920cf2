"""Per-class node masks in sequential-commit mode on the GPU (msh_schedule_sequential_classes and friends;
csrc/msh_seq_classes.hip).

Every comparison is bit-exact on idx, score, status, node_pod_counts(), the `used` half of node_resources(),
spread_counts() and node_class_bits(). The expected values come from tests/classes_ref.py: the plain serial loop
for tiny shapes, the numpy per-pod loop otherwise (tests/test_classes.py shows on the CPU that the two agree).

The kernels hold NPL nodes per thread on 1, 4 or 16 waves; the limits are read from msh_seq_classes_max_nodes, never
hard-coded."""
from __future__ import annotations

import numpy as np
import pytest

import classes_ref as KR
import node_capacity_ref as CR
import spread_ref as S
from test_classes import SWEEP_SEEDS, case_plugins

pytestmark = pytest.mark.gpu
I32MAX = S.INT32_MAX
NONE, LEAST, MOST = KR.NONE, KR.LEAST, KR.MOST
MODE_NAMES = {NONE: "none", LEAST: "least", MOST: "most"}
U1 = np.uint64(1)


@pytest.fixture(scope="module")
def ctx(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    c = msh.DeviceContext(0)
    yield c
    c.close()


def set_plugins(ctx, msh, ps):
    ctx.set_plugins(ps.filters, ps.prescore,
                    [msh.ScorePluginConfig(s, w, msh.Normalize(m)) for s, w, m in zip(ps.score, ps.weights, ps.normalize)])


def refused(msh, code, fn, *a, **kw):
    with pytest.raises(msh.MshError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value
    return str(ei.value)


def mask_bits(masks) -> np.ndarray:
    """{class: bool mask over the nodes} -> the column."""
    n = len(next(iter(masks.values())))
    bits = np.zeros(n, np.uint64)
    for c, m in masks.items():
        bits |= np.asarray(m, bool).astype(np.uint64) << np.uint64(c)
    return bits


class Mirror:
    """The table on the device and the state the reference carries for it: every call is compared with the
    reference, every read-back with the carried state."""

    def __init__(self, ctx, msh, O, ps, u, nd, zone=None, skew=(), alloc=None, used=None, cap=None, mode=NONE,
                 weight=1, rw=None, bits=None, C=0):
        self.ctx, self.O, self.ps, self.u, self.nd = ctx, O, ps, np.asarray(u, np.uint8), np.asarray(nd, np.int8)
        n = len(u)
        set_plugins(ctx, msh, ps)
        ctx.set_tiebreak("first")
        ctx.upload_nodes(u, nd)  # zeroes the counts, drops the columns and the table
        self.alloc = np.zeros((0, n), np.int64) if alloc is None else np.asarray(alloc, np.int64)
        self.used = np.zeros_like(self.alloc) if used is None else np.array(used, np.int64)
        if alloc is not None:
            ctx.upload_node_resources(self.alloc, self.used)
        self.cap = None if cap is None else np.asarray(cap, np.int64)
        if cap is not None:
            ctx.upload_node_capacity(cap)
        self.skew = np.asarray(skew, np.int32)
        ctx.set_spread_groups(self.skew)
        self.zone = None if zone is None else np.asarray(zone, np.int32)
        if zone is not None:
            ctx.upload_node_zones(self.zone)  # zeroes the spread counts
        self.counts = np.zeros(n, np.int32)
        self.cnt = np.zeros((len(self.skew), S.MAX_ZONES), np.int32)
        self.bits, self.C = None, 0
        if bits is not None:
            self.classes(C, bits)
        self.score(mode, weight, rw)

    def classes(self, C, bits):
        self.ctx.upload_node_class_bits(C, bits)
        self.bits, self.C = np.array(bits, np.uint64), C

    def patch(self, idx, words):
        self.ctx.patch_node_class_bits(idx, words)
        self.bits[np.asarray(idx)] = np.asarray(words, np.uint64)

    def score(self, mode, weight=1, rw=None):
        self.mode, self.weight = mode, weight
        self.rw = [1] * self.alloc.shape[0] if rw is None else list(rw)
        if mode == NONE:
            self.ctx.set_resource_score("none")
        else:
            self.ctx.set_resource_score(MODE_NAMES[mode], weight, self.rw)

    def eff(self, scalar=0):
        n = len(self.u)
        if self.cap is None:
            return np.full(n, scalar, np.int64) if scalar > 0 else S.no_limit(n)
        return CR.effective(self.cap, scalar)

    def expect(self, pd, pt, grp, cls, req=None, scalar=0):
        n, p = len(self.u), len(pd)
        ref = KR.serial if n * p <= 2 * 10**4 else KR.per_pod
        if req is None:
            a, us, rq = S.no_res(n, p)
        else:
            a, us, rq = self.alloc, self.used, np.asarray(req, np.int64)
        return ref(self.O, self.u, self.nd, pd, pt, self.ps, self.eff(scalar), a, us, rq, self.zone, grp, self.skew,
                   self.mode, self.weight, self.rw, self.bits, self.C, cls, self.counts, self.cnt)

    def commit(self, want, with_req=True):
        self.counts, self.cnt = want[3], want[5]
        if with_req:
            self.used = want[4]

    def compare(self, got, want, what):
        for g, w, name in zip(got, want[:3], ("idx", "score", "status")):
            g = np.asarray(g)
            assert np.array_equal(g, w), f"{what}: {name} differs at {np.flatnonzero(g != np.asarray(w))[:5]}"

    def call(self, pd, pt, grp, cls, req=None, scalar=0, what=""):
        got = self.ctx.schedule_sequential_classes(pd, pt, grp, cls, req, scalar)
        want = self.expect(pd, pt, grp, cls, req, scalar)
        self.compare(got, want, what)
        self.commit(want, req is not None)
        self.verify(what)
        return want

    def verify(self, what=""):
        assert np.array_equal(self.ctx.node_pod_counts(), self.counts), f"{what}: counts"
        if self.alloc.shape[0]:
            a, b = self.ctx.node_resources()
            assert np.array_equal(a, self.alloc), f"{what}: alloc moved"
            assert np.array_equal(b, self.used), f"{what}: used differs at {np.argwhere(b != self.used)[:5].tolist()}"
        got = self.ctx.spread_counts()
        assert np.array_equal(got, self.cnt), f"{what}: spread counts differ at {np.argwhere(got != self.cnt)[:5].tolist()}"
        col = self.ctx.node_class_bits()
        if self.bits is None:
            assert col is None, f"{what}: a class column appeared"
        else:
            assert col is not None and col[0] == self.C and np.array_equal(col[1], self.bits), f"{what}: class bits"


def rand_case(rng, n, p, digits=3, p_unsched=0.2):
    u = (rng.random(n) < p_unsched).astype(np.uint8)
    nd = rng.integers(-1, digits, n).astype(np.int8)
    pd = rng.integers(0, digits, p).astype(np.int8)
    pt = (rng.random(p) < 0.4).astype(np.uint8)
    return u, nd, pd, pt


def rand_amounts(rng, nres, n, p, unit=1):
    alloc = (rng.integers(20, 200, (nres, n)) * unit).astype(np.int64)
    used = (rng.integers(0, 10, (nres, n)) * unit).astype(np.int64)
    req = (rng.integers(0, 4, (nres, p)) * unit).astype(np.int64)
    return alloc, used, req


def limit(ctx, nres, mode):
    if mode == NONE:
        ctx.set_resource_score("none")
    else:
        ctx.set_resource_score(MODE_NAMES[mode], 1, [1] * nres)
    return ctx.seq_classes_max_nodes(nres)


def halves_bits(rng, n):
    """Classes 0, 31, 32 and 63 in use at once with C = 64: the word halves and the top bit."""
    masks = {c: rng.random(n) < f for c, f in ((0, 0.5), (31, 0.1), (32, 0.5), (63, 0.3))}
    return mask_bits(masks), np.array([0, 31, 32, 63, -1], np.int32)


# a resource score needs a resource: nres = 0 runs unscored only (the scored refusal is in test_refusals_change_nothing)
@pytest.mark.parametrize("nres,mode", [(0, NONE)] + [(r, m) for r in (1, 2, 3, 4) for m in (NONE, LEAST, MOST)])
def test_instance_thresholds(msh, oracle, ctx, nres, mode):
    """n = 1, 5, around 64, at each wave threshold of the instance, one on either side of it and the limit; one node
    past the limit is refused with the limit in the message. Classes 0, 31, 32 and 63 of C = 64 throughout; every
    other table with spread groups, the others without a zone column and with pod_group None."""
    rng = np.random.default_rng(100 * mode + nres)
    lim = limit(ctx, nres, mode)
    assert lim == ctx.seq_spread_scored_max_nodes(nres) and lim % 1024 == 0
    # a KX normalize mode (REVERSE / MINMAX) and an identity-like one, by nres
    ps = oracle.PluginSet(weights=[3], normalize=[(2, 0, 3, 1, 2)[nres]])
    sizes = (1, 5, 63, 64, 65, lim // 16 - 1, lim // 16, lim // 16 + 1, lim // 4 - 1, lim // 4, lim // 4 + 1, lim)
    for t, n in enumerate(sizes):
        p = int(rng.integers(200, 300)) | 1
        u, nd, pd, pt = rand_case(rng, n, p)
        bits, pool = halves_bits(rng, n)
        cls = rng.choice(pool, p)
        grouped = t % 2 == 0
        zone = rng.integers(-1, 8, n) if grouped else None
        grp = rng.integers(-1, 16, p) if grouped else None
        alloc = used = req = None
        if nres:
            alloc, used, req = rand_amounts(rng, nres, n, p, int(rng.choice([1, 2**33])))
        # pod capacities that sum to about half the batch, so that the pods fill the table to its last wave
        cap = rng.integers(0, 4, n) if n < 300 else rng.integers(1, 4, n) * (rng.random(n) < 0.25 * p / n)
        m = Mirror(ctx, msh, oracle, ps, u, nd, zone, rng.choice([1, 2, 3], 16) if grouped else (), alloc, used,
                   cap, mode, int(rng.choice([1, 7])), rng.integers(1, 101, nres), bits, 64)
        want = m.call(pd, pt, grp, cls, req, what=f"mode={mode} nres={nres} n={n} p={p} grouped={grouped}")
        if n > 300:
            assert want[0].max() >= n - n // 4  # the pods reached the last wave
    n = lim + 1
    m = Mirror(ctx, msh, oracle, ps, np.zeros(n, np.uint8), np.zeros(n, np.int8),
               alloc=np.ones((nres, n), np.int64) if nres else None, mode=mode, bits=np.ones(n, np.uint64), C=1)
    msg = refused(msh, msh._native.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_classes, np.zeros(3, np.int8),
                  np.zeros(3, np.uint8), None, np.zeros(3, np.int32), np.ones((nres, 3), np.int64) if nres else None)
    assert f"{lim} nodes" in msg
    m.verify("past the limit")


def test_a_class_admitting_no_node(msh, oracle, ctx):
    rng = np.random.default_rng(7)
    n, p = 700, 120
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, alloc=alloc, used=used, mode=LEAST,
               bits=mask_bits({0: np.ones(n, bool), 1: np.zeros(n, bool)}), C=2)
    want = m.call(pd, pt, None, np.ones(p, np.int32), req, what="class 1 admits nothing")
    assert (want[2] == KR.FIT_ERROR).all() and (want[0] == -1).all()
    assert not m.counts.any() and np.array_equal(m.used, used)


@pytest.mark.parametrize("mode", [NONE, MOST])
def test_one_admitted_node_fills_mid_batch(msh, oracle, ctx, mode):
    """A class admitting exactly one node, at the first and last slot of a thread, of a wave and of a 32-node word,
    under a capacity that fills it mid-batch: PLACED until it is full, FIT_ERROR after."""
    nres = 2
    lim = limit(ctx, nres, mode)
    npl = lim // 1024
    n = lim // 4  # the 4-wave instance
    spots = sorted({0, npl - 1, npl, 31, 32, 64 * npl - 1, 64 * npl, n - 1})
    rng = np.random.default_rng(11)
    for spot in spots:
        p, room = 40, 13
        u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.0)
        one = np.zeros(n, bool)
        one[spot] = True
        cap = np.full(n, 100)
        cap[spot] = room
        alloc = np.full((nres, n), 10**6, np.int64)
        req = rng.integers(0, 5, (nres, p)).astype(np.int64)
        m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, alloc=alloc, cap=cap, mode=mode,
                   bits=mask_bits({5: one, 6: ~one}), C=7)
        want = m.call(pd, pt, None, np.full(p, 5, np.int32), req, what=f"node {spot}")
        assert (want[2][:room] == KR.PLACED).all() and (want[0][:room] == spot).all()
        assert (want[2][room:] == KR.FIT_ERROR).all() and m.counts[spot] == room and m.counts.sum() == room


@pytest.mark.parametrize("mode", [NONE, LEAST])
def test_a_class_whose_nodes_lie_in_a_zone_that_spread_forbids(msh, oracle, ctx, mode):
    n, p = 600, 6
    zone = np.arange(n) % 2
    u, nd = np.zeros(n, np.uint8), np.zeros(n, np.int8)
    alloc = np.full((1, n), 1000, np.int64)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, zone, [1], alloc, mode=mode,
               bits=mask_bits({0: zone == 0, 1: np.ones(n, bool)}), C=2)
    pd, pt = np.zeros(p, np.int8), np.zeros(p, np.uint8)
    # pod 0 (class 1) goes to zone 0; zone 0 then leads by one, and class 0's nodes all lie there
    cls = np.array([1, 0, 0, 1, 0, 0], np.int32)
    want = m.call(pd, pt, np.zeros(p, np.int32), cls, np.full((1, p), 10, np.int64), what="barred zone")
    assert want[2].tolist() == [0, 1, 1, 0, 0, 1] and zone[want[0][3]] == 1 and zone[want[0][4]] == 0


@pytest.mark.parametrize("mode", [NONE, LEAST])
@pytest.mark.parametrize("nm", [1, 2, 3])
def test_extents_come_from_the_class_filtered_set(msh, oracle, ctx, mode, nm):
    """A class that hides every digit match: NodeNumber's normalizer must see non-matches only."""
    rng = np.random.default_rng(nm)
    n, p = 300, 50
    nd = rng.integers(0, 3, n).astype(np.int8)
    u = np.zeros(n, np.uint8)
    alloc, used, req = rand_amounts(rng, 1, n, p)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(weights=[5], normalize=[nm]), u, nd, alloc=alloc, used=used, mode=mode,
               bits=mask_bits({0: nd != 0, 1: np.ones(n, bool)}), C=2)
    pd = np.zeros(p, np.int8)
    cls = (np.arange(p) % 2 == 0).astype(np.int32)  # even pods class 1 (all nodes), odd pods class 0 (no match)
    want = m.call(pd, np.zeros(p, np.uint8), None, cls, req, what=f"normalize {nm}")
    assert (want[2] == KR.PLACED).all() and (nd[want[0][1::2]] != 0).all()
    # a pod that sees every node takes a match, except under REVERSE, where the match scores lowest
    assert (nd[want[0][0::2]] == 0).any() == (nm != 2)


def device_call(torch, fn, pd, pt, grp, cls, req, stream):
    dev = torch.device("cuda:0")
    h = len(pd)
    keep = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pd, pt, grp, cls, req)]
    outs = (torch.full((h,), -7, dtype=torch.int32, device=dev), torch.full((h,), -7, dtype=torch.int64, device=dev),
            torch.full((h,), -7, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ptr = [0 if t is None else t.data_ptr() for t in keep]
    fn(h, ptr[0], ptr[1], ptr[2], ptr[3], 0 if req is None else req.shape[0], ptr[4], 0, outs[0].data_ptr(),
       outs[1].data_ptr(), outs[2].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("mode", [NONE, LEAST])
def test_device_form_without_classes_is_spread_scored(msh, oracle, ctx, mode):
    """pod_class NULL against _spread_scored on the same inputs, with and without a column on the ctx."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(21 + mode)
    n, p = 700, 333
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    zone, grp = rng.integers(-1, 5, n), rng.integers(-1, 4, p).astype(np.int32)
    st = torch.cuda.Stream(torch.device("cuda:0"))
    outs = []
    for bits in (None, mask_bits({0: rng.random(n) < 0.5})):
        for entry in ("classes", "spread_scored"):
            m = Mirror(ctx, msh, oracle, oracle.PluginSet(weights=[3], normalize=[2]), u, nd, zone, [1, 2, 1], alloc, used,
                       np.full(n, 2), mode, bits=bits, C=1 if bits is not None else 0)
            want = m.expect(pd, pt, grp, None, req)
            if entry == "classes":
                got = device_call(torch, ctx.schedule_sequential_classes_device, pd, pt, grp, None, req, st)
            else:
                fn = ctx.schedule_sequential_spread_scored_device
                got = device_call(torch, lambda h, a, b, g, c, *rest: fn(h, a, b, g, *rest), pd, pt, grp, None, req, st)
            m.compare(got, want, f"{entry}, column {bits is not None}")
            m.commit(want)
            m.verify(entry)
            outs.append(got)
    for got in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got, outs[0]))


@pytest.mark.parametrize("mode", [NONE, LEAST])
def test_host_form_without_classes_is_spread_scored(msh, oracle, ctx, mode):
    """The host entry point with pod_class None and groups against _spread_scored on an identically prepared ctx:
    outputs and the state after the call, over two pod blocks (one of them partial) and a C = 3 column on the ctx."""
    rng = np.random.default_rng(23 + mode)
    n, p = 40, 70
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    zone, grp = rng.integers(-1, 3, n), rng.integers(-1, 2, p).astype(np.int32)
    bits = mask_bits({c: rng.random(n) < 0.5 for c in range(3)})
    outs = []
    for entry in ("classes", "spread_scored"):
        m = Mirror(ctx, msh, oracle, oracle.PluginSet(weights=[3], normalize=[2]), u, nd, zone, [1, 2], alloc, used,
                   np.full(n, 3), mode, bits=bits, C=3)
        want = m.expect(pd, pt, grp, None, req)
        if entry == "classes":
            got = ctx.schedule_sequential_classes(pd, pt, grp, None, req)
        else:
            got = ctx.schedule_sequential_spread_scored(pd, pt, grp, req)
        m.compare(got, want, entry)
        m.commit(want)
        m.verify(entry)
        outs.append(got)
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("mode", [NONE, MOST])
def test_device_form_without_groups_or_zones_is_fit(msh, oracle, ctx, mode):
    """pod_group NULL without a zone column against _fit (mode NONE) and the scored _fit."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(31 + mode)
    n, p = 900, 301
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 3, n, p)
    cap = rng.integers(0, 3, n)
    st = torch.cuda.Stream(torch.device("cuda:0"))
    ps = oracle.PluginSet(weights=[2], normalize=[3])
    m = Mirror(ctx, msh, oracle, ps, u, nd, alloc=alloc, used=used, cap=cap, mode=mode)
    assert ctx.node_zones() is None and ctx.node_class_bits() is None
    want = m.expect(pd, pt, None, None, req)
    got = device_call(torch, ctx.schedule_sequential_classes_device, pd, pt, None, None, req, st)
    m.compare(got, want, "classes without groups")
    m.commit(want)
    m.verify("classes without groups")
    m2 = Mirror(ctx, msh, oracle, ps, u, nd, alloc=alloc, used=used, cap=cap, mode=mode)
    fit = ctx.schedule_sequential_fit(pd, pt, req)
    m2.compare(fit, want, "_fit on the same inputs")
    m2.commit(want)
    m2.verify("_fit")


def test_device_form_treats_classes_out_of_range_as_none(msh, oracle, ctx):
    """Ordinary input of the unvalidated device form: -1, -7, C and 2^31 - 1 are pods without a class."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(41)
    n, p, C = 300, 333, 5
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 1, n, p)
    bits, _ = KR.gen_bits(rng, n, C)
    cls = rng.choice(np.array([-1, -7, C, I32MAX, 0, 1, 2, 3, 4], np.int32), p)
    assert all((cls == v).any() for v in (-1, -7, C, I32MAX))
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, alloc=alloc, used=used, mode=LEAST, bits=bits, C=C)
    want = m.expect(pd, pt, None, cls, req)
    clean = m.expect(pd, pt, None, np.where((cls >= 0) & (cls < C), cls, -1), req)
    assert all(np.array_equal(a, b) for a, b in zip(want, clean))
    got = device_call(torch, ctx.schedule_sequential_classes_device, pd, pt, None, cls, req,
                      torch.cuda.Stream(torch.device("cuda:0")))
    m.compare(got, want, "out-of-range classes")
    m.commit(want)
    m.verify("out-of-range classes")
    # the host form refuses them and changes nothing
    for bad in (-7, C, I32MAX):
        msg = refused(msh, msh._native.MSH_ERR_INVALID, ctx.schedule_sequential_classes, pd[:3], pt[:3], None,
                      np.array([0, bad, 1], np.int32), req[:, :3])
        assert "class" in msg
    m.verify("after the refusals")


@pytest.mark.parametrize("mode", [NONE, LEAST])
def test_state_is_carried_and_a_patch_opens_and_closes_classes(msh, oracle, ctx, mode):
    rng = np.random.default_rng(51)
    n, p = 1100, 400
    u, nd, pd, pt = rand_case(rng, n, p, p_unsched=0.0)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    zone, grp = rng.integers(0, 4, n), rng.integers(-1, 3, p).astype(np.int32)
    a = np.zeros(n, bool)
    a[[3, 700]] = True  # class 0: two nodes of capacity 2, full after the first call
    b = rng.random(n) < 0.3
    cap = np.full(n, 5)
    cap[[3, 700]] = 2
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(weights=[2], normalize=[1]), u, nd, zone, [2, 2, 3], alloc, used, cap,
               mode, bits=mask_bits({0: a, 1: b}), C=2)
    cls = rng.integers(-1, 2, p).astype(np.int32)
    cls[:12] = 0
    w1 = m.call(pd, pt, grp, cls, req, what="first call")
    assert m.counts[3] == 2 and m.counts[700] == 2 and (w1[2][cls == 0] == KR.FIT_ERROR).sum() >= 8
    # between the calls: node 900 opens the full class 0, and class 1 closes on every node the patch names
    idx = np.array([900, 3, 10, 11], np.int32)
    m.patch(idx, np.array([1, 0, 0, 2], np.uint64))
    w2 = m.call(pd, pt, grp, cls, req, what="second call")
    z = w2[0][(cls == 0) & (w2[2] == KR.PLACED)]
    assert len(z) and (z == 900).all() and not np.isin(w2[0][cls == 1], [3, 10]).any()


def test_lifetime_rules(msh, oracle, ctx):
    rng = np.random.default_rng(61)
    n, p = 130, 40
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 1, n, p)
    bits, _ = KR.gen_bits(rng, n, 9)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, rng.integers(0, 3, n), [1], alloc, used, rng.integers(1, 4, n),
               bits=bits, C=9)
    cls = rng.integers(-1, 9, p).astype(np.int32)
    m.call(pd, pt, None, cls, req, what="before")
    # every other writer keeps the column
    ctx.patch_nodes([0], [0], [1])
    m.u[0], m.nd[0] = 0, 1
    ctx.patch_node_capacity([1], [3])
    m.cap[1] = 3
    ctx.patch_node_resources([2], alloc[:, [2]] + 5)
    m.alloc = m.alloc.copy()
    m.alloc[:, 2] += 5
    ctx.upload_node_zones(m.zone)
    m.cnt[:] = 0
    ctx.reset_node_pod_counts()
    m.counts[:] = 0
    m.verify("after the other writers")
    # the other sequential entry points ignore the column
    got = ctx.schedule_sequential_spread_scored(pd, pt, np.full(p, -1, np.int32), req)
    want = m.expect(pd, pt, None, None, req)
    m.compare(got, want, "_spread_scored ignores the column")
    m.commit(want)
    m.verify("_spread_scored")
    m.call(pd, pt, np.zeros(p, np.int32), cls, req, what="after")
    # clear: no column; pod_class then needs one, pod_class None does not
    ctx.clear_node_class_bits()
    keep, m.bits, m.C = m.bits, None, 0
    m.verify("cleared")
    refused(msh, msh._native.MSH_ERR_STATE, ctx.schedule_sequential_classes, pd, pt, None, cls, req)
    refused(msh, msh._native.MSH_ERR_STATE, ctx.patch_node_class_bits, [0], [1])
    m.call(pd, pt, None, None, req, what="no column, no classes")
    m.classes(9, keep)
    # upload_nodes drops it
    ctx.upload_nodes(u, nd)
    assert ctx.node_class_bits() is None


def test_refusals_change_nothing(msh, oracle, ctx):
    E = msh._native
    rng = np.random.default_rng(71)
    n, p = 200, 30
    u, nd, pd, pt = rand_case(rng, n, p)
    alloc, used, req = rand_amounts(rng, 2, n, p)
    bits, _ = KR.gen_bits(rng, n, 4)
    m = Mirror(ctx, msh, oracle, oracle.PluginSet(), u, nd, None, [1], alloc, used, bits=bits, C=4)
    cls = rng.integers(-1, 4, p).astype(np.int32)
    m.call(pd, pt, None, cls, req, what="before")
    full = np.full(n, 15, np.uint64)
    # the column's writers
    refused(msh, E.MSH_ERR_INVALID, ctx.upload_node_class_bits, 4, full[:-1])       # n differs
    refused(msh, E.MSH_ERR_INVALID, ctx.upload_node_class_bits, 0, full)            # C outside [1, 64]
    refused(msh, E.MSH_ERR_INVALID, ctx.upload_node_class_bits, 65, full)
    refused(msh, E.MSH_ERR_INVALID, ctx.upload_node_class_bits, 3, full)            # bit 3 with C = 3
    top = full.copy()
    top[7] |= U1 << np.uint64(63)
    refused(msh, E.MSH_ERR_INVALID, ctx.upload_node_class_bits, 63, top)
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_node_class_bits, [0, 0], [1, 1])      # duplicate
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_node_class_bits, [n], [1])            # out of range
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_node_class_bits, [-1], [1])
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_node_class_bits, [0, 1], [1, 16])     # bit 4 with C = 4
    m.verify("after the refused writers")
    # the call: _spread_scored's refusals
    grp = np.zeros(p, np.int32)
    refused(msh, E.MSH_ERR_STATE, ctx.schedule_sequential_classes, pd, pt, grp, cls, req)          # groups, no zones
    refused(msh, E.MSH_ERR_INVALID, ctx.schedule_sequential_classes, pd, pt, None, cls, req[:1])   # nres != table's
    refused(msh, E.MSH_ERR_INVALID, ctx.schedule_sequential_classes, pd, pt, None, cls, -req)
    refused(msh, E.MSH_ERR_INVALID, ctx.schedule_sequential_classes, pd, pt, None, np.full(p, 4, np.int32), req)
    ctx.upload_node_zones(np.zeros(n, np.int32))
    m.zone = np.zeros(n, np.int32)
    refused(msh, E.MSH_ERR_INVALID, ctx.schedule_sequential_classes, pd, pt, np.full(p, 1, np.int32), cls, req)  # G = 1
    m.score(LEAST, 1, [1, 1])
    refused(msh, E.MSH_ERR_STATE, ctx.schedule_sequential_classes, pd, pt, None, cls, None)        # nres != setting's
    ctx.set_tiebreak("random", 1)
    refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_classes, pd, pt, None, cls, req)
    ctx.set_tiebreak("first")
    m.verify("after the refused calls")
    m.call(pd, pt, grp, cls, req, what="after")
    # before msh_upload_nodes
    c2 = msh.DeviceContext(0)
    try:
        refused(msh, E.MSH_ERR_STATE, c2.upload_node_class_bits, 1, np.zeros(0, np.uint64))
        refused(msh, E.MSH_ERR_STATE, c2.patch_node_class_bits, [0], [1])
        refused(msh, E.MSH_ERR_STATE, c2.schedule_sequential_classes, pd, pt, None, None)
    finally:
        c2.close()


SWEEP_CHUNKS = [list(SWEEP_SEEDS)[k:k + 15] for k in range(0, len(SWEEP_SEEDS), 15)]


@pytest.mark.parametrize("seeds", SWEEP_CHUNKS, ids=lambda s: f"{s[0]}-{s[-1]}")
def test_random_sweep(msh, oracle, ctx, seeds):
    for seed in seeds:
        c = KR.gen_case(seed, max_n=1024, max_p=500)
        m = Mirror(ctx, msh, oracle, case_plugins(oracle, c), c["unsched"], c["node_digit"], c["zone"], c["max_skew"],
                   c["alloc"], None, c["cap"], c["score_mode"], c["rs_weight"], c["rw"], c["bits"], c["C"])
        m.call(c["pod_digit"], c["pod_tol"], c["group"], c["pod_class"], c["req"], what=f"seed {seed}")


def test_scheduler_end_to_end(msh, oracle):
    """Object pods and nodes with selectors, affinity terms and taints through Scheduler.schedule_sequential, against
    node_admits + classes_ref."""
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    rng = np.random.default_rng(81)
    n, p = 150, 260
    pools, zones = ("gpu", "cpu", "arm"), ("z0", "z1", "z2")
    nodes = []
    for i in range(n):
        labels = {"pool": pools[int(rng.integers(0, 3))], "zone": zones[int(rng.integers(0, 3))], "gen": str(int(rng.integers(1, 9)))}
        taints = []
        if rng.random() < 0.2:
            taints.append({"key": "dedicated", "value": "ml", "effect": "NoSchedule"})
        if rng.random() < 0.1:
            taints.append({"key": "soft", "value": "", "effect": "PreferNoSchedule"})
        nodes.append({"metadata": {"name": f"node{i:04d}", "labels": labels}, "spec": {"taints": taints, "unschedulable": bool(rng.random() < 0.1)},
                      "status": {"allocatable": {"cpu": "4", "memory": "8Gi", "pods": 3}}})
    shapes = [
        {},
        {"nodeSelector": {"pool": "gpu"}},
        {"nodeSelector": {"pool": "cpu", "zone": "z1"}},
        {"tolerations": [{"key": "dedicated", "operator": "Equal", "value": "ml", "effect": "NoSchedule"}]},
        {"tolerations": [{"operator": "Exists"}], "nodeSelector": {"pool": "arm"}},
        {"affinity": {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
            {"matchExpressions": [{"key": "gen", "operator": "Gt", "values": ["5"]}]},
            {"matchExpressions": [{"key": "pool", "operator": "NotIn", "values": ["gpu", "cpu"]}]}]}}}},
        {"affinity": {"nodeAffinity": {"requiredDuringSchedulingIgnoredDuringExecution": {"nodeSelectorTerms": [
            {"matchFields": [{"key": "metadata.name", "operator": "In", "values": ["node0007"]}]}]}}}},
        {"nodeName": "node0042"},
        {"nodeSelector": {"pool": "tpu"}},
    ]
    pods = []
    for j in range(p):
        spec = dict(shapes[int(rng.integers(0, len(shapes)))])
        spec["containers"] = [{"resources": {"requests": {"cpu": f"{int(rng.integers(0, 3)) * 500}m", "memory": "1Gi"}}}]
        pods.append({"metadata": {"name": f"pod{j}", "labels": {"app": ("web", "db", "x")[j % 3]}}, "spec": spec})
    s = msh.Scheduler(resources=("cpu", "memory"), resource_score="least", zones="zone", spread_groups={"web": 1, "db": 2})
    try:
        res = s.schedule_sequential(pods, nodes)
        # the reference, from node_admits directly: one class per pod shape
        order = s.nodes.order
        nl = [nodes[i] for i in order]
        reps = {}
        for pd_ in pods:
            reps.setdefault(msh.constraints.class_key(pd_), pd_)
        keys = list(reps)
        bits = np.zeros(n, np.uint64)
        for k, kk in enumerate(keys):
            bits |= np.array([msh.node_admits(reps[kk], x) for x in nl], bool).astype(np.uint64) << np.uint64(k)
        cls = np.array([keys.index(msh.constraints.class_key(x)) for x in pods], np.int32)
        table = msh.pack_pods(pods)
        zone = s.node_zone_ids()[0]
        alloc = np.array([[4000, 8 << 30]] * n, np.int64).T
        req = np.array([msh.snapshot.pod_requests(x, ("cpu", "memory")) for x in pods], np.int64).T
        want = KR.per_pod(oracle, s.nodes.unsched, s.nodes.digit, table.digit, table.tolerates, oracle.PluginSet(),
                          np.full(n, 3), alloc, np.zeros_like(alloc), req, zone, s.pod_group_ids(pods), [1, 2], LEAST, 1,
                          [1, 1], bits, len(keys), cls)
        got_idx = np.array([r.node_index if r.outcome == msh.Outcome.PLACED else -1 for r in res])
        assert np.array_equal(got_idx, want[0])
        assert [int(r.outcome == msh.Outcome.PLACED) for r in res] == (want[2] == KR.PLACED).astype(int).tolist()
        assert np.array_equal(s.ctx.node_pod_counts(), want[3])
        placed = want[2] == KR.PLACED
        assert placed.sum() > 50 and (~placed).sum() > 20
        assert not placed[[j for j, x in enumerate(pods) if x["spec"].get("nodeSelector") == {"pool": "tpu"}]].any()
    finally:
        s.close()
