"""Required inter-pod affinity and anti-affinity in sequential-commit mode on the GPU
(msh_schedule_sequential_podaffinity and friends; csrc/msh_seq_podaffinity.hip).

Every comparison is bit-exact on idx, score, status, node_pod_counts(), the `used` half of node_resources(),
spread_counts(), the class and preference columns, the weights, and the read-back terms, profiles and state. The
expected values come from tests/podaffinity_ref.py (tests/test_podaffinity.py checks it on the CPU against hand-written
cases and shows that the seeds used here reach every rule). The kernel holds 4 nodes per thread up to two resources
and 2 above, on 1, 4 or 16 waves: n = 37 / 300 / 1,100 with two resources and 100 / 600 with three reach every
instance; p = 150 crosses a 64-pod block."""
from __future__ import annotations

import re

import numpy as np
import pytest

import classes_ref as KR
import podaffinity_ref as PA
import prefs_ref as PR
import spread_ref as S
from test_balanced_gpu import BMirror
from test_classes_gpu import refused
from test_podaffinity import GPU_CASES, gpu_case

pytestmark = pytest.mark.gpu
NONE, LEAST, MOST = PA.NONE, PA.LEAST, PA.MOST


@pytest.fixture(scope="module")
def ctx(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    c = msh.DeviceContext(0)
    yield c
    c.close()


class AMirror(BMirror):
    """BMirror with the terms, the profiles and the state."""

    def __init__(self, ctx, msh, O, ps, u, nd, *a, topo=(), prof=((), (), ()), **kw):
        super().__init__(ctx, msh, O, ps, u, nd, *a, **kw)  # upload_nodes zeroes the state
        self.terms(topo, prof)

    def terms(self, topo, prof=((), (), ())):
        self.ctx.set_pod_affinity_terms(topo)
        self.st = PA.State(len(self.u), topo)
        if len(topo):
            self.profiles(prof)

    def profiles(self, prof):
        self.ctx.set_pod_profiles(*prof)
        self.st.set_profiles(*prof)

    def expect_pa(self, pd, pt, grp, cls, prf, req=None, scalar=0):
        n, p = len(self.u), len(pd)
        a, us, rq = S.no_res(n, p) if req is None else (self.alloc, self.used, np.asarray(req, np.int64))
        st = self.st.copy()
        want = PA.per_pod(self.O, self.u, self.nd, pd, pt, self.ps, self.eff(scalar), a, us, rq, self.zone, grp,
                          self.skew, self.mode, self.weight, self.rw, self.bits, self.PC or self.C, cls, self.A, self.T,
                          *self.w, self.modes, self.ws, self.wb, st, prf, self.counts, self.cnt)
        return want, st

    def call_pa(self, pd, pt, grp, cls, prf, req=None, scalar=0, what=""):
        got = self.ctx.schedule_sequential_podaffinity(pd, pt, grp, cls, prf, req, scalar)
        want, st = self.expect_pa(pd, pt, grp, cls, prf, req, scalar)
        self.compare(got, want, what)
        self.commit(want, req is not None)
        self.st = st
        self.verify(what)
        return want

    def verify(self, what=""):
        super().verify(what)
        assert np.array_equal(self.ctx.pod_affinity_terms(), self.st.topo), f"{what}: terms"
        if not self.st.topo:
            return
        m, a, f = self.ctx.pod_profiles()
        assert (list(m), list(a), list(f)) == (self.st.match, self.st.anti, self.st.aff), f"{what}: profiles"
        pr, rp = self.ctx.pod_affinity_state()
        assert np.array_equal(pr, self.st.present), f"{what}: present differs at {np.flatnonzero(pr != self.st.present)[:5]}"
        assert np.array_equal(rp, self.st.repel), f"{what}: repel differs at {np.flatnonzero(rp != self.st.repel)[:5]}"


def build(ctx, msh, oracle, c, **over):
    """The mirror of a podaffinity_ref.gen_case dict with test_podaffinity.gpu_case's settings on top."""
    k = dict(c, **over)
    ps = oracle.PluginSet(weights=[k["nn_weight"]], normalize=[k["normalize"]])
    res = k["nres"] > 0
    return AMirror(ctx, msh, oracle, ps, k["unsched"], k["node_digit"], k["zone"], k["skew"],
                   k["alloc"] if res else None, k["used"] if res else None, k["cap"], k["mode"], k["rs_weight"],
                   [1] * k["nres"], k["bits"], k["C"] if k["bits"] is not None else 0, A=k["A"], T=k["T"], PC=k["C"],
                   w=k["w"], modes=k["modes"], ws=k["ws"], wb=k["wb"], topo=k["topo"],
                   prof=(k["match"], k["anti"], k["aff"]))


def pod_args(c):
    return (c["pod_digit"], c["pod_tol"], c["group"], c["pod_class"], c["profile"], c["req"] if c["nres"] else None)


@pytest.mark.parametrize("case", range(len(GPU_CASES)), ids=[f"n{n}-r{r}-T{T}" for n, r, T in GPU_CASES])
def test_matches_the_reference(msh, oracle, ctx, case):
    """Every instance (1, 4 and 16 waves at 4 and at 2 nodes per thread), T = 1 (hostname on even, zone on odd cases)
    and T = 32 with both topologies, LEAST / MOST / NONE, w_balanced 0 and 1, hard and soft groups mixed with
    profiles, classes and preference values present; the state is read back."""
    c = gpu_case(case)
    m = build(ctx, msh, oracle, c)
    want = m.call_pa(*pod_args(c), what=f"case {case}")
    prof = c["profile"] >= 0
    assert (want[2][prof] == PA.PLACED).any() and (want[2][prof] == PA.FIT_ERROR).any()


@pytest.mark.parametrize("nres", [0, 1])
def test_fewer_than_two_resources_without_a_balanced_weight(msh, oracle, ctx, nres):
    """w_balanced == 0: the form takes a table of one resource and a call without requests (the two-resource instance
    with the spare amounts zero), on 1, 4 and 16 waves; with a weight the same call is _balanced's MSH_ERR_STATE."""
    for case in (0, 1, 4):
        c = gpu_case(case)
        over = dict(nres=nres, alloc=c["alloc"][:nres], used=c["used"][:nres], req=c["req"][:nres], wb=0)
        if nres == 0:
            over["mode"] = NONE
        k = dict(c, **over)
        m = build(ctx, msh, oracle, c, **over)
        m.call_pa(*pod_args(k), what=f"case {case}, nres {nres}")
        m.balanced_weight(1)
        refused(msh, msh._native.MSH_ERR_STATE, ctx.schedule_sequential_podaffinity, *pod_args(k))
        m.verify("after the refusal")


def test_null_profile_column_is_balanced(msh, oracle, ctx):
    """pod_profile None: _balanced's outputs and state, the terms' state untouched."""
    c = gpu_case(1)
    outs = []
    for name in ("podaffinity", "balanced"):
        m = build(ctx, msh, oracle, c, wb=1)
        pr = np.arange(c["n"], dtype=np.uint32) % 2
        ctx.upload_pod_affinity_state(pr, None)
        m.st.present[:] = pr
        a = pod_args(c)
        if name == "balanced":
            got = ctx.schedule_sequential_balanced(*a[:4], a[5])
        else:
            got = ctx.schedule_sequential_podaffinity(*a[:4], None, a[5])
        want = m.expect(*a[:4], a[5])
        m.compare(got, want, name)
        m.commit(want, True)
        m.verify(name)
        outs.append(got)
    assert all(np.array_equal(x, y) for x, y in zip(*outs))


def test_all_profiles_minus_one_is_balanced(msh, oracle, ctx):
    """Every pod of profile -1 on the new kernel: _balanced's outputs, and the state stays as uploaded."""
    for case, wb in ((1, 1), (3, 0), (4, 1)):
        c = gpu_case(case)
        m = build(ctx, msh, oracle, c, wb=wb)
        rng = np.random.default_rng(case)
        pr = rng.integers(0, 1 << len(c["topo"]), c["n"]).astype(np.uint32)
        rp = rng.integers(0, 1 << len(c["topo"]), c["n"]).astype(np.uint32)
        ctx.upload_pod_affinity_state(pr, rp)
        m.st.present[:], m.st.repel[:] = pr, rp
        a = pod_args(c)
        none = np.full(c["p"], -1, np.int32)
        want_bal = m.expect(*a[:4], a[5])
        want = m.call_pa(*a[:4], none, a[5], what=f"case {case}")
        assert all(np.array_equal(x, y) for x, y in zip(want, want_bal))
        assert np.array_equal(m.st.present, pr) and np.array_equal(m.st.repel, rp)


def test_state_is_carried_between_calls(msh, oracle, ctx):
    """Two consecutive calls leave what one call of the concatenation leaves."""
    for case in (2, 7):
        c = gpu_case(case)
        h = 70
        a = pod_args(c)
        cut = lambda lo, hi: tuple(None if x is None else (x[:, lo:hi] if x.ndim == 2 else x[lo:hi]) for x in a)
        m = build(ctx, msh, oracle, c)
        w1 = m.call_pa(*cut(0, h), what="first call")
        w2 = m.call_pa(*cut(h, c["p"]), what="second call")
        two = (m.st.present.copy(), m.st.repel.copy(), m.counts.copy())
        whole = build(ctx, msh, oracle, c)
        w = whole.call_pa(*a, what="both at once")
        assert np.array_equal(np.concatenate([w1[0], w2[0]]), w[0]) and np.array_equal(np.concatenate([w1[1], w2[1]]), w[1])
        assert np.array_equal(two[0], whole.st.present) and np.array_equal(two[1], whole.st.repel)
        assert np.array_equal(two[2], whole.counts)


def test_uploaded_and_patched_state_is_read(msh, oracle, ctx):
    """Pods bound before the snapshot, entered by upload and patch, repel and attract like committed ones."""
    c = gpu_case(0)
    m = build(ctx, msh, oracle, c)
    T, n = len(c["topo"]), c["n"]
    rng = np.random.default_rng(77)
    pr, rp = (rng.integers(0, 1 << T, n) * (rng.random(n) < 0.2)).astype(np.uint32), \
             (rng.integers(0, 1 << T, n) * (rng.random(n) < 0.2)).astype(np.uint32)
    ctx.upload_pod_affinity_state(pr, rp)
    m.st.present[:], m.st.repel[:] = pr, rp
    m.verify("after the upload")
    idx = np.array([5, 0, n - 1], np.int32)
    ctx.patch_pod_affinity_state(idx, np.array([1, 0, 1], np.uint32), None)
    m.st.present[idx], m.st.repel[idx] = [1, 0, 1], 0
    m.verify("after the patch")
    m.call_pa(*pod_args(c), what="after upload and patch")
    ctx.upload_pod_affinity_state(None, None)
    m.st.present[:], m.st.repel[:] = 0, 0
    m.verify("zeros")


def test_device_form_treats_profiles_out_of_range_as_none(msh, oracle, ctx):
    torch = pytest.importorskip("torch")
    c = gpu_case(3)
    m = build(ctx, msh, oracle, c)
    Q = len(c["match"])
    rng = np.random.default_rng(5)
    prf = rng.choice(np.array([-1, -5, Q, Q + 7, S.INT32_MAX] + list(range(Q)), np.int32), c["p"])
    a = pod_args(c)
    want, st = m.expect_pa(*a[:4], prf, a[5])
    dev = torch.device("cuda:0")
    keep = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (*a[:4], prf, a[5])]
    p = c["p"]
    outs = (torch.full((p,), -7, dtype=torch.int32, device=dev), torch.full((p,), -7, dtype=torch.int64, device=dev),
            torch.full((p,), -7, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ptr = [0 if t is None else t.data_ptr() for t in keep]
    stream = torch.cuda.Stream(dev)
    ctx.schedule_sequential_podaffinity_device(p, *ptr[:5], c["nres"], ptr[5], 0, outs[0].data_ptr(), outs[1].data_ptr(),
                                               outs[2].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    m.compare([o.cpu().numpy() for o in outs], want, "device form")
    m.commit(want, True)
    m.st = st
    m.verify("device form")
    refused(msh, msh._native.MSH_ERR_INVALID, ctx.schedule_sequential_podaffinity, *a[:4], prf, a[5])
    m.verify("after the host form's refusal")


def test_lds_budget(msh, oracle, ctx):
    """128 groups on 1,100 nodes (the 16-wave instance with 4 nodes per thread) would pass 64 KiB of workgroup memory:
    refused with the count that fits in the message; that count runs, one more does not; 600 nodes with three
    resources take all 128."""
    E = msh._native
    c = gpu_case(4)
    assert (c["n"], c["nres"]) == (1100, 2)
    rng = np.random.default_rng(11)
    grp = rng.integers(-1, 128, c["p"]).astype(np.int32)
    a = pod_args(c)
    m = build(ctx, msh, oracle, c, skew=np.full(128, 2, np.int32), modes=np.zeros(128, np.uint8))
    msg = refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_podaffinity, a[0], a[1], grp, *a[3:])
    fits = int(re.search(r"at most (\d+) spread groups", msg).group(1))
    assert 96 <= fits < 128
    m.verify("after the refusal")
    m.call_pa(a[0], a[1], None, *a[3:], what="128 groups on the ctx, none in the call")
    m = build(ctx, msh, oracle, c, skew=np.full(fits + 1, 2, np.int32), modes=np.zeros(fits + 1, np.uint8))
    refused(msh, E.MSH_ERR_UNSUPPORTED, ctx.schedule_sequential_podaffinity, a[0], a[1], grp % (fits + 1), *a[3:])
    m = build(ctx, msh, oracle, c, skew=np.full(fits, 2, np.int32), modes=np.zeros(fits, np.uint8))
    m.call_pa(a[0], a[1], grp % fits, *a[3:], what=f"{fits} groups")
    c = gpu_case(8)
    assert (c["n"], c["nres"]) == (600, 3)
    a = pod_args(c)
    m = build(ctx, msh, oracle, c, skew=np.full(128, 2, np.int32), modes=np.zeros(128, np.uint8))
    m.call_pa(a[0], a[1], grp, *a[3:], what="128 groups at 2 nodes per thread")


def test_refusals_change_nothing(msh, oracle, ctx):
    E = msh._native
    c = gpu_case(1)
    a = pod_args(c)
    call = ctx.schedule_sequential_podaffinity
    T = len(c["topo"])
    assert T == 1
    # the writers
    m = build(ctx, msh, oracle, c)
    refused(msh, E.MSH_ERR_INVALID, ctx.set_pod_affinity_terms, [0] * 33)
    refused(msh, E.MSH_ERR_INVALID, ctx.set_pod_affinity_terms, [0, 2])
    refused(msh, E.MSH_ERR_INVALID, ctx.set_pod_profiles, [2], [0], [-1])        # a bit at T
    refused(msh, E.MSH_ERR_INVALID, ctx.set_pod_profiles, [0], [2], [-1])
    refused(msh, E.MSH_ERR_INVALID, ctx.set_pod_profiles, [1], [1], [1])         # aff at T
    refused(msh, E.MSH_ERR_INVALID, ctx.set_pod_profiles, [1], [1], [-2])
    refused(msh, E.MSH_ERR_INVALID, ctx.set_pod_profiles, [0] * 65, [0] * 65, [-1] * 65)
    n = c["n"]
    refused(msh, E.MSH_ERR_INVALID, ctx.upload_pod_affinity_state, np.full(n, 2, np.uint32), None)
    lib = msh._native.lib()
    z = np.zeros(n + 1, np.uint32)
    assert lib.msh_upload_pod_affinity_state(ctx.handle, n + 1, msh._native.ptr(z), None) == E.MSH_ERR_INVALID
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_pod_affinity_state, [1, 1], [0, 0], [0, 0])
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_pod_affinity_state, [n], [0], [0])
    refused(msh, E.MSH_ERR_INVALID, ctx.patch_pod_affinity_state, [0], [0], [2])
    m.verify("after the writers' refusals")
    # a profile outside [-1, Q) in the host form
    bad = c["profile"].copy()
    bad[9] = len(c["match"])
    refused(msh, E.MSH_ERR_INVALID, call, *a[:4], bad, a[5])
    # _balanced's refusals with its codes: random tie-break, score columns, the key's sum, nres against the table's
    ctx.set_tiebreak("random", 1)
    refused(msh, E.MSH_ERR_UNSUPPORTED, call, *a)
    ctx.set_tiebreak("first")
    m.score(LEAST, 700, [1, 1])
    assert "the weights" in refused(msh, E.MSH_ERR_UNSUPPORTED, call, *a)
    m.score(c["mode"], c["rs_weight"], [1, 1])
    refused(msh, E.MSH_ERR_INVALID, call, *a[:5], a[5][:1])
    m.balanced_weight(1)
    refused(msh, E.MSH_ERR_STATE, call, *a[:5], None)
    m.balanced_weight(c["wb"])
    m.verify("after _balanced's refusals")
    # no profiles, no terms
    ctx.set_pod_profiles((), (), ())
    assert "msh_set_pod_profiles" in refused(msh, E.MSH_ERR_STATE, call, *a)
    ctx.set_pod_affinity_terms(())
    assert "msh_set_pod_affinity_terms" in refused(msh, E.MSH_ERR_STATE, call, *a)
    for fn, args in ((ctx.set_pod_profiles, ([0], [0], [-1])), (ctx.upload_pod_affinity_state, (None, None)),
                     (ctx.patch_pod_affinity_state, ([0], [0], [0])), (ctx.pod_affinity_state, ())):
        refused(msh, E.MSH_ERR_STATE, fn, *args)
    # a zone term without a zone column
    m = build(ctx, msh, oracle, c, topo=[PA.ZONE])
    ctx.clear_node_zones()
    assert "zone" in refused(msh, E.MSH_ERR_STATE, call, a[0], a[1], None, *a[3:])
    ctx.upload_node_zones(c["zone"])
    m.cnt[:] = 0
    m.call_pa(*a, what="after the refusals")


def test_other_entry_points_ignore_the_terms(msh, oracle, ctx):
    """_balanced and _soft on a ctx that holds terms, profiles and a nonzero state: their own outputs, the state kept."""
    c = gpu_case(2)
    for name in ("schedule_sequential_balanced", "schedule_sequential_soft"):
        m = build(ctx, msh, oracle, c, wb=1 if "balanced" in name else 0)
        m.call_pa(*pod_args(c), what="to have a state")
        assert m.st.present.any() and m.st.repel.any()
        a = pod_args(c)
        got = getattr(ctx, name)(*a[:4], a[5])
        want = m.expect(*a[:4], a[5])
        m.compare(got, want, name)
        m.commit(want, True)
        m.verify(name)


def test_upload_nodes_zeroes_the_state_and_keeps_the_tables(msh, oracle, ctx):
    c = gpu_case(0)
    m = build(ctx, msh, oracle, c)
    m.call_pa(*pod_args(c), what="first")
    assert m.st.present.any()
    ctx.upload_nodes(c["unsched"], c["node_digit"])
    assert np.array_equal(ctx.pod_affinity_terms(), c["topo"])
    assert [list(x) for x in ctx.pod_profiles()] == [c["match"], c["anti"], c["aff"]]
    pr, rp = ctx.pod_affinity_state()
    assert not pr.any() and not rp.any()
    ctx.set_pod_affinity_terms(c["topo"])
    assert len(ctx.pod_profiles()[0]) == 0
