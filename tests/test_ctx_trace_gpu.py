"""Seeded call traces replayed on one context against the model of tests/ctx_model.py.

The fixed trace set of tests/test_ctx_model.py (TRACE_COUNT traces from TRACE_SEED0) mixes every operation that
changes what a context carries between calls: plugin lists, the tie-break, uploads up and down a ladder of table
sizes (across the 32,768-node line between 64 count replicas and one), patches, score columns, the capacity column,
the resource table, the resource score, and every scheduling entry point. After every step idx / score / status, the
commit callbacks and a refusal's code are compared bit for bit with the model; the read-backs (counts, capacity
column, alloc / used, tie-break, resource score) after every step in the eager half of the traces, and only where the
trace says so in the lazy half, which is what leaves the counts in their replicas across calls so that the next
kernel has to fold them.

The expected values are computed once per session (the CPU references dominate) and shared by all parametrizations.
Measured on an MI355X with the 12 traces of the fixed set (about 110 steps each, 1,321 in all): 5.7 s for the whole
file: 1.4 s for the model computing the expected values once, 0.2 s per pageable replay of the set, 1.0 s per pinned
one, 0.6 s for the two-context test. The first schedule_batches_device step of a process also imports torch and
initialises its device (11 s in a fresh process; nothing when an earlier test of the session has done so), which is
not counted. That is the range of the bounded fuzz sweep (test_fuzz_gpu: 500 cases, about 4 s), so the count stays
at 12.
"""
from __future__ import annotations

import numpy as np
import pytest

import ctx_model as M
from test_ctx_model import READS, _trace_set, describe, expected

pytestmark = pytest.mark.gpu


def _same(a, b):
    return M.same_value(a, b)


class Replay:
    """One trace on one DeviceContext, a step at a time."""

    def __init__(self, msh, ctx, trace, records, pinned, label):
        self.msh, self.ctx, self.trace, self.records = msh, ctx, trace, records
        self.pinned, self.label = pinned, label
        self.k = 0
        self.last_reads = None

    @property
    def done(self):
        return self.k >= len(self.trace["steps"])

    def where(self):
        ops = " ; ".join(describe(s) for s in self.trace["steps"][: self.k + 1])
        return f"{self.label} trace seed {self.trace['seed']} ({'lazy' if self.trace['lazy'] else 'eager'}) step {self.k}: {ops}"

    def _buf(self, a):
        if not self.pinned:
            return a
        out = self.msh.pinned_empty(a.shape, a.dtype)
        out[...] = a
        return out

    def _out(self, p):
        if not self.pinned:
            return None
        pe = self.msh.pinned_empty
        return pe(p, np.int32), pe(p, np.int64), pe(p, np.int32)

    def _call(self, op, a):
        msh, ctx = self.msh, self.ctx
        if op == "set_plugins":
            return ctx.set_plugins(a["filters"], a["prescore"],
                                   [msh.ScorePluginConfig(s, w, msh.Normalize(m)) for s, w, m in a["score"]])
        if op == "upload_nodes":
            return ctx.upload_nodes(a["u"], a["nd"])
        if op == "patch_nodes":
            return ctx.patch_nodes(a["idx"], a["u"], a["nd"])
        if op == "upload_score_column":
            return ctx.upload_score_column(M.COLS[a["k"]], a["scores"])
        if op == "set_resource_score":
            return ctx.set_resource_score(a["mode"], a["weight"], a["rw"])
        if op == "schedule_batch":
            p = len(a["pd"])
            return tuple(np.array(x) for x in ctx.schedule_batch(self._buf(a["pd"]), self._buf(a["pt"]), out=self._out(p)))
        if op == "schedule_batches_device":
            import torch  # only this entry point is driven through torch tensors (as in test_fuzz_gpu)
            dev = torch.device("cuda:0")
            pd, pt, cuts = a["pd"], a["pt"], a["cuts"]
            bufs = [[torch.from_numpy(pd[x:y].copy()).to(dev), torch.from_numpy(pt[x:y].copy()).to(dev),
                     torch.full((y - x,), -7, dtype=torch.int32, device=dev),
                     torch.full((y - x,), -7, dtype=torch.int64, device=dev),
                     torch.full((y - x,), -7, dtype=torch.int32, device=dev)] for x, y in zip(cuts, cuts[1:])]
            descs = ctx.batch_descs([(len(b[0]), *[t.data_ptr() for t in b]) for b in bufs])
            torch.cuda.synchronize()
            ctx.schedule_batches_device(descs, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return tuple(np.concatenate([b[i].cpu().numpy() for b in bufs]) for i in (2, 3, 4))
        if op in ("schedule_sequential", "schedule_sequential_fit"):
            seen = []
            cb = (lambda j, i, s: seen.append((j, i, s))) if a["cb"] else None
            p = len(a["pd"])
            if op == "schedule_sequential":
                got = ctx.schedule_sequential(self._buf(a["pd"]), self._buf(a["pt"]), a["scalar"], on_commit=cb, out=self._out(p))
            else:
                got = ctx.schedule_sequential_fit(self._buf(a["pd"]), self._buf(a["pt"]), a["req"], a["scalar"], on_commit=cb,
                                                  out=self._out(p))
            return tuple(np.array(x) for x in got) + (seen if a["cb"] else None,)
        return getattr(ctx, op)(**a)

    def _read(self, name):
        try:
            return ("ok", getattr(self.ctx, name)())
        except self.msh.MshError as e:
            return ("err", e.code)

    def _check_reads(self, want):
        got = {name: self._read(name) for name in want}
        for name in want:
            assert _same(got[name], want[name]), f"{self.where()}: {name}() differs\n got {got[name]}\nwant {want[name]}"
        return got

    def step(self):
        op, args = self.trace["steps"][self.k]
        rec = self.records[self.k]
        if op == "read":
            self._check_reads(rec["reads"])
        else:
            try:
                got = ("ok", self._call(op, args))
            except self.msh.MshError as e:
                got = ("err", e.code)
            want = rec["result"]
            assert got[0] == want[0] and (got[0] == "ok" or got[1] == want[1]), \
                f"{self.where()}: returned {got if got[0] == 'err' else 'ok'}, the model says {want if want[0] == 'err' else 'ok'}"
            if got[0] == "ok" and want[1] is not None:
                for g, w, name in zip(got[1], want[1], ("idx", "score", "status", "commit callbacks")):
                    if isinstance(w, np.ndarray):
                        bad = np.flatnonzero(np.asarray(g) != w)
                        assert bad.size == 0, (f"{self.where()}: {name} differs at pods {bad[:5].tolist()}: got "
                                               f"{np.asarray(g)[bad[:5]].tolist()} want {w[bad[:5]].tolist()}")
                    else:
                        assert g == w, f"{self.where()}: {name} differ"
            if rec["reads"] is not None:  # the eager policy
                reads = self._check_reads(rec["reads"])
                if got[0] == "err" and self.last_reads is not None:  # a failed call changes nothing
                    for name in READS:
                        assert _same(reads[name], self.last_reads[name]), f"{self.where()}: the refused call changed {name}()"
                self.last_reads = reads
        self.k += 1
        if self.done:
            self._check_reads(self.records[-1]["reads"])


@pytest.fixture(scope="module")
def device(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    return 0


@pytest.mark.parametrize("buffers", ["pageable", "pinned"])
@pytest.mark.parametrize("split", ["auto", "serial", "blocks"])
def test_traces_against_the_model(msh, oracle, device, split, buffers):
    """seq_split decides which of the three count-commit paths a no-capacity call takes (the pair kernel's epilogue,
    64-pod blocks, one workgroup in place) and so whether the next call has to fold; pinned_empty buffers take the
    host entry points' zero-copy path."""
    for t in _trace_set():
        with msh.DeviceContext(0, {"seq_split": split}) as ctx:
            r = Replay(msh, ctx, t, expected(oracle, t["index"]), buffers == "pinned", f"seq_split={split} {buffers}")
            while not r.done:
                r.step()


def test_two_contexts_step_by_step(msh, oracle, device):
    """Two contexts on one device, each on a trace of its own, advanced alternately: what a context carries is its
    own, not the process's."""
    ts = _trace_set()
    for a, b in zip(ts[0::2], ts[1::2]):
        with msh.DeviceContext(0) as c1, msh.DeviceContext(0) as c2:
            r1 = Replay(msh, c1, a, expected(oracle, a["index"]), False, "first of two contexts")
            r2 = Replay(msh, c2, b, expected(oracle, b["index"]), True, "second of two contexts")
            while not (r1.done and r2.done):
                for r in (r1, r2):
                    if not r.done:
                        r.step()
