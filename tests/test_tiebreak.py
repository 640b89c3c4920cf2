"""MSH_TIEBREAK_RANDOM without a GPU: the draw, the CPU reference (tiebreak_ref.pick) against the oracle,
its uniformity, the two ABI symbols and the Python mirror's argument checks."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import tiebreak_ref as ref

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "mini-kube-scheduler_amd" / "csrc"


def test_draw_is_splitmix64():
    """The published SplitMix64 test vector (seed 0), and the vectorised form against the scalar one."""
    assert [ref.draw64(0, k) for k in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert [ref.draw(0, k) for k in range(3)] == [0xE220A839, 0x6E789E6A, 0x06C45D18]
    for seed, base in [(0, 0), (0x6D696E69, 5), ((1 << 64) - 1, (1 << 64) - 3)]:
        assert [int(x) for x in ref.draws(seed, base, 7)] == [ref.draw(seed, (base + j) & ref.M64) for j in range(7)]


def _case(rng, n, p):
    unsched = (rng.random(n) < 0.3).astype(np.uint8)
    nd = rng.integers(0, 10, n).astype(np.int8)
    nd[rng.random(n) < 0.02] = -1
    pd = rng.integers(0, 10, p).astype(np.int8)
    pd[rng.random(p) < 0.02] = -1
    pt = (rng.random(p) < 0.05).astype(np.uint8)
    return unsched, nd, pd, pt


@pytest.mark.parametrize("weight", [1, 3, 1 << 32])
@pytest.mark.parametrize("norm", [0, 1, 2, 3])
def test_reference_against_oracle(oracle, norm, weight):
    """Score and status are the first-max oracle's (the tie-break only chooses among equal totals); the
    chosen node is feasible and, by the oracle's per-pair arithmetic, carries the oracle's score."""
    rng = np.random.default_rng(7 + 10 * norm + weight % 97)
    u, nd, pd, pt = _case(rng, 300, 500)
    ps = oracle.PluginSet(weights=[weight], normalize=[norm])
    idx, score, status = ref.pick(u, nd, pd, pt, ps, seed=0x6D696E69, base=11)
    oi, osc, ost, _ = oracle.c_schedule_batch(u, nd, pd, pt, ps)
    assert np.array_equal(status, ost) and np.array_equal(score, osc)
    placed = status == 0
    assert np.array_equal(idx < 0, ~placed) and placed.any()
    j = np.flatnonzero(placed)
    assert not np.any(u[idx[j]].astype(bool) & ~pt[j].astype(bool)), "an infeasible node was chosen"
    # the chosen node's total equals the maximum: with that node moved to the head of the same node list
    # (the same feasible set, so the same extents and the same maximum), the first-max oracle picks it
    for jj in j[:80]:
        order = np.r_[idx[jj], np.delete(np.arange(len(u)), idx[jj])]
        i1, s1, st1, _ = oracle.c_schedule_batch(u[order], nd[order], pd[jj:jj + 1], pt[jj:jj + 1], ps)
        assert (i1[0], s1[0], st1[0]) == (0, osc[jj], 0), (jj, idx[jj], i1[0], s1[0], osc[jj])
    assert np.any(idx[j] != oi[j]), "the random tie-break never left the first maximum"


def test_reference_is_uniform():
    """10 tied nodes, 64,000 pods of one digit: every node receives 6,400 pods within 5%."""
    n, p = 10, 64_000
    ps = type("P", (), dict(filters=["NodeUnschedulable"], prescore=["NodeNumber"], score=["NodeNumber"],
                            weights=[1], normalize=[0]))
    idx, _, status = ref.pick(np.zeros(n, np.uint8), np.full(n, 3, np.int8), np.full(p, 3, np.int8),
                              np.zeros(p, np.uint8), ps, seed=0x6D696E69, base=0)
    assert (status == 0).all()
    counts = np.bincount(idx, minlength=n)
    print("per-node share of 6,400:", counts.min() / 6400, counts.max() / 6400)
    assert counts.min() >= 0.95 * 6400 and counts.max() <= 1.05 * 6400


def test_abi_symbols_and_null_ctx(msh):
    lib = msh._native.lib()
    assert "msh_set_tiebreak" in msh._native.EXPORTED and "msh_get_tiebreak" in msh._native.EXPORTED
    assert hasattr(lib, "msh_set_tiebreak") and hasattr(lib, "msh_get_tiebreak")
    assert lib.msh_set_tiebreak(None, 1, 0, 0) == msh._native.MSH_ERR_INVALID
    m, s, c = C.c_int32(), C.c_uint64(), C.c_uint64()
    assert lib.msh_get_tiebreak(None, C.byref(m), C.byref(s), C.byref(c)) == msh._native.MSH_ERR_INVALID
    assert (msh._native.MSH_TIEBREAK_FIRST, msh._native.MSH_TIEBREAK_RANDOM) == (0, 1)


class _NoCall:
    """A DeviceContext stand-in whose library must not be reached."""

    handle = None

    def __getattr__(self, name):
        raise AssertionError(f"the C library was reached ({name})")


@pytest.mark.parametrize("mode", [2, -1, "bogus", None, True])
def test_python_mirror_rejects_bad_mode_before_the_c_call(msh, mode):
    sched = importlib_scheduler(msh)
    ctx = object.__new__(sched.DeviceContext)
    ctx._lib = _NoCall()
    with pytest.raises(msh._native.MshError) as e:
        ctx.set_tiebreak(mode)
    assert e.value.code == msh._native.MSH_ERR_INVALID


def importlib_scheduler(msh):
    import importlib
    return importlib.import_module(msh.__name__ + ".scheduler")


def test_lds_limit_matches_the_first_max_launcher():
    """pair_pick_kernel stages the planes in LDS up to the limit launch_pairs uses for pair_lds_kernel."""
    mine = re.search(r"TIEBREAK_LDS_MAX_GROUPS\s*=\s*(\d+)", (CSRC / "msh_internal.h").read_text())
    theirs = re.search(r"PAIR_LDS_BIG_GROUPS\s*=\s*(\d+)", (CSRC / "msh_pair.hip").read_text())
    assert mine and theirs and int(mine.group(1)) == int(theirs.group(1))


def test_pod_sharded_ranks_draw_from_one_stream(msh):
    """distributed.PodShardedScheduler(tie_break="random"): each rank's counter is the global index of its
    slice's first pod, batch after batch; nothing is set under the default."""
    import importlib
    D = importlib.import_module(msh.__name__ + ".distributed")

    class Ctx:
        def __init__(self):
            self.calls = []

        def upload_nodes(self, u, d):
            pass

        def set_tiebreak(self, mode, seed=0, counter=0):
            self.calls.append((mode, seed, counter))

    u, d = np.zeros(4, np.uint8), np.zeros(4, np.int8)
    for rank in range(3):
        c = Ctx()
        s = D.PodShardedScheduler(c, u, d, 3, rank, tie_break="random", tie_seed=9)
        lo1, _ = s.begin_batch(1000)
        lo2, _ = s.begin_batch(500)
        assert (lo1, lo2) == (D.shard_range(1000, 3, rank)[0], D.shard_range(500, 3, rank)[0])
        assert c.calls == [("random", 9, 0), ("random", 9, lo1), ("random", 9, 1000 + lo2)]
    c = Ctx()
    s = D.PodShardedScheduler(c, u, d, 3, 1)
    assert s.begin_batch(1000) == s.pod_range(1000) and c.calls == []
