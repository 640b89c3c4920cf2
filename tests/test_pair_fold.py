"""pair_lds_kernel, identity-like modes (NONE, DefaultNormalizeScore) in 4-wave workgroups: the workgroup's
pods of class 0 (not tolerating, code bit 3 clear; class = tolerates << 1 | code >> 3) moved to its first
blocks, blocks of class 0 only scanned with the term X | D3 built on the scalar unit, every other block
with the general chain.

Every case forces the LDS-staged kernel (pair_planes lds), runs with the fold on (the default) and off
(pair_fold off: every block takes the general chain, in launch order) and compares idx / score / status
bit-exact with tests/closed_form.py's closed_form_modes, in NONE at weight 1 and DEFAULT at weight 3.
The closed form of a (table, pods, mode) is computed once and shared by both runs.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from closed_form import closed_form_modes
from test_gpu_parity import _assert_same, _desc, _dev_batch

pytestmark = pytest.mark.gpu

NU, NN = ["NodeUnschedulable"], ["NodeNumber"]
IDENT = [(1, 0), (3, 1)]  # (weight, msh_normalize): NONE w = 1, DEFAULT w = 3
FOLDS = ["on", "off"]
G = 256  # nodes per group


@pytest.fixture(scope="module")
def ctxs(msh):
    made = {f: msh.DeviceContext(0, {"pair_planes": "lds", "pair_fold": f}) for f in FOLDS}
    yield made
    for c in made.values():
        c.close()


# ---- node tables (unsched uint8, digit int8; -1: a name without a digit suffix) ----
@functools.lru_cache(maxsize=None)
def table(n: int):
    """n random nodes: 10% unschedulable, digits 0-9 uniform, 2% without a digit. 300: group 0 and one padded
    group; 1,025: a second 1,024-node pad step (5 groups with nodes, the last one padded); 5,000: 20 groups."""
    rng = np.random.default_rng(1000 + n)
    u = (rng.random(n) < 0.10).astype(np.uint8)
    d = rng.integers(0, 10, n).astype(np.int8)
    d[rng.random(n) < 0.02] = -1
    return u, d


@functools.lru_cache(maxsize=None)
def late_table(n: int, at: int, digit: int = 7):
    """Every node unschedulable and of another digit, except node `at`: schedulable, the table's only node of
    `digit`. A non-tolerating pod's only feasible node is `at` (a match for `digit`, the first feasible node for
    the rest); a tolerating pod of `digit` finds its first match there too, the others in group 0."""
    rng = np.random.default_rng(7 * n + at)
    d = rng.choice(np.array([k for k in range(10) if k != digit], np.int8), n)
    u = np.ones(n, np.uint8)
    u[at], d[at] = 0, digit
    return u, d


@functools.lru_cache(maxsize=None)
def padded_table():
    """300 nodes: group 1 holds 44 real nodes, all unschedulable and of digit 7, then padding; group 0 holds no
    node of digit 7. A pod of digit 7 that tolerates matches node 256; one that does not has no match (the
    padding slots, node code 15, must not give it one) and takes its first feasible node at score 0."""
    rng = np.random.default_rng(300)
    n = 300
    d = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 8, 9], np.int8), n)
    u = (rng.random(n) < 0.10).astype(np.uint8)
    d[G:], u[G:] = 7, 1
    return u, d


# ---- pod sets (digit int8, tolerates uint8) ----
def mix(p: int, seed: int = 0):
    """The synthetic proportions: digits in turn (20% with code bit 3), 1% without a digit, 5% tolerating."""
    rng = np.random.default_rng(50 + p + seed)
    d = (np.arange(p) % 10).astype(np.int8)
    d[rng.random(p) < 0.01] = -1
    t = (rng.random(p) < 0.05).astype(np.uint8)
    return d, t


def by_counts(c0: int, c1: int, c2: int, c3: int, seed: int = 0):
    """c_k pods of class k = tolerates << 1 | code >> 3, shuffled: digits 0-7 (P3 = 0) or 8, 9, none (P3 = 1)."""
    rng = np.random.default_rng(seed + 1000 * c0 + c3)
    lo = lambda c: rng.integers(0, 8, c)
    hi = lambda c: rng.choice(np.array([8, 9, -1]), c)
    d = np.concatenate([lo(c0), hi(c1), lo(c2), hi(c3)]).astype(np.int8)
    t = np.concatenate([np.zeros(c0 + c1), np.ones(c2 + c3)]).astype(np.uint8)
    perm = rng.permutation(len(d))
    return d[perm], t[perm]


def const(p: int, digits, tol: int):
    d = np.resize(np.asarray(digits, np.int8), p)
    return d, np.full(p, tol, np.uint8)


POD_SETS = {
    # 1. all four classes in the synthetic proportions; neither a multiple of 64 nor of 512
    "mix1000": mix(1000),
    "mix2011": mix(2011),
    # 2. class boundaries exactly on 64-pod block edges (no block of several classes): a full workgroup; one
    # whose last 64 lanes are padding (they join class 1: 128 + 64); two workgroups. Then one more pod per
    # class: every boundary splits a block
    "edges512": by_counts(256, 128, 64, 64),
    "edges448": by_counts(192, 128, 64, 64),
    "edges1024": by_counts(576, 192, 128, 128, seed=3),
    "split452": by_counts(193, 129, 65, 65),
    "split260": by_counts(65, 65, 65, 65),
    # 3. one class: every block is pure
    "all_tolerate": const(700, [0, 1, 2, 3, 4, 5, 6, 7], 1),
    "all_tolerate_89": const(130, [8, 9, -1], 1),
    "all_nodigit": const(513, [-1], 0),
    "all_89": const(700, [8, 9], 0),
    "all_class0": const(1000, [0, 1, 2, 3, 4, 5, 6, 7], 0),
    # 5. digit 7 (differs from the padding's code 15 in D3 only), with pods without a digit among them
    "sevens": (np.where(np.arange(333) % 11 == 5, -1, 7).astype(np.int8), (np.arange(333) % 3 == 0).astype(np.uint8)),
}


@functools.lru_cache(maxsize=None)
def want(tab_key, pods_key, w, norm):
    u, nd = TABLES[tab_key]()
    pd, pt = POD_SETS[pods_key]
    return closed_form_modes(u, nd, pd, pt, w, norm)


TABLES = {
    "n300": lambda: table(300),
    "n1025": lambda: table(1025),
    "n5000": lambda: table(5000),
    # 4. late matches: the flag above group 0 and the upward walk, from a sorted lane
    "late_last": lambda: late_table(5000, 19 * G + 135),
    "late_group1": lambda: late_table(5000, G + 37),
    "late_1025": lambda: late_table(1025, 4 * G),  # the padded group's only real node
    "padded7": padded_table,
}

CASES = ([(t, p) for t in ("n300", "n1025", "n5000") for p in ("mix1000", "mix2011", "split452")] +
         [("n5000", p) for p in ("edges512", "edges448", "edges1024", "split260", "all_tolerate", "all_tolerate_89",
                                 "all_nodigit", "all_89", "all_class0")] +
         [("n300", "all_89"), ("n1025", "edges512"), ("n300", "all_tolerate")] +
         [(t, p) for t in ("late_last", "late_group1", "late_1025") for p in ("mix1000", "split452", "all_class0", "sevens")] +
         [("padded7", p) for p in ("sevens", "mix1000", "all_class0", "split260")])


def _plug(ctx, msh, w, norm):
    ctx.set_plugins(NU, NN, [msh.ScorePluginConfig("NodeNumber", w, msh.Normalize(norm))])


@pytest.mark.parametrize("tab,pods", CASES, ids=lambda v: v)
def test_fold_equals_closed_form(msh, ctxs, tab, pods):
    u, nd = TABLES[tab]()
    pd, pt = POD_SETS[pods]
    for w, norm in IDENT:
        exp = want(tab, pods, w, norm)
        for f in FOLDS:
            _plug(ctxs[f], msh, w, norm)
            ctxs[f].upload_nodes(u, nd)
            _assert_same(ctxs[f].schedule_batch(pd, pt), exp, f"{tab} {pods} w={w} norm={norm} fold={f}")


def test_late_tables_reach_above_group0():
    """The late tables do what they are for: non-tolerating pods of digit 7 match the lone node above group 0,
    every other non-tolerating pod with a digit takes it at score 0."""
    for key, at in (("late_last", 19 * G + 135), ("late_group1", G + 37), ("late_1025", 4 * G)):
        pd, pt = POD_SETS["mix1000"]
        idx, score, status = want(key, "mix1000", 1, 0)
        nt = (pt == 0) & (pd >= 0)
        assert at >= G and (idx[nt] == at).all() and nt.sum() > 800
        assert (score[nt & (pd == 7)] == 10).all() and (score[nt & (pd != 7)] == 0).all()
        assert (status[pd < 0] == 2).all() and (status[pd >= 0] == 0).all()


def test_padding_never_matches(msh, ctxs):
    """Pods of digit 7 against the table whose padded group holds only unschedulable nodes of digit 7: a pod that
    does not tolerate gets no match (score 0, its first feasible node, in group 0), one that does matches node
    256, and a pod without a digit reports status 2."""
    u, nd = padded_table()
    pd, pt = POD_SETS["sevens"]
    first = int(np.argmax(u == 0))
    for f in FOLDS:
        _plug(ctxs[f], msh, 1, 0)
        ctxs[f].upload_nodes(u, nd)
        idx, score, status = ctxs[f].schedule_batch(pd, pt)
        seven = pd == 7
        assert (status[~seven] == 2).all() and (idx[~seven] == -1).all(), f
        assert (status[seven] == 0).all(), f
        assert (idx[seven & (pt == 0)] == first).all() and (score[seven & (pt == 0)] == 0).all(), f
        assert (idx[seven & (pt == 1)] == G).all() and (score[seven & (pt == 1)] == 10).all(), f


@pytest.mark.parametrize("tab", ["n5000", "late_last"])
def test_two_batches_one_launch(msh, ctxs, tab):
    """Two batches of different sizes in one msh_schedule_batches_device call, one shorter than a workgroup."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    u, nd = TABLES[tab]()
    names = ["mix1000", "split260"]
    for w, norm in IDENT:
        for f in FOLDS:
            ctx = ctxs[f]
            _plug(ctx, msh, w, norm)
            ctx.upload_nodes(u, nd)
            bufs = [_dev_batch(torch, dev, *POD_SETS[k]) for k in names]
            ctx.schedule_batches_device(ctx.batch_descs([_desc(t) for t in bufs]),
                                        stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            for k, t in zip(names, bufs):
                _assert_same([t[i].cpu().numpy() for i in (2, 3, 4)], want(tab, k, w, norm),
                             f"{tab} {k} w={w} norm={norm} fold={f}")


@pytest.mark.parametrize("norm", [2, 3], ids=["reverse", "minmax"])
def test_reverse_minmax_unchanged(msh, ctxs, norm):
    """REVERSE and MINMAX keep their two-class sort; the option does not bear on them."""
    u, nd = table(5000)
    for pods in ("mix2011", "split452"):
        pd, pt = POD_SETS[pods]
        exp = want("n5000", pods, 3, norm)
        for f in FOLDS:
            _plug(ctxs[f], msh, 3, norm)
            ctxs[f].upload_nodes(u, nd)
            _assert_same(ctxs[f].schedule_batch(pd, pt), exp, f"{pods} norm={norm} fold={f}")
