"""Case generator for the LDS pair kernel's one-flag scan (identity-like modes): tables and pods that
send chosen lanes past group 0, and the numpy proof that they do.

In the identity-like modes pair_lds_kernel keeps one match flag per lane for the whole scan of the
groups above 0. A lane with a digit, no feasible match in group 0 (nodes 0-255) and a flag that says
one lies above walks the groups upward for its first match. Random tables never take that path, so
these tables are built for it:

  digit 7   group 0 holds it only on unschedulable nodes (a tolerating pod matches there, a
            non-tolerating pod does not); its first schedulable node is `pos`
  digit 8   no node of group 0 carries it; its first node is `pos_u`, unschedulable (a tolerating
            pod's answer), its first schedulable node `pos_s` lies in a later word or group (a
            non-tolerating pod's answer)
  digit 9   on no node: no match anywhere, the pod takes its first feasible node (node 0 is
            unschedulable and node 1 is not, so the two tolerates values differ there too)
  0-6       on nodes 2-8, schedulable: resolved in group 0's lower half

`check_coverage` asserts, from the oracle's expected indices, that every targeted pod's expected node
is the intended one at or above 256 and every other pod's lies below 256. A case whose precondition
fails raises: it is an error, never a skip.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

G = 256  # nodes per group
IDENT = [(1, 0), (3, 0), (1, 1), (3, 1)]  # (weight, normalize): NONE and DEFAULT at weights 1 and 3
PODS = [1, 63, 64, 65, 130, 513]  # 65: a block with one pod; 130: a wave's second block all padding; 513: two workgroups
T7_G0 = (40, 200)  # group 0's digit-7 nodes, both unschedulable (one per half)


@dataclass
class Case:
    name: str
    u: np.ndarray
    nd: np.ndarray
    expect: dict  # (digit, tolerates) -> expected node for a pod of that kind
    above: set = field(default_factory=set)  # the kinds whose expected node must be >= 256


def _base(n, seed):
    rng = np.random.default_rng(seed)
    u = (rng.random(n) < 0.3).astype(np.uint8)
    nd = rng.integers(0, 7, n).astype(np.int8)  # digits 0-6 only; 7, 8 placed below, 9 nowhere
    nd[rng.random(n) < 0.1] = -1
    u[0], u[1] = 1, 0
    nd[:2] = -1  # nodes 0 and 1 carry no digit: they are first feasible nodes only
    k = min(n, 9)
    nd[2:k] = np.arange(0, k - 2)
    u[2:k] = 0
    return u, nd


def above_case(n, pos, pos_u, pos_s, seed=0):
    """First feasible digit-7 match at pos, digit 8 at pos_u (unschedulable) / pos_s; all >= 256."""
    assert G <= pos < n and G <= pos_u < pos_s < n and pos not in (pos_u, pos_s)
    u, nd = _base(n, 1000 * n + pos + seed)
    for k in T7_G0:
        nd[k], u[k] = 7, 1
    nd[pos], u[pos] = 7, 0
    nd[pos_u], u[pos_u] = 8, 1
    nd[pos_s], u[pos_s] = 8, 0
    # more 7s and 8s after the first ones, so that "first" is tested and not "only"
    rng = np.random.default_rng(seed + 5)
    for k in rng.integers(max(pos, pos_s) + 1, n, 4) if max(pos, pos_s) + 1 < n else []:
        nd[k] = 7 + (k & 1)
    expect = {(7, 0): pos, (7, 1): T7_G0[0], (8, 0): pos_s, (8, 1): pos_u, (9, 0): 1, (9, 1): 0}
    for d in range(7):
        expect[(d, 0)] = expect[(d, 1)] = 2 + d
    return Case(f"n{n}-7@{pos}-8@{pos_u}/{pos_s}", u, nd, expect, {(7, 0), (8, 0), (8, 1)})


def group0_case(n, pos, seed=0):
    """Digit 7's first match at node pos of group 0 (schedulable), nothing of it before; n may be below 256."""
    assert n >= 9 and pos < min(n, G) and (pos == 0 or pos >= 9)  # nodes 2-8 hold the digits 0-6
    u, nd = _base(n, 77 * n + pos + seed)
    if pos == 0:  # node 0 itself: schedulable here, so the first feasible node is node 0 for every pod
        u[0] = 0
    nd[pos], u[pos] = 7, 0
    if pos + 1 < n:
        nd[n - 1] = 7
    first = 0 if pos == 0 else 1
    expect = {(7, 0): pos, (7, 1): pos, (9, 0): first, (9, 1): 0, (8, 0): first, (8, 1): 0}
    for d in range(7):
        expect[(d, 0)] = expect[(d, 1)] = 2 + d
    return Case(f"g0-n{n}-7@{pos}", u, nd, expect)


def only_unschedulable_case(n=300):
    """Group 0's only digit-7 node is unschedulable and no other node carries 7: a tolerating pod takes
    it, a non-tolerating pod has no match anywhere."""
    u, nd = _base(n, 4242)
    nd[77], u[77] = 7, 1
    expect = {(7, 0): 1, (7, 1): 77, (8, 0): 1, (8, 1): 0, (9, 0): 1, (9, 1): 0}
    for d in range(7):
        expect[(d, 0)] = expect[(d, 1)] = 2 + d
    return Case(f"g0-n{n}-7-only-unschedulable", u, nd, expect)


def pods(p, shift=0):
    """p pods: every (digit in 7, 8, 9, 0-6, none) x tolerates kind inside each 64-lane block, so one
    wave holds lanes that resolve in group 0, above it in different groups, and nowhere. Pod 0 is a
    non-tolerating digit-7 pod (the one-pod batch is a targeted pod)."""
    j = np.arange(p) + shift
    digits = np.array([7, 8, 3, 9, 7, -1, 8, 0, 5, 9, 1, 8, 7, 6, 2, 4, -1], np.int8)
    pd = digits[j % len(digits)]
    pt = ((j % 3) == 1).astype(np.uint8)  # 17 and 3 are coprime: every kind within 51 lanes
    return pd, pt


def check_coverage(case, pd, pt, want_idx, want_status, base=0):
    """The generator's own proof, from the oracle's expected indices (DEFAULT, weight 3): every pod
    with a digit is placed on the node the case intends; the targeted kinds at or above base + 256,
    every other kind below it. Returns the number of targeted pods."""
    has = pd >= 0
    assert (want_status[has] == 0).all(), f"{case.name}: a pod with a digit is not placed"
    hit = 0
    for j in np.nonzero(has)[0]:
        kind = (int(pd[j]), int(pt[j]))
        e = case.expect[kind]
        assert want_idx[j] == e, f"{case.name}: pod {j} {kind} expected node {e}, oracle says {want_idx[j]}"
        if kind in case.above:
            assert e - base >= G, f"{case.name}: targeted kind {kind} resolves in group 0 ({e})"
            hit += 1
        else:
            assert 0 <= e - base < G or e < base, f"{case.name}: kind {kind} should resolve in group 0, got {e}"
    if case.above:
        assert hit > 0, f"{case.name}: no targeted pod among {len(pd)}"
    return hit


def _w(g, word, last=False):
    return g * G + 32 * word + (31 if last else 0)


# Tables of 2, 3, 5 and 20 groups (the last one holds padding). Digit 7 / digit 8 firsts at the first
# or last node of a word in group 1, a middle group, the last full group and the padded last group,
# always in different groups or words.
ABOVE = [
    (257, 256, None, None),          # group 1 = node 256 alone (digit 8 below: absent -> see above_cases)
    (600, _w(1, 0), _w(1, 3, True), _w(2, 0)),          # group 1's first node; 8: word 3's last, then padded group's first
    (600, _w(1, 0, True), _w(1, 1), _w(1, 7, True)),    # last node of word 0; 8: the last full group's last node
    (600, _w(1, 7, True), _w(2, 1, True), 599),         # node 511; 8: padded group, a word's last, then the last real node
    (600, 599, _w(1, 4), _w(2, 2)),                     # the table's last node
    (600, _w(2, 0), _w(1, 2, True), _w(1, 5)),          # padded group's first node
    (1100, _w(1, 0), _w(2, 0, True), _w(3, 7, True)),   # group 1; 8: middle group, then the last full group's last node
    (1100, _w(2, 1), _w(3, 0), _w(4, 0)),               # middle group, a word's first (upper group of the pair 3, 2)
    (1100, _w(3, 7, True), _w(1, 7, True), _w(2, 4)),   # last full group's last node
    (1100, _w(4, 0), _w(2, 3), _w(4, 1, True)),        # padded last group's first node
    (1100, 1099, _w(4, 0, True), _w(4, 1)),             # last real node; 8: both in the padded group, adjacent words
    (5000, _w(1, 7, True), _w(10, 2), _w(10, 2, True)), # group 1's last node; 8: same word of a middle group
    (5000, _w(10, 2), _w(9, 0), _w(19, 0)),             # middle group
    (5000, _w(10, 2, True), _w(18, 0), _w(18, 7, True)),
    (5000, _w(18, 0), _w(2, 0), _w(3, 0)),              # last full group's first node
    (5000, _w(18, 7, True), _w(19, 0, True), 4999),     # last full group's last node; 8: the padded group
    (5000, _w(19, 0), _w(17, 5), _w(18, 5)),            # padded last group's first node
    (5000, 4999, _w(1, 0), _w(19, 4)),                  # the last real node
]


def above_cases():
    out = []
    for n, pos, pu, ps in ABOVE:
        if pu is None:  # 257 nodes: node 256 is all there is above group 0
            u, nd = _base(n, 257)
            for k in T7_G0:
                nd[k], u[k] = 7, 1
            nd[256], u[256] = 7, 0
            expect = {(7, 0): 256, (7, 1): T7_G0[0], (8, 0): 1, (8, 1): 0, (9, 0): 1, (9, 1): 0}
            for d in range(7):
                expect[(d, 0)] = expect[(d, 1)] = 2 + d
            out.append(Case("n257-7@256", u, nd, expect, {(7, 0)}))
        else:
            out.append(above_case(n, pos, pu, ps))
    return out


def group0_cases():
    out = [group0_case(600, p) for p in (0, 31, 32, 127, 128, 255)]
    out += [group0_case(100, p) for p in (0, 31, 32, 99)]  # group 0 holds padding
    out += [group0_case(200, p) for p in (128, 199)]      # ... in its upper half only
    out.append(only_unschedulable_case())
    return out


def big_case():
    """129 full groups (33,024 nodes): the 16-wave instance. 7 at the table's last node, 8 in the middle."""
    return above_case(129 * G, 129 * G - 1, _w(64, 3, True), _w(100, 0))


def shard_case(cut=700):
    """Two node shards [0, cut) and [cut, cut + 600). Shard 0 holds digit 7 on unschedulable nodes only
    and no digit 8; shard 1's own group 0 (global cut .. cut + 255) likewise, so its lanes go past its
    group 0 with a non-zero node_base. Returns the case over the whole table and the cut."""
    n = cut + 600
    local = above_case(600, _w(1, 1), _w(1, 6, True), _w(2, 1, True), seed=3)
    u0, nd0 = _base(cut, 99)
    for k in T7_G0:
        nd0[k], u0[k] = 7, 1
    u = np.concatenate([u0, local.u])
    nd = np.concatenate([nd0, local.nd])
    expect = {(7, 0): cut + _w(1, 1), (7, 1): T7_G0[0], (8, 0): cut + _w(2, 1, True), (8, 1): cut + _w(1, 6, True),
              (9, 0): 1, (9, 1): 0}
    for d in range(7):
        expect[(d, 0)] = expect[(d, 1)] = 2 + d
    return Case(f"shards-{cut}+600", u, nd, expect, {(7, 0), (8, 0), (8, 1)}), cut


def all_cases():
    return above_cases() + group0_cases() + [big_case(), shard_case()[0]]
