"""csrc/msh_seq_quot.h on the CPU: the integer code through a host build of the header (tests/probe), and the
properties of the references that tests/test_quot_probe_gpu.py holds the device to."""
from __future__ import annotations

import numpy as np

import quot_probe as QP


def test_wsum_div_on_its_whole_domain_host_build():
    """acc / sum == wsum_div(acc, wsum_magic(sum)) for every sum in 1..400 and acc in 0..100 * sum (8,020,400
    inputs), by the host build's own `/` and again by numpy on the raw outputs. About 0.1 s."""
    h = QP.host_lib()
    n_out = 50 * QP.WSUM_MAX * (QP.WSUM_MAX + 1) + QP.WSUM_MAX
    out = np.full(n_out, 0xFFFFFFFF, np.uint32)
    first = np.zeros(3, np.uint32)
    bad = h.msh_host_wsum(QP.WSUM_MAX, QP.ptr(first), QP.ptr(out))
    assert bad == 0, f"{bad} wrong quotients, first (acc, sum, got) = {first.tolist()}"
    for s in (1, 2, 3, 7, 100, 399, 400):
        assert h.msh_host_wsum_magic(s) == -((-(1 << 31)) // s)
    sums = np.repeat(np.arange(1, QP.WSUM_MAX + 1, dtype=np.int64), 100 * np.arange(1, QP.WSUM_MAX + 1) + 1)
    start = 50 * sums * (sums - 1) + (sums - 1)
    acc = np.arange(n_out, dtype=np.int64) - start
    assert acc.min() == 0 and (acc <= 100 * sums).all()       # the layout covers out exactly once
    wrong = np.flatnonzero(out.astype(np.int64) != acc // sums)
    assert len(wrong) == 0, f"first (acc, sum, got) = {(int(acc[wrong[0]]), int(sums[wrong[0]]), int(out[wrong[0]]))}"


def test_boundary_pairs_are_the_quotient_boundaries():
    for m in (1, 3, 7, 99, 100, 101, 65535, (1 << 28) - 1, (1 << 55) - 3, 1 << 55):
        a, mm = QP.boundary_pairs(np.array([m]))
        a = [int(x) for x in a]
        assert min(a) == 0 and max(a) == m
        for k in range(101):
            b = -((-k * m) // 100)
            assert b in a and 100 * b // m >= k and (b == 0 or 100 * (b - 1) // m < k)
            assert max(b - 1, 0) in a and min(b + 1, m) in a
        q = QP.exact_quot(np.array(a), np.array([m] * len(a)))
        assert [int(x) for x in q] == [100 * x // m for x in a]


def test_soft_raw_decider_search():
    """The search of quot_probe.soft_raw_deciders over the whole domain (counts 0..2^25, sizes 0..64, the three
    skews): 2^-20-window candidates settled in exact arithmetic. It finds the inputs on which a fused multiply-add
    returns another integer than the rule: of 4,188 candidates exactly one, count 32,153,763 over 53 zones
    (w = log 55) with max_skew 2^24, which the GPU test asserts on by name. The host build of soft_raw (contraction
    off) must follow the rule on it. About 5 s."""
    deciders, candidates = QP.soft_raw_deciders()
    print(f"soft_raw: {candidates} candidates, {len(deciders)} deciders: {deciders[:8]}")
    assert candidates > 1000          # about 2^-19 of 65 * 2^25 counts: the filter saw the domain
    assert deciders == QP.SOFT_RAW_DECIDERS
    h = QP.host_lib()
    for c, size, s in deciders:
        w = QP.soft_weight(size)
        want = QP.soft_raw_separate(c, w, s)
        assert want != QP.soft_raw_fused(c, w, s)
        assert h.msh_host_soft_raw(c, w, s) == want
        assert int(QP.soft_raw_numpy(np.array([float(c)]), w, s)[0]) == want


def test_soft_raw_references_agree_on_edges():
    """numpy's three operations against the exact-arithmetic restatement at the domain's corners and on ties."""
    cs = [0, 1, 2, 3, 1000, (1 << 24) - 1, 1 << 24, (1 << 25) - 1, 1 << 25]
    for size in (0, 1, 2, 14, 62, 63, 64):
        w = QP.soft_weight(size)
        for s in QP.SKEWS:
            got = QP.soft_raw_numpy(np.array(cs, np.float64), w, s)
            assert [int(x) for x in got] == [QP.soft_raw_separate(c, w, s) for c in cs]
    assert QP.round_half_away(0.5) == 1 and QP.round_half_away(2.5) == 3 and QP.round_half_away(2.4999) == 2
