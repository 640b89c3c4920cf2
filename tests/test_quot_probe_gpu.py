"""csrc/msh_seq_quot.h on the device, over the whole domain each helper documents: tests/probe/msh_probe.hip runs the
helper with the reciprocal formed on the device as the kernels form it, counts the inputs on which it differs from
the device's integer `/` and those whose remainder before the one correction step leaves [-m, 2m), and returns the raw
outputs of a boundary set (quot_probe's head comment) that numpy or Python integers judge here. Every comparison is
equality. Wall times are one MI355X's, per case."""
from __future__ import annotations

import numpy as np
import pytest

import balanced_ref as BR
import quot_probe as QP
from test_balanced import big_quads, decider_triples

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    return QP.device_lib()


def clean(rep: QP.Report, seen: int):
    """The probe evaluated the whole domain, and nothing in it was wrong."""
    print(rep)
    assert rep.seen == seen, repr(rep)
    assert rep.mismatches == 0 and rep.outside == 0, repr(rep)


def raw(fn, a, m, dtype, arg) -> np.ndarray:
    a, m = np.ascontiguousarray(a, dtype), np.ascontiguousarray(m, dtype)
    out = np.full(len(a), 0xFFFFFFFF, np.uint32)
    rc = fn(QP.ptr(a), QP.ptr(m), len(a), arg, QP.ptr(out))
    assert rc == 0, f"hipError_t {rc}"
    return out.astype(np.int64)


def same(got, a, m):
    want = QP.exact_quot(a, m)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (f"{len(bad)} wrong, first (a, m, got, want) = "
                           f"{(int(a[bad[0]]), int(m[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))}")


# ---- quot_u16 ----
@pytest.mark.parametrize("ulps", [0, -1, 1, -2, 2])
def test_quot_u16_every_pair(probe, ulps):
    """100 * a / m for every 0 <= a <= 65,535 and 1 <= m <= 65,535 (4.29e9 pairs) with rm = rcp(float(m)) moved by
    `ulps`: no wrong quotient and no remainder outside [-m, 2m), the pairs with a > m (which the kernels compute and
    never use) included; their counts are reported apart. Then the raw quotients of the boundary sets of every
    m <= 2^12, of 2^e + d (e in 12..16, |d| <= 16) and of 2^13 seeded random m, judged by numpy. 0.9 s."""
    clean(QP.run_report(probe.msh_probe_quot_u16, ulps), 65536 * 65535)
    near = np.array([(1 << e) + d for e in range(12, 17) for d in range(-16, 17)], np.int64)
    rnd = np.random.default_rng(1616).integers(1, 65536, 1 << 13, dtype=np.int64)
    m = np.concatenate([np.arange(1, (1 << 12) + 1, dtype=np.int64), near[near <= 65535], rnd])
    a, mm = QP.boundary_pairs(m)
    same(raw(probe.msh_probe_quot_u16_raw, a, mm, np.uint32, ulps), a, mm)


# ---- quot_soft ----
SOFT_SPLIT = 4  # ranges of m per nudge


@pytest.mark.parametrize("part", range(SOFT_SPLIT))
@pytest.mark.parametrize("ulps", [0, -1, 1])
def test_quot_soft_every_divisor(probe, ulps, part):
    """100 * a / m for every 1 <= m < 2^28 (a quarter of them per case) at the boundary set of m (305 numerators),
    rm = rcp(float(m)) moved by `ulps`: 8.1e10 quotients per nudge. 0.03 s per case."""
    lo = max(1, part * (QP.SOFT_M_END // SOFT_SPLIT))
    hi = (part + 1) * (QP.SOFT_M_END // SOFT_SPLIT)
    clean(QP.run_report(probe.msh_probe_quot_soft, lo, hi, ulps), QP.boundary_count(np.arange(lo, hi)))


@pytest.mark.parametrize("ulps", [0, -1, 1])
def test_quot_soft_boundaries_judged_on_the_host(probe, ulps):
    """The raw quotients of the boundary sets of every m <= 2^12, of 2^e + d (e in 12..28, |d| <= 16) and of 2^14
    seeded random m below 2^28, against numpy's integer division. 0.1 s."""
    near = np.array([(1 << e) + d for e in range(12, 29) for d in range(-16, 17)], np.int64)
    rnd = np.random.default_rng(2828).integers(1, QP.SOFT_M_END, 1 << 14, dtype=np.int64)
    m = np.concatenate([np.arange(1, (1 << 12) + 1, dtype=np.int64), near[near < QP.SOFT_M_END], rnd])
    a, mm = QP.boundary_pairs(m)
    same(raw(probe.msh_probe_quot_soft_raw, a, mm, np.uint32, ulps), a, mm)


# ---- quot100 ----
@pytest.mark.parametrize("form", [0, 1], ids=["ieee_division", "rcp_times_100"])
def test_quot100_both_reciprocals(probe, form):
    """num * 100 / c over quot_probe.quot100_divisors() (every c <= 2^20, the neighbours of 2^20..2^55, 2^20 random
    55-bit values) at the boundary set of c, with rc = 100 / float(c) (form 0: score, spread-score, classes, prefs,
    soft) and rc = 100 * rcp(float(double(c))) (form 1: balanced, podaffinity): no wrong quotient, no remainder
    outside [-c, 2c). Then the raw quotients of the neighbours' and of 2^13 random divisors' boundary sets against
    Python integers. 0.1 s."""
    cs = QP.quot100_divisors()
    assert cs.min() == 1 and cs.max() == QP.Q100_MAX
    clean(QP.run_report(probe.msh_probe_quot100, QP.ptr(cs), len(cs), form), QP.boundary_count(cs))
    sub = np.concatenate([cs[:1 << 12], cs[1 << 20:(1 << 20) + 36 * 33 + (1 << 13)]])
    # k * c stays below 2^63 for c <= 2^55 and k <= 100
    a, mm = QP.boundary_pairs(sub)
    same(raw(probe.msh_probe_quot100_raw, a, mm, np.int64, form), a, mm)


# ---- wsum_div ----
def test_wsum_div_on_its_whole_domain(probe):
    """acc / sum for every sum in 1..400 and acc in 0..100 * sum on the device, by its own `/` and by numpy. 0.1 s."""
    n_out = int(probe.msh_probe_wsum_out())
    out = np.full(n_out, 0xFFFFFFFF, np.uint32)
    words = np.zeros(int(probe.msh_probe_rep_words()), np.uint64)
    assert probe.msh_probe_wsum(QP.ptr(words), QP.ptr(out)) == 0
    clean(QP.Report(words), n_out)
    sums = np.repeat(np.arange(1, QP.WSUM_MAX + 1, dtype=np.int64), 100 * np.arange(1, QP.WSUM_MAX + 1) + 1)
    assert len(sums) == n_out
    acc = np.arange(n_out, dtype=np.int64) - (50 * sums * (sums - 1) + (sums - 1))
    assert np.array_equal(out.astype(np.int64), acc // sums)


# ---- soft_raw ----
@pytest.fixture(scope="module")
def counts():
    c = np.arange(QP.COUNT_MAX + 1, dtype=np.float64)
    c.setflags(write=False)
    return c


@pytest.mark.parametrize("size", list(QP.SIZES))
def test_soft_raw_every_count(probe, counts, size):
    """soft_raw(c, log(size + 2), skew1) for every count c in [0, 2^25] and skew1 in {0, 1, 2^24 - 1} against numpy
    float64 doing the same three separately rounded operations. 0.5 s per size, most of it numpy's."""
    w = QP.soft_weight(size)
    out = np.empty(QP.COUNT_MAX + 1, np.int32)
    for s in QP.SKEWS:
        out.fill(-1)
        assert probe.msh_probe_soft_raw(0, QP.COUNT_MAX, w, s, QP.ptr(out)) == 0
        bad = np.flatnonzero(out != QP.soft_raw_numpy(counts, w, s))
        assert len(bad) == 0, f"{len(bad)} wrong at skew1 {s}, first count {int(bad[0])}: got {int(out[bad[0]])}"


def test_soft_raw_on_the_fused_multiply_add_deciders(probe):
    """The one input of the domain on which a fused multiply-add returns another integer (quot_probe's search, run by
    tests/test_quot_probe.py): the device returns the separately rounded value."""
    assert len(QP.SOFT_RAW_DECIDERS) == 1
    for c, size, s in QP.SOFT_RAW_DECIDERS:
        w = QP.soft_weight(size)
        out = np.full(1, -1, np.int32)
        assert probe.msh_probe_soft_raw(c, c, w, s, QP.ptr(out)) == 0
        assert QP.soft_raw_separate(c, w, s) != QP.soft_raw_fused(c, w, s)
        assert int(out[0]) == QP.soft_raw_separate(c, w, s)


# ---- balanced_bs ----
def test_balanced_bs_against_the_rule(probe):
    """balanced_bs against balanced_ref.bs: the 48 decider triples (the inputs that tell the float64 rule from the
    exact floor, from float32 and from rounding to nearest) at units 1 and 2^43, big_quads() (amounts that are no
    doubles, up to 2^55, as they are: no unit fits above them), and 2^20 seeded random quadruples with capacities up
    to 2^55 (one in 32 of them 0) and used-plus-requested amounts up to twice the capacity. 1.1 s, the
    Python reference's."""
    triples, _ = decider_triples()
    assert len(triples) == 48
    quads = [tuple(x * u for x in q) for u in (1, 1 << 43) for _, q, _, _ in triples] + list(big_quads())
    rng = np.random.default_rng(5543)
    n = 1 << 20
    bits = rng.integers(1, 56, (n, 2))
    c = rng.integers(0, 1 << 55, (n, 2), endpoint=True) >> (55 - bits)
    c[rng.random((n, 2)) < 1 / 32] = 0
    q = rng.integers(0, np.where(rng.random((n, 2)) < 0.5, c, 2 * c), endpoint=True)
    q = np.where(rng.random((n, 2)) < 0.1, c, q)                       # a full node now and then
    rnd = np.stack([q[:, 0], c[:, 0], q[:, 1], c[:, 1]], axis=1)
    allq = np.ascontiguousarray(np.concatenate([np.array(quads, np.int64), rnd]))
    assert allq.min() >= 0 and allq[:, 1::2].max() <= 1 << 55 and allq[:, 0::2].max() <= 1 << 56
    out = np.full(len(allq), 0xFFFFFFFF, np.uint32)
    assert probe.msh_probe_balanced_bs(QP.ptr(allq), len(allq), QP.ptr(out)) == 0
    for k, (_, quad, v, _) in enumerate(triples):
        assert int(out[k]) == v == int(out[48 + k]), (quad, int(out[k]), v)
    want = np.array([BR.bs(*row) for row in allq.tolist()], np.int64)
    bad = np.flatnonzero(out.astype(np.int64) != want)
    assert len(bad) == 0, f"{len(bad)} wrong, first {allq[bad[0]].tolist()}: got {int(out[bad[0]])}, want {int(want[bad[0]])}"
