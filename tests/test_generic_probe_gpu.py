"""The batch kernels' pure helpers on the device, each alone (tests/probe/msh_gprobe.hip): generic_kernel's
NormalizeScore by reciprocal (csrc/msh_generic_norm.h) over the divisor domain of tests/generic_probe.py, with r and b
formed by gen_norm_params as the kernel forms them; col_term's weight operand at each key type's bound; key_mask and
vmax_f64; msh_device.h's decodes against oracle/oracle.py and its bit helpers against numpy. Every comparison is
equality.

The divisor domain run is the FULL one: every d in [1, 2^32], at all three key types. Wall times are one MI355X's, per
case."""
from __future__ import annotations

import functools
import itertools

import numpy as np
import pytest

import generic_probe as GP
import quot_probe as QP
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KTS = [0, 1, 2]
PARTS = 8  # ranges of [1, 2^32] per key type and nudge


@pytest.fixture(scope="module")
def probe(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    return GP.device_lib()


def clean(rep: GP.Report, seen: int):
    print(rep)
    assert rep.seen == seen, repr(rep)
    assert rep.mismatches == 0 and rep.norm_mismatches == 0, repr(rep)


# ---- the normalizing quotient ----
@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("ulps", [0, -1, 1])
@pytest.mark.parametrize("kt", KTS, ids=GP.KT_NAMES)
def test_quotient_every_divisor(probe, kt, ulps, part):
    """trunc((100 raw - b) r) through col_term<KT> for every d in [1, 2^32] (an eighth per case) at generic_probe's
    numerators (MIN-MAX at three offsets, DEFAULT and REVERSE with the negated set and the raws at -2^31), r moved by
    `ulps`: every term equals the device's int64 `/` and gen_normalize; 9.1e12 quotients per key type and nudge.
    2.7 to 3.2 s per case."""
    step = GP.D_MAX // PARTS
    lo = max(1, part * step)
    hi = (part + 1) * step + (1 if part == PARTS - 1 else 0)
    clean(GP.run_quot(kt, None, lo, hi - lo, ulps), GP.count_range(lo, hi, kt))


@pytest.mark.parametrize("kt", KTS, ids=GP.KT_NAMES)
def test_unbiased_reciprocal_is_seen(probe, kt):
    """r = 1 / d without GEN_RCP_BIAS (probe-local) over every d <= 2^20: the probe reports wrong terms, gen_normalize
    stays right, and the reported tuples are wrong in Python integers too."""
    n = 1 << 20
    rep = GP.run_quot(kt, None, 1, n, 0, unbiased=True)
    print(rep)
    assert rep.seen == GP.count_range(1, n + 1, kt) and rep.norm_mismatches == 0
    assert rep.mismatches > 0 and rep.first
    for mode, raw, mx, mn, got, want in rep.first:
        assert want == GP.normalized(mode, raw, mx, mn) and got != want


@functools.lru_cache(maxsize=None)
def judged_rows(kt):
    """Every numerator of d <= 64, of 2^e + c (e in 7..32, |c| <= 1) and of 32 seeded random divisors, as arrays, and
    their normalized scores in Python integers (Go's division)."""
    near = [(1 << e) + c for e in range(7, 33) for c in (-1, 0, 1)]
    rnd = np.random.default_rng(77).integers(65, GP.D_MAX, 32, endpoint=True).tolist()
    rows = [t for d in list(range(1, 65)) + [d for d in near if d <= GP.D_MAX] + rnd for t in GP.numerators(int(d), kt)]
    mode = np.array([t[0] for t in rows], np.int32)
    raw = np.array([t[1] for t in rows], np.int64)
    mx = np.array([t[2] for t in rows], np.int64)
    mn = np.array([np.iinfo(np.int64).max if t[3] is None else t[3] for t in rows], np.int64)
    want = np.array([GP.normalized(*t) for t in rows], np.int64)
    return rows, mode, raw, mx, mn, want


@pytest.mark.parametrize("ulps", [0, -1, 1])
@pytest.mark.parametrize("kt", KTS, ids=GP.KT_NAMES)
def test_quotient_judged_on_the_host(probe, kt, ulps):
    """The raw terms of judged_rows(kt), r moved by `ulps`, against Python integers."""
    rows, mode, raw, mx, mn, want = judged_rows(kt)
    out = np.full(len(rows), -12345, np.int64)
    rc = probe.msh_gprobe_quot_raw(kt, QP.ptr(mode), QP.ptr(raw), QP.ptr(mx), QP.ptr(mn), len(rows), ulps, QP.ptr(out))
    assert rc == 0, f"hipError_t {rc}"
    bad = np.flatnonzero(out != want)
    assert len(bad) == 0, f"{len(bad)} wrong, first {rows[bad[0]]}: got {int(out[bad[0]])}, want {int(want[bad[0]])}"


# ---- col_term's weight operand ----
def terms(probe, kt, q, cw_bits):
    """col_term<KT, false>(q, 0, 1.0, cw): the key's bits."""
    q = np.ascontiguousarray(q, np.float64)
    cw = np.ascontiguousarray(cw_bits, np.uint64)
    one, zero = np.ones_like(q), np.zeros_like(q)
    out = np.zeros(len(q), np.uint64)
    rc = probe.msh_gprobe_term_raw(kt, 0, QP.ptr(q), QP.ptr(zero), QP.ptr(one), QP.ptr(cw), len(q), QP.ptr(out))
    assert rc == 0, f"hipError_t {rc}"
    return out


def edges(bound: int, seed: int) -> list[int]:
    """Magnitudes up to `bound`: the ends, the powers of two and their neighbours, and 2^12 seeded ones."""
    near = {(1 << e) + c for e in range(bound.bit_length()) for c in (-1, 0, 1)}
    rnd = np.random.default_rng(seed).integers(0, bound, 1 << 12, endpoint=True).tolist()
    return sorted({x for x in near | {0, 1, 2, 3, bound - 1, bound} | set(rnd) if 0 <= x <= bound})


def test_col_term_k32_weights(probe):
    """KT 0: (uint32_t)(n w) by the signed 24-bit multiply for |n| <= 2^23 - 1 (both signs, and with a fraction that
    truncates toward zero) and w in {1, 3, 2^23 - 1} and their negatives (REVERSE's weight)."""
    top = (1 << 23) - 1
    ns = [s * n for n in edges(top, 23) for s in (1, -1)]
    for w in (1, 3, top, -1, -3, -top):
        for frac in (0.0, 0.75):
            q = [n + (frac if n >= 0 else -frac) for n in ns]
            out = terms(probe, 0, q, [w & 0xFFFFFFFF] * len(ns))
            want = np.array([(n * w) & 0xFFFFFFFF for n in ns], np.uint64)
            assert np.array_equal(out, want), (w, frac)


def test_col_term_u64_weights(probe):
    """KT 1: n w in wrapping 64-bit arithmetic for |n| <= 2^40 (the documented bound) and w in {1, 2^32} and their
    negatives; the clamp's values and what lies past them (an infeasible pair's) must only come back."""
    ns = [s * n for n in edges(1 << 40, 40) for s in (1, -1)]
    for w in (1, 1 << 32, -1, -(1 << 32)):
        out = terms(probe, 1, [float(n) for n in ns], [w & (2 ** 64 - 1)] * len(ns))
        want = np.array([(n * w) & (2 ** 64 - 1) for n in ns], np.uint64)
        assert np.array_equal(out, want), w
    past = [2.0 ** 62, -2.0 ** 62, 2.0 ** 63, -2.0 ** 63, 1e300, -1e300, np.inf, -np.inf, np.nan]
    assert len(terms(probe, 1, past, [1 << 32] * len(past))) == len(past)
    clamped = terms(probe, 1, past[:8], [1] * 8).view(np.int64)
    assert clamped.tolist() == [1 << 62, -(1 << 62)] * 4


def test_col_term_f53_products(probe):
    """KT 2: trunc(q) w exact for products up to 2^53 - 2."""
    top = (1 << 53) - 2
    pairs = [(n, w) for w in (1, 3, 1 << 20, 1 << 32) for n in edges(top // w, w)] + [(top, 1), ((1 << 21) - 1, 1 << 32)]
    pairs = [(s * n, t * w) for n, w in pairs for s in (1, -1) for t in (1, -1)]
    assert max(abs(n * w) for n, w in pairs) == top
    out = terms(probe, 2, [float(n) for n, _ in pairs], np.array([float(w) for _, w in pairs]).view(np.uint64))
    got = out.view(np.float64)
    assert [int(x) for x in got] == [n * w for n, w in pairs]
    frac = terms(probe, 2, [2.75, -2.75, 0.999, -0.999], np.array([3.0] * 4).view(np.uint64)).view(np.float64)
    assert frac.tolist() == [6.0, -6.0, 0.0, 0.0]


# ---- keys and masks ----
I32 = [-(1 << 31) + 1, -1, 0, 1, (1 << 31) - 2]
I64 = [-(1 << 63) + 1, -1, 0, 1, (1 << 63) - 2]
F53 = [-float((1 << 53) - 2), -1.0, -0.0, 0.0, 1.0, float((1 << 53) - 2)]
ONES = 0xFFFFFFFF


def masked(probe, kt, bits, xm, nt):
    t = np.ascontiguousarray(bits, np.uint64)
    out = np.zeros(len(t), np.uint64)
    x, n = np.full(len(t), xm, np.uint32), np.full(len(t), nt, np.uint32)
    rc = probe.msh_gprobe_key_mask_raw(kt, QP.ptr(t), QP.ptr(x), QP.ptr(n), len(t), QP.ptr(out))
    assert rc == 0, f"hipError_t {rc}"
    return out


@pytest.mark.parametrize("kt", KTS, ids=GP.KT_NAMES)
def test_key_mask_and_key_order(probe, kt):
    """An infeasible pair (xm all-ones, the pod not tolerating: nt all-ones) gives 0, or a NaN; every other pair gives
    the key back bit for bit. The biased unsigned keys (total + 2^31, total ^ 2^63) are above 0 and keep the order of
    the totals at the edges; so do the doubles."""
    if kt == 0:
        bits = [(t + (1 << 31)) & ONES for t in I32]
    elif kt == 1:
        bits = [(t & (2 ** 64 - 1)) ^ (1 << 63) for t in I64]
    else:
        bits = np.array(F53).view(np.uint64).tolist()
    rnd = np.random.default_rng(kt).integers(0, 2 ** 64, 256, dtype=np.uint64)
    if kt == 0:
        rnd &= np.uint64(ONES)
    if kt == 2:   # finite doubles only: a key is a total
        rnd = rnd[((rnd >> np.uint64(52)) & np.uint64(0x7FF)) != 0x7FF]
    allbits = np.concatenate([np.array(bits, np.uint64), rnd])
    for xm, nt in ((0, 0), (0, ONES), (ONES, 0)):
        assert np.array_equal(masked(probe, kt, allbits, xm, nt), allbits), (xm, nt)
    gone = masked(probe, kt, allbits, ONES, ONES)
    if kt == 2:
        assert np.isnan(gone.view(np.float64)).all()
    else:
        assert not gone.any()
    kept = masked(probe, kt, bits, 0, ONES)
    if kt == 2:
        k = kept.view(np.float64)
        assert (np.diff(k) >= 0).all() and k.tolist() == F53
    else:
        assert kept[0] > 0 and (np.diff(kept.astype(object)) > 0).all()


def test_vmax_f64_skips_a_nan(probe):
    """vmax_f64(NaN, x) == x == vmax_f64(x, NaN) for the edge totals and for key_mask's own NaNs; two numbers give
    the larger."""
    nans = [np.nan] + masked(probe, 2, np.array(F53).view(np.uint64), ONES, ONES).view(np.float64).tolist()
    a, b = [], []
    for x in F53:
        for q in nans:
            a += [q, x]
            b += [x, q]
    pairs = list(itertools.product(F53, F53))
    a += [p[0] for p in pairs]
    b += [p[1] for p in pairs]
    a, b = np.array(a), np.array(b)
    out = np.full(len(a), 12345.0)
    assert probe.msh_gprobe_vmax_raw(QP.ptr(a), QP.ptr(b), len(a), QP.ptr(out)) == 0
    n = 2 * len(F53) * len(nans)
    want = np.where(np.isnan(a[:n]), b[:n], a[:n])
    print(out[:n].view(np.uint64), want.view(np.uint64))
    assert not np.isnan(out).any() and (out[:n] == want).all()
    assert (out[n:] == np.maximum(a[n:], b[n:])).all()


# ---- decode ----
WEIGHTS = (1, 3, 1 << 32)
BONUS = 1 << 50


def decode_rows():
    """Every consistent presence pattern of a feasible match node M and a feasible non-match node X behind an
    unschedulable filler (so no index is 0), in both orders; a pod without a digit matches nothing."""
    rows = []
    for order in (("M",), ("X",), ("M", "X"), ("X", "M"), ()):
        for pdv, hs, ps, mode, w in itertools.product((1, 0), (1, 0), (1, 0), range(4), WEIGHTS):
            kinds = [k if pdv else "X" for k in order]
            im = next((1 + i for i, k in enumerate(kinds) if k == "M"), -1)
            ix = next((1 + i for i, k in enumerate(kinds) if k == "X"), -1)
            rows.append(dict(kinds=kinds, inp=(im, ix, 1 if kinds else -1, pdv, hs, ps, mode, w)))
    return rows


def oracle_of(row, bonus_on=None):
    im, ix, ia, pdv, hs, ps, mode, w = row["inp"]
    nodes = [O.Node("a-filler7", True)] + [O.Node(f"b{i}-{'3' if k == 'M' else '5'}") for i, k in enumerate(row["kinds"])]
    ps_ = O.PluginSet(filters=["NodeUnschedulable"], prescore=["NodeNumber"] if ps else [],
                      score=["NodeNumber"] if hs else [], weights=[w] if hs else [], normalize=[mode] if hs else [])
    cols = None
    if bonus_on is not None:
        ps_.score.append("ScoreColumn0")
        ps_.weights.append(1)
        ps_.normalize.append(O.NORM_NONE)
        cols = {"ScoreColumn0": {n.name: (BONUS if k == bonus_on else 0) for n, k in zip(nodes, ["F"] + row["kinds"])}}
    return O.ObjectOracle(ps_, cols).schedule([O.Pod("pod-3" if pdv else "pod-x")], nodes)[0]


def test_decodes_against_the_oracle(probe):
    """decode_pod's (node, score, status) against oracle.ObjectOracle on the two- or three-node table of each row;
    decode_ident equals decode_pod on modes 0 and 1 (judged on the device and here); decode_classes' totals of a match
    and of a non-match against the oracle's winner when a NONE column lifts that class above the other."""
    rows = decode_rows()
    cin, cout = np.zeros(1, np.int32), np.zeros(1, np.int32)
    probe.msh_gprobe_decode_cols(QP.ptr(cin), QP.ptr(cout))
    inp = np.ascontiguousarray([r["inp"] for r in rows], np.int64)
    assert inp.shape[1] == int(cin[0])
    out = np.full((len(rows), int(cout[0])), -777, np.int64)
    assert probe.msh_gprobe_decode_raw(QP.ptr(inp), len(rows), QP.ptr(out)) == 0
    assert len(rows) == 5 * 2 * 2 * 2 * 4 * 3
    for r, o in zip(rows, out.tolist()):
        res = oracle_of(r)
        want = (res.index, res.score, res.status) if res.status == O.PLACED else (-1, 0, res.status)
        assert tuple(o[0:3]) == want, (r, o)
        mode = r["inp"][6]
        assert o[9] == 0 and (tuple(o[3:6]) == want if mode <= 1 else tuple(o[3:6]) == (-9, -9, -9)), (r, o)
        assert o[8] == res.status, (r, o)
        if res.status == O.PLACED and r["inp"][4]:
            for col, kind in ((6, "M"), (7, "X")):
                if kind in r["kinds"]:
                    lifted = oracle_of(r, bonus_on=kind)
                    assert lifted.status == O.PLACED and lifted.score - BONUS == o[col], (r, o, kind)


# ---- bit helpers ----
def test_lowbit(probe):
    """lowbit over 0 (all-ones), every single bit, and 2^16 seeded words."""
    x = np.concatenate([np.array([0] + [1 << b for b in range(32)], np.uint32),
                        np.random.default_rng(32).integers(0, 1 << 32, 1 << 16, dtype=np.uint32)])
    out = np.zeros(len(x), np.uint32)
    assert probe.msh_gprobe_lowbit_raw(QP.ptr(x), len(x), QP.ptr(out)) == 0
    want = np.array([ONES if v == 0 else (v & -v).bit_length() - 1 for v in x.tolist()], np.uint32)
    assert np.array_equal(out, want)


def test_hits_first(probe):
    """hits_first for every word and bit of the first hit, with seeded noise in the later words and above the bit."""
    gw, gn = np.zeros(1, np.int32), np.zeros(1, np.int32)
    probe.msh_gprobe_group_shape(QP.ptr(gw), QP.ptr(gn))
    gw, gn = int(gw[0]), int(gn[0])
    assert gn == 32 * gw
    rng = np.random.default_rng(256)
    h, g, want = [], [], []
    for c, b, rep in itertools.product(range(gw), range(32), range(4)):
        w = rng.integers(0, 1 << 32, gw, dtype=np.uint64) if rep else np.zeros(gw, np.uint64)
        w[:c] = 0
        w[c] = ((int(w[c]) >> b) << b | (1 << b)) & ONES if rep > 1 else 1 << b
        grp = int(rng.integers(0, 1 << 16))
        h.append(w.astype(np.uint32))
        g.append(grp)
        want.append(grp * gn + 32 * c + b)
    h, g = np.ascontiguousarray(h, np.uint32), np.array(g, np.uint32)
    out = np.zeros(len(g), np.uint32)
    assert probe.msh_gprobe_hits_first_raw(QP.ptr(h), QP.ptr(g), len(g), QP.ptr(out)) == 0
    assert np.array_equal(out, np.array(want, np.uint32))


def test_bop3_forms(probe):
    """Each bop3_* form against its commented boolean expression on the 8 input bit combinations spread over a word,
    and on seeded words."""
    rng = np.random.default_rng(3)
    a = np.concatenate([np.array([0xF0F0F0F0, 0x0F0F0F0F], np.uint32), rng.integers(0, 1 << 32, 256, dtype=np.uint32)])
    b = np.concatenate([np.array([0xCCCCCCCC, 0x33333333], np.uint32), rng.integers(0, 1 << 32, 256, dtype=np.uint32)])
    c = np.concatenate([np.array([0xAAAAAAAA, 0x55555555], np.uint32), rng.integers(0, 1 << 32, 256, dtype=np.uint32)])
    assert {(int(a[0]) >> i & 1, int(b[0]) >> i & 1, int(c[0]) >> i & 1) for i in range(32)} == \
        set(itertools.product((0, 1), repeat=3))
    out = np.zeros((7, len(a)), np.uint32)
    assert probe.msh_gprobe_bop3_raw(QP.ptr(a), QP.ptr(b), QP.ptr(c), len(a), QP.ptr(out)) == 0
    want = [a & ~b, a & b & c, a | (b & ~c), a & ~b & c, a | (b ^ c), a & ~(b & c), a | (b & c)]
    for name, got, w in zip(("andn", "and3", "or_andn", "andn_and", "or_xor", "andn_of_and", "or_and"), out, want):
        assert np.array_equal(got, w), name
