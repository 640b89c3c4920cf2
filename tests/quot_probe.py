"""What tests/test_quot_probe.py (CPU) and tests/test_quot_probe_gpu.py share: the probe libraries of tests/probe
(built by mini-kube-scheduler_amd/build.py's build_probe, loaded with ctypes), the boundary sets, and the float64
references of soft_raw. Test infrastructure only; none of it is the code under test.

The boundary set of a divisor m: for each k in 0..100 the smallest numerator whose quotient 100 * a / m reaches k,
ceil(k * m / 100), and its two neighbours, kept within [0, m], plus 0 and m: the inputs at which an estimate that is
off by one ulp changes the truncated quotient.
"""
from __future__ import annotations

import ctypes
import functools
import importlib
import math
from fractions import Fraction

import numpy as np

SOFT_M_END = 1 << 28          # quot_soft: 1 <= m < 2^28
Q100_MAX = 1 << 55            # quot100: 1 <= c <= 2^55
COUNT_MAX = 1 << 25           # soft_raw: counts in [0, 2^25]
SIZES = range(0, 65)          # soft_raw: w = log(size + 2)
SKEWS = (0, 1, (1 << 24) - 1)
WSUM_MAX = 400
HALF_WINDOW = 2.0 ** -20
# what soft_raw_deciders() finds (tests/test_quot_probe.py runs the search): (count, size, skew1)
SOFT_RAW_DECIDERS = ((32153763, 53, (1 << 24) - 1),)


def _load(which: int):
    b = importlib.import_module("mini-kube-scheduler_amd.build")
    # compiles the one library asked for, and only when it is missing or stale; a failure is an error, never a skip
    path = b.build_probe(device=which == 0, host=which == 1)[which]
    return ctypes.CDLL(str(path))


@functools.lru_cache(maxsize=None)
def host_lib():
    h = _load(1)
    h.msh_host_wsum.restype = ctypes.c_int64
    h.msh_host_wsum.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    h.msh_host_wsum_magic.restype = ctypes.c_uint32
    h.msh_host_wsum_magic.argtypes = [ctypes.c_uint32]
    h.msh_host_half_candidates.restype = ctypes.c_int64
    h.msh_host_half_candidates.argtypes = [ctypes.c_double, ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                           ctypes.c_void_p, ctypes.c_int64]
    h.msh_host_soft_raw.restype = ctypes.c_int32
    h.msh_host_soft_raw.argtypes = [ctypes.c_int32, ctypes.c_double, ctypes.c_int32]
    return h


@functools.lru_cache(maxsize=None)
def device_lib():
    d = _load(0)
    p, i, i64, u32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_double
    d.msh_probe_wsum_out.restype = i64
    for name, args in (("quot_u16", [i, p]), ("quot_u16_raw", [p, p, i64, i, p]),
                       ("quot_soft", [u32, u32, i, p]), ("quot_soft_raw", [p, p, i64, i, p]),
                       ("quot100", [p, i64, i, p]), ("quot100_raw", [p, p, i64, i, p]),
                       ("wsum", [p, p]), ("soft_raw", [ctypes.c_int32, ctypes.c_int32, f64, ctypes.c_int32, p]),
                       ("balanced_bs", [p, i64, p])):
        f = getattr(d, "msh_probe_" + name)
        f.restype, f.argtypes = i, args
    return d


class Report:
    """An exhaustive entry point's report (tests/probe/msh_probe.hip's head comment)."""

    def __init__(self, words: np.ndarray):
        self.mismatches, self.outside, self.mismatches_beyond, self.outside_beyond = (int(x) for x in words[:4])
        self.first = [tuple(int(x) for x in words[4 + 4 * k: 8 + 4 * k]) for k in range(min(int(words[-2]), 8))]
        self.seen = int(words[-1])

    def __repr__(self):
        return (f"seen={self.seen}, mismatches={self.mismatches} (a > m: {self.mismatches_beyond}), remainders outside="
                f"{self.outside} (a > m: {self.outside_beyond}), first (num, div, got, want)={self.first}")


def run_report(fn, *args) -> Report:
    words = np.zeros(int(device_lib().msh_probe_rep_words()), np.uint64)
    rc = fn(*args, words.ctypes.data)
    assert rc == 0, f"the probe's HIP call failed: hipError_t {rc}"
    return Report(words)


def ptr(a: np.ndarray):
    assert a.flags.c_contiguous
    return a.ctypes.data


def boundary_pairs(m: np.ndarray, top: np.ndarray | None = None):
    """(a, m) int64 arrays: the boundary set of every divisor in m (k * m < 2^63). `top`, when given, is the largest
    numerator per divisor instead of m itself."""
    m = np.asarray(m, np.int64)
    top = m if top is None else np.asarray(top, np.int64)
    k = np.arange(101, dtype=np.int64)[None, :]
    b = -((-k * m[:, None]) // 100)                     # ceil(k m / 100)
    a = np.concatenate([b - 1, b, b + 1, np.zeros((len(m), 1), np.int64), top[:, None]], axis=1)
    a = np.clip(a, 0, top[:, None])
    mm = np.broadcast_to(m[:, None], a.shape)
    return np.ascontiguousarray(a.ravel()), np.ascontiguousarray(mm.ravel())


def boundary_count(m: np.ndarray) -> int:
    """How many evaluations the device makes over the boundary sets of the divisors m: 0, m and ceil(k m / 100) for
    k in 0..100, the one below where it is not negative (k >= 1), the one above where it is within m
    (m (100 - k) >= 100; k <= 99 when m >= 100)."""
    m = np.asarray(m, np.int64)
    k = np.arange(101, dtype=np.int64)[None, :]
    small = m[m < 100]
    above = 100 * int((m >= 100).sum()) + int((small[:, None] * (100 - k) >= 100).sum())
    return (2 + 101 + 100) * len(m) + above


def exact_quot(a: np.ndarray, m: np.ndarray) -> np.ndarray:
    """100 * a // m for int64 arrays whose product may pass 2^63: in Python ints where it does."""
    a, m = np.asarray(a, np.int64), np.asarray(m, np.int64)
    small = a < (1 << 56)
    out = np.empty(len(a), np.int64)
    out[small] = a[small] * 100 // m[small]
    big = np.flatnonzero(~small)
    out[big] = [100 * int(a[i]) // int(m[i]) for i in big]
    return out


def quot100_divisors() -> np.ndarray:
    """Every c in [1, 2^20]; 2^e + d for e in 20..55, |d| <= 16, within [1, 2^55]; 2^20 seeded random 55-bit values."""
    near = np.array([(1 << e) + d for e in range(20, 56) for d in range(-16, 17)], np.int64)
    rnd = np.random.default_rng(550055).integers(1, Q100_MAX, 1 << 20, dtype=np.int64, endpoint=True)
    c = np.concatenate([np.arange(1, (1 << 20) + 1, dtype=np.int64), near[near <= Q100_MAX], rnd])
    return np.ascontiguousarray(c)


def soft_weight(size: int) -> float:
    return math.log(size + 2)


def round_half_away(y):
    """Go's math.Round of a non-negative value, exact for a float or a Fraction."""
    t = math.floor(y)
    return t + (1 if y - t >= Fraction(1, 2) else 0)


def soft_raw_separate(c: int, w: float, skew1: int) -> int:
    """The rule: the product rounded, the sum rounded, then half away from zero."""
    x = float(Fraction(c) * Fraction(w))        # Fraction -> float rounds to nearest even, once
    y = float(Fraction(x) + skew1)
    return round_half_away(Fraction(y))


def soft_raw_fused(c: int, w: float, skew1: int) -> int:
    """Not the rule: c * w + skew1 rounded once, as a fused multiply-add would."""
    return round_half_away(Fraction(float(Fraction(c) * Fraction(w) + skew1)))


@functools.lru_cache(maxsize=None)
def soft_raw_deciders() -> tuple:
    """Every (c, size, skew1) of the domain on which a fused multiply-add changes the returned integer. The two
    evaluations differ by at most half an ulp of a value below 2^28, 2^-26, so the result can differ only where the
    product's fraction is within 2^-24 of 0.5: the candidates are every count whose fl(c * w) has a fraction within
    2^-20 of 0.5 (a C loop over the whole domain in libmsh_probe_host.so), each then settled in exact arithmetic."""
    h = host_lib()
    buf = np.zeros(1 << 16, np.int32)
    found, candidates = [], 0
    for size in SIZES:
        w = soft_weight(size)
        n = int(h.msh_host_half_candidates(w, 0, COUNT_MAX, HALF_WINDOW, ptr(buf), len(buf)))
        assert n <= len(buf), "the candidate list was cut"
        candidates += n
        for c in buf[:n].tolist():
            for s in SKEWS:
                if soft_raw_separate(c, w, s) != soft_raw_fused(c, w, s):
                    found.append((c, size, s))
    return tuple(found), candidates


def soft_raw_numpy(counts_f64: np.ndarray, w: float, skew1: int) -> np.ndarray:
    """soft_raw in numpy float64: three separately rounded operations (numpy fuses nothing), half away from zero."""
    x = counts_f64 * np.float64(w)
    y = x + np.float64(skew1)
    t = np.trunc(y)
    np.subtract(y, t, out=y)                      # exact
    return (t + (y >= 0.5)).astype(np.int32)
