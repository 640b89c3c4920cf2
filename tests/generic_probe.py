"""What tests/test_generic_probe.py (CPU) and tests/test_generic_probe_gpu.py share: the entry points of
tests/probe/msh_gprobe.hip (libmsh_probe.so) and of the host build of csrc/msh_generic_norm.h's double paths
(libmsh_probe_host.so), the divisor domains and the numerators of the normalizing quotient, and their counts. Test
infrastructure only; none of it is the code under test.

A score column holds values in [-2^31, 2^31] (msh_upload_score_column's contract in include/minisched_hip.h), so the
largest divisor of a NormalizeScore, mx - mn of MIN-MAX, is 2^32; DEFAULT and REVERSE divide by max(mx, 0) <= 2^31 and
are run over the same divisors (their numerators stay below 2^39, all the claim of DESIGN.md §4.3 asks).

The divisor domain is the full one: every d in [1, 2^32].

Per divisor d the numerators are the boundary set S(d) of tests/quot_probe.py: MIN-MAX at mn = -2^31, 0 (where
d <= 2^31) and 2^31 - d, raws mn + a; DEFAULT and REVERSE at raws a and -a, and the six raws -2^31, -2^31 + 1,
-2^31 + 2 and e - 1, e, e + 1 (kept >= -2^31) around e, the largest raw whose quotient is that of -2^31. The 32-bit keys
hold terms below 2^23 (col_term's comment), so they take those six only where 100 * 2^31 / d is: d > 25,600.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import quot_probe as QP

RAW_LO, RAW_HI = -(1 << 31), 1 << 31
D_MAX = RAW_HI - RAW_LO                 # 2^32
K32_NEG_D = 25600
NONE, DEFAULT, REVERSE, MINMAX = 0, 1, 2, 3
KT_NAMES = ("k32", "u64", "f53")


@functools.lru_cache(maxsize=None)
def device_lib():
    d = QP.device_lib()
    p, i, i64, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    for name, args in (("quot", [i, p, u64, i64, i, i, p]), ("quot_raw", [i, p, p, p, p, i64, i, p]),
                       ("term_raw", [i, i, p, p, p, p, i64, p]), ("key_mask_raw", [i, p, p, p, i64, p]),
                       ("vmax_raw", [p, p, i64, p]), ("decode_cols", [p, p]), ("decode_raw", [p, i64, p]),
                       ("lowbit_raw", [p, i64, p]), ("group_shape", [p, p]), ("hits_first_raw", [p, p, i64, p]),
                       ("bop3_raw", [p, p, p, i64, p])):
        f = getattr(d, "msh_gprobe_" + name)
        f.restype, f.argtypes = i, args
    return d


@functools.lru_cache(maxsize=None)
def host_lib():
    h = QP.host_lib()
    h.msh_host_gquot.restype = ctypes.c_int
    h.msh_host_gquot.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return h


class Report:
    """msh_gprobe_quot's report (tests/probe/msh_gprobe.hip's head comment)."""

    def __init__(self, words: np.ndarray):
        s = words.astype(np.uint64).view(np.int64)
        self.mismatches, self.norm_mismatches, self.seen = int(s[0]), int(s[1]), int(s[-1])
        self.first = [tuple(int(x) for x in s[2 + 6 * k: 8 + 6 * k]) for k in range(min(int(s[-2]), 8))]

    def __repr__(self):
        return (f"seen={self.seen}, term != device `/`: {self.mismatches}, gen_normalize != device `/`: "
                f"{self.norm_mismatches}, first (mode, raw, mx, mn, got, want)={self.first}")


def run_quot(kt: int, ds, d_lo: int, nd: int, ulps: int, unbiased: bool = False) -> Report:
    lib = device_lib()
    words = np.zeros(int(lib.msh_gprobe_rep_words()), np.uint64)
    rc = lib.msh_gprobe_quot(kt, None if ds is None else QP.ptr(ds), d_lo, nd, ulps, int(unbiased), QP.ptr(words))
    assert rc == 0, f"the probe's HIP call failed: hipError_t {rc}"
    return Report(words)


def run_quot_host(kt: int, ds, d_lo: int, nd: int, ulps: int, unbiased: bool = False, threads: int = 8):
    """(term mismatches, gen_normalize mismatches, evaluations, first mismatch) of the host build."""
    rep = np.zeros(9, np.uint64)
    rc = host_lib().msh_host_gquot(kt, None if ds is None else QP.ptr(ds), d_lo, nd, ulps, int(unbiased), threads,
                                   QP.ptr(rep))
    assert rc == 0
    s = rep.view(np.int64)
    return int(s[0]), int(s[1]), int(s[2]), tuple(int(x) for x in s[3:])


def set_size(d: int) -> int:
    """|S(d)| as the probes walk it (quot_probe.boundary_count for one divisor)."""
    return 303 if d >= 100 else int(QP.boundary_count(np.array([d])))


def evaluations(d: int, kt: int) -> int:
    offsets = 3 if d <= RAW_HI else 2
    return (offsets + 4) * set_size(d) + (12 if kt != 0 or d > K32_NEG_D else 0)


def count_range(lo: int, hi: int, kt: int) -> int:
    """The evaluations over every d in [lo, hi), 1 <= lo, in Python integers."""
    total = sum(evaluations(d, kt) for d in range(lo, min(hi, 100)))
    lo = max(lo, 100)
    if hi <= lo:
        return total
    three = max(0, min(hi, RAW_HI + 1) - lo)               # d <= 2^31: three MIN-MAX offsets
    total += 303 * (7 * three + 6 * (hi - lo - three))
    total += 12 * ((hi - lo) if kt != 0 else max(0, hi - max(lo, K32_NEG_D + 1)))
    return total


def count_list(ds: np.ndarray, kt: int) -> int:
    ds = np.asarray(ds, np.uint64)
    small = sum(evaluations(int(d), kt) for d in ds[ds < 100])
    big = ds[ds >= 100]
    three = int((big <= RAW_HI).sum())
    neg = len(big) if kt != 0 else int((big > K32_NEG_D).sum())
    return small + 303 * (7 * three + 6 * (len(big) - three)) + 12 * neg


def near_powers(e_lo: int, e_hi: int, lo: int, hi: int, reach: int) -> np.ndarray:
    """Every d within `reach` of 2^e, e in [e_lo, e_hi], kept within [lo, hi]."""
    d = np.concatenate([np.arange((1 << e) - reach, (1 << e) + reach + 1, dtype=np.int64) for e in range(e_lo, e_hi + 1)])
    return np.unique(d[(d >= lo) & (d <= hi)]).astype(np.uint64)


def boundary_set(d: int) -> list[int]:
    """S(d) in Python integers, in the probes' order and with their repeats."""
    out = [0, d]
    for k in range(101):
        a = -((-k * d) // 100)
        out += ([a - 1] if a > 0 else []) + [a] + ([a + 1] if a < d else [])
    return out


def numerators(d: int, kt: int) -> list[tuple]:
    """Every (mode, raw, mx, mn) the probes evaluate for divisor d (mn of DEFAULT / REVERSE: unused, None)."""
    s = boundary_set(d)
    out = []
    for mn in [RAW_LO] + ([0] if d <= RAW_HI else []) + [RAW_HI - d]:
        out += [(MINMAX, mn + a, mn + d, mn) for a in s]
    for mode in (DEFAULT, REVERSE):
        out += [(mode, a, d, None) for a in s] + [(mode, -a, d, None) for a in s]
        if kt != 0 or d > K32_NEG_D:
            k0 = (100 << 31) // d
            e = -(-((-k0 * d) // 100))
            for o in range(3):
                out += [(mode, RAW_LO + o, d, None), (mode, max(e - 1 + o, RAW_LO), d, None)]
    return out


def go_div(a: int, b: int) -> int:
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def normalized(mode: int, raw: int, mx: int, mn) -> int:
    """NormalizeScore of one raw in Go's int64 division (mx > 0, mx != mn)."""
    if mode == MINMAX:
        return go_div((raw - mn) * 100, mx - mn)
    q = go_div(100 * raw, mx)
    return q if mode == DEFAULT else 100 - q
