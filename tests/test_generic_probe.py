"""generic_kernel's NormalizeScore by reciprocal (csrc/msh_generic_norm.h) on the CPU: the numerators
and counts of tests/generic_probe.py against Python integers, and a host build of the header's double paths (the
8-byte key types) over the probes' numerators. The host build is evidence about the arithmetic, not about the device:
IEEE doubles give the same quotients on both, so when a case of tests/test_generic_probe_gpu.py fails, this file tells
a host/device difference (these pass) from a wrong claim (these fail too)."""
from __future__ import annotations

import numpy as np
import pytest

import generic_probe as GP
import quot_probe as QP

EDGE_DIVISORS = (1, 2, 3, 7, 99, 100, 101, 25600, 25601, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32)


def test_boundary_numerators_are_the_quotient_boundaries():
    """The generator against Python integers: every k in 0..100 has the smallest numerator reaching it and both
    neighbours, every raw and extent is one a score column can hold (MIN-MAX; DEFAULT and REVERSE stay within
    [-2^32, 2^32]), the negative edge raws sit on a quotient boundary, and the counts are the generator's."""
    for d in EDGE_DIVISORS:
        s = GP.boundary_set(d)
        assert len(s) == GP.set_size(d) and min(s) == 0 and max(s) == d
        for k in range(101):
            b = -((-k * d) // 100)
            assert b in s and 100 * b // d >= k and (b == 0 or 100 * (b - 1) // d < k)
            assert max(b - 1, 0) in s and min(b + 1, d) in s
        for kt in (0, 1, 2):
            nums = GP.numerators(d, kt)
            assert len(nums) == GP.evaluations(d, kt) == GP.count_list(np.array([d], np.uint64), kt)
            assert GP.count_range(d, d + 1, kt) == len(nums)
            for mode, raw, mx, mn in nums:
                if mode == GP.MINMAX:
                    assert GP.RAW_LO <= mn <= raw <= mx <= GP.RAW_HI and mx - mn == d
                else:
                    assert abs(raw) <= GP.D_MAX and mx == d
                assert abs(100 * raw) < 1 << 39
                if kt == 0:
                    assert abs(GP.normalized(mode, raw, mx, mn)) < (1 << 23) + 100
            if kt != 0 or d > GP.K32_NEG_D:   # e: the largest raw with the quotient of -2^31; e + 1 has a higher one
                q_lo = GP.go_div(100 * GP.RAW_LO, d)
                e = (q_lo * d) // 100                # -ceil(-q_lo * d / 100)
                assert e >= GP.RAW_LO and GP.go_div(100 * e, d) == q_lo and GP.go_div(100 * (e + 1), d) > q_lo
                for raw in (GP.RAW_LO, GP.RAW_LO + 1, GP.RAW_LO + 2, max(e - 1, GP.RAW_LO), e, e + 1):
                    assert (GP.DEFAULT, raw, d, None) in nums and (GP.REVERSE, raw, d, None) in nums
    assert GP.count_range(1, 30000, 0) == sum(GP.evaluations(d, 0) for d in range(1, 30000))
    assert GP.count_range(90, 300, 2) == GP.count_list(np.arange(90, 300, dtype=np.uint64), 2)
    hi = np.array([GP.RAW_HI - 1, GP.RAW_HI, GP.RAW_HI + 1, GP.D_MAX], np.uint64)
    assert GP.count_list(hi, 1) == GP.count_range(GP.RAW_HI - 1, GP.RAW_HI + 2, 1) + GP.evaluations(GP.D_MAX, 1)


def host_divisors() -> np.ndarray:
    """Above 2^20: every d within 2^8 of a power of two up to 2^32 and 2^14 seeded random divisors."""
    rnd = np.random.default_rng(2032).integers(1 << 20, GP.D_MAX, 1 << 14, dtype=np.uint64, endpoint=True)
    return np.ascontiguousarray(np.concatenate([GP.near_powers(20, 32, 1 << 20, GP.D_MAX, 1 << 8), rnd]))


@pytest.mark.parametrize("kt", [1, 2], ids=["u64", "f53"])
def test_host_build_every_divisor_to_2_20(kt):
    """The host build of gen_norm_params and col_term<KT> at every d <= 2^20 and at host_divisors(), r as
    gen_norm_params forms it: every term equals the host's int64 `/` and gen_normalize. Evidence about the arithmetic,
    not about the device. About 4 s on 8 threads."""
    n = 1 << 20
    mis, misn, seen, first = GP.run_quot_host(kt, None, 1, n, 0)
    assert seen == GP.count_range(1, n + 1, kt)
    assert mis == 0 and misn == 0, f"{mis} / {misn} wrong, first (mode, raw, mx, mn, got, want) = {first}"
    ds = host_divisors()
    mis, misn, seen, first = GP.run_quot_host(kt, ds, 0, len(ds), 0)
    assert seen == GP.count_list(ds, kt)
    assert mis == 0 and misn == 0, f"{mis} / {misn} wrong, first (mode, raw, mx, mn, got, want) = {first}"


@pytest.mark.parametrize("ulps", [-1, 1])
@pytest.mark.parametrize("kt", [1, 2], ids=["u64", "f53"])
def test_host_build_one_ulp_either_way(kt, ulps):
    """The same at r one ulp either way, over every d <= 2^16 and host_divisors(): the claim's margin."""
    ds = np.ascontiguousarray(np.concatenate([np.arange(1, (1 << 16) + 1, dtype=np.uint64), host_divisors()]))
    mis, misn, seen, first = GP.run_quot_host(kt, ds, 0, len(ds), ulps)
    assert seen == GP.count_list(ds, kt)
    assert mis == 0 and misn == 0, f"{mis} / {misn} wrong, first (mode, raw, mx, mn, got, want) = {first}"


@pytest.mark.parametrize("kt", [1, 2], ids=["u64", "f53"])
def test_host_build_unbiased_reciprocal_fails(kt):
    """r = 1 / d without GEN_RCP_BIAS gives wrong quotients, and the first one reported is wrong in Python integers
    too: the check sees the error the bias exists for."""
    ds = np.ascontiguousarray(np.arange(1, (1 << 16) + 1, dtype=np.uint64))
    mis, misn, seen, first = GP.run_quot_host(kt, ds, 0, len(ds), 0, unbiased=True)
    assert seen == GP.count_list(ds, kt) and misn == 0
    assert mis > 0
    mode, raw, mx, mn, got, want = first
    assert want == GP.normalized(mode, raw, mx, mn) and got != want
