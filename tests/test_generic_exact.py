"""The cases of tests/generic_exact.py on the CPU: the construction shows every listed quotient in some pod's output."""
from __future__ import annotations

import pytest

import generic_exact as GE

CASES = GE.cases()


def test_case_list_covers_the_issue():
    names = {c["name"] for c in CASES}
    for tag in ("default", "reverse", "minmax"):
        for m in GE.DIVISORS:
            for width in GE.WIDTHS:
                assert f"{tag}-{m}-{width}" in names
    assert all(f"minmax-{(1 << 32) - 1}-{w}" in names for w in GE.WIDTHS)
    assert all(100 < c["n"] - c["pad"] < 400 or c["L"] < 20 for c in CASES)
    pd, pt = GE.pods()
    assert len(pd) == GE.P == 130 and all(0 < pt[b:b + 64].sum() < len(pt[b:b + 64]) for b in (0, 64, 128))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_listed_quotient_decides_an_output(c):
    """Unperturbed, the pod that does not tolerate the taint takes the head node at the common total at every step. With one
    listed pair's quotient off by +1 or by -1, one pair at a time, some pod's node or score differs at step 0 or at
    the step where that node is the head: every listed pair is detected in both directions."""
    base = {(t, tol): GE.outcome(c, t, tol) for t in range(c["L"]) for tol in (False, True)}
    for t in range(c["L"]):
        assert base[t, False] == (c["pad"] + t, GE.base_total(c))
    missed = []
    for k in range(c["L"]):
        i = c["pad"] + k
        for s in (1, -1):
            if not any(GE.outcome(c, t, tol, (i, s)) != base[t, tol] for t in {0, k} for tol in (False, True)):
                missed.append((c["raws"][i], s))
    assert not missed, missed
