"""The written cases, the seeded traces and the seq_waves checks of tests/table_readback.py on a DeviceContext.

After every operation both observers read all n nodes back: the planes through eleven capacity-1 sweeps of the
sequential kernel, the columns through one export of 11 pod kinds. The comparison with the model is exact equality; a
failure names the operation, the observer and the first differing nodes with got and want. One test holds one context and
one family of cases.

Measured on an MI355X: 2.4 s for the file; one_node[2500] (105 read-backs) 0.99 s, the one-node families at 1,000, 1,024
and 1,025 nodes 0.4 s each, sequences[2500] 0.36 s, every other family, trace and seq_waves test under 0.2 s.
"""
from __future__ import annotations

import pytest

import table_readback as T

pytestmark = pytest.mark.gpu

FAMILIES = T.hand_families()
TRACES = T.trace_set()


@pytest.fixture(scope="module")
def device(msh):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    return 0


@pytest.mark.parametrize("family", list(FAMILIES))
def test_hand_cases(msh, oracle, device, family):
    with msh.DeviceContext(0) as ctx:
        for name, ops in FAMILIES[family]:
            T.run_case(ctx, ops, refused=msh.MshError, oracle=oracle, label=name)


@pytest.mark.parametrize("k", range(T.TRACE_COUNT))
def test_traces(msh, oracle, device, k):
    name, ops = TRACES[k]
    with msh.DeviceContext(0) as ctx:
        T.run_case(ctx, ops, refused=msh.MshError, oracle=oracle, label=name)


@pytest.mark.parametrize("seq_waves", ["1", "4", "16"])
def test_plane_consumers(msh, oracle, device, seq_waves):
    """The planes after an inline and a scattered patch at n = 2,500, read by each instance of the sequential kernel."""
    with msh.DeviceContext(0, {"seq_waves": seq_waves}) as ctx:
        T.run_case(ctx, T.seq_waves_case(), refused=msh.MshError, oracle=oracle, label=f"seq_waves={seq_waves}")
