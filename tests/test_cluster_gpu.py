"""The object-level differential of tests/test_cluster.py on the device: the same seeded scenarios scheduled through
Scheduler over a real DeviceContext against tests/cluster_ref.py, bit-exact on every pod's outcome, node name and score
and, after every call, on node_pod_counts(), the `used` half of node_resources(), spread_counts() and, once the
snapshot has an inter-pod term, pod_affinity_state() against the words derived from the reference's placed list under
the scheduler's current term order. One test per scenario; the time is the reference's Python, not the kernel's. A
fresh context per scenario: a Scheduler sets only what it is configured with."""
from __future__ import annotations

import pytest

import cluster_gen as G
from test_cluster import run_scenario

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(G.SCENARIOS))
def test_scheduler_on_the_device_matches_the_object_reference(msh, oracle, name):
    if msh.device_count() < 1:
        pytest.skip("no GPU")
    with msh.DeviceContext(0) as ctx:
        run_scenario(msh, oracle, G.scenario(name), ctx)
