"""The driver's multi-GPU bench command, rehearsed on one GPU (verdict r4, next #4).

At round end the driver runs `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
--master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W` on an 8-GPU node.
These tests launch exactly that command as a fresh child process at N = 2 with MSH_BENCH_REHEARSE=1
(every rank on cuda:0, the process group on gloo: RCCL refuses two ranks on one device), in each mode
bench.py has: pod-sharded batches (the default), the node-sharded C4 shape (keys merged by an
all-reduce MAX across the ranks) and pod-sharded sequential commit, with --full added so that rank 0
checks the outputs. Each must print one JSON line whose outputs were checked bit-exact against the
closed form on rank 0, with n_gpus = 2. Not a measurement: the ranks share one device.

A plain one-GPU run (no --full) is launched too: the headline keys only, and --dump-outputs.
"""
from __future__ import annotations

import importlib.util
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from closed_form import closed_form_modes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("extra", [[], ["--mode", "nodeshard", "--nodes", "20000", "--pods", "100000"],
                                   ["--mode", "sequential"]], ids=["batch", "nodeshard", "sequential"])
def test_driver_command_two_ranks(msh, extra):
    env = dict(os.environ, MSH_BENCH_REHEARSE="1", OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "4"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(ROOT / "bench.py"),
           "--gpus", "2", "--steps", "4", "--warmup", "1", "--full", *extra]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2
    assert line["check"] == "bit-exact vs closed form", line["check"]
    assert line["config"].get("rehearsal"), line["config"]
    assert line["value"] > 0 and line["steps"] == 4 and line["warmup"] == 1


def test_plain_run_headline_only_and_dump(msh, synth, tmp_path):
    """A plain one-GPU run prints the headline keys and nothing that takes a run of its own, and
    --dump-outputs writes what the last of the K timed steps computed: step K - 1 schedules batch
    K - 1 of the pod stream (cut here exactly as bench.py cuts it), checked against the closed form."""
    n, p, k = 1000, 4096, 3
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(k), "--warmup", "1",
           "--nodes", str(n), "--pods", str(p), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["steps"] == k and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(n * p / (line["ms_per_step"] * 1e-3))
    for key in ("check", "roofline", "cpu_baseline", "c3_plugin_variants", "generic", "e2e", "c4_one_gpu"):
        assert key not in line, key
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)  # for the headline plugin list's weight and normalizer
    spec.loader.exec_module(bench)
    u, nd = synth.make_nodes(n)[1:]
    G = msh._native.BATCHES_PER_LAUNCH
    pd_all, pt_all = synth._make_pods_fast(p * G, synth.SEED)[1:]
    lo = ((k - 1) % G) * p
    want = closed_form_modes(u, nd, pd_all[lo:lo + p], pt_all[lo:lo + p], bench.HEADLINE_WEIGHT, bench.HEADLINE_NORM)
    for name, w in zip(("idx", "score", "status"), want):
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == (p,)
        assert (got == w).all(), name
