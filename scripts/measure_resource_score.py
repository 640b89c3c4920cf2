#!/usr/bin/env python3
"""Resource-aware scoring on C5 (not part of bench.py): bench.py's synthetic snapshot cut to the scored form's table
limit for two resources (msh_seq_fit_max_nodes: 4,096 of C5's 5,000 nodes) x 100,000 pods, one sequential launch.
Written into profiles/resource_score_c5.json:

(a) the unscored msh_schedule_sequential_fit_device with two resources and mixed requests (cpu 100..2,000 milli
    against 16,000; memory 128..4,096 MiB against 64 GiB), on a library built from the parent commit
    (--parent-lib) and on this tree's, in alternating rounds of one process each. The outputs must be equal and the
    new mean has to lie within the parent's own min..max of the session: the existing kernel is untouched.
(b) LEAST_ALLOCATED and MOST_ALLOCATED (weight 1, resource weights 1, 1) on the same inputs: per-launch and per-pod
    time, the ratio to (a), the pods placed and the distinct nodes used.
(c) the host wall time of one msh_set_resource_score call.

Every launch is timed with msh_timing_begin / _end (the kernel's own start and end) after a count reset and a fresh
upload of the table, so all launches of a mode do the same work; WARMUP warm-up launches, then LAUNCHES per round.
Each worker process runs under its own time limit, and nothing more is started once one fails. The workers bind the
library with plain ctypes, so one script drives both builds.

    python scripts/measure_resource_score.py --parent-lib /path/to/parent/libminisched_hip.so
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import importlib
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]

C5_NODES, P, NRES = 5_000, 100_000, 2
WARMUP, LAUNCHES, ROUNDS, WORKER_LIMIT_S = 2, 8, 2, 400
SET_REPS = 2000
MIB = 1 << 20
MODES = {"fit": 0, "least": 1, "most": 2}


def tables(n: int):
    rng = np.random.default_rng(5)
    alloc = np.stack([np.full(n, 16_000, np.int64), np.full(n, 64 * 1024 * MIB, np.int64)])
    req = np.stack([rng.integers(1, 21, P) * 100, rng.integers(1, 33, P) * 128 * MIB]).astype(np.int64)
    return alloc, req


def bind(path: str):
    native = importlib.import_module("mini-kube-scheduler_amd._native")
    native._share_hip_runtime_with_torch()
    return C.CDLL(path)


def ok(lib, ctx, rc, what):
    if rc != 0:
        lib.msh_last_error.restype = C.c_char_p
        raise RuntimeError(f"{what}: {rc}: {lib.msh_last_error(ctx).decode()}")


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def worker(lib_path: str, n: int, modes: list[str]) -> int:
    import torch
    synth = importlib.import_module("mini-kube-scheduler_amd.synthetic")
    lib = bind(lib_path)
    ctx = C.c_void_p()
    ok(lib, None, lib.msh_create(0, C.byref(ctx)), "msh_create")
    u, nd, pd, pt = synth.make_soa(C5_NODES, P)
    u, nd = np.ascontiguousarray(u[:n]), np.ascontiguousarray(nd[:n])
    ok(lib, ctx, lib.msh_upload_nodes(ctx, n, vp(u), vp(nd)), "msh_upload_nodes")
    dev = torch.device("cuda:0")
    d_pd, d_pt = torch.from_numpy(pd).to(dev), torch.from_numpy(pt).to(dev)
    oi = torch.empty(P, dtype=torch.int32, device=dev)
    osc = torch.empty(P, dtype=torch.int64, device=dev)
    ost = torch.empty(P, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    alloc, req = tables(n)
    d_rq = torch.from_numpy(req).to(dev)
    rw = np.ones(NRES, np.int32)
    out = {}
    for mode in modes:
        if MODES[mode]:
            ok(lib, ctx, lib.msh_set_resource_score(ctx, MODES[mode], C.c_int64(1), NRES, vp(rw)), "msh_set_resource_score")
        us = []
        for k in range(WARMUP + LAUNCHES):
            ok(lib, ctx, lib.msh_reset_node_pod_counts(ctx), "msh_reset_node_pod_counts")
            ok(lib, ctx, lib.msh_upload_node_resources(ctx, n, NRES, vp(alloc), None), "msh_upload_node_resources")
            ok(lib, ctx, lib.msh_timing_begin(ctx, 1), "msh_timing_begin")
            ok(lib, ctx, lib.msh_schedule_sequential_fit_device(ctx, P, p(d_pd), p(d_pt), NRES, p(d_rq), 0, p(oi), p(osc),
                                                                p(ost), stream), "msh_schedule_sequential_fit_device")
            cnt, tot, mx = C.c_int32(), C.c_double(), C.c_double()
            ok(lib, ctx, lib.msh_timing_end(ctx, C.byref(cnt), C.byref(tot), C.byref(mx)), "msh_timing_end")
            assert cnt.value == 1
            if k >= WARMUP:
                us.append(tot.value * 1e3)
        torch.cuda.synchronize()
        counts = np.zeros(n, np.int32)
        ok(lib, ctx, lib.msh_node_pod_counts(ctx, vp(counts)), "msh_node_pod_counts")
        h = hashlib.sha256()
        for a in (oi.cpu().numpy(), osc.cpu().numpy(), ost.cpu().numpy(), counts):
            h.update(a.tobytes())
        out[mode] = {"us": us, "outputs_sha256": h.hexdigest(), "placed": int((ost == 0).sum().item()),
                     "distinct_nodes": int((counts > 0).sum()), "max_count": int(counts.max())}
    lib.msh_destroy(ctx)
    print("RESULT " + json.dumps(out))
    return 0


def set_worker(lib_path: str) -> int:
    """Host wall time of one msh_set_resource_score call."""
    lib = bind(lib_path)
    ctx = C.c_void_p()
    ok(lib, None, lib.msh_create(0, C.byref(ctx)), "msh_create")
    rw = np.ones(NRES, np.int32)
    us = []
    for k in range(SET_REPS + 20):
        t0 = time.perf_counter()
        rc = lib.msh_set_resource_score(ctx, 1 + k % 2, C.c_int64(1 + k % 5), NRES, vp(rw))
        t1 = time.perf_counter()
        ok(lib, ctx, rc, "msh_set_resource_score")
        if k >= 20:
            us.append((t1 - t0) * 1e6)
    lib.msh_destroy(ctx)
    print("RESULT " + json.dumps({"us_median": round(statistics.median(us), 3),
                                  "us_min_max": [round(min(us), 3), round(max(us), 3)], "reps": SET_REPS}))
    return 0


def run_worker(args: list[str]) -> dict:
    r = subprocess.run([sys.executable, __file__, *args], capture_output=True, text=True, timeout=WORKER_LIMIT_S)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"worker {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][7:])


def dist(us: list[float]) -> dict:
    mean = statistics.fmean(us)
    return {"launches": len(us), "ms_mean": round(mean / 1e3, 4), "ms_median": round(statistics.median(us) / 1e3, 4),
            "ms_min": round(min(us) / 1e3, 4), "ms_max": round(max(us) / 1e3, 4), "us_per_pod_mean": round(mean / P, 5),
            "ms_all": [round(x / 1e3, 4) for x in us]}


def scored_limit(lib_path: str) -> int:
    lib = bind(lib_path)
    ctx = C.c_void_p()
    ok(lib, None, lib.msh_create(0, C.byref(ctx)), "msh_create")
    out = C.c_int32()
    ok(lib, ctx, lib.msh_seq_fit_max_nodes(ctx, NRES, 1, C.byref(out)), "msh_seq_fit_max_nodes")
    lib.msh_destroy(ctx)
    return out.value


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libminisched_hip.so built from the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resource_score_c5.json"))
    ap.add_argument("--worker", nargs="+", metavar=("LIB", "N"))
    ap.add_argument("--set-worker", metavar="LIB")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], int(args.worker[1]), args.worker[2:])
    if args.set_worker:
        return set_worker(args.set_worker)
    build = importlib.import_module("mini-kube-scheduler_amd.build")
    new_lib = str(build.LIB)
    if not args.parent_lib or not Path(args.parent_lib).exists() or not Path(new_lib).exists():
        ap.error("--parent-lib and this tree's built library are both needed")
    n = min(C5_NODES, scored_limit(new_lib))
    modes = ("fit", "least", "most")
    us = {"parent_fit": [], **{m: [] for m in modes}}
    info = {}
    for _ in range(ROUNDS):  # parent and new alternate, one process each
        r = run_worker(["--worker", args.parent_lib, str(n), "fit"])
        us["parent_fit"] += r["fit"]["us"]
        info["parent_fit"] = r["fit"]
        r = run_worker(["--worker", new_lib, str(n), *modes])
        for m in modes:
            us[m] += r[m]["us"]
            info[m] = r[m]
    setter = run_worker(["--set-worker", new_lib])
    d = {k: dist(v) for k, v in us.items()}
    lo, hi = d["parent_fit"]["ms_min"], d["parent_fit"]["ms_max"]
    a = d["fit"]["ms_mean"]
    ratio = lambda m: {"mean": round(d[m]["ms_mean"] / a, 2), "min": round(d[m]["ms_min"] / a, 2),  # noqa: E731
                       "max": round(d[m]["ms_max"] / a, 2)}
    rec = {"workload": f"C5 cut to the scored table limit: {n} of {C5_NODES} nodes x {P} pods, one sequential launch, "
                       "default plugins, two resources, mixed requests",
           "timer": "msh_timing_begin/end (kernel start to end), counts reset and the table uploaded before every launch",
           "warmup": WARMUP, "launches_per_round": LAUNCHES, "rounds": ROUNDS,
           "a_fit_unscored_parent": d["parent_fit"], "a_fit_unscored_new": d["fit"],
           "a_new_mean_within_parent_min_max": bool(lo <= a <= hi),
           "check_a_outputs_equal_parent": info["fit"]["outputs_sha256"] == info["parent_fit"]["outputs_sha256"],
           "b_least_allocated": d["least"], "b_most_allocated": d["most"],
           "b_least_over_a": ratio("least"), "b_most_over_a": ratio("most"),
           "placed": {m: info[m]["placed"] for m in modes},
           "distinct_nodes": {m: info[m]["distinct_nodes"] for m in modes},
           "max_count": {m: info[m]["max_count"] for m in modes},
           "c_set_resource_score_host_wall": setter, "sources_sha256": build.sources_digest()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({k: ({x: y for x, y in v.items() if x != "ms_all"} if isinstance(v, dict) else v) for k, v in rec.items()},
                     indent=1))
    return 0 if rec["check_a_outputs_equal_parent"] and rec["a_new_mean_within_parent_min_max"] else 1


if __name__ == "__main__":
    sys.exit(main())
