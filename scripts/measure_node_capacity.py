#!/usr/bin/env python3
"""The capacity column on C5 at full size (not part of bench.py): 5,000 nodes x 100,000 pods, one sequential
launch on the one-wave capacity kernel, bench.py's synthetic snapshot.

Three questions, answered into profiles/node_capacity_c5.json:

1. Did the scalar path move? max_pods_per_node = 15 and no column, timed on a library built from the parent
   commit (--parent-lib) and on this tree's, in alternating rounds of one process each. The new median has
   to lie within the parent's own min..max of the session.
2. What does the column cost? The same workload with a uniform column of 15 and scalar 0, and with a mixed
   column (a third of the nodes each at 5, 15 and 40): ms per launch and us per pod beside the scalar figure.
3. What does a one-node msh_patch_node_capacity cost on the host, at 5,000 and 100,000 nodes, beside a
   one-node msh_patch_nodes (the cordon flip)?

Every launch is timed with msh_timing_begin / _end (the kernel's own start and end) after a count reset, so
all launches of a mode do the same work; 5 warm-up launches, then LAUNCHES per round. Each worker process runs
under its own time limit, and nothing more is started once one fails. The workers bind the library with plain
ctypes, so one script drives both builds.

    python scripts/measure_node_capacity.py --parent-lib /path/to/parent/libminisched_hip.so
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

N_NODES, P, SCALAR = 5_000, 100_000, 15
WARMUP, LAUNCHES, ROUNDS, WORKER_LIMIT_S = 5, 20, 2, 240
PATCH_REPS = 200


def mixed_column(n: int) -> np.ndarray:
    return np.array([5, 15, 40], np.int32)[np.arange(n) % 3]


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


def worker(lib_path: str, modes: list[str]) -> int:
    import torch
    synth = importlib.import_module("mini-kube-scheduler_amd.synthetic")
    lib = bind(lib_path)
    ctx = C.c_void_p()
    ok(lib, None, lib.msh_create(0, C.byref(ctx)), "msh_create")
    u, nd, pd, pt = synth.make_soa(N_NODES, P)
    ok(lib, ctx, lib.msh_upload_nodes(ctx, N_NODES, vp(u), vp(nd)), "msh_upload_nodes")
    dev = torch.device("cuda:0")
    d_pd, d_pt = torch.from_numpy(pd).to(dev), torch.from_numpy(pt).to(dev)
    oi = torch.empty(P, dtype=torch.int32, device=dev)
    osc = torch.empty(P, dtype=torch.int64, device=dev)
    ost = torch.empty(P, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for mode in modes:
        scalar = SCALAR
        if mode != "scalar":
            col = np.full(N_NODES, SCALAR, np.int32) if mode == "uniform" else mixed_column(N_NODES)
            ok(lib, ctx, lib.msh_upload_node_capacity(ctx, N_NODES, vp(col)), "msh_upload_node_capacity")
            scalar = 0
        us = []
        for k in range(WARMUP + LAUNCHES):
            ok(lib, ctx, lib.msh_reset_node_pod_counts(ctx), "msh_reset_node_pod_counts")
            ok(lib, ctx, lib.msh_timing_begin(ctx, 1), "msh_timing_begin")
            ok(lib, ctx, lib.msh_schedule_sequential_device(
                ctx, P, C.c_void_p(d_pd.data_ptr()), C.c_void_p(d_pt.data_ptr()), scalar, C.c_void_p(oi.data_ptr()),
                C.c_void_p(osc.data_ptr()), C.c_void_p(ost.data_ptr()), stream), "msh_schedule_sequential_device")
            n, tot, mx = C.c_int32(), C.c_double(), C.c_double()
            ok(lib, ctx, lib.msh_timing_end(ctx, C.byref(n), C.byref(tot), C.byref(mx)), "msh_timing_end")
            assert n.value == 1
            if k >= WARMUP:
                us.append(tot.value * 1e3)
        torch.cuda.synchronize()
        counts = np.zeros(N_NODES, np.int32)
        ok(lib, ctx, lib.msh_node_pod_counts(ctx, vp(counts)), "msh_node_pod_counts")
        h = hashlib.sha256()
        for a in (oi.cpu().numpy(), osc.cpu().numpy(), ost.cpu().numpy(), counts):
            h.update(a.tobytes())
        out[mode] = {"us": us, "outputs_sha256": h.hexdigest(), "placed": int((ost == 0).sum().item()),
                     "max_count": int(counts.max())}
    lib.msh_destroy(ctx)
    print("RESULT " + json.dumps(out))
    return 0


def patch_worker(lib_path: str) -> int:
    """Host wall time of a one-node msh_patch_node_capacity and of a one-node msh_patch_nodes."""
    lib = bind(lib_path)
    ctx = C.c_void_p()
    ok(lib, None, lib.msh_create(0, C.byref(ctx)), "msh_create")
    out = {}
    for n in (5_000, 100_000):
        u, nd = np.zeros(n, np.uint8), (np.arange(n) % 10).astype(np.int8)
        ok(lib, ctx, lib.msh_upload_nodes(ctx, n, vp(u), vp(nd)), "msh_upload_nodes")
        ok(lib, ctx, lib.msh_upload_node_capacity(ctx, n, vp(np.full(n, 15, np.int32))), "msh_upload_node_capacity")
        cap_us, cordon_us = [], []
        for k in range(PATCH_REPS + 20):
            idx = np.array([(k * 7919) % n], np.int32)
            cap, flag, dig = np.array([k % 50], np.int32), np.array([k & 1], np.uint8), nd[idx]
            t0 = time.perf_counter()
            rc = lib.msh_patch_node_capacity(ctx, 1, vp(idx), vp(cap))
            t1 = time.perf_counter()
            rc2 = lib.msh_patch_nodes(ctx, 1, vp(idx), vp(flag), vp(dig))
            t2 = time.perf_counter()
            ok(lib, ctx, rc, "msh_patch_node_capacity")
            ok(lib, ctx, rc2, "msh_patch_nodes")
            if k >= 20:
                cap_us.append((t1 - t0) * 1e6)
                cordon_us.append((t2 - t1) * 1e6)
        out[str(n)] = {"patch_node_capacity_us_median": round(statistics.median(cap_us), 2),
                       "patch_node_capacity_us_min_max": [round(min(cap_us), 2), round(max(cap_us), 2)],
                       "patch_nodes_us_median": round(statistics.median(cordon_us), 2), "reps": PATCH_REPS}
    lib.msh_destroy(ctx)
    print("RESULT " + json.dumps(out))
    return 0


def run_worker(args: list[str]) -> dict:
    r = subprocess.run([sys.executable, __file__, *args], capture_output=True, text=True, timeout=WORKER_LIMIT_S)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"worker {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][7:])


def dist(us: list[float]) -> dict:
    med = statistics.median(us)
    return {"launches": len(us), "ms_median": round(med / 1e3, 4), "ms_min": round(min(us) / 1e3, 4),
            "ms_max": round(max(us) / 1e3, 4), "us_per_pod_median": round(med / P, 5),
            "ms_all": [round(x / 1e3, 4) for x in us]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libminisched_hip.so built from the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "node_capacity_c5.json"))
    ap.add_argument("--worker", nargs="+", metavar=("LIB", "MODE"))
    ap.add_argument("--patch-worker", metavar="LIB")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1:])
    if args.patch_worker:
        return patch_worker(args.patch_worker)
    build = importlib.import_module("mini-kube-scheduler_amd.build")
    new_lib = str(build.LIB)
    if not args.parent_lib or not Path(args.parent_lib).exists() or not Path(new_lib).exists():
        ap.error("--parent-lib and this tree's built library are both needed")
    us = {"parent_scalar": [], "scalar": [], "uniform": [], "mixed": []}
    sha = {}
    for _ in range(ROUNDS):  # parent and new alternate, one process each
        r = run_worker(["--worker", args.parent_lib, "scalar"])
        us["parent_scalar"] += r["scalar"]["us"]
        sha["parent_scalar"] = r["scalar"]["outputs_sha256"]
        r = run_worker(["--worker", new_lib, "scalar", "uniform", "mixed"])
        for m in ("scalar", "uniform", "mixed"):
            us[m] += r[m]["us"]
            sha[m] = r[m]["outputs_sha256"]
            sha[m + "_placed"] = r[m]["placed"]
    patch = run_worker(["--patch-worker", new_lib])
    d = {k: dist(v) for k, v in us.items()}
    lo, hi = d["parent_scalar"]["ms_min"], d["parent_scalar"]["ms_max"]
    within = lo <= d["scalar"]["ms_median"] <= hi
    spread_us_per_pod = (hi - lo) * 1e3 / P
    rec = {"workload": f"C5: {N_NODES} nodes x {P} pods, one msh_schedule_sequential_device launch, default plugins",
           "timer": "msh_timing_begin/end (kernel start to end), counts reset before every launch",
           "warmup": WARMUP, "launches_per_round": LAUNCHES, "rounds": ROUNDS,
           "scalar_15_no_column_parent": d["parent_scalar"], "scalar_15_no_column_new": d["scalar"],
           "scalar_path_new_median_within_parent_min_max": bool(within),
           "scalar_path_new_median_below_parent_min": bool(d["scalar"]["ms_median"] < lo),
           "column_uniform_15_scalar_0": d["uniform"], "column_mixed_5_15_40_scalar_0": d["mixed"],
           "parent_spread_us_per_pod": round(spread_us_per_pod, 5),
           "uniform_minus_scalar_us_per_pod": round(d["uniform"]["us_per_pod_median"] - d["scalar"]["us_per_pod_median"], 5),
           "mixed_minus_scalar_us_per_pod": round(d["mixed"]["us_per_pod_median"] - d["scalar"]["us_per_pod_median"], 5),
           "check_scalar_outputs_equal_parent": sha["scalar"] == sha["parent_scalar"],
           "check_uniform_column_outputs_equal_scalar": sha["uniform"] == sha["scalar"],
           "placed": {m: sha[m + "_placed"] for m in ("scalar", "uniform", "mixed")},
           "one_node_patch_host_wall_us": patch, "sources_sha256": build.sources_digest()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({k: v for k, v in rec.items() if not isinstance(v, dict) or "ms_all" not in v}))
    for k in ("scalar_15_no_column_parent", "scalar_15_no_column_new", "column_uniform_15_scalar_0", "column_mixed_5_15_40_scalar_0"):
        print(k, {a: b for a, b in rec[k].items() if a != "ms_all"})
    good = rec["check_scalar_outputs_equal_parent"] and rec["check_uniform_column_outputs_equal_scalar"]
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
