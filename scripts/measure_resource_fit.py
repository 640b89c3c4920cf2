#!/usr/bin/env python3
"""Resource requests on C5 at full size (not part of bench.py): 5,000 nodes x 100,000 pods, one sequential launch,
bench.py's synthetic snapshot. Written into profiles/resource_fit_c5.json:

(a) the existing scalar capacity form, max_pods_per_node = 15, no column and no table: on a library built from
    the parent commit (--parent-lib) and on this tree's, in alternating rounds of one process each. The new
    median has to lie within the parent's own min..max of the session: the new code must not have moved it.
(b) msh_schedule_sequential_fit_device with two resources, alloc 15 units each and every request 1 unit, which
    reproduces (a)'s placements (checked by the outputs' digest).
(c) the same with mixed requests (cpu 100..2,000 milli against 16,000; memory 128..4,096 MiB against 64 GiB).
(d) the host wall time of a one-node msh_patch_node_resources.

Every launch is timed with msh_timing_begin / _end (the kernel's own start and end) after a count reset and, for
(b) and (c), a fresh upload of the table, so all launches of a mode do the same work; 5 warm-up launches, then
LAUNCHES per round. Each worker process runs under its own time limit, and nothing more is started once one
fails. The workers bind the library with plain ctypes, so one script drives both builds.

    python scripts/measure_resource_fit.py --parent-lib /path/to/parent/libminisched_hip.so
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

N_NODES, P, SCALAR, NRES = 5_000, 100_000, 15, 2
WARMUP, LAUNCHES, ROUNDS, WORKER_LIMIT_S = 5, 20, 2, 300
PATCH_REPS = 200
MIB = 1 << 20


def tables(mode: str):
    """(alloc, req) of a _fit mode, shaped (NRES, n) and (NRES, p)."""
    if mode == "fit_unit":
        return np.full((NRES, N_NODES), SCALAR, np.int64), np.ones((NRES, P), np.int64)
    rng = np.random.default_rng(5)
    alloc = np.stack([np.full(N_NODES, 16_000, np.int64), np.full(N_NODES, 64 * 1024 * MIB, np.int64)])
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
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = {}
    for mode in modes:
        fit = mode != "scalar"
        if fit:
            alloc, req = tables(mode)
            d_rq = torch.from_numpy(req).to(dev)
        us = []
        for k in range(WARMUP + LAUNCHES):
            ok(lib, ctx, lib.msh_reset_node_pod_counts(ctx), "msh_reset_node_pod_counts")
            if fit:
                ok(lib, ctx, lib.msh_upload_node_resources(ctx, N_NODES, NRES, vp(alloc), None), "msh_upload_node_resources")
            ok(lib, ctx, lib.msh_timing_begin(ctx, 1), "msh_timing_begin")
            if fit:
                ok(lib, ctx, lib.msh_schedule_sequential_fit_device(ctx, P, p(d_pd), p(d_pt), NRES, p(d_rq), 0, p(oi), p(osc),
                                                                    p(ost), stream), "msh_schedule_sequential_fit_device")
            else:
                ok(lib, ctx, lib.msh_schedule_sequential_device(ctx, P, p(d_pd), p(d_pt), SCALAR, p(oi), p(osc), p(ost),
                                                                stream), "msh_schedule_sequential_device")
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
        if fit:
            ok(lib, ctx, lib.msh_clear_node_resources(ctx), "msh_clear_node_resources")
    lib.msh_destroy(ctx)
    print("RESULT " + json.dumps(out))
    return 0


def patch_worker(lib_path: str) -> int:
    """Host wall time of a one-node msh_patch_node_resources (alloc and used of both resources)."""
    lib = bind(lib_path)
    ctx = C.c_void_p()
    ok(lib, None, lib.msh_create(0, C.byref(ctx)), "msh_create")
    n = N_NODES
    u, nd = np.zeros(n, np.uint8), (np.arange(n) % 10).astype(np.int8)
    ok(lib, ctx, lib.msh_upload_nodes(ctx, n, vp(u), vp(nd)), "msh_upload_nodes")
    ok(lib, ctx, lib.msh_upload_node_resources(ctx, n, NRES, vp(np.full((NRES, n), 15, np.int64)), None),
       "msh_upload_node_resources")
    us = []
    for k in range(PATCH_REPS + 20):
        idx = np.array([(k * 7919) % n], np.int32)
        a, b = np.full((NRES, 1), 20 + k % 50, np.int64), np.full((NRES, 1), k % 7, np.int64)
        t0 = time.perf_counter()
        rc = lib.msh_patch_node_resources(ctx, 1, vp(idx), vp(a), vp(b))
        t1 = time.perf_counter()
        ok(lib, ctx, rc, "msh_patch_node_resources")
        if k >= 20:
            us.append((t1 - t0) * 1e6)
    lib.msh_destroy(ctx)
    print("RESULT " + json.dumps({"nodes": n, "us_median": round(statistics.median(us), 2),
                                  "us_min_max": [round(min(us), 2), round(max(us), 2)], "reps": PATCH_REPS}))
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "resource_fit_c5.json"))
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
    modes = ("scalar", "fit_unit", "fit_mixed")
    us = {"parent_scalar": [], **{m: [] for m in modes}}
    info = {}
    for _ in range(ROUNDS):  # parent and new alternate, one process each
        r = run_worker(["--worker", args.parent_lib, "scalar"])
        us["parent_scalar"] += r["scalar"]["us"]
        info["parent_scalar"] = r["scalar"]
        r = run_worker(["--worker", new_lib, *modes])
        for m in modes:
            us[m] += r[m]["us"]
            info[m] = r[m]
    patch = run_worker(["--patch-worker", new_lib])
    d = {k: dist(v) for k, v in us.items()}
    lo, hi = d["parent_scalar"]["ms_min"], d["parent_scalar"]["ms_max"]
    a = d["scalar"]["ms_median"]
    ratio = lambda m: {"median": round(d[m]["ms_median"] / a, 2), "min": round(d[m]["ms_min"] / a, 2),  # noqa: E731
                       "max": round(d[m]["ms_max"] / a, 2)}
    rec = {"workload": f"C5: {N_NODES} nodes x {P} pods, one sequential launch, default plugins",
           "timer": "msh_timing_begin/end (kernel start to end), counts reset (and the table uploaded) before every launch",
           "warmup": WARMUP, "launches_per_round": LAUNCHES, "rounds": ROUNDS,
           "a_scalar_15_parent": d["parent_scalar"], "a_scalar_15_new": d["scalar"],
           "a_new_median_within_parent_min_max": bool(lo <= a <= hi),
           "a_new_median_below_parent_min": bool(a < lo),
           "b_fit_2_resources_unit_requests": d["fit_unit"], "c_fit_2_resources_mixed_requests": d["fit_mixed"],
           "b_over_a": ratio("fit_unit"), "c_over_a": ratio("fit_mixed"),
           "check_a_outputs_equal_parent": info["scalar"]["outputs_sha256"] == info["parent_scalar"]["outputs_sha256"],
           "check_b_outputs_equal_a": info["fit_unit"]["outputs_sha256"] == info["scalar"]["outputs_sha256"],
           "placed": {m: info[m]["placed"] for m in modes}, "max_count": {m: info[m]["max_count"] for m in modes},
           "d_one_node_patch_node_resources_host_wall": patch, "sources_sha256": build.sources_digest()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({k: ({x: y for x, y in v.items() if x != "ms_all"} if isinstance(v, dict) else v) for k, v in rec.items()},
                     indent=1))
    return 0 if rec["check_a_outputs_equal_parent"] and rec["check_b_outputs_equal_a"] else 1


if __name__ == "__main__":
    sys.exit(main())
