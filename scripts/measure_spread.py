#!/usr/bin/env python3
"""Pod topology spread on C5 (not part of bench.py): bench.py's synthetic snapshot at C5's own size, 5,000 nodes x
100,000 pods, two resources, one sequential launch. Written into profiles/spread_c5.json:

(a) msh_schedule_sequential_fit_device on a library built from the parent commit (--parent-lib) and on this tree's,
    in alternating rounds of one process each. The outputs must be equal and the new mean has to lie within the
    parent's own min..max of the session: the existing kernel is untouched.
(b) msh_schedule_sequential_spread_device with every pod ungrouped on the same inputs, against (a): the cost of the
    frame (the group loads, the zone bytes, the mask test).
(c) 16 groups x 8 zones at max_skew = 1, pods dealt to the groups in turn; (d) one group holding every pod (8 zones,
    max_skew = 1): every step takes the row read, the wave minimum, the ballot and, when it places, the second
    barrier. Per case: ms per launch, us per pod, pods placed and the FIT_ERROR count.

Every launch is timed with msh_timing_begin / _end (the kernel's own start and end) after a reset of the pod and
spread counts and a fresh upload of the table, so all launches of a case do the same work; WARMUP warm-up launches,
then LAUNCHES per round. Each worker process runs under its own time limit, and nothing more is started once one
fails. The workers bind the library with plain ctypes, so one script drives both builds.

    python scripts/measure_spread.py --parent-lib /path/to/parent/libminisched_hip.so
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
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]

N, P, NRES, ZONES = 5_000, 100_000, 2, 8
WARMUP, LAUNCHES, ROUNDS, WORKER_LIMIT_S = 2, 6, 2, 400
MIB = 1 << 20
CASES = ("fit", "ungrouped", "groups16", "group1")


def tables():
    rng = np.random.default_rng(5)
    alloc = np.stack([np.full(N, 16_000, np.int64), np.full(N, 64 * 1024 * MIB, np.int64)])
    req = np.stack([rng.integers(1, 21, P) * 100, rng.integers(1, 33, P) * 128 * MIB]).astype(np.int64)
    zone = rng.integers(0, ZONES, N).astype(np.int32)
    return alloc, req, zone


def groups(case: str):
    """(max_skew per group, group per pod)"""
    if case == "groups16":
        return np.ones(16, np.int32), (np.arange(P) % 16).astype(np.int32)
    if case == "group1":
        return np.ones(1, np.int32), np.zeros(P, np.int32)
    return np.ones(1, np.int32), np.full(P, -1, np.int32)


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


def worker(lib_path: str, cases: list[str]) -> int:
    import torch
    synth = importlib.import_module("mini-kube-scheduler_amd.synthetic")
    lib = bind(lib_path)
    ctx = C.c_void_p()
    ok(lib, None, lib.msh_create(0, C.byref(ctx)), "msh_create")
    u, nd, pd, pt = synth.make_soa(N, P)
    ok(lib, ctx, lib.msh_upload_nodes(ctx, N, vp(u), vp(nd)), "msh_upload_nodes")
    dev = torch.device("cuda:0")
    d_pd, d_pt = torch.from_numpy(pd).to(dev), torch.from_numpy(pt).to(dev)
    oi = torch.empty(P, dtype=torch.int32, device=dev)
    osc = torch.empty(P, dtype=torch.int64, device=dev)
    ost = torch.empty(P, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    alloc, req, zone = tables()
    d_rq = torch.from_numpy(req).to(dev)
    out = {}
    for case in cases:
        spread = case != "fit"
        if spread:
            skew, grp = groups(case)
            d_grp = torch.from_numpy(grp).to(dev)
            ok(lib, ctx, lib.msh_set_spread_groups(ctx, len(skew), vp(skew)), "msh_set_spread_groups")
            ok(lib, ctx, lib.msh_upload_node_zones(ctx, N, vp(zone)), "msh_upload_node_zones")
        us = []
        for k in range(WARMUP + LAUNCHES):
            ok(lib, ctx, lib.msh_reset_node_pod_counts(ctx), "msh_reset_node_pod_counts")
            ok(lib, ctx, lib.msh_upload_node_resources(ctx, N, NRES, vp(alloc), None), "msh_upload_node_resources")
            if spread:
                ok(lib, ctx, lib.msh_reset_spread_counts(ctx), "msh_reset_spread_counts")
            ok(lib, ctx, lib.msh_timing_begin(ctx, 1), "msh_timing_begin")
            if spread:
                rc = lib.msh_schedule_sequential_spread_device(ctx, P, p(d_pd), p(d_pt), p(d_grp), NRES, p(d_rq), 0, p(oi),
                                                               p(osc), p(ost), stream)
            else:
                rc = lib.msh_schedule_sequential_fit_device(ctx, P, p(d_pd), p(d_pt), NRES, p(d_rq), 0, p(oi), p(osc),
                                                            p(ost), stream)
            ok(lib, ctx, rc, case)
            cnt, tot, mx = C.c_int32(), C.c_double(), C.c_double()
            ok(lib, ctx, lib.msh_timing_end(ctx, C.byref(cnt), C.byref(tot), C.byref(mx)), "msh_timing_end")
            assert cnt.value == 1
            if k >= WARMUP:
                us.append(tot.value * 1e3)
        torch.cuda.synchronize()
        counts = np.zeros(N, np.int32)
        ok(lib, ctx, lib.msh_node_pod_counts(ctx, vp(counts)), "msh_node_pod_counts")
        h = hashlib.sha256()
        for a in (oi.cpu().numpy(), osc.cpu().numpy(), ost.cpu().numpy(), counts):
            h.update(a.tobytes())
        st = ost.cpu().numpy()
        out[case] = {"us": us, "outputs_sha256": h.hexdigest(), "placed": int((st == 0).sum()),
                     "fit_errors": int((st == 1).sum()), "distinct_nodes": int((counts > 0).sum())}
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
    mean = statistics.fmean(us)
    return {"launches": len(us), "ms_mean": round(mean / 1e3, 4), "ms_median": round(statistics.median(us) / 1e3, 4),
            "ms_min": round(min(us) / 1e3, 4), "ms_max": round(max(us) / 1e3, 4), "us_per_pod_mean": round(mean / P, 5),
            "ms_all": [round(x / 1e3, 4) for x in us]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libminisched_hip.so built from the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spread_c5.json"))
    ap.add_argument("--worker", nargs="+", metavar=("LIB", "CASE"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1:])
    build = importlib.import_module("mini-kube-scheduler_amd.build")
    new_lib = str(build.LIB)
    if not args.parent_lib or not Path(args.parent_lib).exists() or not Path(new_lib).exists():
        ap.error("--parent-lib and this tree's built library are both needed")
    us = {"parent_fit": [], **{c: [] for c in CASES}}
    info = {}
    for _ in range(ROUNDS):  # parent and new alternate, one process each
        r = run_worker(["--worker", args.parent_lib, "fit"])
        us["parent_fit"] += r["fit"]["us"]
        info["parent_fit"] = r["fit"]
        r = run_worker(["--worker", new_lib, *CASES])
        for c in CASES:
            us[c] += r[c]["us"]
            info[c] = r[c]
    d = {k: dist(v) for k, v in us.items()}
    lo, hi = d["parent_fit"]["ms_min"], d["parent_fit"]["ms_max"]
    a = d["fit"]["ms_mean"]
    ratio = lambda c: {"mean": round(d[c]["ms_mean"] / a, 3), "min": round(d[c]["ms_min"] / a, 3),  # noqa: E731
                       "max": round(d[c]["ms_max"] / a, 3)}
    rec = {"workload": f"C5: {N} nodes x {P} pods, one sequential launch, default plugins, two resources, mixed "
                       f"requests, {ZONES} zones drawn uniformly per node",
           "timer": "msh_timing_begin/end (kernel start to end); pod counts, spread counts and the table reset before every launch",
           "warmup": WARMUP, "launches_per_round": LAUNCHES, "rounds": ROUNDS,
           "form": "a second LDS barrier after the commit of a placed grouped pod (the two-copy scheme was not tried)",
           "a_fit_parent": d["parent_fit"], "a_fit_new": d["fit"],
           "a_new_mean_within_parent_min_max": bool(lo <= a <= hi),
           "check_a_outputs_equal_parent": info["fit"]["outputs_sha256"] == info["parent_fit"]["outputs_sha256"],
           "b_spread_all_ungrouped": d["ungrouped"], "b_over_a": ratio("ungrouped"),
           "check_b_outputs_equal_a": info["ungrouped"]["outputs_sha256"] == info["fit"]["outputs_sha256"],
           "c_16_groups_8_zones_skew_1": d["groups16"], "c_over_a": ratio("groups16"),
           "d_one_group_8_zones_skew_1": d["group1"], "d_over_a": ratio("group1"),
           "placed": {c: info[c]["placed"] for c in CASES}, "fit_errors": {c: info[c]["fit_errors"] for c in CASES},
           "distinct_nodes": {c: info[c]["distinct_nodes"] for c in CASES},
           "sources_sha256": build.sources_digest()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps({k: ({x: y for x, y in v.items() if x != "ms_all"} if isinstance(v, dict) else v) for k, v in rec.items()},
                     indent=1))
    good = rec["check_a_outputs_equal_parent"] and rec["a_new_mean_within_parent_min_max"] and rec["check_b_outputs_equal_a"]
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
