#!/usr/bin/env python3
"""Topology spread together with a resource score on C5 (not part of bench.py): bench.py's synthetic snapshot cut to
the scored limit, 4,096 nodes x 100,000 pods, two resources, mixed requests, 8 zones, one sequential launch, LEAST
and MOST. Written into profiles/spread_score_c5.json:

(a) the scored msh_schedule_sequential_fit_device call (LEAST, MOST) and the ungrouped
    msh_schedule_sequential_spread_device call (mode NONE) on a library built from the parent commit (--parent-lib)
    and on this tree's, in alternating rounds of one process each. The outputs must be equal and each new mean has
    to lie within the parent's own min..max of the session: the existing kernels did not move.
(b) msh_schedule_sequential_spread_scored_device with every pod ungrouped against the scored _fit call of the same
    mode: outputs equal, the ratio is the cost of the spread additions when nothing uses them.
(c) 16 groups x 8 zones at max_skew = 1, pods dealt to the groups in turn; (d) one group holding every pod.
    Per case and mode: ms per launch, us per pod, pods placed, FIT_ERRORs, the ratio to (a)'s scored _fit call.

Every launch is timed with msh_timing_begin / _end (the kernel's own start and end) after a reset of the pod and
spread counts and a fresh upload of the table, so all launches of a case do the same work; WARMUP warm-up launches,
then LAUNCHES per round. Each worker process runs under its own time limit, and nothing more is started once one
fails. The workers bind the library with plain ctypes, so one script drives both builds.

    python scripts/measure_spread_score.py --parent-lib /path/to/parent/libminisched_hip.so
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

N, P, NRES, ZONES = 4_096, 100_000, 2, 8
WARMUP, LAUNCHES, ROUNDS, WORKER_LIMIT_S = 2, 6, 2, 500
MIB = 1 << 20
MODES = {"least": 1, "most": 2}
PARENT_CASES = ("fit_least", "fit_most", "spread_ungrouped")  # the calls both builds have
NEW_CASES = PARENT_CASES + tuple(f"{c}_{m}" for m in MODES for c in ("ungrouped", "groups16", "group1"))


def tables():
    rng = np.random.default_rng(5)
    alloc = np.stack([np.full(N, 16_000, np.int64), np.full(N, 64 * 1024 * MIB, np.int64)])
    req = np.stack([rng.integers(1, 21, P) * 100, rng.integers(1, 33, P) * 128 * MIB]).astype(np.int64)
    zone = rng.integers(0, ZONES, N).astype(np.int32)
    return alloc, req, zone


def groups(kind: str):
    """(max_skew per group, group per pod)"""
    if kind == "groups16":
        return np.ones(16, np.int32), (np.arange(P) % 16).astype(np.int32)
    if kind == "group1":
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
    ones = np.ones(NRES, np.int32)
    out = {}
    for case in cases:
        kind, _, mode = case.rpartition("_")
        if case == "spread_ungrouped":
            kind, mode = "spread", "none"
        ok(lib, ctx, lib.msh_set_resource_score(ctx, MODES.get(mode, 0), C.c_int64(1), NRES, vp(ones)), "msh_set_resource_score")
        spread = kind != "fit"
        if spread:
            skew, grp = groups(kind)
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
            if kind == "fit":
                rc = lib.msh_schedule_sequential_fit_device(ctx, P, p(d_pd), p(d_pt), NRES, p(d_rq), 0, p(oi), p(osc),
                                                            p(ost), stream)
            else:
                fn = lib.msh_schedule_sequential_spread_device if kind == "spread" else \
                    lib.msh_schedule_sequential_spread_scored_device
                rc = fn(ctx, P, p(d_pd), p(d_pt), p(d_grp), NRES, p(d_rq), 0, p(oi), p(osc), p(ost), stream)
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "spread_score_c5.json"))
    ap.add_argument("--worker", nargs="+", metavar=("LIB", "CASE"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1:])
    build = importlib.import_module("mini-kube-scheduler_amd.build")
    new_lib = str(build.LIB)
    if not args.parent_lib or not Path(args.parent_lib).exists() or not Path(new_lib).exists():
        ap.error("--parent-lib and this tree's built library are both needed")
    us = {**{"parent_" + c: [] for c in PARENT_CASES}, **{c: [] for c in NEW_CASES}}
    info = {}
    for _ in range(ROUNDS):  # parent and new alternate, one process each
        r = run_worker(["--worker", args.parent_lib, *PARENT_CASES])
        for c in PARENT_CASES:
            us["parent_" + c] += r[c]["us"]
            info["parent_" + c] = r[c]
        r = run_worker(["--worker", new_lib, *NEW_CASES])
        for c in NEW_CASES:
            us[c] += r[c]["us"]
            info[c] = r[c]
    d = {k: dist(v) for k, v in us.items()}
    same = lambda x, y: info[x]["outputs_sha256"] == info[y]["outputs_sha256"]  # noqa: E731
    a = {}
    for c in PARENT_CASES:
        lo, hi = d["parent_" + c]["ms_min"], d["parent_" + c]["ms_max"]
        a[c] = {"parent": d["parent_" + c], "new": d[c], "new_mean_within_parent_min_max": bool(lo <= d[c]["ms_mean"] <= hi),
                "outputs_equal_parent": same(c, "parent_" + c)}
    new = {}
    for m in MODES:
        base = d["fit_" + m]["ms_mean"]
        for kind in ("ungrouped", "groups16", "group1"):
            c = f"{kind}_{m}"
            new[c] = {**d[c], "over_scored_fit": {"mean": round(d[c]["ms_mean"] / base, 3), "min": round(d[c]["ms_min"] / base, 3),
                                                  "max": round(d[c]["ms_max"] / base, 3)},
                      "placed": info[c]["placed"], "fit_errors": info[c]["fit_errors"], "distinct_nodes": info[c]["distinct_nodes"]}
        new[f"ungrouped_{m}"]["outputs_equal_scored_fit"] = same(f"ungrouped_{m}", "fit_" + m)
    rec = {"workload": f"C5 cut to the scored limit: {N} nodes x {P} pods, one sequential launch, default plugins, two "
                       f"resources at weight 1, mixed requests, {ZONES} zones drawn uniformly per node, plugin weight 1",
           "timer": "msh_timing_begin/end (kernel start to end); pod counts, spread counts and the table reset before every launch",
           "warmup": WARMUP, "launches_per_round": LAUNCHES, "rounds": ROUNDS,
           "form": "a second LDS barrier after the commit of a placed grouped pod (the two-copy scheme was not tried)",
           "a_existing_kernels": a,
           "b_ungrouped_c_16_groups_d_one_group": new,
           "scored_fit": {m: {"placed": info["fit_" + m]["placed"], "fit_errors": info["fit_" + m]["fit_errors"],
                              "distinct_nodes": info["fit_" + m]["distinct_nodes"]} for m in MODES},
           "sources_sha256": build.sources_digest()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")

    def brief(v):
        return {x: brief(y) for x, y in v.items() if x != "ms_all"} if isinstance(v, dict) else v
    print(json.dumps(brief(rec), indent=1))
    good = all(v["new_mean_within_parent_min_max"] and v["outputs_equal_parent"] for v in a.values()) and \
        all(new[f"ungrouped_{m}"]["outputs_equal_scored_fit"] for m in MODES)
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
