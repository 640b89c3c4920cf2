#!/usr/bin/env python3
"""Per-class node masks on C5 (not part of bench.py): bench.py's synthetic snapshot, 5,000 nodes x 100,000 pods
unscored and cut to the scored limit of 4,096 nodes for LEAST / MOST, two resources, mixed requests, 8 zones, one
sequential launch. Written into profiles/classes_c5.json:

(a) the existing calls both builds have (the unscored and scored msh_schedule_sequential_fit_device, the ungrouped
    msh_schedule_sequential_spread_device and msh_schedule_sequential_spread_scored_device LEAST / MOST) on a
    library built from the parent commit (--parent-lib) and on this tree's, in alternating rounds of one process
    each. The outputs must be equal and each new mean has to lie within the parent's own min..max of the session:
    the existing kernels did not move.
(b) msh_schedule_sequential_classes_device with pod_class all -1 (a column on the ctx, so the class kernel runs),
    (c) 16 classes each admitting a seeded random half of the nodes, (d) 64 classes each admitting one zone (class c
    admits zone c % 8). Per case and mode (none, least, most): ms per launch, us per pod, pods placed, FIT_ERRORs,
    and the ratio to _spread (none) / _spread_scored (least, most) on the same inputs in the same session.
    Every output of a class case is checked against tests/classes_ref.per_pod on a prefix of the batch.

Every launch is timed with msh_timing_begin / _end (the kernel's own start and end) after a reset of the pod and
spread counts and a fresh upload of the table, so all launches of a case do the same work; WARMUP warm-up launches,
then LAUNCHES per round. Each worker process runs under its own time limit, and nothing more is started once one
fails. The workers bind the library with plain ctypes, so one script drives both builds.

    python scripts/measure_classes.py --parent-lib /path/to/parent/libminisched_hip.so
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
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

N_UNSCORED, N_SCORED, P, NRES, ZONES = 5_000, 4_096, 100_000, 2, 8
WARMUP, LAUNCHES, ROUNDS, WORKER_LIMIT_S = 2, 6, 2, 500  # measure_spread_score.py's
CHECK_PODS = 1_500  # the prefix compared with classes_ref.per_pod
MIB = 1 << 20
MODES = {"none": 0, "least": 1, "most": 2}
PARENT_CASES = ("fit_none", "fit_least", "fit_most", "spread_none", "spreadscored_least", "spreadscored_most")
CLASS_KINDS = ("noclass", "half16", "zone64")
NEW_CASES = PARENT_CASES + tuple(f"{k}_{m}" for m in MODES for k in CLASS_KINDS)


def n_nodes(mode: str) -> int:
    return N_UNSCORED if mode == "none" else N_SCORED


def tables(n: int):
    rng = np.random.default_rng(5)
    alloc = np.stack([np.full(n, 16_000, np.int64), np.full(n, 64 * 1024 * MIB, np.int64)])
    req = np.stack([rng.integers(1, 21, P) * 100, rng.integers(1, 33, P) * 128 * MIB]).astype(np.int64)
    zone = rng.integers(0, ZONES, n).astype(np.int32)
    return alloc, req, zone


def classes(kind: str, n: int, zone: np.ndarray):
    """(C, bits per node, class per pod)"""
    rng = np.random.default_rng(17)
    bits = np.zeros(n, np.uint64)
    if kind == "half16":
        for c in range(16):
            bits |= (rng.random(n) < 0.5).astype(np.uint64) << np.uint64(c)
        return 16, bits, (np.arange(P) % 16).astype(np.int32)
    if kind == "zone64":
        for c in range(64):
            bits |= (zone == c % ZONES).astype(np.uint64) << np.uint64(c)
        return 64, bits, (np.arange(P) % 64).astype(np.int32)
    return 1, np.ones(n, np.uint64), np.full(P, -1, np.int32)


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


def reference_prefix(u, nd, pd, pt, alloc, req, zone, grp, skew, mode, bits, n_classes, cls):
    import classes_ref as KR
    O = importlib.import_module("oracle.oracle")
    h = CHECK_PODS
    n = len(u)
    return KR.per_pod(O, u, nd, pd[:h], pt[:h], O.PluginSet(), np.full(n, 2**31 - 1, np.int64), alloc,
                      np.zeros_like(alloc), req[:, :h], zone, grp[:h], skew, MODES[mode], 1, [1] * NRES, bits, n_classes,
                      cls[:h])


def worker(lib_path: str, cases: list[str]) -> int:
    import torch
    synth = importlib.import_module("mini-kube-scheduler_amd.synthetic")
    lib = bind(lib_path)
    ctx = C.c_void_p()
    ok(lib, None, lib.msh_create(0, C.byref(ctx)), "msh_create")
    dev = torch.device("cuda:0")
    oi = torch.empty(P, dtype=torch.int32, device=dev)
    osc = torch.empty(P, dtype=torch.int64, device=dev)
    ost = torch.empty(P, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ones = np.ones(NRES, np.int32)
    skew, grp = np.ones(1, np.int32), np.full(P, -1, np.int32)  # every pod ungrouped: the cost of the classes alone
    d_grp = torch.from_numpy(grp).to(dev)
    out = {}
    for case in cases:
        kind, _, mode = case.rpartition("_")
        n = n_nodes(mode)
        u, nd, pd, pt = synth.make_soa(n, P)
        ok(lib, ctx, lib.msh_upload_nodes(ctx, n, vp(u), vp(nd)), "msh_upload_nodes")
        d_pd, d_pt = torch.from_numpy(pd).to(dev), torch.from_numpy(pt).to(dev)
        alloc, req, zone = tables(n)
        d_rq = torch.from_numpy(req).to(dev)
        ok(lib, ctx, lib.msh_set_resource_score(ctx, MODES[mode], C.c_int64(1), NRES, vp(ones)), "msh_set_resource_score")
        if kind != "fit":
            ok(lib, ctx, lib.msh_set_spread_groups(ctx, len(skew), vp(skew)), "msh_set_spread_groups")
            ok(lib, ctx, lib.msh_upload_node_zones(ctx, n, vp(zone)), "msh_upload_node_zones")
        if kind in CLASS_KINDS:
            n_classes, bits, cls = classes(kind, n, zone)
            d_cls = torch.from_numpy(cls).to(dev)
            ok(lib, ctx, lib.msh_upload_node_class_bits(ctx, n, n_classes, vp(bits)), "msh_upload_node_class_bits")
        us = []
        for k in range(WARMUP + LAUNCHES):
            ok(lib, ctx, lib.msh_reset_node_pod_counts(ctx), "msh_reset_node_pod_counts")
            ok(lib, ctx, lib.msh_upload_node_resources(ctx, n, NRES, vp(alloc), None), "msh_upload_node_resources")
            if kind != "fit":
                ok(lib, ctx, lib.msh_reset_spread_counts(ctx), "msh_reset_spread_counts")
            ok(lib, ctx, lib.msh_timing_begin(ctx, 1), "msh_timing_begin")
            tail = (NRES, p(d_rq), 0, p(oi), p(osc), p(ost), stream)
            if kind == "fit":
                rc = lib.msh_schedule_sequential_fit_device(ctx, P, p(d_pd), p(d_pt), *tail)
            elif kind == "spread":
                rc = lib.msh_schedule_sequential_spread_device(ctx, P, p(d_pd), p(d_pt), p(d_grp), *tail)
            elif kind == "spreadscored":
                rc = lib.msh_schedule_sequential_spread_scored_device(ctx, P, p(d_pd), p(d_pt), p(d_grp), *tail)
            else:
                rc = lib.msh_schedule_sequential_classes_device(ctx, P, p(d_pd), p(d_pt), p(d_grp), p(d_cls), *tail)
            ok(lib, ctx, rc, case)
            cnt, tot, mx = C.c_int32(), C.c_double(), C.c_double()
            ok(lib, ctx, lib.msh_timing_end(ctx, C.byref(cnt), C.byref(tot), C.byref(mx)), "msh_timing_end")
            assert cnt.value == 1
            if k >= WARMUP:
                us.append(tot.value * 1e3)
        torch.cuda.synchronize()
        counts = np.zeros(n, np.int32)
        ok(lib, ctx, lib.msh_node_pod_counts(ctx, vp(counts)), "msh_node_pod_counts")
        got = (oi.cpu().numpy(), osc.cpu().numpy(), ost.cpu().numpy())
        h = hashlib.sha256()
        for a in (*got, counts):
            h.update(a.tobytes())
        st = got[2]
        out[case] = {"us": us, "outputs_sha256": h.hexdigest(), "placed": int((st == 0).sum()),
                     "fit_errors": int((st == 1).sum()), "distinct_nodes": int((counts > 0).sum())}
        if kind in CLASS_KINDS:
            want = reference_prefix(u, nd, pd, pt, alloc, req, zone, grp, skew, mode, bits, n_classes, cls)
            out[case]["prefix_equals_reference"] = bool(all(np.array_equal(g[:CHECK_PODS], w) for g, w in zip(got, want[:3])))
            out[case]["prefix_pods"] = CHECK_PODS
            ok(lib, ctx, lib.msh_clear_node_class_bits(ctx), "msh_clear_node_class_bits")
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "classes_c5.json"))
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
        base_case = "spread_none" if m == "none" else "spreadscored_" + m
        base = d[base_case]["ms_mean"]
        for kind in CLASS_KINDS:
            c = f"{kind}_{m}"
            new[c] = {**d[c], "baseline": base_case,
                      "over_baseline": {"mean": round(d[c]["ms_mean"] / base, 3), "min": round(d[c]["ms_min"] / base, 3),
                                        "max": round(d[c]["ms_max"] / base, 3)},
                      "placed": info[c]["placed"], "fit_errors": info[c]["fit_errors"],
                      "distinct_nodes": info[c]["distinct_nodes"],
                      "prefix_equals_reference": info[c]["prefix_equals_reference"], "prefix_pods": info[c]["prefix_pods"]}
        new[f"noclass_{m}"]["outputs_equal_baseline"] = same(f"noclass_{m}", base_case)
    rec = {"workload": f"C5: {N_UNSCORED} nodes x {P} pods unscored, cut to the scored limit of {N_SCORED} nodes for LEAST / "
                       f"MOST; one sequential launch, default plugins, two resources at weight 1, mixed requests, {ZONES} "
                       f"zones drawn uniformly per node, every pod ungrouped, plugin weight 1",
           "timer": "msh_timing_begin/end (kernel start to end); pod counts, spread counts and the table reset before every launch",
           "warmup": WARMUP, "launches_per_round": LAUNCHES, "rounds": ROUNDS,
           "layout": "registers: 2 x NPL VGPRs of class bits per thread, NPL 64-bit shifts per classed pod",
           "a_existing_kernels": a,
           "b_no_class_c_16_half_classes_d_64_zone_classes": new,
           "sources_sha256": build.sources_digest()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")

    def brief(v):
        return {x: brief(y) for x, y in v.items() if x != "ms_all"} if isinstance(v, dict) else v
    print(json.dumps(brief(rec), indent=1))
    good = all(v["new_mean_within_parent_min_max"] and v["outputs_equal_parent"] for v in a.values()) and \
        all(v["prefix_equals_reference"] for v in new.values()) and \
        all(new[f"noclass_{m}"]["outputs_equal_baseline"] for m in MODES)
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
