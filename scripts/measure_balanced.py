#!/usr/bin/env python3
"""NodeResourcesBalancedAllocation on C5 (not part of bench.py): bench.py's synthetic snapshot cut to the balanced
call's node limit, 4,096 nodes x 100,000 pods, two resources, mixed requests, 8 zones, 4 spread groups (two of them
SCHEDULE_ANYWAY), 4 pod classes with preference values, one sequential launch. Written into profiles/balanced_c5.json:

(a) msh_schedule_sequential_prefs_device and msh_schedule_sequential_soft_device (LEAST) on a library built from the
    parent commit (--parent-lib) and on this tree's, in alternating rounds of one process each. The outputs must be
    equal and each new mean has to lie within the parent's own min..max of the session: the existing kernels did not
    move. These are also the C5 figures of _prefs and _soft, which had none.
(b) msh_schedule_sequential_balanced_device with w_balanced = 0 (it must give _soft's outputs), and with
    w_balanced = 1 under LEAST and under NONE: ms per launch, us per pod, pods placed, FIT_ERRORs, and the ratio to
    _soft on the same inputs in the same session (for NONE: to _soft under NONE). Every output of a balanced case is
    checked against tests/balanced_ref.per_pod on a prefix of the batch.

Every launch is timed with msh_timing_begin / _end (the kernel's own start and end) after a reset of the pod and
spread counts and a fresh upload of the table, so all launches of a case do the same work; WARMUP warm-up launches,
then LAUNCHES per round, ROUNDS rounds: 12 launches per figure. Each worker process runs under its own time limit,
and nothing more is started once one fails. The workers bind the library with plain ctypes, so one script drives
both builds.

    python scripts/measure_balanced.py --parent-lib /path/to/parent/libminisched_hip.so
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

N, P, NRES, ZONES, GROUPS, CLASSES = 4_096, 100_000, 2, 8, 4, 4
WARMUP, LAUNCHES, ROUNDS, WORKER_LIMIT_S = 2, 6, 2, 500
CHECK_PODS = 1_500  # the prefix compared with balanced_ref.per_pod
MIB = 1 << 20
MODES = {"none": 0, "least": 1, "most": 2}
SKEW = np.array([1000, 1000, 1000, 1000], np.int32)
SOFT = np.array([1, 0, 1, 0], np.uint8)
W_AFF, W_TAINT, W_SPREAD = 1, 1, 1
PARENT_CASES = ("prefs_least", "soft_least")
NEW_CASES = PARENT_CASES + ("soft_none", "balanced0_least", "balanced1_least", "balanced1_none")


def tables():
    """Uneven nodes (a third cpu-rich, a third memory-rich) and cpu-heavy / memory-heavy pods."""
    rng = np.random.default_rng(5)
    kind = rng.integers(0, 3, N)
    alloc = np.stack([np.where(kind == 0, 48_000, 16_000), np.where(kind == 1, 192, 64) * 1024 * MIB]).astype(np.int64)
    pk = rng.integers(0, 2, P)
    req = np.stack([rng.integers(1, 11, P) * 100 * np.where(pk == 0, 4, 1),
                    rng.integers(1, 17, P) * 128 * MIB * np.where(pk == 1, 4, 1)]).astype(np.int64)
    zone = rng.integers(0, ZONES, N).astype(np.int32)
    grp = rng.integers(-1, GROUPS, P).astype(np.int32)
    cls = rng.integers(-1, CLASSES, P).astype(np.int32)
    A = (rng.integers(0, 4, (CLASSES, N)) * 25).astype(np.uint16)
    T = rng.integers(0, 3, (CLASSES, N)).astype(np.uint16)
    return alloc, req, zone, grp, cls, A, T


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


def reference_prefix(u, nd, pd, pt, alloc, req, zone, grp, cls, A, T, mode, wb):
    import balanced_ref as BR
    O = importlib.import_module("oracle.oracle")
    h = CHECK_PODS
    return BR.per_pod(O, u, nd, pd[:h], pt[:h], O.PluginSet(), np.full(N, 2**31 - 1, np.int64), alloc,
                      np.zeros_like(alloc), req[:, :h], zone, grp[:h], SKEW, MODES[mode], 1, [1] * NRES, None, CLASSES,
                      cls[:h], A, T, W_AFF, W_TAINT, SOFT, W_SPREAD, wb)


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
    u, nd, pd, pt = synth.make_soa(N, P)
    alloc, req, zone, grp, cls, A, T = tables()
    d_pd, d_pt = torch.from_numpy(pd).to(dev), torch.from_numpy(pt).to(dev)
    d_rq, d_grp, d_cls = torch.from_numpy(req).to(dev), torch.from_numpy(grp).to(dev), torch.from_numpy(cls).to(dev)
    out = {}
    for case in cases:
        kind, _, mode = case.rpartition("_")
        ok(lib, ctx, lib.msh_upload_nodes(ctx, N, vp(u), vp(nd)), "msh_upload_nodes")
        ok(lib, ctx, lib.msh_set_resource_score(ctx, MODES[mode], C.c_int64(1), NRES, vp(ones)), "msh_set_resource_score")
        ok(lib, ctx, lib.msh_set_spread_groups(ctx, GROUPS, vp(SKEW)), "msh_set_spread_groups")
        ok(lib, ctx, lib.msh_upload_node_zones(ctx, N, vp(zone)), "msh_upload_node_zones")
        ok(lib, ctx, lib.msh_upload_node_class_prefs(ctx, N, CLASSES, vp(A), vp(T)), "msh_upload_node_class_prefs")
        ok(lib, ctx, lib.msh_set_preference_weights(ctx, W_AFF, W_TAINT), "msh_set_preference_weights")
        soft = kind != "prefs"  # _prefs takes pod groups only on a ctx without a SCHEDULE_ANYWAY group
        ok(lib, ctx, lib.msh_set_spread_group_modes(ctx, GROUPS, vp(SOFT if soft else np.zeros(GROUPS, np.uint8))),
           "msh_set_spread_group_modes")
        ok(lib, ctx, lib.msh_set_spread_score_weight(ctx, W_SPREAD), "msh_set_spread_score_weight")
        wb = int(kind[-1]) if kind.startswith("balanced") else 0
        if kind.startswith("balanced"):
            ok(lib, ctx, lib.msh_set_balanced_score(ctx, wb), "msh_set_balanced_score")
        fn = getattr(lib, {"prefs": "msh_schedule_sequential_prefs_device", "soft": "msh_schedule_sequential_soft_device"}
                     .get(kind, "msh_schedule_sequential_balanced_device"))
        us = []
        for k in range(WARMUP + LAUNCHES):
            ok(lib, ctx, lib.msh_reset_node_pod_counts(ctx), "msh_reset_node_pod_counts")
            ok(lib, ctx, lib.msh_upload_node_resources(ctx, N, NRES, vp(alloc), None), "msh_upload_node_resources")
            ok(lib, ctx, lib.msh_reset_spread_counts(ctx), "msh_reset_spread_counts")
            ok(lib, ctx, lib.msh_timing_begin(ctx, 1), "msh_timing_begin")
            ok(lib, ctx, fn(ctx, P, p(d_pd), p(d_pt), p(d_grp), p(d_cls), NRES, p(d_rq), 0, p(oi), p(osc), p(ost), stream), case)
            cnt, tot, mx = C.c_int32(), C.c_double(), C.c_double()
            ok(lib, ctx, lib.msh_timing_end(ctx, C.byref(cnt), C.byref(tot), C.byref(mx)), "msh_timing_end")
            assert cnt.value == 1
            if k >= WARMUP:
                us.append(tot.value * 1e3)
        torch.cuda.synchronize()
        counts = np.zeros(N, np.int32)
        ok(lib, ctx, lib.msh_node_pod_counts(ctx, vp(counts)), "msh_node_pod_counts")
        got = (oi.cpu().numpy(), osc.cpu().numpy(), ost.cpu().numpy())
        h = hashlib.sha256()
        for a in (*got, counts):
            h.update(a.tobytes())
        st = got[2]
        out[case] = {"us": us, "outputs_sha256": h.hexdigest(), "placed": int((st == 0).sum()),
                     "fit_errors": int((st == 1).sum()), "distinct_nodes": int((counts > 0).sum())}
        if kind.startswith("balanced"):
            want = reference_prefix(u, nd, pd, pt, alloc, req, zone, grp, cls, A, T, mode, wb)
            out[case]["prefix_equals_reference"] = bool(all(np.array_equal(g[:CHECK_PODS], w) for g, w in zip(got, want[:3])))
            out[case]["prefix_pods"] = CHECK_PODS
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "balanced_c5.json"))
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
                "outputs_equal_parent": same(c, "parent_" + c), "placed": info[c]["placed"], "fit_errors": info[c]["fit_errors"]}
    new = {}
    for c in ("balanced0_least", "balanced1_least", "balanced1_none"):
        base_case = "soft_" + c.rpartition("_")[2]
        base = d[base_case]["ms_mean"]
        new[c] = {**d[c], "baseline": base_case, "baseline_ms_mean": base,
                  "over_soft": {"mean": round(d[c]["ms_mean"] / base, 3), "min": round(d[c]["ms_min"] / base, 3),
                                "max": round(d[c]["ms_max"] / base, 3)},
                  "placed": info[c]["placed"], "fit_errors": info[c]["fit_errors"], "distinct_nodes": info[c]["distinct_nodes"],
                  "prefix_equals_reference": info[c]["prefix_equals_reference"], "prefix_pods": info[c]["prefix_pods"]}
    new["balanced0_least"]["outputs_equal_soft"] = same("balanced0_least", "soft_least")
    new["balanced1_least"]["outputs_differ_from_soft"] = not same("balanced1_least", "soft_least")
    rec = {"workload": f"C5 cut to the balanced call's node limit: {N} nodes x {P} pods, one sequential launch, default "
                       f"plugins, two resources at weight 1, nodes of three shapes, cpu-heavy and memory-heavy requests, "
                       f"{ZONES} zones, {GROUPS} spread groups (max_skew 1000; groups 0 and 2 SCHEDULE_ANYWAY), {CLASSES} pod "
                       f"classes with preference values, every weight 1",
           "timer": "msh_timing_begin/end (kernel start to end); pod counts, spread counts and the table reset before every launch",
           "warmup": WARMUP, "launches_per_round": LAUNCHES, "rounds": ROUNDS,
           "a_existing_kernels": a, "soft_none": d["soft_none"],
           "b_balanced": new,
           "sources_sha256": build.sources_digest()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")

    def brief(v):
        return {x: brief(y) for x, y in v.items() if x != "ms_all"} if isinstance(v, dict) else v
    print(json.dumps(brief(rec), indent=1))
    good = all(v["new_mean_within_parent_min_max"] and v["outputs_equal_parent"] for v in a.values()) and \
        all(v["prefix_equals_reference"] for v in new.values()) and new["balanced0_least"]["outputs_equal_soft"]
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
