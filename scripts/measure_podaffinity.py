#!/usr/bin/env python3
"""Required inter-pod affinity and anti-affinity on C5 (not part of bench.py): scripts/measure_balanced.py's workload,
4,096 nodes x 100,000 pods, two resources under LEAST, 8 zones, 4 spread groups (two of them SCHEDULE_ANYWAY), 4 pod
classes with preference values, w_balanced = 1, one sequential launch. Written into profiles/podaffinity_c5.json:

(a) msh_schedule_sequential_soft_device and msh_schedule_sequential_balanced_device on a library built from the parent
    commit (--parent-lib) and on this tree's, in alternating rounds of one process each. The outputs must be equal and
    each new mean has to lie within the parent's own min..max of the session: the existing kernels did not move.
(b) msh_schedule_sequential_podaffinity_device, every case against the _balanced call of the same session and inputs:
      none   every pod of profile -1 (the new kernel, no pod reads the state)
      host   8 hostname anti-affinity "apps": one replica per node (a fifth of the pods, the rest -1)
      zone   8 zone self-affinity series: the first pod of a series opens a zone for the rest
      mix    the 16 profiles of both over 16 terms
    ms per launch, us per pod, pods placed, FIT_ERRORs and the ratio to _balanced. Every case's outputs and read-back
    state are checked against tests/podaffinity_ref.per_pod on the first 1,500 pods; `none` must give _balanced's
    outputs. No ratio is asserted: nothing about these times was known when the script was written.

Every launch is timed with msh_timing_begin / _end (the kernel's own start and end) after a reset of the pod and spread
counts, a fresh upload of the table and a zeroed state, so all launches of a case do the same work; WARMUP warm-up
launches, then LAUNCHES per round, ROUNDS rounds: 12 launches per figure. Each worker process runs under its own time
limit, and nothing more is started once one fails. The workers bind the library with plain ctypes, so one script drives
both builds.

    python scripts/measure_podaffinity.py --parent-lib /path/to/parent/libminisched_hip.so
    python scripts/measure_podaffinity.py --check-cpu     # the cases and their reference prefixes alone, no GPU
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import importlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "scripts")]

import measure_balanced as MB  # noqa: E402  (the workload, the binding helpers and the statistics)

N, P, NRES, GROUPS, CLASSES, ZONES = MB.N, MB.P, MB.NRES, MB.GROUPS, MB.CLASSES, MB.ZONES
WARMUP, LAUNCHES, ROUNDS, WORKER_LIMIT_S = 2, 6, 2, 700
CHECK_PODS = 1_500
APPS = 8
PROFILED = 0.2  # the share of the pods that has a profile
PARENT_CASES = ("soft_least", "balanced1_least")
PA_CASES = ("pa_none", "pa_host", "pa_zone", "pa_mix")
NEW_CASES = PARENT_CASES + PA_CASES
HOSTNAME, ZONE = 0, 1


def affinity_case(kind: str):
    """(topo, match, anti, aff, pod_profile) of a pod-affinity case."""
    rng = np.random.default_rng(50 + PA_CASES.index("pa_" + kind))
    host = ([HOSTNAME] * APPS, [1 << a for a in range(APPS)], [1 << a for a in range(APPS)], [-1] * APPS)
    zone = ([ZONE] * APPS, [1 << s for s in range(APPS)], [0] * APPS, list(range(APPS)))
    if kind in ("none", "host"):
        topo, match, anti, aff = host
    elif kind == "zone":
        topo, match, anti, aff = zone
    else:  # terms 0..7 on the hostname, 8..15 on the zone
        topo = host[0] + zone[0]
        match = host[1] + [m << APPS for m in zone[1]]
        anti = host[2] + zone[2]
        aff = host[3] + [a + APPS for a in zone[3]]
    prof = rng.integers(0, len(match), P).astype(np.int32)
    prof[rng.random(P) >= PROFILED] = -1
    if kind == "none":
        prof[:] = -1
    return topo, match, anti, aff, prof


def reference_prefix(u, nd, pd, pt, alloc, req, zone, grp, cls, A, T, kind):
    import podaffinity_ref as PA
    O = importlib.import_module("oracle.oracle")
    h = CHECK_PODS
    topo, match, anti, aff, prof = affinity_case(kind)
    st = PA.State(N, topo, match, anti, aff)
    out = PA.per_pod(O, u, nd, pd[:h], pt[:h], O.PluginSet(), np.full(N, 2**31 - 1, np.int64), alloc, np.zeros_like(alloc),
                     req[:, :h], zone, grp[:h], MB.SKEW, MB.MODES["least"], 1, [1] * NRES, None, CLASSES, cls[:h], A, T,
                     MB.W_AFF, MB.W_TAINT, MB.SOFT, MB.W_SPREAD, 1, st, prof[:h])
    return out, st


def inputs():
    synth = importlib.import_module("mini-kube-scheduler_amd.synthetic")
    u, nd, pd, pt = synth.make_soa(N, P)
    return (u, nd, pd, pt, *MB.tables())


def check_cpu() -> int:
    """The cases as the GPU run would see them, through the reference alone: what each prefix places and why not."""
    u, nd, pd, pt, alloc, req, zone, grp, cls, A, T = inputs()
    for case in PA_CASES:
        kind = case[3:]
        (idx, _, status, *_), st = reference_prefix(u, nd, pd, pt, alloc, req, zone, grp, cls, A, T, kind)
        prof = affinity_case(kind)[4][:CHECK_PODS]
        print(json.dumps({"case": case, "prefix_pods": CHECK_PODS, "profiled": int((prof >= 0).sum()),
                          "placed": int((status == 0).sum()), "profiled_placed": int((status[prof >= 0] == 0).sum()),
                          "nodes_present": int((st.present != 0).sum()), "nodes_repel": int((st.repel != 0).sum()),
                          "counters": st.stats}))
    return 0


def worker(lib_path: str, cases: list[str]) -> int:
    import torch
    ok, vp = MB.ok, MB.vp
    lib = MB.bind(lib_path)
    ctx = C.c_void_p()
    ok(lib, None, lib.msh_create(0, C.byref(ctx)), "msh_create")
    dev = torch.device("cuda:0")
    oi = torch.empty(P, dtype=torch.int32, device=dev)
    osc = torch.empty(P, dtype=torch.int64, device=dev)
    ost = torch.empty(P, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ones = np.ones(NRES, np.int32)
    u, nd, pd, pt, alloc, req, zone, grp, cls, A, T = inputs()
    d_pd, d_pt = torch.from_numpy(pd).to(dev), torch.from_numpy(pt).to(dev)
    d_rq, d_grp, d_cls = torch.from_numpy(req).to(dev), torch.from_numpy(grp).to(dev), torch.from_numpy(cls).to(dev)
    out = {}
    for case in cases:
        affine = case.startswith("pa_")
        ok(lib, ctx, lib.msh_upload_nodes(ctx, N, vp(u), vp(nd)), "msh_upload_nodes")
        ok(lib, ctx, lib.msh_set_resource_score(ctx, MB.MODES["least"], C.c_int64(1), NRES, vp(ones)), "msh_set_resource_score")
        ok(lib, ctx, lib.msh_set_spread_groups(ctx, GROUPS, vp(MB.SKEW)), "msh_set_spread_groups")
        ok(lib, ctx, lib.msh_upload_node_zones(ctx, N, vp(zone)), "msh_upload_node_zones")
        ok(lib, ctx, lib.msh_upload_node_class_prefs(ctx, N, CLASSES, vp(A), vp(T)), "msh_upload_node_class_prefs")
        ok(lib, ctx, lib.msh_set_preference_weights(ctx, MB.W_AFF, MB.W_TAINT), "msh_set_preference_weights")
        ok(lib, ctx, lib.msh_set_spread_group_modes(ctx, GROUPS, vp(MB.SOFT)), "msh_set_spread_group_modes")
        ok(lib, ctx, lib.msh_set_spread_score_weight(ctx, MB.W_SPREAD), "msh_set_spread_score_weight")
        ok(lib, ctx, lib.msh_set_balanced_score(ctx, 1), "msh_set_balanced_score")
        d_prof = None
        if affine:
            topo, match, anti, aff, prof = affinity_case(case[3:])
            t8, m32 = np.asarray(topo, np.uint8), np.asarray(match, np.uint32)
            a32, f32 = np.asarray(anti, np.uint32), np.asarray(aff, np.int32)
            ok(lib, ctx, lib.msh_set_pod_affinity_terms(ctx, len(t8), vp(t8)), "msh_set_pod_affinity_terms")
            ok(lib, ctx, lib.msh_set_pod_profiles(ctx, len(m32), vp(m32), vp(a32), vp(f32)), "msh_set_pod_profiles")
            d_prof = torch.from_numpy(prof).to(dev)
        name = {"soft_least": "msh_schedule_sequential_soft_device",
                "balanced1_least": "msh_schedule_sequential_balanced_device"}.get(case, "msh_schedule_sequential_podaffinity_device")
        fn = getattr(lib, name)
        us = []
        for k in range(WARMUP + LAUNCHES):
            ok(lib, ctx, lib.msh_reset_node_pod_counts(ctx), "msh_reset_node_pod_counts")
            ok(lib, ctx, lib.msh_upload_node_resources(ctx, N, NRES, vp(alloc), None), "msh_upload_node_resources")
            ok(lib, ctx, lib.msh_reset_spread_counts(ctx), "msh_reset_spread_counts")
            if affine:
                ok(lib, ctx, lib.msh_upload_pod_affinity_state(ctx, N, None, None), "msh_upload_pod_affinity_state")
            ok(lib, ctx, lib.msh_timing_begin(ctx, 1), "msh_timing_begin")
            if affine:
                rc = fn(ctx, P, p(d_pd), p(d_pt), p(d_grp), p(d_cls), p(d_prof), NRES, p(d_rq), 0, p(oi), p(osc), p(ost), stream)
            else:
                rc = fn(ctx, P, p(d_pd), p(d_pt), p(d_grp), p(d_cls), NRES, p(d_rq), 0, p(oi), p(osc), p(ost), stream)
            ok(lib, ctx, rc, case)
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
        if affine:
            want, ref_state = reference_prefix(u, nd, pd, pt, alloc, req, zone, grp, cls, A, T, case[3:])
            out[case]["prefix_equals_reference"] = bool(all(np.array_equal(g[:CHECK_PODS], w) for g, w in zip(got, want[:3])))
            out[case]["prefix_pods"] = CHECK_PODS
            prof = affinity_case(case[3:])[4]
            out[case]["profiled_pods"] = int((prof >= 0).sum())
            out[case]["profiled_placed"] = int((st[prof >= 0] == 0).sum())
            # the state after the prefix alone, from a launch of its own on a zeroed state and table
            ok(lib, ctx, lib.msh_reset_node_pod_counts(ctx), "msh_reset_node_pod_counts")
            ok(lib, ctx, lib.msh_upload_node_resources(ctx, N, NRES, vp(alloc), None), "msh_upload_node_resources")
            ok(lib, ctx, lib.msh_reset_spread_counts(ctx), "msh_reset_spread_counts")
            ok(lib, ctx, lib.msh_upload_pod_affinity_state(ctx, N, None, None), "msh_upload_pod_affinity_state")
            hq = CHECK_PODS
            d_rq_h = torch.from_numpy(np.ascontiguousarray(req[:, :hq])).to(dev)
            ok(lib, ctx, fn(ctx, hq, p(d_pd), p(d_pt), p(d_grp), p(d_cls), p(d_prof), NRES, p(d_rq_h), 0, p(oi), p(osc), p(ost),
                            stream), case + " (prefix)")
            torch.cuda.synchronize()
            pr, rp = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
            ok(lib, ctx, lib.msh_pod_affinity_state(ctx, vp(pr), vp(rp)), "msh_pod_affinity_state")
            out[case]["prefix_state_equals_reference"] = bool(np.array_equal(pr, ref_state.present) and
                                                              np.array_equal(rp, ref_state.repel))
    lib.msh_destroy(ctx)
    print("RESULT " + json.dumps(out))
    return 0


def run_worker(args: list[str]) -> dict:
    r = subprocess.run([sys.executable, __file__, *args], capture_output=True, text=True, timeout=WORKER_LIMIT_S)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"worker {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(lines[-1][7:])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libminisched_hip.so built from the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "podaffinity_c5.json"))
    ap.add_argument("--check-cpu", action="store_true", help="generate the cases and run their reference prefixes; no GPU")
    ap.add_argument("--worker", nargs="+", metavar=("LIB", "CASE"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1:])
    if args.check_cpu:
        return check_cpu()
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
    d = {k: MB.dist(v) for k, v in us.items()}
    same = lambda x, y: info[x]["outputs_sha256"] == info[y]["outputs_sha256"]  # noqa: E731
    a = {}
    for c in PARENT_CASES:
        lo, hi = d["parent_" + c]["ms_min"], d["parent_" + c]["ms_max"]
        a[c] = {"parent": d["parent_" + c], "new": d[c], "new_mean_within_parent_min_max": bool(lo <= d[c]["ms_mean"] <= hi),
                "outputs_equal_parent": same(c, "parent_" + c), "placed": info[c]["placed"], "fit_errors": info[c]["fit_errors"]}
    base = d["balanced1_least"]["ms_mean"]
    new = {}
    for c in PA_CASES:
        new[c] = {**d[c], "baseline": "balanced1_least", "baseline_ms_mean": base,
                  "over_balanced": {"mean": round(d[c]["ms_mean"] / base, 3), "min": round(d[c]["ms_min"] / base, 3),
                                    "max": round(d[c]["ms_max"] / base, 3)},
                  **{k: info[c][k] for k in ("placed", "fit_errors", "distinct_nodes", "profiled_pods", "profiled_placed",
                                             "prefix_equals_reference", "prefix_state_equals_reference", "prefix_pods")}}
    new["pa_none"]["outputs_equal_balanced"] = same("pa_none", "balanced1_least")
    rec = {"workload": f"scripts/measure_balanced.py's: {N} nodes x {P} pods, one sequential launch, two resources under "
                       f"LEAST, {ZONES} zones, {GROUPS} spread groups (groups 0 and 2 SCHEDULE_ANYWAY), {CLASSES} pod classes "
                       f"with preference values, every weight 1, w_balanced 1; a fifth of the pods has a profile: {APPS} "
                       f"hostname anti-affinity apps, {APPS} zone self-affinity series, or both",
           "timer": "msh_timing_begin/end (kernel start to end); pod counts, spread counts, the table and the affinity state "
                    "reset before every launch",
           "warmup": WARMUP, "launches_per_round": LAUNCHES, "rounds": ROUNDS,
           "a_existing_kernels": a, "b_podaffinity": new, "sources_sha256": build.sources_digest()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")

    def brief(v):
        return {x: brief(y) for x, y in v.items() if x != "ms_all"} if isinstance(v, dict) else v
    print(json.dumps(brief(rec), indent=1))
    good = all(v["new_mean_within_parent_min_max"] and v["outputs_equal_parent"] for v in a.values()) and \
        all(v["prefix_equals_reference"] and v["prefix_state_equals_reference"] for v in new.values()) and \
        new["pa_none"]["outputs_equal_balanced"]
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
