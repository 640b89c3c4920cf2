#!/usr/bin/env python3
"""MSH_TIEBREAK_RANDOM against MSH_TIEBREAK_FIRST on the headline launch (not part of bench.py).

One ctx, C3's node table (5,000 nodes), the headline plugin list (NodeNumber w=3, DefaultNormalizeScore),
32 batches of 100,000 pods per msh_schedule_batches_device launch, device buffers. After 5 warm-up launches
per mode, 30 launches per mode are timed with msh_timing_begin / _end (the kernel's own start and end),
FIRST and RANDOM interleaved in blocks of 10 in the same process; the medians, their ratio and the distinct
nodes used per batch go to profiles/tiebreak_c3.json. Both modes' last outputs are checked: FIRST against
the closed form, RANDOM against tests/tiebreak_ref.pick on a 2,000-pod sample per batch.

    python scripts/measure_tiebreak.py [--out profiles/tiebreak_c3.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

N_NODES, P, WEIGHT, NORM, SEED = 5_000, 100_000, 3, 1, 0x6D696E69
WARMUP, LAUNCHES, BLOCK, SAMPLE = 5, 30, 10, 2_000


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tiebreak_c3.json"))
    args = ap.parse_args()
    import torch
    from closed_form import closed_form_modes
    import tiebreak_ref as ref
    msh = importlib.import_module("mini-kube-scheduler_amd")
    synth = importlib.import_module("mini-kube-scheduler_amd.synthetic")
    build = importlib.import_module("mini-kube-scheduler_amd.build")
    build.build()
    dev = torch.device("cuda:0")
    G = msh._native.BATCHES_PER_LAUNCH
    ctx = msh.DeviceContext(0)
    ctx.set_plugins([msh.NODE_UNSCHEDULABLE], [msh.NODE_NUMBER],
                    [msh.ScorePluginConfig(msh.NODE_NUMBER, WEIGHT, msh.Normalize(NORM))])
    plugins = type("P", (), dict(filters=["NodeUnschedulable"], prescore=["NodeNumber"], score=["NodeNumber"],
                                 weights=[WEIGHT], normalize=[NORM]))
    u, nd = synth.make_nodes(N_NODES)[1:]
    ctx.upload_nodes(u, nd)
    pd_all, pt_all = synth._make_pods_fast(P * G, synth.SEED)[1:]
    pods = [(np.ascontiguousarray(pd_all[i * P:(i + 1) * P]), np.ascontiguousarray(pt_all[i * P:(i + 1) * P]))
            for i in range(G)]
    bufs = [{"pd": torch.from_numpy(a).to(dev), "pt": torch.from_numpy(b).to(dev),
             "idx": torch.empty(P, dtype=torch.int32, device=dev), "score": torch.empty(P, dtype=torch.int64, device=dev),
             "status": torch.empty(P, dtype=torch.int32, device=dev)} for a, b in pods]
    descs = ctx.batch_descs([(P, b["pd"].data_ptr(), b["pt"].data_ptr(), b["idx"].data_ptr(), b["score"].data_ptr(),
                              b["status"].data_ptr()) for b in bufs])
    sh = torch.cuda.current_stream(dev).cuda_stream

    def launches(mode: str, k: int, timed: bool) -> list[float]:
        """k launches in `mode`, each timed on its own (RANDOM: every launch from counter 0)."""
        out = []
        for _ in range(k):
            ctx.set_tiebreak(mode, SEED, 0)
            if timed:
                ctx.timing_begin(1)
            ctx.schedule_batches_device(descs, stream=sh)
            if timed:
                n, total_ms, _ = ctx.timing_end()
                assert n == 1
                out.append(total_ms * 1e3)
        torch.cuda.synchronize()
        return out

    def outputs():
        return [(b["idx"].cpu().numpy(), b["score"].cpu().numpy(), b["status"].cpu().numpy()) for b in bufs]

    times = {"first": [], "random": []}
    for mode in times:
        launches(mode, WARMUP, False)
    last = {}
    for _ in range(LAUNCHES // BLOCK):
        for mode in times:
            times[mode] += launches(mode, BLOCK, True)
            last[mode] = outputs()
    # checks: FIRST against the closed form; RANDOM against the reference on a sample of each batch
    ok_first = all(all(np.array_equal(g, w) for g, w in zip(got, closed_form_modes(u, nd, pd, pt, WEIGHT, NORM)))
                   for got, (pd, pt) in zip(last["first"], pods))
    rng = np.random.default_rng(SEED)
    ok_random = True
    for i, (got, (pd, pt)) in enumerate(zip(last["random"], pods)):
        want = ref.pick(u, nd, pd, pt, plugins, SEED, i * P)  # batch i starts where batch i - 1 ended
        js = rng.choice(P, SAMPLE, replace=False)
        ok_random = ok_random and all(np.array_equal(g[js], w[js]) for g, w in zip(got, want))

    def distinct(outs):
        return [int(len(np.unique(i[st == 0]))) for i, _, st in outs]

    med = {m: statistics.median(t) for m, t in times.items()}
    prov = build.load_provenance() or {}
    rec = {"workload": f"{N_NODES} nodes x {P} pods x {G} batches per launch, NodeNumber w={WEIGHT} normalize=DEFAULT",
           "launches_per_mode": LAUNCHES, "interleave_block": BLOCK, "timer": "msh_timing_begin/end (kernel start to end)",
           "first_us_median": round(med["first"], 2), "random_us_median": round(med["random"], 2),
           "ratio_random_over_first": round(med["random"] / med["first"], 3),
           "first_us_min_max": [round(min(times["first"]), 2), round(max(times["first"]), 2)],
           "random_us_min_max": [round(min(times["random"]), 2), round(max(times["random"]), 2)],
           "distinct_nodes_per_batch_first": distinct(last["first"]),
           "distinct_nodes_per_batch_random": distinct(last["random"]),
           "check_first_vs_closed_form": bool(ok_first), "check_random_vs_reference_sample": bool(ok_random),
           "sources_sha256": prov.get("sources_sha256") or build.sources_digest()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    ctx.close()
    return 0 if ok_first and ok_random else 1


if __name__ == "__main__":
    sys.exit(main())
