#!/usr/bin/env python3
"""What sample_weight costs, and what deduplication buys.

Part 1, on bench.py's C2 point set (pypardis_amd.synth, as bench.py builds
it): three trains alternated step by step in one process after a warm-up,
    (a) unweighted,
    (b) weighted, every weight 1 (labels must equal (a)'s),
    (c) weighted, integer weights drawn from 1..3,
with the per-stage HIP-event times of PD_OPT_TIMING (gather, count, total;
the record-weight kernels are timed inside "gather").

Part 2, deduplication: a C4-style synth.gps_skew set snapped to a lattice of
eps/8, its distinct points and multiplicities (torch.unique on the device,
uniques ordered by first occurrence so that cluster numbers line up), a
weighted train on the distinct points against an unweighted train on all
points.  The label of every point must equal the label of its distinct point.

    python tools/weight_bench.py [--steps 20] [--warmup 3] [--points N]
                                 [--dedup-points M] [--json-out FILE]

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def med(v):
    return round(statistics.median(v), 4)


def c2_part(args, torch, DBSCAN, _native, synth, ctx):
    X, cfg = synth.make_config("C2", n=args.points)
    n = len(X)
    eps, ms, P = cfg["eps"], cfg["min_samples"], cfg.get("max_partitions") or 1
    Xd = torch.from_numpy(X).cuda()
    del X
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    w1 = torch.ones(n, dtype=torch.float64, device="cuda")
    w13 = torch.randint(1, 4, (n,), generator=g, device="cuda").to(torch.float64)
    variants = [("unweighted", None), ("unit_weights", w1), ("weights_1_3", w13)]

    def step(w):
        return DBSCAN(eps=eps, min_samples=ms, max_partitions=P).train(Xd, sample_weight=w)

    labels = {}
    for _ in range(args.warmup):
        for name, w in variants:
            labels[name] = step(w).labels_
    if not torch.equal(labels["unweighted"], labels["unit_weights"]):
        raise SystemExit("unit weights changed the labels")
    torch.cuda.synchronize()
    ctx.set_option(_native.PD_OPT_TIMING, 1)
    t = {name: {"gather": [], "count": [], "total": [], "wall": []} for name, _ in variants}
    for _ in range(args.steps):
        for name, w in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = step(w)
            torch.cuda.synchronize()
            t[name]["wall"].append(1e3 * (time.perf_counter() - t0))
            tm = ctx.timings()
            for k in ("gather", "count", "total"):
                t[name][k].append(tm[k])
    ctx.set_option(_native.PD_OPT_TIMING, 0)
    out = {"points": n, "eps": eps, "min_samples": ms, "max_partitions": P, "steps": args.steps,
           "median_ms": {name: {k: med(v) for k, v in s.items()} for name, s in t.items()},
           "n_clusters": {"unweighted": int(labels["unweighted"].max()) + 1,
                          "weights_1_3": int(m.n_clusters_)}}
    a, b, c = (out["median_ms"][k] for k, _ in variants)
    out["ratio_unit_over_unweighted"] = {k: round(b[k] / a[k], 4) for k in ("gather", "count", "total")}
    out["ratio_1_3_over_unweighted"] = {k: round(c[k] / a[k], 4) for k in ("gather", "count", "total")}
    return out


def dedup_part(args, torch, DBSCAN, _native, synth, ctx):
    cfg = synth.CONFIGS["C4"]
    eps, ms, P = cfg["eps"], cfg["min_samples"], cfg["max_partitions"]
    n = args.dedup_points
    h = eps / 8.0
    raw = synth.gps_skew(n, seed=cfg["seed"], device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    q = torch.round(raw.to(torch.float64) / h).to(torch.int64)
    key = ((q[:, 0] + (1 << 30)) << 32) | (q[:, 1] + (1 << 30))
    uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    U = uniq.shape[0]
    # uniques in order of first occurrence: cluster numbers (ranks of the
    # smallest core index) then agree between the two trains
    first = torch.full((U,), n, dtype=torch.int64, device="cuda")
    first.scatter_reduce_(0, inv, torch.arange(n, device="cuda"), reduce="amin")
    order = torch.argsort(first)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(U, device="cuda")
    inv = rank[inv]
    uniq, cnt = uniq[order], cnt[order]
    ux = torch.stack([(uniq >> 32) - (1 << 30), (uniq & 0xFFFFFFFF) - (1 << 30)], 1)
    Xu = (ux.to(torch.float64) * h).to(torch.float32).contiguous()
    torch.cuda.synchronize()
    dedup_ms = 1e3 * (time.perf_counter() - t0)
    if torch.unique(Xu, dim=0).shape[0] != U:
        raise SystemExit("lattice points collide in float32")
    Xall = Xu[inv].contiguous()
    w = cnt.to(torch.float64)
    del raw, q, key, ux

    def run(X, sw):
        return DBSCAN(eps=eps, min_samples=ms, max_partitions=P).train(X, sample_weight=sw)

    for _ in range(args.warmup):
        mu, ma = run(Xu, w), run(Xall, None)
    same = bool(torch.equal(mu.labels_[inv], ma.labels_)) and \
        bool(torch.equal(mu.core_sample_mask_[inv], ma.core_sample_mask_))
    if not same:
        raise SystemExit("dedup: the weighted train on the distinct points disagrees")
    ctx.set_option(_native.PD_OPT_TIMING, 1)
    t = {"all_points": {"total": [], "wall": []}, "distinct_weighted": {"total": [], "wall": []}}
    for _ in range(args.steps):
        for name, X, sw in (("all_points", Xall, None), ("distinct_weighted", Xu, w)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(X, sw)
            torch.cuda.synchronize()
            t[name]["wall"].append(1e3 * (time.perf_counter() - t0))
            t[name]["total"].append(ctx.timings()["total"])
    ctx.set_option(_native.PD_OPT_TIMING, 0)
    out = {"points": n, "distinct": U, "eps": eps, "lattice": h, "min_samples": ms,
           "max_partitions": P, "labels_equal": same, "n_clusters": int(ma.n_clusters_),
           "dedup_ms": round(dedup_ms, 2),
           "median_ms": {k: {s: med(v) for s, v in d.items()} for k, d in t.items()}}
    a, b = out["median_ms"]["all_points"], out["median_ms"]["distinct_weighted"]
    out["speedup"] = {k: round(a[k] / b[k], 3) for k in ("total", "wall")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=None, help="C2 point count (default: full)")
    ap.add_argument("--dedup-points", type=int, default=50_000_000)
    ap.add_argument("--skip-dedup", action="store_true")
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 1:
        raise SystemExit("steps and warmup must be >= 1")

    import torch
    from pypardis_amd import DBSCAN, _native, synth
    ctx = _native.context(torch.cuda.current_device())
    res = {"tool": "weight_bench", "lib": os.path.basename(_native.LIB_PATH),
           "c2": c2_part(args, torch, DBSCAN, _native, synth, ctx)}
    torch.cuda.empty_cache()
    if not args.skip_dedup:
        res["dedup"] = dedup_part(args, torch, DBSCAN, _native, synth, ctx)
    line = json.dumps(res)
    print(line)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
