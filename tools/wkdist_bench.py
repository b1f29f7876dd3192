"""Time sample_weight on the index (pd_index_set_weights, pd_index_kdist_weighted,
pd_index_mreach_forest_weighted), each beside its unweighted twin in the same
process.

Part 1, C2's points (min_samples 10, r_max = eps), on one over_rows index:

  (a) set_weights                 index.set_weights(w)
  (b) kdist, every point          index.kdist(X, k)                 the yardstick
  (c) weighted kdist, unit        index.kdist_weighted(X, k), w = 1
  (d) weighted kdist, 1..3        the same with weights drawn from {1, 2, 3}
  (e) forest                      index.mreach_forest(k)
  (f) weighted forest, unit / 1..3

Part 2, deduplication: a C4-style synth.gps_skew set snapped to a lattice of
eps/8 (tools/weight_bench.py's), the unweighted forest of all points against
the weighted forest of the distinct points with their multiplicities, and the
zero edges of each.

HIP events on the current stream for the queries, wall time for the forests
(they read the host once per round); one warm-up, --reps repetitions, medians.
One JSON line per figure, appended to --out as well when given.

  python tools/wkdist_bench.py [--points N] [--dedup-points N] [--reps 3]
                               [--skip-forest] [--skip-dedup] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pypardis_amd import _native, synth  # noqa: E402

OUT = [None]


def emit(rec):
    s = json.dumps(rec)
    print(s, flush=True)
    if OUT[0]:
        with open(OUT[0], "a") as f:
            f.write(s + "\n")
    return rec


def timed(f, reps, wall=False, warmup=1):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        if wall:
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
    return ms


def line(name, ms, **extra):
    return emit(dict(measure=name, median_ms=round(statistics.median(ms), 4),
                     min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms), **extra))


def c2_part(args):
    X, cfg = synth.make_config("C2", n=args.points)
    n, d = X.shape
    eps, k = cfg["eps"], args.k or cfg["min_samples"]
    Xd = torch.from_numpy(X).cuda()
    del X
    emit(dict(measure="setup", config="C2", n=n, d=d, eps=eps, k=k, dtype=str(Xd.dtype),
              device=torch.cuda.get_device_name()))
    g = torch.Generator(device="cuda").manual_seed(7)
    unit = torch.ones(n, dtype=torch.float64, device="cuda")
    w13 = torch.randint(1, 4, (n,), device="cuda", generator=g).to(torch.float64)
    ix = _native.Index.over_rows(Xd, eps)
    out = {}
    try:
        sw = line("set_weights", timed(lambda: ix.set_weights(w13), args.reps), n=n)
        base = line("kdist_all_points", timed(lambda: out.update(a=ix.kdist(Xd, k)), args.reps),
                    m=n)
        res = dict(set_weights_ms=sw["median_ms"], kdist_ms=base["median_ms"])
        for name, w in (("unit", unit), ("1_3", w13)):
            ix.set_weights(w)
            r = line(f"kdist_weighted_{name}",
                     timed(lambda: out.update(b=ix.kdist_weighted(Xd, k)), args.reps), m=n)
            res[f"kdist_weighted_{name}_ms"] = r["median_ms"]
            res[f"kdist_weighted_{name}_ratio"] = round(r["median_ms"] / base["median_ms"], 4)
            if name == "unit" and not torch.equal(out["a"], out["b"]):
                raise SystemExit("unit weights: the weighted k-distances differ")
            res[f"core_rows_{name}"] = int(torch.isfinite(out["b"]).sum())
        out.clear()
        if not args.skip_forest:
            f0 = line("forest", timed(lambda: out.update(f=ix.mreach_forest(k)), args.reps, True),
                      n=n)
            res.update(forest_ms=f0["median_ms"], forest_edges=int(out["f"][0].shape[0]),
                       forest_rounds=out["f"][4])
            for name, w in (("unit", unit), ("1_3", w13)):
                ix.set_weights(w)
                out.clear()
                r = line(f"forest_weighted_{name}",
                         timed(lambda: out.update(f=ix.mreach_forest(k, weighted=True)), args.reps,
                               True), n=n)
                res[f"forest_weighted_{name}_ms"] = r["median_ms"]
                res[f"forest_weighted_{name}_ratio"] = round(r["median_ms"] / f0["median_ms"], 4)
                res[f"forest_weighted_{name}_edges"] = int(out["f"][0].shape[0])
                res[f"forest_weighted_{name}_rounds"] = out["f"][4]
    finally:
        ix.close()
    emit(dict(measure="wkdist_c2", n=n, k=k, eps=eps, **res))


def dedup_part(args):
    cfg = synth.CONFIGS["C4"]
    eps, k = cfg["eps"], cfg["min_samples"]
    n = args.dedup_points
    h = eps / 8.0
    raw = synth.gps_skew(n, seed=cfg["seed"], device="cuda")
    q = torch.round(raw.to(torch.float64) / h).to(torch.int64)
    key = ((q[:, 0] + (1 << 30)) << 32) | (q[:, 1] + (1 << 30))
    uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    U = uniq.shape[0]
    ux = torch.stack([(uniq >> 32) - (1 << 30), (uniq & 0xFFFFFFFF) - (1 << 30)], 1)
    Xu = (ux.to(torch.float64) * h).to(torch.float32).contiguous()
    Xall = Xu[inv].contiguous()
    w = cnt.to(torch.float64)
    del raw, q, key, ux, uniq
    res = dict(points=n, distinct=U, eps=eps, k=k, max_multiplicity=int(cnt.max()))
    out = {}
    for name, X, sw in (("all_points", Xall, None), ("distinct_weighted", Xu, w)):
        def run():
            ix = _native.Index.over_rows(X, eps)
            try:
                if sw is not None:
                    ix.set_weights(sw)
                out["f"] = ix.mreach_forest(k, weighted=sw is not None)
            finally:
                ix.close()
        r = line(f"dedup_forest_{name}", timed(run, args.reps, True), n=int(X.shape[0]))
        u, v, acc, cd, rounds = out["f"]
        res[f"{name}_ms"] = r["median_ms"]
        res[f"{name}_edges"] = int(u.shape[0])
        res[f"{name}_zero_edges"] = int((acc == 0).sum())
        res[f"{name}_core_rows"] = int(torch.isfinite(cd).sum())
        res[f"{name}_rounds"] = rounds
        out.clear()
    res["ratio_distinct_over_all"] = round(res["distinct_weighted_ms"] / res["all_points_ms"], 4)
    emit(dict(measure="wkdist_dedup", **res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--dedup-points", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--skip-forest", action="store_true")
    ap.add_argument("--skip-c2", action="store_true")
    ap.add_argument("--skip-dedup", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    OUT[0] = args.out
    _native.require_gpu()
    if not args.skip_c2:
        c2_part(args)
    if not args.skip_dedup:
        dedup_part(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
