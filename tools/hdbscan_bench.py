"""Time HDBSCAN from the forest (pd_forest_condense, pd_condensed_select,
pd_condensed_labels) on C2's points at min_samples = 10, r_max = eps, beside
the forest build on the same points in the same process (the yardstick):

  (a) forest            index.mreach_forest(k), wall ms of the whole call
  (b) condense, per m   synchronised wall ms of each stage (stage_ms_host):
                        checks, the stage-1 rounds (with their count), classify,
                        blobs, the host tree, locate, reductions
  (c) select            the host selection (excess of mass)
  (d) labels            the label and probability pass

for min_cluster_size 10 and 100, on a density-preserving slice of --sample
points and on the full set.  One warm-up call, --reps repetitions, medians.
Beside the times: T (true splits), the clusters of the condensed tree and the
clusters selected.  One JSON line per measurement, a summary line last; every
line is also appended to --out.

  python tools/hdbscan_bench.py [--points N] [--sample 1000000] [--reps 3] [--k 10]
                                [--m 10,100] [--out profiles/hdbscan_c2_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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


def wall(f, reps, warmup=1):
    """-> (ms per repetition, the last result)."""
    res = None
    for _ in range(warmup):
        res = f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = f()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, res


def med(ms):
    return round(statistics.median(ms), 3)


def one_set(name, n, k, ms_list, reps):
    X, cfg = synth.make_config("C2", n=n)
    n, d = X.shape
    r = cfg["eps"]
    Xd = torch.from_numpy(X).cuda()
    del X
    head = dict(config="C2", set=name, n=n, d=d, r_max=r, k=k, dtype=str(Xd.dtype),
                device=torch.cuda.get_device_name())
    emit(dict(measure="setup", **head))
    ix = _native.Index.over_rows(Xd, r)
    fms, forest = wall(lambda: ix.mreach_forest(k), reps)
    u, v, w, cd, frounds = forest
    ix.close()
    emit(dict(measure="forest", median_ms=med(fms), all_ms=[round(t, 3) for t in fms],
              edges=int(u.shape[0]), forest_rounds=frounds, **head))
    out = dict(head, forest_ms=med(fms), edges=int(u.shape[0]), by_m=[])
    if u.shape[0] and float(w[0]) == 0.0:
        emit(dict(measure="refused", reason="the lightest edge weighs 0", **head))
        return out
    for m in ms_list:
        runs = []

        def condense():
            runs.append(_native.forest_condense(n, u, v, w, True, m, timings=True))
            return runs[-1]

        cms, tree = wall(condense, reps)
        stages = {s: med([t["stage_ms"][s] for t in runs[-reps:]])
                  for s in _native.CONDENSE_STAGES}
        parent = tree["parent"]
        clusters = int(parent.shape[0])
        T = int(np.unique(parent[parent >= 0]).shape[0])
        sms, target = wall(lambda: _native.condensed_select(parent, tree["stability"]), reps)
        lms, lab = wall(lambda: _native.condensed_labels(tree["point_cluster"],
                                                         tree["point_lambda"], target,
                                                         tree["lambda_max"]), reps)
        rec = emit(dict(measure="hdbscan", m=m, condense_ms=med(cms), stage_ms=stages,
                        rounds=tree["rounds"], select_ms=med(sms), labels_ms=med(lms),
                        total_ms=round(med(cms) + med(sms) + med(lms), 3),
                        over_forest=round((med(cms) + med(sms) + med(lms)) / med(fms), 3),
                        true_splits=T, clusters=clusters, selected=lab[2],
                        noise_rows=int((lab[0] < 0).sum()), **head))
        out["by_m"].append({key: rec[key] for key in
                            ("m", "condense_ms", "stage_ms", "rounds", "select_ms", "labels_ms",
                             "total_ms", "over_forest", "true_splits", "clusters", "selected",
                             "noise_rows")})
        del tree, lab, runs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--sample", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--m", default="10,100")
    ap.add_argument("--skip-all", action="store_true", help="the sample only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    OUT[0] = args.out
    _native.require_gpu()
    ms_list = [int(s) for s in args.m.split(",")]
    results = [one_set("sample", args.sample, args.k, ms_list, args.reps)] if args.sample else []
    if not args.skip_all:
        results.append(one_set("all", args.points, args.k, ms_list, args.reps))
    emit(dict(measure="hdbscan_bench", results=results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
