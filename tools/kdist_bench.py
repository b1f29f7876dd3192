"""Time the k-distance query (pd_index_kdist) on C2's points, at r_max = eps
and r_max = 2 eps:

  (a) index build                 _native.Index.over_all(X, r_max)      (all n rows)
  (b) kdist of every point        index.kdist(X, k)                     (n queries, cell-sorted)
  (c) kdist of a sample           index.kdist(X[sample], k)             (--sample queries)
  (d) count stage of a train      DBSCAN(eps=r_max).train(X) with PD_OPT_FULL_COUNTS: the
                                  sweep that visits the same candidates (its own HIP events)

plus the rows a query visits (the records of the 3^d cells around it, counted
on the device for the sample's queries from a cell histogram of the index's own
cell width) and the bytes per second that makes of (b) and (c): rows visited x
record bytes / time.  HIP events on the current stream, one warm-up, --reps
repetitions; medians.  One JSON line per measurement, a summary line last.

  python tools/kdist_bench.py [--points N] [--reps 5] [--sample 1000000] [--k 10]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pypardis_amd import DBSCAN, _native, synth  # noqa: E402


def timed(f, reps, warmup=1):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def line(name, ms, **extra):
    rec = dict(measure=name, median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4),
               max_ms=round(max(ms), 4), reps=len(ms), **extra)
    print(json.dumps(rec), flush=True)
    return rec


def rows_visited(Xd, Q, r_max):
    """Mean and max number of rows in the 3^d cells around each query of Q, on
    the index's grid (origin: the data's minimum, cells r_max * (1 + 2^-20)
    wide; the grid does not grow at these extents)."""
    d = Xd.shape[1]
    lo = Xd.min(dim=0).values.to(torch.float64)
    inv = 1.0 / (r_max * (1.0 + 1.0 / 1048576.0))
    nc = (torch.floor((Xd.max(dim=0).values.to(torch.float64) - lo) * inv) + 1).to(torch.int64)
    stride = torch.ones(d, dtype=torch.int64, device=Xd.device)
    for j in range(1, d):
        stride[j] = stride[j - 1] * nc[j - 1]

    def cells(P):
        return torch.floor((P.to(torch.float64) - lo) * inv).to(torch.int64)

    keys = torch.empty(Xd.shape[0], dtype=torch.int64, device=Xd.device)
    step = 1 << 24
    for s in range(0, Xd.shape[0], step):
        keys[s:s + step] = (cells(Xd[s:s + step]) * stride).sum(dim=1)
    ukeys, counts = torch.unique(keys, return_counts=True)
    del keys
    cq = cells(Q)
    total = torch.zeros(Q.shape[0], dtype=torch.int64, device=Xd.device)
    for off in np.ndindex(*([3] * d)):
        c = cq + torch.tensor(off, device=Xd.device) - 1
        ok = ((c >= 0) & (c < nc)).all(dim=1)
        k = (c * stride).sum(dim=1)
        pos = torch.searchsorted(ukeys, k).clamp_(max=ukeys.shape[0] - 1)
        hit = ok & (ukeys[pos] == k)
        total += torch.where(hit, counts[pos], torch.zeros_like(total))
    return float(total.double().mean()), int(total.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    _native.require_gpu()
    X, cfg = synth.make_config("C2", n=args.points)
    n, d = X.shape
    eps, ms_, P = cfg["eps"], cfg["min_samples"], cfg.get("max_partitions") or 1
    k = args.k or ms_
    Xd = torch.from_numpy(X).cuda()
    del X
    rec_bytes = Xd.element_size() * (4 if d == 3 else d)     # the index's padded record
    head = dict(config="C2", n=n, d=d, eps=eps, k=k, dtype=str(Xd.dtype),
                device=torch.cuda.get_device_name())
    print(json.dumps(dict(measure="setup", **head)), flush=True)
    g = torch.Generator(device="cuda").manual_seed(5)
    sample = Xd[torch.randperm(n, device="cuda", generator=g)[:min(args.sample, n)]].contiguous()
    ctx = _native.context(Xd.device.index)
    summary = []
    for mult in (1.0, 2.0):
        r = eps * mult
        built = [None]

        def build():
            if built[0] is not None:
                built[0].close()
            built[0] = _native.Index.over_all(Xd, r)

        b = line("index_build", timed(build, args.reps), r_max=r)
        ix = built[0]
        out = [None]

        def sweep(Q):
            out[0] = ix.kdist(Q, k)

        a = line("kdist_all_points", timed(lambda: sweep(Xd), args.reps), r_max=r, m=n)
        finite_all = int(torch.isfinite(out[0]).sum())
        s = line("kdist_sample", timed(lambda: sweep(sample), args.reps), r_max=r,
                 m=sample.shape[0])
        ix.close()
        mean_rows, max_rows = rows_visited(Xd, sample, r)
        rec = dict(r_max=r, index_build_ms=b["median_ms"], kdist_all_ms=a["median_ms"],
                   kdist_sample_ms=s["median_ms"], sample=sample.shape[0],
                   rows_visited_per_query=round(mean_rows, 2), rows_visited_max=max_rows,
                   finite_all=finite_all,
                   bytes_per_s_all=round(mean_rows * n * rec_bytes / (a["median_ms"] * 1e-3)),
                   bytes_per_s_sample=round(mean_rows * sample.shape[0] * rec_bytes /
                                            (s["median_ms"] * 1e-3)))
        if not args.skip_train:
            ctx.set_option(_native.PD_OPT_FULL_COUNTS, 1)
            ctx.set_option(_native.PD_OPT_TIMING, 1)
            count, total = [], []
            try:
                for i in range(1 + min(args.reps, 3)):
                    DBSCAN(eps=r, min_samples=ms_, max_partitions=P).train(Xd)
                    torch.cuda.synchronize()
                    if i:
                        t = ctx.timings()
                        count.append(t["count"])
                        total.append(t["total"])
            finally:
                ctx.set_option(_native.PD_OPT_TIMING, 0)
                ctx.set_option(_native.PD_OPT_FULL_COUNTS, 0)
            rec.update(train_full_counts_count_ms=round(statistics.median(count), 4),
                       train_full_counts_total_ms=round(statistics.median(total), 4))
        print(json.dumps(dict(measure="kdist_r", **rec)), flush=True)
        summary.append(rec)
    print(json.dumps(dict(measure="kdist_bench", **head, results=summary)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
