"""Time DBSCAN.predict beside the train it follows, on one config:

  (a) train                       DBSCAN(...).train(X)
  (b) index build                 _native.Index(X, core_sample_mask_, labels_, eps)
  (c) predict of the training set index.query(X)              (n points; also with the cell
                                                               sort off: *_direct)
  (d) predict of a batch          index.query(batch)          (--batch points: half jittered
                                                               training points, half uniform
                                                               over the data box)
  (e) sorted vs direct sweep      (d) at several batch sizes with the cell sort forced on and
                                  off (PD_INDEX_SORT_MIN), alternating — grid path only

HIP events on the current stream, one warm-up, then --reps repetitions of each;
median, min and max in ms.  One JSON line per measurement on stdout; the last
line ("predict_bench") states the derived bar: (c) must not exceed (a) of the
same run.  (c) is also checked against labels_ (predict(X_train) == labels_).

  python tools/predict_bench.py --config C2 [--points N] [--reps 10] [--batch 1000000]
  python tools/predict_bench.py --config C3 --batch 100000 --reps 3
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=["C1", "C2", "C3"])
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--ab-sizes", default="4096,16384,65536,262144,1000000")
    args = ap.parse_args()
    _native.require_gpu()
    X, cfg = synth.make_config(args.config, n=args.points)
    n, d = X.shape
    eps, ms_, P = cfg["eps"], cfg["min_samples"], cfg.get("max_partitions") or 1
    lo, hi = X.min(axis=0), X.max(axis=0)
    Xd = torch.from_numpy(X).cuda()
    del X
    head = dict(config=args.config, n=n, d=d, eps=eps, min_samples=ms_, max_partitions=P,
                dtype=str(Xd.dtype), device=torch.cuda.get_device_name())
    print(json.dumps(dict(measure="setup", **head)), flush=True)

    model = [None]

    def train():
        model[0] = DBSCAN(eps=eps, min_samples=ms_, max_partitions=P).train(Xd)

    a = line("train", timed(train, args.reps), **head)
    m = model[0]
    metric = _native.PD_EUCLIDEAN
    built = [None]

    def build():
        if built[0] is not None:
            built[0].close()
        built[0] = _native.Index(Xd, m.core_sample_mask_, m.labels_, eps, metric)

    b = line("index_build", timed(build, args.reps), n_core=None)
    ix = built[0]
    out = [None]

    def all_points():
        out[0] = ix.query(Xd)

    c = line("predict_train_set", timed(all_points, args.reps), m=n, n_core=ix.n_core)
    same = bool(torch.equal(out[0], m.labels_))
    c2 = None
    if d <= 4:   # the same queries swept in input order (no cell sort)
        os.environ["PD_INDEX_SORT_MIN"] = str(1 << 62)
        c2 = line("predict_train_set_direct", timed(all_points, args.reps), m=n)
        os.environ.pop("PD_INDEX_SORT_MIN", None)
        same = same and bool(torch.equal(out[0], m.labels_))

    g = torch.Generator(device="cuda").manual_seed(5)
    mb = min(args.batch, n)
    half = mb // 2
    pick = torch.randint(0, n, (half,), device="cuda", generator=g)
    jit = Xd[pick] + (eps / 2) * torch.randn((half, d), device="cuda", dtype=Xd.dtype, generator=g)
    lo_t = torch.from_numpy(lo).cuda().to(Xd.dtype)
    hi_t = torch.from_numpy(hi).cuda().to(Xd.dtype)
    uni = lo_t + (hi_t - lo_t) * torch.rand((mb - half, d), device="cuda", dtype=Xd.dtype,
                                            generator=g)
    batch = torch.cat([jit, uni])[torch.randperm(mb, device="cuda", generator=g)].contiguous()
    dd = line("predict_batch", timed(lambda: ix.query(batch), args.reps), m=mb)

    ab = []
    if d <= 4:
        for size in [int(s) for s in args.ab_sizes.split(",") if int(s) <= mb]:
            q = batch[:size].contiguous()
            t = {"sorted": [], "direct": []}
            for mode, val in (("sorted", "0"), ("direct", str(1 << 62))):   # warm both
                os.environ["PD_INDEX_SORT_MIN"] = val
                ix.query(q)
            for _ in range(args.reps):
                for mode, val in (("sorted", "0"), ("direct", str(1 << 62))):
                    os.environ["PD_INDEX_SORT_MIN"] = val
                    t[mode] += timed(lambda: ix.query(q), 1, warmup=0)
            os.environ.pop("PD_INDEX_SORT_MIN", None)
            ab.append(dict(m=size, sorted_ms=round(statistics.median(t["sorted"]), 4),
                           direct_ms=round(statistics.median(t["direct"]), 4)))
            print(json.dumps(dict(measure="sweep_order_ab", **ab[-1])), flush=True)

    print(json.dumps(dict(measure="predict_bench", **head, n_core=ix.n_core,
                          train_ms=a["median_ms"], index_build_ms=b["median_ms"],
                          predict_train_set_ms=c["median_ms"],
                          predict_train_set_direct_ms=c2["median_ms"] if c2 else None,
                          predict_batch_ms=dd["median_ms"],
                          batch=mb, predict_equals_labels=same,
                          bar_predict_le_train=c["median_ms"] <= a["median_ms"],
                          queries_per_s_train_set=round(n / (c["median_ms"] * 1e-3)),
                          queries_per_s_batch=round(mb / (dd["median_ms"] * 1e-3)),
                          sweep_order_ab=ab)), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
