"""Time the radius query (pd_index_radius_count / pd_index_radius_fill) on C2's
points at radius = eps:

  (a) index build            _native.Index.over_rows(X, eps)            (all n rows)
  (b) count pass             index.radius_count(Q)                      (counts, 64-bit scan, total)
  (c) fill, ids only         index.radius_fill(Q, eps, indptr, ids)
  (d) fill, ids and acc      index.radius_fill(Q, eps, indptr, ids, acc)

each of (b)-(d) for Q = every point (cell-sorted sweep) and for a sample of
--sample points, plus the number of pairs (nnz) and the bytes a fill writes
(4 per pair, 12 with the accumulators).  ids / acc are allocated once, outside
the timed region.  HIP events on the current stream, one warm-up, --reps
repetitions; medians.  One JSON line per measurement, a summary line last, on
stdout and appended to --out.

  python tools/radius_bench.py [--points N] [--reps 5] [--sample 1000000]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from pypardis_amd import _native, synth  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "radius_c2_bench.jsonl"))
    args = ap.parse_args()
    _native.require_gpu()
    sink = open(args.out, "a")

    def line(name, ms=None, **extra):
        rec = dict(measure=name)
        if ms is not None:
            rec.update(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4),
                       max_ms=round(max(ms), 4), reps=len(ms))
        rec.update(extra)
        for out in (sys.stdout, sink):
            print(json.dumps(rec), file=out, flush=True)
        return rec

    X, cfg = synth.make_config("C2", n=args.points)
    n, d = X.shape
    eps = cfg["eps"]
    Xd = torch.from_numpy(X).cuda()
    del X
    head = dict(config="C2", n=n, d=d, eps=eps, radius=eps, dtype=str(Xd.dtype),
                device=torch.cuda.get_device_name())
    line("setup", **head)
    g = torch.Generator(device="cuda").manual_seed(5)
    sample = Xd[torch.randperm(n, device="cuda", generator=g)[:min(args.sample, n)]].contiguous()
    built = [None]

    def build():
        if built[0] is not None:
            built[0].close()
        built[0] = _native.Index.over_rows(Xd, eps)

    summary = dict(index_build_ms=line("index_build", timed(build, args.reps))["median_ms"])
    ix = built[0]
    for tag, Q in (("all_points", Xd), ("sample", sample)):
        m = Q.shape[0]
        res = [None]

        def count():
            res[0] = ix.radius_count(Q, eps)

        c = line("radius_count_" + tag, timed(count, args.reps), m=m)
        indptr, nnz = res[0]
        ids = torch.empty(nnz, dtype=torch.int32, device="cuda")
        f1 = line("radius_fill_ids_" + tag, timed(lambda: ix.radius_fill(Q, eps, indptr, ids),
                                                   args.reps), m=m, nnz=nnz, bytes_written=4 * nnz)
        acc = torch.empty(nnz, dtype=torch.float64, device="cuda")
        f2 = line("radius_fill_ids_acc_" + tag,
                  timed(lambda: ix.radius_fill(Q, eps, indptr, ids, acc), args.reps), m=m, nnz=nnz,
                  bytes_written=12 * nnz)
        summary[tag] = dict(m=m, nnz=nnz, pairs_per_query=round(nnz / m, 2),
                            count_ms=c["median_ms"], fill_ids_ms=f1["median_ms"],
                            fill_ids_acc_ms=f2["median_ms"], bytes_ids=4 * nnz,
                            bytes_ids_acc=12 * nnz,
                            fill_ids_acc_bytes_per_s=round(12 * nnz / (f2["median_ms"] * 1e-3)))
        del ids, acc, indptr
    ix.close()
    line("radius_bench", **head, **summary)
    sink.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
