"""Time the k-nearest query (pd_index_kneighbors) on C2's points at r_max = eps,
beside the k-distance query (pd_index_kdist) that does the same walk:

  (a) index build                 _native.Index.over_rows(X, r_max)     (all n rows)
  (b) kdist                       index.kdist(Q, k)                     (the yardstick)
  (c) kneighbors, ids only        index.kneighbors(Q, k, False)         (4 k bytes per query)
  (d) kneighbors, ids + acc       index.kneighbors(Q, k, True)          (12 k bytes per query)

each for Q = every point (n queries, cell-sorted) and Q = a sample (--sample
queries).  Per k: the bytes (c) and (d) write, their ratio to (b), and the rate
the excess over (b) makes of those bytes.  HIP events on the current stream,
one warm-up, --reps repetitions; medians.  The output tensors are allocated
once, outside the timed region.  One JSON line per measurement, a summary line
last.

  python tools/kneighbors_bench.py [--points N] [--reps 5] [--sample 1000000] [--k 4,10]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pypardis_amd import _native, synth  # noqa: E402
from pypardis_amd._native import _check, _stream, load  # noqa: E402


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
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1_000_000)
    ap.add_argument("--k", default="4,10")
    args = ap.parse_args()
    _native.require_gpu()
    X, cfg = synth.make_config("C2", n=args.points)
    n, d = X.shape
    r = cfg["eps"]
    ks = [int(v) for v in args.k.split(",")]
    Xd = torch.from_numpy(X).cuda()
    del X
    head = dict(config="C2", n=n, d=d, r_max=r, dtype=str(Xd.dtype),
                device=torch.cuda.get_device_name())
    print(json.dumps(dict(measure="setup", **head)), flush=True)
    g = torch.Generator(device="cuda").manual_seed(5)
    sample = Xd[torch.randperm(n, device="cuda", generator=g)[:min(args.sample, n)]].contiguous()
    built = [None]

    def build():
        if built[0] is not None:
            built[0].close()
        built[0] = _native.Index.over_rows(Xd, r)

    b = line("index_build", timed(build, args.reps), r_max=r)
    ix = built[0]
    dt = _native._check_points(Xd)
    summary = []
    for k in ks:
        rec = dict(k=k, index_build_ms=b["median_ms"])
        for what, Q in (("all", Xd), ("sample", sample)):
            m = Q.shape[0]
            kd = line("kdist_" + what, timed(lambda: ix.kdist(Q, k), args.reps), k=k, m=m)
            ids = torch.empty((m, k), dtype=torch.int32, device="cuda")
            acc = torch.empty((m, k), dtype=torch.float64, device="cuda")

            def ask(with_acc):
                _check(load().pd_index_kneighbors(ix.ptr, Q.data_ptr(), dt, m, k, ids.data_ptr(),
                                                  acc.data_ptr() if with_acc else None,
                                                  _stream(Q.device)))

            i_ = line("kneighbors_ids_" + what, timed(lambda: ask(False), args.reps), k=k, m=m,
                      bytes_written=4 * k * m)
            a_ = line("kneighbors_ids_acc_" + what, timed(lambda: ask(True), args.reps), k=k, m=m,
                      bytes_written=12 * k * m)
            full = int((ids[:, k - 1] >= 0).sum())
            same = bool(torch.equal(acc[:, k - 1], ix.kdist(Q, k)))
            del ids, acc
            rec.update({
                "m_" + what: m, "kdist_%s_ms" % what: kd["median_ms"],
                "ids_%s_ms" % what: i_["median_ms"], "ids_acc_%s_ms" % what: a_["median_ms"],
                "ids_%s_bytes" % what: 4 * k * m, "ids_acc_%s_bytes" % what: 12 * k * m,
                "ids_%s_over_kdist" % what: round(i_["median_ms"] / kd["median_ms"], 3),
                "ids_acc_%s_over_kdist" % what: round(a_["median_ms"] / kd["median_ms"], 3),
                "ids_acc_%s_excess_bytes_per_s" % what: round(
                    12 * k * m / max((a_["median_ms"] - kd["median_ms"]) * 1e-3, 1e-9)),
                "full_rows_" + what: full, "last_column_equals_kdist_" + what: same})
        print(json.dumps(dict(measure="kneighbors_k", **rec)), flush=True)
        summary.append(rec)
    ix.close()
    print(json.dumps(dict(measure="kneighbors_bench", **head, results=summary)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
