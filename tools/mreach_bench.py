"""Time the mutual-reachability forest (pd_index_mreach_forest) on C2's points
at min_samples = 10, r_max = eps, beside the k-distance query over the same
points on the same build (the yardstick: the forest's first round does about
that walk plus the reads of each surviving candidate's core accumulator,
component and row number):

  (a) index build                 _native.Index.over_rows(X, r_max)
  (b) kdist, every point          index.kdist(X, k)
  (c) forest, cell short cut on   index.mreach_forest(k)
  (d) forest, cell short cut off  the same with PD_MREACH_CELL_SKIP=0

for the full set and for a density-preserving slice of --sample points.  (c)
and (d) are wall times of the whole call (its k-distance pass, the rounds with
one host read each, the final sort); per round, from PD_MREACH_TRACE: the wall
time up to the host read, the edges emitted and the share of the cells the
lanes met that the short cut skipped.  One warm-up call, --reps repetitions,
medians; the rounds are those of the last repetition.  One JSON line per
measurement, a summary line last.

  python tools/mreach_bench.py [--points N] [--sample 1000000] [--reps 3] [--k 10]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def line(name, ms, **extra):
    rec = dict(measure=name, median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4),
               max_ms=round(max(ms), 4), reps=len(ms), **extra)
    print(json.dumps(rec), flush=True)
    return rec


def forest_runs(ix, k, reps, skip):
    """Wall ms of `reps` forests after a warm-up, and the last one's rounds."""
    os.environ["PD_MREACH_CELL_SKIP"] = "1" if skip else "0"
    ix.mreach_forest(k)
    torch.cuda.synchronize()
    ms, rounds, edges = [], [], 0
    for _ in range(reps):
        with tempfile.NamedTemporaryFile("r", suffix=".jsonl") as tf:
            os.environ["PD_MREACH_TRACE"] = tf.name
            t0 = time.perf_counter()
            u, _, _, cd, _ = ix.mreach_forest(k)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            del os.environ["PD_MREACH_TRACE"]
            rounds = [json.loads(ln) for ln in tf.read().splitlines() if ln.strip()]
        edges = int(u.shape[0])
        core = int(torch.isfinite(cd).sum())
        del u, cd
    del os.environ["PD_MREACH_CELL_SKIP"]
    for r in rounds:
        r["skipped_share"] = round(r["cells_skipped"] / max(r["cells"], 1), 4)
    return ms, rounds, edges, core


def one_set(name, n, k, reps):
    X, cfg = synth.make_config("C2", n=n)
    n, d = X.shape
    r = cfg["eps"]
    Xd = torch.from_numpy(X).cuda()
    del X
    head = dict(config="C2", set=name, n=n, d=d, r_max=r, k=k, dtype=str(Xd.dtype),
                device=torch.cuda.get_device_name())
    print(json.dumps(dict(measure="setup", **head)), flush=True)
    built = [None]

    def build():
        if built[0] is not None:
            built[0].close()
        built[0] = _native.Index.over_rows(Xd, r)

    b = line("index_build", timed(build, reps), **head)
    ix = built[0]
    kd = line("kdist_all_points", timed(lambda: ix.kdist(Xd, k), reps), **head)
    out = dict(head, index_build_ms=b["median_ms"], kdist_ms=kd["median_ms"])
    for skip in (True, False):
        ms, rounds, edges, core = forest_runs(ix, k, reps, skip)
        tag = "skip_on" if skip else "skip_off"
        rec = line("forest_" + tag, ms, edges=edges, core_rows=core, n_rounds=len(rounds),
                   rounds=rounds, over_kdist=round(statistics.median(ms) / kd["median_ms"], 3),
                   **head)
        out["forest_%s_ms" % tag] = rec["median_ms"]
        out["rounds_" + tag] = rounds
        out["edges"] = edges
        out["core_rows"] = core
    ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--sample", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    _native.require_gpu()
    results = [one_set("sample", args.sample, args.k, args.reps)] if args.sample else []
    results.append(one_set("all", args.points, args.k, args.reps))
    print(json.dumps(dict(measure="mreach_bench", results=results)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
