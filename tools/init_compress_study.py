"""Offline study (CPU): how deep the window union's root walks go in the forest
init_kernel writes, and what compressing that forest inside tiles of T
consecutive records buys (a sibling of tools/init_forest_study.py: same
density-preserving C2 slice, same record order, the engine's parent rule).

Parent rule (engine.hip, init_kernel): the count sweep keeps the two smallest
neighbours it saw (centre batch first, early exit at min_samples after a group
of four); par[r] is the smaller of them that is core and below r, else r.

Compression inside a tile: every record points at its first ancestor outside
its tile of T consecutive records, or at the chain's root when that lies in
the tile (roots and trees unchanged).

Walk model (window_uf_kernel): a wave is 256 consecutive records; each core
record steps along `par` to a root, one round per hop, and the wave waits for
its deepest walk.  Records in groups more than `lag` groups behind the wave's
own count as flattened by earlier waves (one hop to their root): lag 0 is a
strictly sequential dispatch, lag inf means nothing is flattened yet.  The
unions (they deepen chains) and the XCD block mapping are ignored.

Prints where the parents lie, and per forest and lag the deepest walk per wave
(mean and p90 over the waves that hold a core record) and the mean hops per
core record.  The neighbour lists take
minutes at 1e6 points, so they are cached in a file.

  python tools/init_compress_study.py [n] [--cache DIR] [--tiles 256,1024,4096]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, ".")
import oracle  # noqa: E402
from pypardis_amd import synth  # noqa: E402

WAVE = 256
LAGS = (0, 2, 8, None)   # None: nothing flattened


def neighbours(X, eps, n, cache):
    """CSR neighbour lists (self included) of the slice, cached by n and eps."""
    os.makedirs(cache, exist_ok=True)
    path = os.path.join(cache, f"init_study_nbr_C2_{n}.npz")
    if os.path.exists(path):
        z = np.load(path)
        if z["off"].shape[0] == n + 1 and float(z["eps"]) == float(eps):
            return z["off"], z["nbr"]
    off, nbr = oracle.neighbors(X, eps)
    np.savez(path, off=off, nbr=nbr, eps=np.float64(eps))
    return off, nbr


def engine_forest(X, eps, ms, off, nbr):
    """(par, core) in record space: the forest init_kernel writes."""
    n = len(X)
    X64 = X.astype(np.float64)
    cw = eps * (1 + 2.0 ** -20)
    c = np.floor((X64 - X64.min(0)) / np.array([cw / 2, cw, cw])).astype(np.int64)
    nc = c.max(0) + 1
    key = c[:, 0] + nc[0] * (c[:, 1] + nc[1] * c[:, 2])
    order = np.argsort(key, kind="stable")
    rec = np.empty(n, np.int64)
    rec[order] = np.arange(n)
    cnt = np.diff(off)
    core = (cnt >= ms)[order]
    src = np.repeat(np.arange(n), cnt)
    i_r, j_r = rec[src], rec[nbr]
    dy, dz = c[nbr, 1] - c[src, 1], c[nbr, 2] - c[src, 2]
    need = np.minimum(cnt[order], ms)
    # the count sweep's scan order: batches by dz (0, +1, -1), rows by dy
    # (0, -1, +1), then the record index; it stops after the group of four in
    # which the count reaches min_samples
    bt = np.select([dz == v for v in (0, 1, -1)], [0, 1, 2])
    row = np.select([dy == v for v in (0, -1, 1)], [0, 1, 2])
    o = np.lexsort((j_r, row, bt, i_r))
    i_s, j_s = i_r[o], j_r[o]
    pos = np.arange(len(i_s)) - np.searchsorted(i_s, np.arange(n))[i_s]
    seen = pos < ((need[i_s] + 3) // 4) * 4
    i2, j2 = i_s[seen], j_s[seen]
    o2 = np.lexsort((j2, i2))
    i2, j2 = i2[o2], j2[o2]
    rank = np.arange(len(i2)) - np.searchsorted(i2, np.arange(n))[i2]
    keep = (rank < 2) & core[j2]            # the two smallest seen, core ones
    mn = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(mn, i2[keep], j2[keep])
    ar = np.arange(n)
    par = np.where(core & (mn < ar), mn, ar)
    return par, core


def compress(par, T):
    """Pointer jumping inside tiles of T records (what init_kernel does in
    LDS): a record whose parent lies in its tile and is not a root takes the
    parent's parent, until nothing moves.  Returns (forest, rounds)."""
    par = par.copy()
    ar = np.arange(len(par))
    rounds = 0
    while True:
        p = par[ar]
        g = par[p]
        move = (p // T == ar // T) & (g != p)
        rounds += 1
        if not move.any():
            return par, rounds
        par[move] = g[move]


def roots_of(par):
    root = par.copy()
    while True:
        nxt = root[root]
        if np.array_equal(nxt, root):
            return root
        root = nxt


def walk_hops(par, root, core, lag):
    """Hops of every core record's walk to a root under the lagged flatten."""
    n = len(par)
    ar = np.arange(n)
    grp = ar // WAVE
    cur = ar.copy()
    hops = np.zeros(n, np.int64)
    act = core.copy()
    while act.any():
        a = np.flatnonzero(act)
        x = cur[a]
        flat = np.zeros(len(a), bool) if lag is None else grp[x] < grp[a] - lag
        nxt = np.where(flat, root[x], par[x])
        moved = nxt != x
        hops[a[moved]] += 1
        cur[a] = nxt
        act[a[~moved]] = False
    return hops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=300_000)
    ap.add_argument("--cache", default="bench_out", help="directory of the neighbour-list cache")
    ap.add_argument("--tiles", default="256,1024,4096")
    args = ap.parse_args()
    n = args.n
    X, cfg = synth.make_config("C2", n=n)
    eps, ms = cfg["eps"], cfg["min_samples"]
    off, nbr = neighbours(X, eps, n, args.cache)
    par, core = engine_forest(X, eps, ms, off, nbr)
    ar = np.arange(n)
    nonroot = core & (par != ar)
    d = (ar - par)[nonroot]
    same = (par // WAVE == ar // WAVE)[nonroot]
    print(f"n={n} core={int(core.sum())} roots={int((core & (par == ar)).sum())} "
          f"non-root core={int(nonroot.sum())}")
    print(f"parent in the record's own {WAVE}-record group: {same.mean():.2f}; "
          f"within 16 records: {(d <= 16).mean():.2f}; within 256: {(d <= 256).mean():.2f}")
    root = roots_of(par)
    forests = [("the parent rule alone (not compressed)", par, None)]
    for T in (int(t) for t in args.tiles.split(",")):
        pc, rounds = compress(par, T)
        assert np.array_equal(roots_of(pc), root), "compression changed a root"
        assert (pc <= ar).all() and core[pc[core]].all()
        forests.append((f"compressed inside {T}-record tiles", pc, rounds))
    nw = (n + WAVE - 1) // WAVE
    busy = np.zeros(nw, bool)   # waves with a core record (the others walk nothing)
    busy[(ar // WAVE)[core]] = True
    head = "".join(f" | lag {'inf' if g is None else g}" for g in LAGS)
    print(f"\ndeepest walk per wave, mean (p90); mean hops per core record in []\n"
          f"| forest the window kernel reads{head} |")
    print("|---" * (len(LAGS) + 1) + "|")
    for name, p, rounds in forests:
        cells = []
        for lag in LAGS:
            hops = walk_hops(p, root, core, lag)
            deep = np.zeros(nw, np.int64)
            np.maximum.at(deep, ar // WAVE, hops)
            deep = deep[busy]
            cells.append(f"{deep.mean():.1f} ({np.percentile(deep, 90):.0f}) "
                         f"[{hops[core].mean():.2f}]")
        note = "" if rounds is None else f" ({rounds} jumping rounds)"
        print(f"| {name}{note} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
