"""Brute-force weighted core accumulator and weighted mutual-reachability
forest in numpy, O(n m) (kdist_ref's cap of 3,000 rows): the reference the
sample_weight tests of k_distances and of the forest compare the GPU against.

W_j = rint(w_j * 2^20) as an integer (weighted_ref.fixed_point, the train's
rule), T = k * 2^20, acc the train's accumulator (kdist_ref.accumulators), thr
= r_max * r_max (cityblock: r_max).

cdw(q): over the rows j with acc(q, j) <= thr and W_j > 0, ascending by acc,
the acc at which the running (integer) sum of W reaches T; +inf when it never
does.  Ties in acc do not matter: the value at the crossing is the same in any
order.  `cdw` is this unbounded definition; `cdw_bounded` is what a kernel can
hold: only the slots = ceil(T / W_min) smallest positive-weight candidates,
their weights clamped to T, ties at the list's end cut arbitrarily.

The weighted forest is mreach_ref's with cd = cdw: graph_edges, then kruskal.
"""
import numpy as np

import kdist_ref
import mreach_ref
from weighted_ref import FRAC_BITS, fixed_point

MAX_SLOTS = 64


def target(k):
    return int(k) << FRAC_BITS


def sorted_table(acc, W):
    """-> (a, w): each query's accumulators ascending and the rows' integer
    weights (as fp64: <= 2^51 each, exact) beside them — computed once and
    shared by the tests that ask several k and caps of one point set."""
    order = np.argsort(acc, axis=1, kind="stable")
    return (np.take_along_axis(acc, order, axis=1),
            np.asarray(W, np.uint64).astype(np.float64)[order])


def cdw_of_table(acc, W, k, r_max, metric="euclidean", table=None):
    """cdw[m] from the m x n table of accumulators and the integer weights
    (or from sorted_table of them)."""
    m, n = acc.shape if table is None else table[0].shape
    out = np.full(m, np.inf)
    if n == 0 or m == 0:
        return out
    thr = kdist_ref.threshold(r_max, metric)
    a, w = sorted_table(acc, W) if table is None else table
    # clamped to T the running sums stay below n * 2^26 < 2^53: exact
    w = np.where(a <= thr, np.minimum(w, float(target(k))), 0.0)
    run = np.cumsum(w, axis=1)
    hit = run >= float(target(k))
    has = hit.any(axis=1)
    first = hit.argmax(axis=1)
    rows = np.flatnonzero(has)
    out[rows] = a[rows, first[rows]]
    return out


def cdw(X, weight, k, r_max, metric="euclidean", Q=None):
    """-> float64[m]: the weighted core accumulator of each query (default: the
    rows themselves)."""
    if k < 1:
        raise ValueError("k must be >= 1")
    X = np.asarray(X)
    Q = X if Q is None else np.asarray(Q)
    W = fixed_point(weight)
    if len(W) != len(X):
        raise ValueError("one weight per row")
    if len(Q) == 0 or len(X) == 0:
        return np.full(len(Q), np.inf)
    return cdw_of_table(kdist_ref.accumulators(Q, X, metric), W, k, r_max, metric)


def slots_needed(weight, k):
    """ceil(T / W_min), W_min the smallest non-zero fixed-point weight; 1 when
    no row has weight."""
    W = fixed_point(weight)
    pos = W[W > 0]
    if len(pos) == 0:
        return 1
    wmin = int(pos.min())
    return (target(k) + wmin - 1) // wmin


def cdw_bounded(X, weight, k, r_max, metric="euclidean", Q=None, rng=None):
    """The bounded list, row by row in Python: candidates in a random order
    (rng), a list of `slots` (acc, min(W, T)) pairs that keeps the smallest and
    drops a tie with its largest entry, the crossing taken at the end."""
    X = np.asarray(X)
    Q = X if Q is None else np.asarray(Q)
    W = fixed_point(weight)
    slots = slots_needed(weight, k)
    if slots > MAX_SLOTS:
        raise ValueError(f"{slots} slots pass the limit of {MAX_SLOTS}")
    T = target(k)
    thr = kdist_ref.threshold(r_max, metric)
    rng = rng or np.random.default_rng(0)
    acc = kdist_ref.accumulators(Q, X, metric) if len(Q) and len(X) else np.zeros((len(Q), 0))
    out = np.full(len(Q), np.inf)
    for qi in range(len(Q)):
        best = []                                   # (acc, weight), unordered
        for j in rng.permutation(acc.shape[1]).tolist():
            a = acc[qi, j]
            if not a <= thr or W[j] == 0:
                continue
            if len(best) < slots:
                best.append((a, min(int(W[j]), T)))
                continue
            top = max(range(slots), key=lambda s: best[s][0])
            if a < best[top][0]:
                best[top] = (a, min(int(W[j]), T))
        run = 0
        for a, wj in sorted(best):
            run += wj
            if run >= T:
                out[qi] = a
                break
    return out


def forest(X, weight, k, r_max, metric="euclidean"):
    """-> (u, v, w, cd): the weighted forest's edges ascending by (w, u, v) and
    cd = cdw of the rows."""
    X = np.asarray(X)
    if len(X) == 0:
        return (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))
    table = kdist_ref.accumulators(X, X, metric)
    cd = cdw_of_table(table, fixed_point(weight), k, r_max, metric)
    u, v, w = mreach_ref.graph_edges(table, cd, r_max, metric)
    fu, fv, fw = mreach_ref.kruskal(len(X), u, v, w)
    return fu, fv, fw, cd
