"""Brute-force k nearest rows in numpy, O(n m), on kdist_ref's accumulators:
the reference the kneighbors tests compare the GPU against.

The candidates of a query are the rows with acc <= thr (kdist_ref.threshold;
ties at thr are in); the result is the k smallest of them under the total
order (acc, row) ascending — np.lexsort((row, acc)) per query — written in
that order, then k - c slots of (-1, +inf) where only c < k rows qualify.
``labels`` replaces the row number by a label per row (a predict index): the
order is then (acc, label), and equal pairs each appear.
"""
import numpy as np

import kdist_ref


def smallest_pairs(acc, kmax, labels=None):
    """-> (ids int32[m, kmax], acc float64[m, kmax]): each query's first kmax
    rows under (acc, label), uncapped, (-1, inf) past the n rows there are —
    computed once and shared by the tests that ask several k and caps of one
    table (cut).  The table is left unchanged."""
    acc = np.asarray(acc, np.float64)
    m, n = acc.shape
    lab = np.arange(n, dtype=np.int64) if labels is None else np.asarray(labels, np.int64)
    ids = np.full((m, kmax), -1, np.int32)
    out = np.full((m, kmax), np.inf)
    kk = min(kmax, n)
    if kk == 0 or m == 0:
        return ids, out
    kth = np.partition(acc, kk - 1, axis=1)[:, kk - 1]
    for q in range(m):
        # only a row at or below the kk-th smallest value can be among the first
        # kk; the lexsort of those is the head of the lexsort of all
        cand = np.flatnonzero(acc[q] <= kth[q])
        order = cand[np.lexsort((lab[cand], acc[q, cand]))][:kk]
        ids[q, :kk] = lab[order]
        out[q, :kk] = acc[q, order]
    return ids, out


def cut(pairs, k, r_max, metric="euclidean"):
    """kneighbors from smallest_pairs()' table: its first k columns, (-1, inf)
    where the accumulator passes the cap."""
    ids, acc = pairs
    if k < 1 or k > ids.shape[1]:
        raise ValueError("k must be in 1 .. kmax")
    ids, acc = ids[:, :k].copy(), acc[:, :k].copy()
    out = ~(acc <= kdist_ref.threshold(r_max, metric))
    ids[out] = -1
    acc[out] = np.inf
    return ids, acc


def from_accumulators(acc, k, r_max, metric="euclidean", labels=None):
    """-> (ids int32[m, k], acc float64[m, k]) from kdist_ref.accumulators' table."""
    return cut(smallest_pairs(acc, k, labels), k, r_max, metric)


def kneighbors(X, k, r_max, metric="euclidean", Q=None, labels=None):
    X = np.asarray(X)
    Q = X if Q is None else np.asarray(Q)
    return from_accumulators(kdist_ref.accumulators(Q, X, metric), k, r_max, metric, labels)
