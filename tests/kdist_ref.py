"""Brute-force k-distance in numpy, O(n m), capped at 3,000 x 3,000: the
reference the k-distance tests compare the GPU against.

acc(q, x) is the train's accumulator (as weighted_ref.adjacency): fp64,
per-axis difference, squares (euclidean) or absolute values (cityblock) summed
in axis order; numpy rounds every product and sum separately, as the kernels
do.  kdist(q) = the k-th smallest acc(q, x) over the rows x with acc <= thr,
thr = r_max * r_max (cityblock: r_max); +inf when fewer than k rows qualify.
The result is the accumulator itself (the squared distance for euclidean).
"""
import numpy as np

MAX_N = 3000


def threshold(r_max, metric="euclidean"):
    r_max = float(r_max)
    return r_max * r_max if metric == "euclidean" else r_max


def accumulators(Q, X, metric="euclidean"):
    """acc[m, n] between the rows of Q and X, both widened to fp64 exactly."""
    X = np.asarray(X).astype(np.float64)
    Q = np.asarray(Q).astype(np.float64)
    if len(X) > MAX_N or len(Q) > MAX_N:
        raise ValueError(f"kdist_ref is O(n m): {len(Q)} x {len(X)} passes {MAX_N}")
    if X.ndim != 2 or Q.ndim != 2 or X.shape[1] != Q.shape[1]:
        raise ValueError("Q and X must be (m, d) and (n, d)")
    acc = np.zeros((len(Q), len(X)), np.float64)
    with np.errstate(over="ignore"):     # a far query's square may overflow to inf: beyond any cap
        for j in range(X.shape[1]):
            diff = Q[:, None, j] - X[None, :, j]
            acc = acc + (diff * diff if metric == "euclidean" else np.abs(diff))
    return acc


def smallest(X, kmax, metric="euclidean", Q=None):
    """-> float64[m, min(kmax, n)]: each query's smallest accumulators, ascending,
    uncapped — computed once and shared by the tests that ask several k and caps
    of one point set (kth_of)."""
    X = np.asarray(X)
    Q = X if Q is None else np.asarray(Q)
    acc = accumulators(Q, X, metric)
    kk = min(kmax, acc.shape[1])
    if kk == 0:
        return acc[:, :0]
    return np.sort(np.partition(acc, kk - 1, axis=1)[:, :kk], axis=1)


def kth_of(sm, k, r_max, metric="euclidean"):
    """kdist from smallest()'s table: column k - 1 where it is within the cap."""
    out = np.full(sm.shape[0], np.inf)
    if k > sm.shape[1]:
        return out
    kth = sm[:, k - 1]
    ok = kth <= threshold(r_max, metric)
    out[ok] = kth[ok]
    return out


def kdist(X, k, r_max, metric="euclidean", Q=None):
    """-> float64[m]: the k-th smallest accumulator within the cap, inf if none."""
    if k < 1:
        raise ValueError("k must be >= 1")
    X = np.asarray(X)
    Q = X if Q is None else np.asarray(Q)
    out = np.full(len(Q), np.inf)
    if len(X) < k or len(Q) == 0:
        return out
    acc = accumulators(Q, X, metric)
    kth = np.partition(acc, k - 1, axis=1)[:, k - 1]
    ok = kth <= threshold(r_max, metric)
    out[ok] = kth[ok]
    return out
