"""Brute-force weighted DBSCAN in numpy, O(n^2), for n <= 3,000: the
reference the sample_weight tests compare the GPU against where sklearn is
not the yardstick (the documented fixed-point rule on non-dyadic weights).

The rule (include/pardis.h, pd_*_weighted): W_i = rint(w_i * 2^20) (round half
to even) as an integer; a point is core iff the W of the points within eps of
it, itself included, sum to min_samples * 2^20 or more.  Labels as sklearn's
dbscan_inner: the component of a core point is keyed by its smallest core
index, a border point takes the smallest key among its core neighbours, keys
are ranked.

The neighbour predicate is the train's: fp64, per-axis difference, squares
(euclidean) or absolute values (cityblock) summed in axis order, compared
with eps*eps (eps).  numpy rounds every product and sum separately, as the
kernels do.
"""
import numpy as np

FRAC_BITS = 20
MAX_N = 3000


def fixed_point(w):
    """The integer weights (Python-int exact: uint64 holds them all)."""
    w = np.asarray(w, np.float64)
    if not (np.isfinite(w).all() and (w >= 0).all() and (w <= 2.0 ** 31).all()):
        raise ValueError("weights must be finite and in [0, 2^31]")
    return np.rint(w * float(1 << FRAC_BITS)).astype(np.uint64)


def adjacency(X, eps, metric="euclidean"):
    X = np.asarray(X).astype(np.float64)
    n, d = X.shape
    if n > MAX_N:
        raise ValueError(f"weighted_ref is O(n^2): n = {n} > {MAX_N}")
    acc = np.zeros((n, n), np.float64)
    for j in range(d):
        diff = X[:, None, j] - X[None, :, j]
        acc = acc + (diff * diff if metric == "euclidean" else np.abs(diff))
    return acc <= (eps * eps if metric == "euclidean" else eps)


def weighted_dbscan(X, eps, min_samples, weight, metric="euclidean"):
    """-> (labels int64[n], core bool[n])."""
    adj = adjacency(X, eps, metric)
    n = adj.shape[0]
    W = fixed_point(weight)
    # sums stay below n * 2^51 < 2^63: exact in uint64
    sums = (adj.astype(np.uint64) * W[None, :]).sum(axis=1, dtype=np.uint64)
    core = sums >= np.uint64(int(min_samples) << FRAC_BITS)
    key = np.full(n, -1, np.int64)
    for i in np.flatnonzero(core):
        if key[i] >= 0:
            continue
        key[i] = i
        stack = [i]
        while stack:
            u = stack.pop()
            for v in np.flatnonzero(adj[u] & core & (key < 0)):
                key[v] = i
                stack.append(v)
    out = key.copy()
    big = np.iinfo(np.int64).max
    ck = np.where(core, key, big)
    for i in np.flatnonzero(~core):
        m = np.where(adj[i], ck, big).min()
        out[i] = -1 if m == big else m
    roots = np.unique(out[out >= 0])
    labels = np.where(out >= 0, np.searchsorted(roots, out), -1).astype(np.int64)
    return labels, core
