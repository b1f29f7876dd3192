"""Brute-force radius neighbours in numpy, O(n m), on kdist_ref.accumulators
(capped at 3,000 x 3,000): the reference the radius-query tests compare the GPU
against, and the CPU derivation of DBSCAN's labels from such a graph.

neighbours(q) = the rows x with acc(q, x) <= thr, thr = radius * radius in
double (cityblock: radius) — kdist_ref.threshold, the predicate of a train at
eps = radius.  Ties at exactly thr are in, duplicates each appear, a query that
is a row contains itself at 0.
"""
import numpy as np

import kdist_ref


def radius_neighbors(X, radius, metric="euclidean", Q=None):
    """-> (indptr int64[m + 1], indices int32[nnz] ascending inside each row,
    acc float64[nnz]): CSR in query order."""
    X = np.asarray(X)
    Q = X if Q is None else np.asarray(Q)
    return from_accumulators(kdist_ref.accumulators(Q, X, metric), radius, metric)


def from_accumulators(acc, radius, metric="euclidean"):
    """radius_neighbors from a table of kdist_ref.accumulators, which is left
    unchanged: the tests that ask several radii of one point set share it."""
    hit = acc <= kdist_ref.threshold(radius, metric)
    indptr = np.zeros(acc.shape[0] + 1, np.int64)
    np.cumsum(hit.sum(axis=1), out=indptr[1:])
    rows, cols = np.nonzero(hit)          # row-major: ascending columns inside a row
    return indptr, cols.astype(np.int32), acc[rows, cols]


def radius_neighbors_blocked(X, radius, metric="euclidean", block=2500):
    """radius_neighbors(X, radius, metric) of a point set larger than the cap,
    against itself: the same brute force over block x block tiles of
    kdist_ref.accumulators, each within the cap."""
    X = np.asarray(X)
    n = len(X)
    thr = kdist_ref.threshold(radius, metric)
    counts, cols, accs = [], [], []
    for q0 in range(0, n, block):
        hits = []
        for x0 in range(0, n, block):
            acc = kdist_ref.accumulators(X[q0:q0 + block], X[x0:x0 + block], metric)
            r, c = np.nonzero(acc <= thr)
            hits.append((r, c + x0, acc[r, c]))
        r = np.concatenate([h[0] for h in hits])
        order = np.argsort(r, kind="stable")     # tiles come in ascending column order
        counts.append(np.bincount(r, minlength=len(X[q0:q0 + block])))
        cols.append(np.concatenate([h[1] for h in hits])[order])
        accs.append(np.concatenate([h[2] for h in hits])[order])
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.concatenate(counts), out=indptr[1:])
    return indptr, np.concatenate(cols).astype(np.int32), np.concatenate(accs)


def sort_rows(indptr, indices, *values):
    """The CSR rows re-ordered by index (the GPU leaves the order inside a row
    unspecified): -> (indices, *values), each permuted alike."""
    indptr = np.asarray(indptr)
    indices = np.asarray(indices)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    perm = np.lexsort((indices, rows))
    return (indices[perm],) + tuple(np.asarray(v)[perm] for v in values)


def labels_from_graph(indptr, indices, min_samples):
    """DBSCAN's labels from the eps-graph of a point set against itself:
    core = at least min_samples neighbours (itself included); clusters = the
    components of the core-core edges, numbered by their smallest core index;
    a border point takes the smallest label among its core neighbours; noise
    is -1.  -> (labels int64[n], core bool[n])."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    n = len(indptr) - 1
    core = np.diff(indptr) >= min_samples
    rows = np.repeat(np.arange(n), np.diff(indptr))
    cc = core[rows] & core[indices]
    g = csr_matrix((np.ones(int(cc.sum()), np.int8), (rows[cc], indices[cc])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    labels = np.full(n, -1, np.int64)
    ci = np.flatnonzero(core)
    if len(ci) == 0:
        return labels, core
    # components in the order of their smallest core index
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp[ci], ci)
    rank = np.full(comp.max() + 1, -1, np.int64)
    seen = np.flatnonzero(first < n)
    rank[seen[np.argsort(first[seen])]] = np.arange(len(seen))
    labels[ci] = rank[comp[ci]]
    # border: the smallest label among the core neighbours
    be = ~core[rows] & core[indices]
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, rows[be], labels[indices[be]])
    got = best != np.iinfo(np.int64).max
    labels[got] = best[got]
    return labels, core
