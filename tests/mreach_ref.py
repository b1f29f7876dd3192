"""Brute-force mutual-reachability forest in numpy, O(n^2) memory (kdist_ref's
cap of 3,000 rows): the reference the forest tests compare the GPU against.

acc(i, j) is the train's accumulator (kdist_ref.accumulators), thr = r_max *
r_max (cityblock: r_max).  cd[i] = the k-th smallest acc(i, .) when it is <=
thr, else inf (row i counts itself).  w(i, j) = max(acc(i, j), cd[i], cd[j]).
G = the pairs i < j with w <= thr.  Kruskal over G's edges in the strict order
(w, u, v) gives THE minimum spanning forest under that order: one edge list,
which the GPU's must equal element for element.
"""
import numpy as np

import kdist_ref


def core_accumulators(table, k, r_max, metric="euclidean"):
    """cd from the n x n table of accumulators."""
    n = table.shape[0]
    cd = np.full(n, np.inf)
    if k > n:
        return cd
    kth = np.partition(table, k - 1, axis=1)[:, k - 1]
    ok = kth <= kdist_ref.threshold(r_max, metric)
    cd[ok] = kth[ok]
    return cd


def pairs_within(table, r_max, metric="euclidean"):
    """-> (u, v, acc) of the pairs u < v with acc <= thr: what every k shares."""
    u, v = np.triu_indices(table.shape[0], 1)
    a = table[u, v]
    keep = a <= kdist_ref.threshold(r_max, metric)
    return u[keep], v[keep], a[keep]


def graph_edges(table, cd, r_max, metric="euclidean", pairs=None):
    """-> (u, v, w) of every edge of G, ascending by (w, u, v)."""
    u, v, a = pairs_within(table, r_max, metric) if pairs is None else pairs
    w = np.maximum(a, np.maximum(cd[u], cd[v]))
    keep = w <= kdist_ref.threshold(r_max, metric)
    u, v, w = u[keep], v[keep], w[keep]
    order = np.lexsort((v, u, w))
    return u[order].astype(np.int32), v[order].astype(np.int32), w[order]


def kruskal(n, u, v, w):
    """The forest of edges given ascending by (w, u, v): -> (u, v, w) of the
    edges kept, in that order."""
    par = list(range(n))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    keep = []
    for e, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        ra, rb = find(a), find(b)
        if ra != rb:
            par[max(ra, rb)] = min(ra, rb)
            keep.append(e)
            if len(keep) == n - 1:
                break
    keep = np.asarray(keep, np.int64)
    return u[keep], v[keep], w[keep]


def forest_of_table(table, k, r_max, metric="euclidean", pairs=None):
    """-> (u, v, w, cd) from a precomputed table (and pairs_within of it):
    shared by the tests that ask several k of one point set."""
    cd = core_accumulators(table, k, r_max, metric)
    u, v, w = graph_edges(table, cd, r_max, metric, pairs)
    fu, fv, fw = kruskal(table.shape[0], u, v, w)
    return fu, fv, fw, cd


def forest(X, k, r_max, metric="euclidean"):
    """-> (u, v, w, cd): int32 u < v and float64 w of the forest's edges,
    ascending by (w, u, v); float64 cd[n]."""
    X = np.asarray(X)
    if len(X) == 0:
        return (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))
    return forest_of_table(kdist_ref.accumulators(X, X, metric), k, r_max, metric)


def kruskal_pairs(n, i, j, acc, cd, thr):
    """The forest from a list of pairs (any order, both directions and self
    pairs allowed) with their accumulators and the core accumulators: what a
    radius_neighbors CSR holds.  -> (u, v, w) ascending by (w, u, v).  For the
    sets too large for the Python loop: scipy's Kruskal over the edges' RANKS in
    the order (w, u, v) — distinct weights, so its tree is the unique one."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    up = i < j
    u, v, a = i[up], j[up], np.asarray(acc)[up]
    w = np.maximum(a, np.maximum(cd[u], cd[v]))
    keep = w <= thr
    u, v, w = u[keep], v[keep], w[keep]
    order = np.lexsort((v, u, w))
    u, v, w = u[order], v[order], w[order]
    rank = np.arange(1, len(u) + 1, dtype=np.float64)
    tree = minimum_spanning_tree(coo_matrix((rank, (u, v)), shape=(n, n)).tocsr()).tocoo()
    at = np.sort(tree.data.astype(np.int64) - 1)
    return u[at].astype(np.int32), v[at].astype(np.int32), w[at]


def cut(forest_uvw, cd, eps, metric="euclidean"):
    """-> (member, labels): member = cd <= t, t = eps * eps (cityblock: eps);
    labels int32[n]: the components of the forest's edges with w <= t on the
    member rows, numbered by smallest member row; -1 on the other rows."""
    u, v, w = forest_uvw
    n = len(cd)
    t = kdist_ref.threshold(eps, metric)
    member = cd <= t
    par = np.arange(n)

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    for a, b in zip(u[w <= t].tolist(), v[w <= t].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            par[max(ra, rb)] = min(ra, rb)
    labels = np.full(n, -1, np.int32)
    seen = {}
    for i in np.flatnonzero(member).tolist():
        labels[i] = seen.setdefault(find(i), len(seen))
    return member, labels


def tie_eps(w, r_max):
    """A radius <= r_max that sits exactly on an edge of the forest: sqrt(w0)
    of the euclidean weight w0 nearest the median whose root squares back to it
    bit for bit (so the cut's bound IS that edge's weight); 0.75 * r_max when
    no positive weight does."""
    pos = np.unique(w[w > 0])
    if len(pos) == 0:
        return 0.75 * float(r_max)
    root = np.sqrt(pos)
    ok = (root * root == pos) & (root <= r_max)
    if not ok.any():
        return 0.75 * float(r_max)
    cand = root[ok]
    return float(cand[np.argmin(np.abs(cand - np.median(np.sqrt(w))))])
