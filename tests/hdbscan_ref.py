"""HDBSCAN from a mutual-reachability forest, in numpy and plain Python: the
reference the HDBSCAN tests compare the GPU against.

Input everywhere: n rows and the forest's E edges (u, v, w) ascending by
(w, u, v), so an edge's position is its rank and the merge order.  dist(e) =
sqrt(w) when `root` (euclidean accumulators) else w; lambda(e) = 1.0 / dist(e).
m = min_cluster_size >= 2.

`sequential` is the definition itself: Kruskal's dendrogram, then the condensed
tree walked top-down.  `staged` is the decomposition the GPU runs (stages 1-4:
small subtrees by rounds of reciprocal pairs, true splits, blobs, the cluster
tree and each row's place in it), written with flat numpy passes.  Both number
the clusters the same way, which is the library's: first the leaf clusters,
ascending by their smallest row, then the clusters that split, ascending by the
rank of the edge they split at.  A cluster's parent therefore has a larger
number than the cluster.
"""
import math

import numpy as np

NONE = np.iinfo(np.int64).max


def lambdas(w, root):
    w = np.asarray(w, np.float64)
    with np.errstate(divide="ignore"):
        return 1.0 / (np.sqrt(w) if root else w)


def _find(par, x):
    while par[x] != x:
        par[x] = par[par[x]]
        x = par[x]
    return x


def dendrogram(n, u, v):
    """Kruskal in rank order.  Node i < n is row i, node n + e is edge e.
    -> (left, right, size, tops): children of every edge node (the sides of u
    and v), rows below every node, the top node of every component."""
    par = list(range(n))
    node = list(range(n))
    E = len(u)
    left, right = np.zeros(E, np.int64), np.zeros(E, np.int64)
    size = np.ones(n + E, np.int64)
    for e, (a, b) in enumerate(zip(np.asarray(u).tolist(), np.asarray(v).tolist())):
        ra, rb = _find(par, a), _find(par, b)
        if ra == rb:
            raise ValueError("the edge list has a cycle")
        left[e], right[e] = node[ra], node[rb]
        size[n + e] = size[node[ra]] + size[node[rb]]
        lo, hi = min(ra, rb), max(ra, rb)
        par[hi] = lo
        node[lo] = n + e
    tops = sorted({node[_find(par, i)] for i in range(n)})
    return left, right, size, tops


def _rows_below(node, n, left, right):
    out, stack = [], [node]
    while stack:
        x = stack.pop()
        if x < n:
            out.append(x)
        else:
            stack.append(left[x - n])
            stack.append(right[x - n])
    return out


def select(parent, stability, method="eom", allow_single=False):
    """-> (target, margin).  target[x]: the selected ancestor-or-self of
    cluster x, -1 when there is none.  margin: the smallest relative gap
    |S(C) - sum of the children's best| / max of the two over the clusters
    that have children (inf when there are none): how far the excess-of-mass
    decisions are from a tie."""
    if method not in ("eom", "leaf"):
        raise ValueError(method)
    C = len(parent)
    sole = int((np.asarray(parent) < 0).sum()) == 1
    childsum = [0.0] * C
    haschild = [False] * C
    sel = [False] * C
    margin = math.inf
    for x in range(C):
        p = int(parent[x])
        assert p == -1 or x < p < C
        ok = not (sole and p < 0 and not allow_single)
        s = float(stability[x])
        if not haschild[x]:
            sel[x], best = ok, s
        else:
            top = max(s, childsum[x])
            margin = min(margin, abs(s - childsum[x]) / top if top > 0 else 0.0)
            if method == "eom" and ok and s >= childsum[x]:
                sel[x], best = True, s
            else:
                best = childsum[x]
        if p >= 0:
            childsum[p] += best
            haschild[p] = True
    target = np.full(C, -1, np.int64)
    for x in range(C - 1, -1, -1):
        p = int(parent[x])
        if p >= 0 and target[p] >= 0:
            target[x] = target[p]
        elif sel[x]:
            target[x] = x
    return target, margin


def eom_margin(parent, stability):
    return select(parent, stability, "eom", True)[1]


def labels_of(point_cluster, point_lambda, target, lambda_max):
    """-> (labels int32, probabilities float64): a row takes the selected
    cluster of the cluster it fell out of; labels are numbered by smallest
    member row; probability = min(lambda_p, lambda_max(S)) / lambda_max(S)."""
    n = len(point_cluster)
    sel = np.full(n, -1, np.int64)
    has = point_cluster >= 0
    sel[has] = target[point_cluster[has]]
    labels = np.full(n, -1, np.int32)
    prob = np.zeros(n)
    seen = {}
    for i in np.flatnonzero(sel >= 0).tolist():
        labels[i] = seen.setdefault(int(sel[i]), len(seen))
    on = sel >= 0
    lm = lambda_max[sel[on]]
    prob[on] = np.minimum(point_lambda[on], lm) / lm
    return labels, prob


def sequential(n, u, v, w, m, root=True, method="eom", allow_single=False):
    """The top-down condensed tree of the definition.  -> dict:
      fall[n]          rank of the edge at which each row leaves its cluster, -1 noise
      splits           ascending ranks of the true splits
      point_cluster[n] the cluster each row falls out of, -1 noise
      point_lambda[n]  lambda of that edge, 0 noise
      parent, birth, death, size, count, stability, lambda_max: per cluster
      terms            per cluster: the number of summands of its stability
      target, labels, probabilities, margin: the selection"""
    assert m >= 2
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    lam = lambdas(w, root)
    left, right, size, tops = dendrogram(n, u, v)
    fall = np.full(n, -1, np.int64)
    pc = np.full(n, -1, np.int64)
    birth, parent, end, is_split = [], [], [], []

    def new(b, p):
        birth.append(b)
        parent.append(p)
        end.append(-1)
        is_split.append(False)
        return len(birth) - 1

    stack = [(t, new(0.0, -1)) for t in tops if size[t] >= m]
    while stack:
        node, c = stack.pop()
        while True:
            e = node - n
            a, b = left[e], right[e]
            big_a, big_b = size[a] >= m, size[b] >= m
            if big_a and big_b:
                end[c], is_split[c] = e, True
                stack.append((a, new(lam[e], c)))
                stack.append((b, new(lam[e], c)))
                break
            for side, big in ((a, big_a), (b, big_b)):
                if not big:
                    rows = _rows_below(side, n, left, right)
                    fall[rows] = e
                    pc[rows] = c
            if not big_a and not big_b:
                end[c] = e
                break
            node = a if big_a else b
    # the library's numbering: leaves by smallest row, then splits by rank
    K = len(birth)
    first = np.full(K, NONE, np.int64)
    np.minimum.at(first, pc[pc >= 0], np.flatnonzero(pc >= 0))
    leaf = [c for c in range(K) if not is_split[c]]
    inner = [c for c in range(K) if is_split[c]]
    order = sorted(leaf, key=lambda c: first[c]) + sorted(inner, key=lambda c: end[c])
    new_id = np.zeros(K, np.int64)
    new_id[order] = np.arange(K)
    pc[pc >= 0] = new_id[pc[pc >= 0]]
    parent = np.array([new_id[parent[c]] if parent[c] >= 0 else -1 for c in order], np.int64)
    birth = np.array([birth[c] for c in order], np.float64)
    end = np.array([end[c] for c in order], np.int64)
    is_split = np.array([is_split[c] for c in order], bool)
    death = lam[end] if K else np.zeros(0)
    point_lambda = np.where(fall >= 0, lam[np.maximum(fall, 0)] if len(lam) else 0.0, 0.0)
    count = np.bincount(pc[pc >= 0], minlength=K).astype(np.int64)
    below = count.copy()
    for x in range(K):
        if parent[x] >= 0:
            below[parent[x]] += below[x]
    stability, lambda_max = np.zeros(K), np.zeros(K)
    members = [[] for _ in range(K)]
    for i in np.flatnonzero(pc >= 0).tolist():
        members[pc[i]].append(point_lambda[i])
    for x in range(K):
        t = [lp - birth[x] for lp in members[x]]
        lm = max(members[x]) if members[x] else 0.0
        if is_split[x]:
            t.append(float(below[x] - count[x]) * (death[x] - birth[x]))
            lm = max(lm, death[x])
        assert all(z >= 0 for z in t)
        stability[x] = math.fsum(t)
        lambda_max[x] = lm
    target, margin = select(parent, stability, method, allow_single)
    labels, prob = labels_of(pc, point_lambda, target, lambda_max)
    return dict(fall=fall, splits=np.sort(end[is_split]), point_cluster=pc,
                point_lambda=point_lambda, parent=parent, birth=birth, death=death, size=below,
                count=count, stability=stability, lambda_max=lambda_max,
                terms=count + is_split, target=target, labels=labels, probabilities=prob,
                margin=margin)


def staged(n, u, v, w, m):
    """Stages 1-4 as the GPU runs them.  -> dict(fall, splits, point_cluster,
    parent, rounds): as `sequential`, rounds = stage-1 rounds run, the last,
    which merges nothing, included."""
    assert m >= 2
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    E = len(u)
    rank = np.arange(E)
    # stage 1: rounds of reciprocal pairs below m rows
    comp, csize, rounds = np.arange(n), np.ones(n, np.int64), 0
    while True:
        rounds += 1
        a, b = comp[u], comp[v]
        live = a != b
        minout = np.full(n, NONE, np.int64)
        np.minimum.at(minout, a[live], rank[live])
        np.minimum.at(minout, b[live], rank[live])
        pair = live & (minout[a] == rank) & (minout[b] == rank) & (csize[a] + csize[b] < m)
        if not pair.any():
            break
        lo, hi = np.minimum(a[pair], b[pair]), np.maximum(a[pair], b[pair])
        hook = np.arange(n)
        hook[hi] = lo
        csize[lo] += csize[hi]
        comp = hook[comp]
    f = minout[comp]
    fall = np.where(f == NONE, -1, f)
    # stage 2: true splits
    split = live & (minout[a] != rank) & (minout[b] != rank)
    srank = np.flatnonzero(split)
    # stage 3: blobs, leaves, the cluster tree
    par = list(range(n))
    for x, y in zip(u[~split].tolist(), v[~split].tolist()):
        rx, ry = _find(par, x), _find(par, y)
        par[max(rx, ry)] = min(rx, ry)
    blob = np.array([_find(par, i) for i in range(n)], np.int64)
    bsize = np.bincount(blob, minlength=n)
    leaf_rows = np.flatnonzero((blob == np.arange(n)) & (bsize >= m))
    L, T = len(leaf_rows), len(srank)
    leafid = np.full(n, -1, np.int64)
    leafid[leaf_rows] = np.arange(L)
    parent = np.full(L + T, -1, np.int64)
    noderank = np.zeros(L + T, np.int64)
    lpar, top = list(range(L)), list(range(L))
    for t, e in enumerate(srank.tolist()):
        ra, rb = _find(lpar, leafid[blob[u[e]]]), _find(lpar, leafid[blob[v[e]]])
        assert ra != rb and ra >= 0 and rb >= 0
        parent[top[ra]] = parent[top[rb]] = L + t
        noderank[L + t] = e
        lo, hi = min(ra, rb), max(ra, rb)
        lpar[hi] = lo
        top[lo] = L + t
    # stage 4: each row's cluster (a plain parent walk here)
    pc = np.full(n, -1, np.int64)
    for i in range(n):
        x = leafid[blob[i]]
        if x < 0:
            continue
        while parent[x] >= 0 and noderank[parent[x]] < f[i]:
            x = parent[x]
        pc[i] = x
    # the blobs' order is not the leaves': renumber the leaves by their smallest row
    first = np.full(L + T, NONE, np.int64)
    np.minimum.at(first, pc[pc >= 0], np.flatnonzero(pc >= 0))
    perm = np.arange(L + T)
    perm[np.argsort(first[:L], kind="stable")] = np.arange(L)
    pc[pc >= 0] = perm[pc[pc >= 0]]
    new_parent = parent.copy()
    new_parent[perm] = parent
    parent = new_parent
    return dict(fall=fall, splits=srank, point_cluster=pc, parent=parent, rounds=rounds)


def random_forest(rng, n, n_comp=1):
    """A random forest of n rows in n_comp trees under a random rank
    permutation, as sorted edges: -> (u, v, w), weights 1, 2, ... (no ties)."""
    perm = rng.permutation(n)
    edges = []
    for i in range(n_comp, n):
        # attach to an earlier row: a random recursive tree, with stretches of path
        j = perm[i - 1] if rng.random() < 0.3 else perm[rng.integers(0, i)]
        edges.append((min(perm[i], j), max(perm[i], j)))
    order = rng.permutation(len(edges))
    u = np.array([edges[k][0] for k in order], np.int32)
    v = np.array([edges[k][1] for k in order], np.int32)
    return u, v, np.arange(1, len(edges) + 1, dtype=np.float64)
