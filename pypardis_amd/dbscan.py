"""``DBSCAN`` driver — the surface of R:dbscan/dbscan.py:56-165 on MI355X.

What ``train`` does, stage by stage, against the reference:

    KDPartitioner(data, max_partitions)      R:dbscan/dbscan.py:110   GPU passes (partition.py)
    _create_neighborhoods: box.expand(2·eps)  R:dbscan/dbscan.py:136-151
    partitionBy + mapPartitions(dbscan_partition)
                                              R:dbscan/dbscan.py:116-124
    _remap_cluster_ids (+ ClusterAggregator)  R:dbscan/dbscan.py:153-165
        └── the last three fused into ONE device call, pd_train (engine.hip):
            halo records → (neighbourhood, eps-cell) sort → neighbour count /
            core flags → union-find on core–core edges → merge of the copies
            of each halo point → border attach → global labels.

The labels are the ones sklearn's ``DBSCAN(eps, min_samples).fit_predict``
gives on the whole data set (what the reference's merge intends; its literal
merge is hash-order dependent), and are independent of
``max_partitions``.
"""
from __future__ import annotations

import collections

import numpy as np
import torch
from scipy.spatial.distance import euclidean

from . import _native
from ._data import PointSet, as_points
from .partition import KDPartitioner


def dbscan_partition(iterable, params):
    """R:dbscan/dbscan.py:12-34: cluster one neighbourhood.

    :param iterable: ((key, partition), vector) records of one neighbourhood
    :param params: {'eps', 'min_samples', 'metric'}
    :return: yields (key, '%i:%i%s' % (partition, cluster_id, '' or '*'))
    Runs ``pd_cluster`` (sklearn fit_predict semantics) on the GPU.  An empty
    neighbourhood yields nothing (the reference raises IndexError, :24).
    """
    data = list(iterable)
    if not data:
        return
    (key, part), vector = data[0]
    X = np.array([v for (_, __), v in data])
    y = [k for (k, _), __ in data]
    pts = as_points(X)
    labels, core, _, _ = _native.cluster(pts.X, params['eps'], params['min_samples'],
                                         _native.metric_code(params.get('metric', 'euclidean')))
    c = labels.cpu().numpy()
    cores = core.cpu().numpy()
    for i in range(len(c)):
        flag = '' if cores[i] else '*'
        yield (y[i], '%i:%i%s' % (part, c[i], flag))


def map_cluster_id(x, broadcast_dict):
    """R:dbscan/dbscan.py:37-53 (string-label compatibility): first label of
    the group, '*' stripped; -1 if it is noise or unmapped."""
    key, cluster_id = x
    cluster_id = next(iter(cluster_id)).strip('*')
    cluster_dict = getattr(broadcast_dict, 'value', broadcast_dict)
    if '-1' not in cluster_id and cluster_id in cluster_dict:
        return key, cluster_dict[cluster_id]
    return key, -1


class _Neighborhood(object):
    """``neighbors[label]``: points inside the 2·eps-expanded box of one KD
    partition (membership computed on the GPU by pd_halo_members)."""

    def __init__(self, owner, label):
        self._owner = owner
        self.label = label

    def indices(self):
        return self._owner._members(self.label)

    def keys(self):
        return self._owner.points.key_array()[self.indices()]

    def collect(self):
        idx = self.indices()
        vecs = self._owner.points.vectors(torch.from_numpy(idx).to(self._owner.points.X.device))
        return [((k, self.label), v) for k, v in zip(self.keys().tolist(), vecs)]

    def count(self):
        return len(self.indices())

    __len__ = count


class _Neighborhoods(dict):
    def __init__(self, points, expanded, ebox=None):
        super().__init__()
        self.points = points
        self._ebox = ebox if ebox is not None else \
            np.array([expanded[L].as_array() for L in sorted(expanded)], np.float64)
        self._cache = None
        for L in sorted(expanded):
            self[L] = _Neighborhood(self, L)

    def _members(self, L):
        if self._cache is None:
            counts, members = _native.halo_members(self.points.X, self._ebox)
            m = members.cpu().numpy()
            off = np.concatenate([[0], np.cumsum(counts)])
            self._cache = [m[off[i]:off[i + 1]] for i in range(len(counts))]
        return self._cache[L]

    def iteritems(self):
        return iter(self.items())


def _partition_records(X, keys, n_parts, members, cluster, params, weight=None):
    """The reference's per-partition records (R:dbscan/dbscan.py:116-125 with
    dbscan_partition, :12-34): for each neighbourhood L (partitionBy order)
    and each of its points in input order, ``(key, 'L:c')`` or ``(key,
    'L:c*')`` — c the neighbourhood's own sklearn label of the point, '*' a
    non-core point.  members(L) -> ascending point indices of neighbourhood
    L; cluster(X_L, eps, min_samples, metric) -> (labels, core) numpy.
    weight (device fp64, one per point): each neighbourhood is clustered with
    its own points' weights, cluster(..., sample_weight=w_L)."""
    recs = []
    metric = _native.metric_code(params.get('metric', 'euclidean'))
    for L in range(n_parts):
        idx = np.asarray(members(L), np.int64)
        if not len(idx):
            continue
        sel = torch.from_numpy(idx).to(X.device)
        XL = X[sel].contiguous()
        if weight is None:
            lab, core = cluster(XL, params['eps'], params['min_samples'], metric)
        else:
            lab, core = cluster(XL, params['eps'], params['min_samples'], metric,
                                sample_weight=weight[sel].contiguous())
        recs.extend((k, '%i:%i%s' % (L, c, '' if f else '*'))
                    for k, c, f in zip(keys[idx].tolist(), np.asarray(lab).tolist(),
                                       np.asarray(core).tolist()))
    return recs


def _device_cluster(X, eps, min_samples, metric, sample_weight=None):
    lab, core, _, _ = _native.cluster(X, eps, min_samples, metric, sample_weight=sample_weight)
    return lab.cpu().numpy(), core.cpu().numpy()


class _PartitionRecords(object):
    """``DBSCAN.data`` after ``train`` (R:dbscan/dbscan.py:116-125): the
    records of the per-partition clustering (_partition_records).  Built
    lazily on first use, one pd_cluster per neighbourhood; the global labels
    never depend on it.  After a weighted train each neighbourhood is
    clustered with its points' weights (pd_cluster_weighted)."""

    def __init__(self, neighbors, params, weight=None):
        self.neighbors = neighbors
        self.params = params
        self.weight = weight
        self._recs = None

    def _build(self):
        if self._recs is None:
            nb = self.neighbors
            self._recs = _partition_records(nb.points.X, nb.points.key_array(), len(nb),
                                            lambda L: nb[L].indices(), _device_cluster,
                                            self.params, self.weight)
        return self._recs

    def collect(self):
        return list(self._build())

    def count(self):
        return sum(len(nb) for nb in self.neighbors.values())

    def take(self, k):
        return self._build()[:k]

    def __iter__(self):
        return iter(self._build())


class _ShardedPartitionRecords(_PartitionRecords):
    """``DBSCAN.data`` after a sharded train: the same records as one device
    would give for the union of every rank's slice (global input order =
    rank order), like the reference's one RDD over all executors.  The
    neighbourhoods span ranks, so ``collect()`` / ``take()`` / iteration are
    collectives (every rank calls them): the slices are all-gathered (keys and
    coordinates, the reference's ``collect`` to the driver), then each
    neighbourhood is clustered on this rank's device (``ops``: pd_halo_members
    + pd_cluster).  ``count()`` all-reduces the neighbourhood sizes of the
    local slices (a collective too)."""

    def __init__(self, points, gid_base, ebox, params, group, ops):
        self.points = points
        self.gid_base = gid_base
        self.ebox = np.ascontiguousarray(ebox, np.float64)
        self.params = params
        self.group = group
        self.ops = ops
        self._recs = None

    def _local_keys(self):
        if self.points.keys is None:
            return self.gid_base + np.arange(self.points.n, dtype=np.int64)
        return np.asarray(self.points.key_array())

    def _build(self):
        if self._recs is None:
            import torch.distributed as dist
            parts = [None] * dist.get_world_size(self.group)
            dist.all_gather_object(parts, (self._local_keys(), self.points.X.cpu().numpy()),
                                   group=self.group)
            keys = np.concatenate([p[0] for p in parts])
            X = torch.from_numpy(np.ascontiguousarray(np.concatenate([p[1] for p in parts])))
            X = X.to(self.ops.device)
            counts, members = self.ops.halo_members(X, self.ebox)
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            self._recs = _partition_records(X, keys, len(self.ebox),
                                            lambda L: members[off[L]:off[L + 1]],
                                            self.ops.cluster, self.params)
        return self._recs

    def count(self):
        import torch.distributed as dist
        counts, _ = self.ops.halo_members(self.points.X.to(self.ops.device), self.ebox)
        t = torch.tensor([int(np.sum(counts))], dtype=torch.int64)
        dist.all_reduce(t, group=self.group)
        return int(t.item())


class _Assignments(object):
    """``DBSCAN.result``: (key, cluster id) pairs sorted by key
    (``.sortByKey()``, R:dbscan/dbscan.py:162-164)."""

    def __init__(self, points, labels):
        self.points = points
        self.labels = labels

    def labels_by_key(self):
        lab = self.labels.cpu().numpy().astype(np.int64)
        keys = self.points.key_array()
        if self.points.keys is None:
            return keys, lab
        order = np.argsort(keys, kind="stable")
        return keys[order], lab[order]

    def collect(self):
        keys, lab = self.labels_by_key()
        return list(zip(keys.tolist(), lab.tolist()))

    def count(self):
        return self.points.n


class _ShardedAssignments(object):
    """``DBSCAN.result`` of a sharded train: this rank holds the (key, label)
    pairs of its input slice, like one partition of the reference's result
    RDD.  ``collect()`` / ``count()`` are collectives (every rank calls them)
    and return the whole, sorted by key (R:dbscan/dbscan.py:162-164)."""

    def __init__(self, points, labels, gid_base, n_total, group):
        self.points = points
        self.labels = labels
        self.gid_base = gid_base
        self.n_total = n_total
        self.group = group

    def local(self):
        lab = self.labels.cpu().numpy().astype(np.int64)
        if self.points.keys is None:
            return self.gid_base + np.arange(self.points.n, dtype=np.int64), lab
        return self.points.keys, lab

    def collect(self):
        import torch.distributed as dist
        keys, lab = self.local()
        parts = [None] * dist.get_world_size(self.group)
        dist.all_gather_object(parts, (keys, lab), group=self.group)
        keys = np.concatenate([p[0] for p in parts])
        lab = np.concatenate([p[1] for p in parts])
        order = np.argsort(keys, kind="stable")
        return list(zip(keys[order].tolist(), lab[order].tolist()))

    def count(self):
        return self.n_total


def _check_kdist_args(k, r_max):
    if int(k) != k or k < 1:
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    if k > _native.KDIST_MAX_K:
        raise ValueError(f"k must be <= {_native.KDIST_MAX_K}, got {k!r}")
    if not (r_max > 0) or not np.isfinite(r_max):
        raise ValueError(f"r_max must be a finite value > 0, got {r_max!r}")
    return int(k), float(r_max)


def _row_weights(sample_weight, data=None):
    """sample_weight of an index query as a 1-D float64 tensor (array, list or
    tensor, as ``DBSCAN._weights`` takes them), wherever it lives.  Where the
    number of rows of ``data`` is known without touching the device (an array
    or a tensor) the length is checked here, before any device work."""
    w = sample_weight
    if isinstance(w, torch.Tensor):
        w = w.detach()
    else:
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float64)))
    n = data.shape[0] if isinstance(data, (torch.Tensor, np.ndarray)) else None
    if w.dim() != 1 or (n is not None and w.shape[0] != n):
        raise ValueError(f"sample_weight must hold one value per row: got shape "
                         f"{tuple(w.shape)}" + ("" if n is None else f" for {n} rows"))
    return w


def _place_weights(w, X):
    """The weights beside the rows of ``X``: float64, contiguous, its device."""
    if w.shape[0] != X.shape[0]:
        raise ValueError(f"sample_weight must hold one value per row: got shape "
                         f"{tuple(w.shape)} for {X.shape[0]} rows")
    if X.shape[0] > 2**31 - 1:
        raise ValueError(f"sample_weight: {X.shape[0]} rows do not fit int32 row numbers")
    return w.to(device=X.device, dtype=torch.float64).contiguous()


def _weight_error(e):
    """An invalid weight (found on the device) and a list that would need more
    than 64 slots are the caller's ValueError."""
    return (e.code in (_native.PD_EINVAL, _native.PD_EUNSUPPORTED)
            and "sample_weight" in str(e))


def _k_distances(X, q, k, r_max, metric, squared, weight=None):
    """kdist of the rows of ``q`` against the rows of ``X`` (device tensors):
    the index over all of X is built, asked once and closed.  ``weight``: the
    rows' weights (``_place_weights``), for the weighted core distance."""
    if q.shape[1] != X.shape[1]:
        raise ValueError(f"k_distances: queries have {q.shape[1]} coordinates, the data "
                         f"{X.shape[1]}")
    if q.dtype != X.dtype:
        q = q.to(X.dtype)
    try:
        if weight is None:
            index = _native.Index.over_all(X, r_max, metric)
        else:
            index = _native.Index.over_rows(X, r_max, metric)
        try:
            if weight is None:
                acc = index.kdist(q, k)
            else:
                index.set_weights(weight)
                acc = index.kdist_weighted(q, k)
        finally:
            index.close()
    except _native.PardisError as e:
        if e.code == _native.PD_EINVAL and "NaN" in str(e):   # sklearn's ValueError
            raise ValueError(str(e)) from None
        if weight is not None and _weight_error(e):
            raise ValueError(str(e)) from None
        raise
    if squared or metric != _native.PD_EUCLIDEAN:
        return acc
    return torch.sqrt(acc)


def k_distances(data, k, r_max, metric='euclidean', queries=None, squared=False, device=None,
                sample_weight=None):
    """
    :param data: the indexed points, in any form ``DBSCAN.train`` takes
    :param k: which neighbour (1 <= k <= 64); a query that is itself a row of
        ``data`` counts itself at distance 0, as ``min_samples`` does
    :param r_max: cap of the search: only rows within ``r_max`` (the
        predicate of a train at ``eps = r_max``) are looked at
    :param metric: 'euclidean' or 'cityblock' (string or scipy callable)
    :param queries: the query points (converted to the data's dtype, as in
        ``predict``); None: the data itself
    :param squared: euclidean only: return the squared distances — the native,
        bit-reproducible accumulator — instead of their square roots
    :param sample_weight: None, or one weight per row of ``data`` (array, list
        or tensor; finite, 0 <= w <= 2**31), as ``DBSCAN.train`` takes them:
        the result is then the weighted core distance — the distance at which
        the weights of the rows, nearest first, sum to ``k`` (a query that is a
        row counts its own weight; a zero-weight row counts nothing).  With
        multiplicities it is ``k_distances`` of the repeated rows.  Fewer than
        2^31 rows; ``k`` divided by the smallest positive weight may not pass
        64 (``ValueError``)
    :return: device float64 tensor in query order: the distance to the k-th
        nearest row of ``data``, ``inf`` where fewer than k rows lie within
        ``r_max``

    The sorted result is the k-distance plot that ``eps`` is read from (k =
    ``min_samples``), the value itself the OPTICS / HDBSCAN core distance.
    Exact: the accumulator is the train's own (fp64, axis order, every product
    and sum rounded separately), so for any ``eps <= r_max`` a train with
    ``min_samples = k`` marks point i core exactly when ``k_distances(...,
    squared=True)[i] <= eps * eps`` (cityblock: ``<= eps``) — with
    ``sample_weight`` a train with the same weights, whose fixed-point sum the
    weighted distance uses.  The cost grows with the number of rows within
    ``r_max``.  Single device.
    """
    k, r_max = _check_kdist_args(k, r_max)
    metric = _native.metric_code(metric)
    w = None if sample_weight is None else _row_weights(sample_weight, data)
    X = as_points(data, device).X
    q = X if queries is None else as_points(queries, X.device).X
    return _k_distances(X, q, k, r_max, metric, squared,
                        None if w is None else _place_weights(w, X))


RadiusNeighbors = collections.namedtuple("RadiusNeighbors", ["indptr", "indices", "distances"])


def _check_radius_args(radius):
    if not (radius > 0) or not np.isfinite(radius):
        raise ValueError(f"radius must be a finite value > 0, got {radius!r}")
    return float(radius)


def _sort_rows(indptr, indices, acc):
    """Each CSR row ordered by (acc, index): three stable sorts, last key
    first.  Temporaries: the int64 row number of every entry and int64
    permutations, about 40 bytes per entry at the peak."""
    counts = indptr[1:] - indptr[:-1]
    rows = torch.repeat_interleave(torch.arange(counts.shape[0], device=indptr.device), counts)
    perm = torch.sort(indices, stable=True).indices
    perm = perm[torch.sort(acc[perm], stable=True).indices]
    perm = perm[torch.sort(rows[perm], stable=True).indices]
    return indices[perm], acc[perm]


def _radius_neighbors(X, q, radius, metric, return_distance, squared, sort_results, count_only):
    """The rows of ``X`` within ``radius`` of the rows of ``q`` (device
    tensors): the index over all of X is built, asked once and closed."""
    if q.shape[1] != X.shape[1]:
        raise ValueError(f"radius_neighbors: queries have {q.shape[1]} coordinates, the data "
                         f"{X.shape[1]}")
    if q.dtype != X.dtype:
        q = q.to(X.dtype)
    try:
        index = _native.Index.over_rows(X, radius, metric)
        try:
            indptr, indices, acc = index.radius(q, radius, return_distance or sort_results,
                                                count_only)
        finally:
            index.close()
    except _native.PardisError as e:
        if e.code == _native.PD_EINVAL and "NaN" in str(e):   # sklearn's ValueError
            raise ValueError(str(e)) from None
        raise
    if count_only:
        return indptr[1:] - indptr[:-1]
    if sort_results:
        indices, acc = _sort_rows(indptr, indices, acc)
    if not return_distance:
        acc = None
    elif not squared and metric == _native.PD_EUCLIDEAN:
        acc = torch.sqrt(acc)
    return RadiusNeighbors(indptr, indices, acc)


def radius_neighbors(data, radius, metric='euclidean', queries=None, return_distance=True,
                     squared=False, sort_results=False, count_only=False, device=None):
    """
    :param data: the indexed points, in any form ``DBSCAN.train`` takes (fewer
        than 2^31 of them)
    :param radius: the neighbourhood's radius: row x is a neighbour of query q
        under the predicate of a train at ``eps = radius`` (ties at exactly
        ``radius`` are in)
    :param metric: 'euclidean' or 'cityblock' (string or scipy callable)
    :param queries: the query points (converted to the data's dtype, as in
        ``predict``); None: the data itself, and every point is then its own
        neighbour at distance 0
    :param return_distance: also return each neighbour's distance
    :param squared: euclidean only: return the squared distances — the native,
        bit-reproducible accumulator — instead of their square roots
    :param sort_results: order each query's neighbours by (distance, index)
        with torch sorts afterwards; needs the distances and about 40 bytes of
        temporaries per pair.  Otherwise the order inside a row is unspecified
        (it is reproducible for a given data set and call)
    :param count_only: return only the int64 device tensor of the neighbour
        counts per query; nothing per pair is allocated or written
    :return: ``RadiusNeighbors(indptr, indices, distances)`` of device tensors,
        the eps-graph in CSR form in query order: the neighbours of query q are
        ``indices[indptr[q]:indptr[q + 1]]`` (int32 row numbers of ``data``;
        ``indptr`` int64), ``distances`` (float64) alongside, None when not
        asked for.  ``scipy.sparse.csr_matrix((distances, indices, indptr))``
        after ``.cpu()`` is what ``sklearn.cluster.DBSCAN(metric=
        'precomputed')`` takes.

    Exact: the accumulator and the test are the train's own (fp64, axis order,
    every product and sum rounded separately, ``<= radius * radius``), so the
    rows with at least ``min_samples`` neighbours are a train's core points at
    ``eps = radius``, and DBSCAN's labels follow from the graph alone.  Time
    and memory grow with the number of pairs (12 bytes each, 4 without the
    distances).  Single device.
    """
    radius = _check_radius_args(radius)
    metric = _native.metric_code(metric)
    X = as_points(data, device).X
    q = X if queries is None else as_points(queries, X.device).X
    return _radius_neighbors(X, q, radius, metric, return_distance, squared, sort_results,
                             count_only)


KNeighbors = collections.namedtuple("KNeighbors", ["indices", "distances"])


def _kneighbors(X, q, k, r_max, metric, return_distance, squared):
    """The k nearest rows of ``X`` within ``r_max`` of the rows of ``q``
    (device tensors): the index over all of X is built, asked once and
    closed."""
    if q.shape[1] != X.shape[1]:
        raise ValueError(f"kneighbors: queries have {q.shape[1]} coordinates, the data "
                         f"{X.shape[1]}")
    if q.dtype != X.dtype:
        q = q.to(X.dtype)
    try:
        index = _native.Index.over_rows(X, r_max, metric)
        try:
            indices, acc = index.kneighbors(q, k, return_distance)
        finally:
            index.close()
    except _native.PardisError as e:
        if e.code == _native.PD_EINVAL and "NaN" in str(e):   # sklearn's ValueError
            raise ValueError(str(e)) from None
        raise
    if return_distance and not squared and metric == _native.PD_EUCLIDEAN:
        acc = torch.sqrt(acc)
    return KNeighbors(indices, acc)


def kneighbors(data, k, r_max, metric='euclidean', queries=None, return_distance=True,
               squared=False, device=None):
    """
    :param data: the indexed points, in any form ``DBSCAN.train`` takes (fewer
        than 2^31 of them)
    :param k: how many neighbours (1 <= k <= 64).  A query that is itself a
        row of ``data`` finds itself first, at distance 0, as everywhere else
        in this API: for sklearn's ``kneighbors(X=None)``, which leaves the
        point itself out, ask for k + 1 and drop column 0
    :param r_max: cap of the search: only rows within ``r_max`` (the
        predicate of a train at ``eps = r_max``, ties at exactly ``r_max``
        in) are looked at
    :param metric: 'euclidean' or 'cityblock' (string or scipy callable)
    :param queries: the query points (converted to the data's dtype, as in
        ``predict``); None: the data itself
    :param return_distance: also return each neighbour's distance
    :param squared: euclidean only: return the squared distances — the native,
        bit-reproducible accumulator — instead of their square roots
    :return: ``KNeighbors(indices, distances)`` of device tensors of shape
        (m, k) in query order: int32 row numbers of ``data`` and float64
        distances (None when not asked for).  Each row is ordered by
        (distance, row number) ascending: among equally distant rows the
        smaller row number wins and comes first, duplicates each appear.  A
        query with fewer than k rows within ``r_max`` has its trailing slots
        at ``-1`` and ``inf``

    Exact: the accumulator is the train's own (fp64, axis order, every product
    and sum rounded separately) and the order is total, so the result is
    bit-reproducible and does not depend on the order of the rows beyond the
    row numbers themselves.  Column k - 1 of the squared distances is
    ``k_distances(data, k, r_max, squared=True)``.  The cost grows with the
    number of rows within ``r_max``; 12 bytes per slot are written (4 without
    the distances).  Single device.
    """
    k, r_max = _check_kdist_args(k, r_max)
    metric = _native.metric_code(metric)
    X = as_points(data, device).X
    q = X if queries is None else as_points(queries, X.device).X
    return _kneighbors(X, q, k, r_max, metric, return_distance, squared)


class ReachabilityForest(collections.namedtuple(
        "ReachabilityForest", ["u", "v", "distances", "core_distances"])):
    """What ``mutual_reachability_forest`` returns: the four device tensors,
    and beside them what ``dbscan_labels`` needs to cut the forest: ``r_max``,
    ``metric``, ``squared`` and the native accumulators (``accumulators``,
    ``core_accumulators``: the distances before any square root).
    ``sample_weight``: None, or the float64 device tensor of the rows' weights
    the forest was built with."""

    def __new__(cls, u, v, acc, core_acc, r_max, metric, squared, sample_weight=None):
        root = not squared and metric == _native.PD_EUCLIDEAN
        self = super().__new__(cls, u, v, torch.sqrt(acc) if root else acc,
                               torch.sqrt(core_acc) if root else core_acc)
        self.accumulators = acc
        self.core_accumulators = core_acc
        self.r_max = float(r_max)
        self.metric = metric
        self.squared = bool(squared)
        self.sample_weight = sample_weight
        return self


def _mreach_forest(X, k, r_max, metric, squared, weight=None):
    """The forest of the rows of ``X`` (a device tensor): the index over all
    rows is built, asked once and closed.  ``weight``: the rows' weights
    (``_place_weights``), for the forest over the weighted core distances."""
    if X.shape[1] > 4:
        raise ValueError(f"mutual_reachability_forest: d = {X.shape[1]} is not supported: the "
                         "forest needs the cell grid of d <= 4")
    try:
        index = _native.Index.over_rows(X, r_max, metric)
        try:
            if weight is not None:
                index.set_weights(weight)
            u, v, acc, cd, _ = index.mreach_forest(k, weighted=weight is not None)
        finally:
            index.close()
    except _native.PardisError as e:
        if e.code == _native.PD_EINVAL and "NaN" in str(e):   # sklearn's ValueError
            raise ValueError(str(e)) from None
        if weight is not None and _weight_error(e):
            raise ValueError(str(e)) from None
        raise
    return ReachabilityForest(u, v, acc, cd, r_max, metric, squared, weight)


def mutual_reachability_forest(data, min_samples, r_max, metric='euclidean', squared=False,
                               device=None, sample_weight=None):
    """
    :param data: the points, in any form ``DBSCAN.train`` takes (d <= 4, fewer
        than 2^31 of them)
    :param min_samples: k of the core distance (1 <= k <= 64), the point itself
        included, as in ``DBSCAN``
    :param r_max: cap: the forest spans the DBSCAN* graph at ``eps = r_max``
    :param metric: 'euclidean' or 'cityblock' (string or scipy callable)
    :param squared: euclidean only: return the squared distances — the native,
        bit-reproducible accumulator — instead of their square roots
    :param sample_weight: None, or one weight per row, as ``k_distances`` takes
        them: the core distances are then the weighted ones, everything else
        is unchanged
    :return: ``ReachabilityForest(u, v, distances, core_distances)`` of device
        tensors: int32 ``u < v`` and float64 ``distances`` of the E edges,
        ascending by (distance, u, v), and float64[n] ``core_distances``
        (``k_distances(data, min_samples, r_max)``; ``inf``: fewer than
        ``min_samples`` rows within ``r_max``)

    The mutual-reachability distance of rows i and j is ``max(dist(i, j),
    core(i), core(j))``.  The edges are the minimum spanning forest of the pairs
    at which it is ``<= r_max`` — unique, because ties are broken by (u, v), so
    the result is one defined list and does not depend on the order of the
    rows beyond their numbers.  E = n minus the number of connected components
    (isolated rows included).  The list is the single-linkage merge order of
    HDBSCAN's hierarchy, and for every ``eps <= r_max`` its prefix with
    ``distance <= eps`` is the clustering of ``DBSCAN(eps, min_samples)`` on
    the core points: see ``dbscan_labels``.  With ``sample_weight`` that holds
    for ``DBSCAN(eps, min_samples).train(data, sample_weight=...)``; on distinct
    rows with their multiplicities the forest is the one of the repeated rows
    without the edges that tie a row's copies together (each at the row's core
    distance), so multiplicities of ``min_samples`` or more give no edge of
    distance 0.  Single device.
    """
    k, r_max = _check_kdist_args(min_samples, r_max)
    metric = _native.metric_code(metric)
    w = None if sample_weight is None else _row_weights(sample_weight, data)
    X = as_points(data, device).X
    return _mreach_forest(X, k, r_max, metric, squared,
                          None if w is None else _place_weights(w, X))


def dbscan_labels(forest, eps, squared=False):
    """
    :param forest: a ``ReachabilityForest``
    :param eps: the radius of the cut, ``<= forest.r_max``
    :param squared: euclidean only: ``eps`` is the squared radius, the bound on
        the accumulator itself
    :return: device int32[n]: on the rows that are core at ``(eps,
        min_samples)`` the ``labels_`` of ``DBSCAN(eps, min_samples).train``
        — the components of the forest's edges within ``eps``, numbered by
        smallest member row —, -1 on every other row (DBSCAN*: border points
        are not attached; ``predict`` on the cut's cores gives them)
    """
    eps = float(eps)
    euclid = forest.metric == _native.PD_EUCLIDEAN
    if not (eps > 0) or not np.isfinite(eps):
        raise ValueError(f"eps must be a finite value > 0, got {eps!r}")
    cap = forest.r_max * forest.r_max if euclid else forest.r_max
    t = eps if (squared or not euclid) else eps * eps
    if t > cap:
        raise ValueError(f"eps = {eps!r} exceeds the forest's r_max = {forest.r_max!r}: it holds "
                         "only the edges within r_max")
    acc, cd = forest.accumulators, forest.core_accumulators
    bound = torch.tensor([t], dtype=torch.float64, device=acc.device)
    n_prefix = int(torch.searchsorted(acc, bound, right=True)[0])
    labels, _ = _native.forest_labels(forest.u, forest.v, n_prefix, cd <= t)
    return labels


class CondensedTree(collections.namedtuple(
        "CondensedTree", ["parent", "birth_lambda", "death_lambda", "size", "stability",
                          "lambda_max", "point_cluster", "point_lambda"])):
    """What ``condensed_tree`` returns.  The six per-cluster arrays are HOST
    numpy arrays (at most 2 * (n // min_cluster_size) entries: the selection
    runs over them on the host); ``point_cluster`` (int32, -1 noise) and
    ``point_lambda`` (float64) are device tensors of one entry per row.
    ``min_cluster_size`` and ``rounds`` (the small-subtree rounds run) ride
    along as attributes."""

    def __new__(cls, raw, min_cluster_size):
        self = super().__new__(cls, raw["parent"], raw["birth"], raw["death"], raw["size"],
                               raw["stability"], raw["lambda_max"], raw["point_cluster"],
                               raw["point_lambda"])
        self.min_cluster_size = int(min_cluster_size)
        self.rounds = raw["rounds"]
        self.stage_ms = raw.get("stage_ms")
        return self


def _check_min_cluster_size(m):
    if int(m) != m or m < 2:
        raise ValueError(f"min_cluster_size must be an integer >= 2, got {m!r}")
    return int(m)


def condensed_tree(forest, min_cluster_size, timings=False):
    """
    :param forest: a ``ReachabilityForest``
    :param min_cluster_size: m >= 2: a side of a merge with fewer rows falls out
        of its cluster instead of splitting it
    :return: ``CondensedTree(parent, birth_lambda, death_lambda, size, stability,
        lambda_max, point_cluster, point_lambda)``: HDBSCAN's condensed tree
        with lambda = 1 / distance.  Clusters are numbered leaves first
        (ascending by smallest row), then the clusters that split (in merge
        order), so ``parent[x] > x``, or -1 for a top-level cluster: a
        component of the forest with at least m rows, born at lambda 0.
        ``point_cluster[p]`` is the cluster row p falls out of, at
        ``point_lambda[p]``; -1 for noise.

    The forest's edge order (distance, u, v) is the merge order, ties included,
    so the tree is one defined, bit-reproducible result; another
    implementation may break tied merges differently.  An edge of distance 0
    (``min_samples`` or more identical rows) makes lambda infinite and raises
    ``ValueError``: deduplicate the rows.  A forest built with
    ``sample_weight`` raises ``ValueError`` too: ``mutual_reachability_forest``
    takes the distinct rows with their multiplicities and ``dbscan_labels`` cuts
    that forest, but row weights in the condensed tree are not supported yet (a
    cluster's size would have to be its rows' weight).  Single device.
    """
    m = _check_min_cluster_size(min_cluster_size)
    if getattr(forest, "sample_weight", None) is not None:
        raise ValueError("condensed_tree: the forest was built with sample_weight; row weights "
                         "in the condensed tree are not supported yet (dbscan_labels cuts a "
                         "weighted forest)")
    n = forest.core_accumulators.shape[0]
    try:
        raw = _native.forest_condense(n, forest.u, forest.v, forest.accumulators,
                                      forest.metric == _native.PD_EUCLIDEAN, m, timings=timings)
    except _native.PardisError as e:
        if e.code == _native.PD_EINVAL and "weight 0" in str(e):
            raise ValueError(str(e)) from None
        raise
    return CondensedTree(raw, m)


def hdbscan_labels(forest, min_cluster_size, cluster_selection_method='eom',
                   allow_single_cluster=False, return_tree=False):
    """
    :param forest: a ``ReachabilityForest``
    :param min_cluster_size: as ``condensed_tree``
    :param cluster_selection_method: 'eom' (excess of mass: a cluster is kept
        when its stability is at least the sum of its children's best) or
        'leaf' (every leaf of the condensed tree)
    :param allow_single_cluster: let the one top-level cluster of a connected
        forest be selected (sklearn's rule); several top-level clusters are
        ordinary candidates either way
    :return: ``(labels, probabilities)``, with ``return_tree`` also the
        ``CondensedTree``: device int32 labels, numbered by smallest member
        row, -1 for noise, and float64 ``min(lambda_p, lambda_max(S)) /
        lambda_max(S)``, 0 for noise
    """
    if cluster_selection_method not in _native.SELECT_METHODS:
        raise ValueError(f"cluster_selection_method {cluster_selection_method!r}: 'eom' or 'leaf'")
    tree = condensed_tree(forest, min_cluster_size)
    target = _native.condensed_select(tree.parent, tree.stability, cluster_selection_method,
                                      allow_single_cluster)
    labels, prob, _ = _native.condensed_labels(tree.point_cluster, tree.point_lambda, target,
                                               tree.lambda_max)
    return (labels, prob, tree) if return_tree else (labels, prob)


def _hdbscan(X, m, min_samples, r_max, metric, method, allow_single, return_tree):
    m = _check_min_cluster_size(m)
    if method not in _native.SELECT_METHODS:
        raise ValueError(f"cluster_selection_method {method!r}: 'eom' or 'leaf'")
    k = min(m, _native.KDIST_MAX_K) if min_samples is None else min_samples
    k, r_max = _check_kdist_args(k, r_max)
    forest = _mreach_forest(X, k, r_max, metric, True)
    return hdbscan_labels(forest, m, method, allow_single, return_tree)


def hdbscan(data, min_cluster_size, min_samples=None, r_max=None, metric='euclidean',
            cluster_selection_method='eom', allow_single_cluster=False, return_tree=False,
            device=None):
    """
    :param data: the points, in any form ``DBSCAN.train`` takes (d <= 4)
    :param min_cluster_size: m >= 2
    :param min_samples: k of the core distance, the point itself included;
        default ``min_cluster_size``, capped at 64
    :param r_max: required: the cap of the forest; pairs further apart count as
        infinitely far, so each component of the DBSCAN* graph at ``r_max`` is
        clustered on its own
    :return: as ``hdbscan_labels``

    ``mutual_reachability_forest`` and ``hdbscan_labels`` in one call.
    """
    if r_max is None:
        raise ValueError("hdbscan needs r_max, the cap of the mutual-reachability forest")
    X = as_points(data, device).X
    return _hdbscan(X, min_cluster_size, min_samples, r_max, _native.metric_code(metric),
                    cluster_selection_method, allow_single_cluster, return_tree)


class DBSCAN(object):
    """
    :eps: nearest neighbor radius
    :min_samples: minimum number of samples within radius eps
    :metric: distance metric (euclidean or cityblock, string or scipy callable)
    :max_partitions: maximum number of partitions used by KDPartitioner
    :data: before ``train`` None; after it the reference's per-partition
        records ``(key, 'L:c[*]')`` as an RDD-like object (``collect``,
        ``count``, ``take``, iteration; R:dbscan/dbscan.py:116-125) — after a
        sharded train the same records over all ranks, its calls collectives
    :result: (key, cluster label) pairs, sorted by key, via ``collect()``
    :bounding_boxes: label -> BoundingBox of each KD partition
    :expanded_boxes: label -> BoundingBox grown by 2·eps
    :neighbors: label -> points inside the expanded box
    :cluster_dict: kept for API parity; the reference never assigns it

    MI355X additions: ``labels_`` (device int32, input order),
    ``core_sample_mask_`` (device uint8), ``core_sample_indices_`` (device
    int64, ascending), ``n_clusters_``; ``predict(points)`` assigns new
    points to the trained clusters, ``fit_predict(data)`` is ``train`` then
    ``labels_``; ``k_distances()`` gives each point's distance to its k-th
    nearest neighbour (the k-distance plot ``eps`` is read from),
    ``radius_neighbors()`` the eps-graph itself in CSR form, ``kneighbors()``
    each point's k nearest points.

    ``sample_weight`` (``train`` / ``fit_predict``; sklearn's ``fit``
    argument): one weight per point; a point is core when the weights of the
    points within ``eps`` of it, itself included, sum to ``min_samples`` or
    more — e.g. multiplicities of deduplicated data.  The sum is taken in
    fixed point, ``W = llrint(w * 2**20)`` (round half to even), core iff
    ``sum W >= min_samples * 2**20``: it does not depend on the order of
    summation or on ``max_partitions``, and equals sklearn's answer exactly
    whenever every weight is a multiple of 2**-20 (integers, dyadic
    fractions); for other weights the core flag can differ from sklearn's
    only where sklearn's own float sum lies within k * 2**-21 of
    ``min_samples`` (k neighbours).  A zero-weight point adds nothing to
    others but can itself be core.  Limits: weights must be finite and in
    [0, 2**31] — negative weights raise (sklearn allows them, but a partial
    neighbourhood could then out-sum the full one, which the halo merge and
    the sweep's early exit rely on never happening); d <= 4; one device (no
    ``group=``, no ``n_gpus`` > 1).

    ``kd_sums``: KD moment summation.  'exact' (default): correctly rounded,
    order-independent double-double sums — the same boxes on one device or
    many; 'sequential': the reference's left-to-right fold, bit-identical to
    its boxes (on C0 a split the reference decides by round-off differs
    otherwise), single device only.  Never changes the labels.

    Multi-GPU (the reference's fan-out over executors, R:dbscan/dbscan.py:
    104-126) is opt-in:
      * ``group=`` a torch.distributed process group (or ``'world'``), one
        process per GPU (e.g. torchrun): ``train(slice)`` clusters the union
        of every rank's slice; each rank passes its own slice and gets
        ``labels_`` / ``core_sample_mask_`` for it (input order), the global
        ``n_clusters_``, the same ``bounding_boxes`` / ``expanded_boxes``,
        ``neighbors`` over its slice, and a ``result`` whose ``collect()`` (a
        collective) returns every (key, label).  Keys of array input are
        global indices (rank offset + row).  Collectives run on RCCL through
        libpardis (pd_comm_*) for an "nccl" group;
      * ``n_gpus=N > 1`` without a group: this process drives GPUs 0..N-1
        itself (one thread per device, pd_comm_init_all), the input split by
        index;
      * neither: one device — also inside an initialised process group (each
        rank clusters its own data, the reference's single-driver behaviour).
    ``device``: where the points go (default: the current CUDA device).
    ``keep_shard_records``: a sharded train keeps the records each rank owns
    (``shard.gid`` / ``shard.labels`` / ``shard.core``: diagnostics, ~13 B
    of HBM per received record); off by default.
    """

    def __init__(self, eps=0.5, min_samples=5, metric=euclidean, max_partitions=None,
                 kd_sums='exact', n_gpus=None, device=None, group=None, keep_shard_records=False):
        self.eps = eps
        self.keep_shard_records = keep_shard_records
        self.kd_sums = kd_sums
        self.n_gpus = n_gpus
        self.device = device
        self.group = group
        self.min_samples = int(min_samples)
        self.metric = metric
        self.max_partitions = max_partitions
        self.data = None
        self.result = None
        self.bounding_boxes = None
        self.expanded_boxes = None
        self.neighbors = None
        self.cluster_dict = None
        self.labels_ = None
        self.core_sample_mask_ = None
        self.n_clusters_ = None
        self.sample_weight_ = None   # the last train's weights (device float64), or None
        self.partitioner = None
        self.shard = None
        self._points = None      # the training points (predict's index is built from them)
        self._trained = None     # (eps, metric code) of the last train
        self._index = None       # _native.Index, built by the first predict
        self._group_trained = False

    def _process_group(self):
        """The process group of an opt-in sharded train: ``group=`` (a
        torch.distributed group, or 'world'), else None — a rank of a
        torchrun / DDP job that does not ask for it clusters its own data on
        its own device, as the reference's ``train`` would."""
        if self.group is None:
            return None
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise ValueError("group= needs an initialised torch.distributed process group")
        group = dist.group.WORLD if isinstance(self.group, str) and self.group == "world" \
            else self.group
        if self.n_gpus not in (None, dist.get_world_size(group)):
            raise ValueError(f"n_gpus={self.n_gpus} inside a process group of "
                             f"{dist.get_world_size(group)} ranks")
        return group

    def _weights(self, sample_weight, points):
        """sample_weight as a float64 tensor on the points' device, one value
        per point (the range check runs on the device, inside the train)."""
        w = sample_weight
        if isinstance(w, torch.Tensor):
            w = w.detach()
        else:
            w = torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float64)))
        if w.dim() != 1 or w.shape[0] != points.n:
            raise ValueError(f"sample_weight must hold one value per point: got shape "
                             f"{tuple(w.shape)} for {points.n} points")
        if points.d > 4:
            raise ValueError("sample_weight is supported for d <= 4 only (the dense d > 4 "
                             "path counts neighbours unweighted)")
        return w.to(device=points.X.device, dtype=torch.float64).contiguous()

    def train(self, data, sample_weight=None):
        """
        :param data: RDD-like / iterable of (key, vector), or (n, d) array/tensor
        :param sample_weight: None, or one weight per point of ``data`` in the
            order given (array, list or tensor; finite, 0 <= w <= 2**31): a
            point is core when the weights within ``eps`` of it sum to
            ``min_samples`` or more (class docstring).  Single device, d <= 4.
        Train the model (R:dbscan/dbscan.py:104-126).
        """
        if not (self.eps > 0):
            raise ValueError("eps must be > 0")
        if self.min_samples < 1:
            raise ValueError("min_samples must be >= 1")
        metric = _native.metric_code(self.metric)
        if sample_weight is not None:
            if self.group is not None:
                raise ValueError("sample_weight is single-device: not supported with group=")
            if self.n_gpus is not None and int(self.n_gpus) > 1:
                raise ValueError("sample_weight is single-device: not supported with n_gpus > 1")
        self._drop_index()
        self._points = None
        self.sample_weight_ = None
        self._trained = (float(self.eps), metric)
        group = self._process_group()
        self._group_trained = group is not None
        if group is not None:
            return self._train_group(data, group, metric)
        if self.n_gpus is not None and int(self.n_gpus) > 1:
            return self._train_devices(data, metric)
        points = as_points(data, self.device)
        weight = None if sample_weight is None else self._weights(sample_weight, points)
        parts = KDPartitioner(points, self.max_partitions, sums=self.kd_sums)
        self.partitioner = parts
        self.bounding_boxes = parts.bounding_boxes
        self.expanded_boxes = {L: box.expand(2 * self.eps)
                               for L, box in sorted(parts.bounding_boxes.items())}
        ebox = np.array([self.expanded_boxes[L].as_array() for L in sorted(self.expanded_boxes)],
                        np.float64)
        self.neighbors = _Neighborhoods(points, self.expanded_boxes, ebox)
        # the reference's self.data after train: the per-partition records
        self.data = _PartitionRecords(self.neighbors, {'eps': self.eps,
                                                       'min_samples': self.min_samples,
                                                       'metric': self.metric}, weight)
        lo, hi = parts.data_box
        tree = parts.split_tree() if len(ebox) > 1 and points.d <= 4 else None
        try:
            if tree is not None:
                # the owner of each point is found by replaying the KD splits in
                # the halo pass (no owner array, no final split pass)
                labels, core, _, ncl = _native.train_tree(points.X, self.eps, self.min_samples,
                                                          metric, ebox, tree,
                                                          data_box=np.stack([lo, hi]),
                                                          sample_weight=weight)
            else:
                owner = parts.labels if len(ebox) > 1 else None
                labels, core, _, ncl = _native.train(points.X, self.eps, self.min_samples, metric,
                                                     ebox, owner=owner,
                                                     data_box=np.stack([lo, hi]),
                                                     sample_weight=weight)
        except _native.PardisError as e:
            # (an invalid weight is found on the device: sklearn's ValueError)
            if weight is not None and e.code == _native.PD_EINVAL and "sample_weight" in str(e):
                raise ValueError(str(e)) from None
            raise
        self.labels_ = labels
        self.core_sample_mask_ = core
        self.n_clusters_ = ncl
        self.sample_weight_ = weight
        self.result = _Assignments(points, labels)
        self._points = points
        return self

    # ------------------------------------------------------------ assignment
    def _drop_index(self):
        index, self._index = self._index, None
        if index is not None:
            index.close()

    @property
    def core_sample_indices_(self):
        """sklearn's attribute: indices of the core points, ascending (device
        int64) — the core list of predict's index."""
        if self.core_sample_mask_ is None:
            return None
        return torch.nonzero(self.core_sample_mask_).flatten()

    def fit_predict(self, data, sample_weight=None):
        """``train(data, sample_weight)``, then ``labels_`` (device int32,
        input order)."""
        return self.train(data, sample_weight).labels_

    def predict(self, data):
        """
        :param data: new points, in any form ``train`` takes
        :return: device int32 tensor in the order of ``data``: for each point
            the smallest label among the trained core points within ``eps``
            of it, -1 if there is none

        The distance test is the train's own (exact fp64 predicate) and the
        minimum is its border rule, so ``predict(X_train)`` equals ``labels_``
        — core, border and noise points — and the answer does not depend on
        ``max_partitions`` or the order of the queries.  Queries are
        converted to the dtype of the training points (float64 queries of a
        float32 model are rounded to float32 first).  A NaN or infinite
        coordinate raises, as in ``train``.

        The device index over the core points (pd_index_build) is built by
        the first call from the stored training points, ``core_sample_mask_``
        and ``labels_``, kept on the model, and dropped by the next ``train``.
        After an ``n_gpus=N`` train the points and labels are on one device
        and this works as after a single-device train; after a ``group=``
        train each rank holds only its slice, and predict raises.
        """
        if self.labels_ is None or self._trained is None:
            raise ValueError("predict before train: the model has no clusters to assign to")
        if self._group_trained:
            raise ValueError("predict after a group= train is not supported: each rank holds "
                             "only its slice of the points and labels (train with n_gpus=, or "
                             "on one device, to predict)")
        X = self._points.X
        q = as_points(data, X.device).X
        if q.shape[1] != X.shape[1]:
            raise ValueError(f"predict: points have {q.shape[1]} coordinates, the model was "
                             f"trained on {X.shape[1]}")
        if q.dtype != X.dtype:
            q = q.to(X.dtype)
        if self._index is None:
            eps, metric = self._trained
            self._index = _native.Index(X, self.core_sample_mask_, self.labels_, eps, metric)
        return self._index.query(q)

    def _query_weights(self, sample_weight, data, who):
        """An explicit ``sample_weight=`` of a model query: it belongs to
        ``data``, which must be given and is then the indexed set."""
        if sample_weight is None:
            return None
        if data is None:
            raise ValueError(f"{who}: sample_weight needs data (its rows are what the weights "
                             "belong to); after a weighted train the train's weights are used "
                             "when neither is given")
        return _row_weights(sample_weight, data)

    def k_distances(self, data=None, k=None, r_max=None, squared=False, sample_weight=None):
        """
        :param data: query points, in any form ``train`` takes; None: the
            training points against themselves
        :param k: default ``min_samples``
        :param r_max: default ``eps``
        :param squared: as the module-level ``k_distances``
        :param sample_weight: one weight per row of ``data`` (which is then
            required, and is the indexed set and the queries); None: after a
            train with ``sample_weight`` the train's weights (``sample_weight_``)
            beside the training points, else unweighted
        :return: as ``k_distances(points, k, r_max, metric)``: device float64,
            the distance of each query to its k-th nearest point (itself
            included), ``inf`` beyond ``r_max``

        After a train the indexed set is the training points, and with the
        defaults ``core_sample_mask_ == (k_distances() <= eps)`` up to the
        rounding of the square root (exactly with ``squared=True`` against
        ``eps * eps``) — also after ``train(..., sample_weight=w)``, whose
        weights the indexed training points then carry: the result is the
        weighted core distance, for the training points and for other
        ``data`` alike.  Before any train ``data`` is required and is both the
        indexed set and the queries.  After a ``group=`` train each rank holds
        only its slice, so ``data=None`` raises; a given ``data`` is then
        answered against itself.  The index is built and closed per call.
        """
        k, r_max = _check_kdist_args(self.min_samples if k is None else k,
                                     self.eps if r_max is None else r_max)
        metric = _native.metric_code(self.metric)
        w = self._query_weights(sample_weight, data, "k_distances")
        have = self._points is not None and not self._group_trained
        if w is not None:
            X = q = as_points(data, self.device).X
            weight = _place_weights(w, X)
        elif data is None:
            if self._group_trained:
                raise ValueError("k_distances() after a group= train needs data: each rank "
                                 "holds only its slice of the points")
            if not have:
                raise ValueError("k_distances before train needs data")
            X = q = self._points.X
            weight = self.sample_weight_
        elif have:
            X = self._points.X
            q = as_points(data, X.device).X
            weight = self.sample_weight_
        else:
            X = q = as_points(data, self.device).X
            weight = None
        return _k_distances(X, q, k, r_max, metric, squared, weight)

    def kneighbors(self, data=None, k=None, r_max=None, return_distance=True, squared=False):
        """
        :param data: query points, in any form ``train`` takes; None: the
            training points against themselves
        :param k: default ``min_samples``
        :param r_max: default ``eps``
        :return: as the module-level ``kneighbors(points, k, r_max, metric,
            ...)``, whose other parameters these are: ``KNeighbors(indices,
            distances)``, (m, k) device tensors, each row ordered by
            (distance, row number), ``-1`` / ``inf`` where fewer than k points
            lie within ``r_max``

        A query that is a training point finds itself first, at distance 0
        (for sklearn's ``kneighbors(X=None)`` ask for k + 1 and drop column
        0).  After a train the indexed set is the training points, and with
        the defaults ``core_sample_mask_ == (indices[:, -1] >= 0)``.  Before
        any train ``data`` is required and is both the indexed set and the
        queries.  After a ``group=`` train each rank holds only its slice, so
        ``data=None`` raises; a given ``data`` is then answered against
        itself.  The index is built and closed per call.  Unweighted, also
        after a train with ``sample_weight`` (the identity above then holds
        for ``k_distances()`` only).
        """
        k, r_max = _check_kdist_args(self.min_samples if k is None else k,
                                     self.eps if r_max is None else r_max)
        metric = _native.metric_code(self.metric)
        have = self._points is not None and not self._group_trained
        if data is None:
            if self._group_trained:
                raise ValueError("kneighbors() after a group= train needs data: each rank "
                                 "holds only its slice of the points")
            if not have:
                raise ValueError("kneighbors before train needs data")
            X = q = self._points.X
        elif have:
            X = self._points.X
            q = as_points(data, X.device).X
        else:
            X = q = as_points(data, self.device).X
        return _kneighbors(X, q, k, r_max, metric, return_distance, squared)

    def mutual_reachability_forest(self, data=None, min_samples=None, r_max=None, squared=False,
                                   sample_weight=None):
        """
        :param data: the points, in any form ``train`` takes; None: the
            training points
        :param min_samples: default the model's ``min_samples``
        :param r_max: default ``eps``
        :param squared: as the module-level ``mutual_reachability_forest``
        :param sample_weight: one weight per row of ``data`` (which is then
            required); None: with ``data=None`` after a train with
            ``sample_weight`` the train's weights, else unweighted
        :return: as ``mutual_reachability_forest(points, min_samples, r_max,
            metric)``: ``ReachabilityForest(u, v, distances, core_distances)``

        After a train, with the defaults, ``dbscan_labels(forest, eps)`` equals
        ``labels_`` on the core rows and is -1 elsewhere, and every smaller
        ``eps`` is another cut of the same forest, with no retrain — also after
        ``train(..., sample_weight=w)``: the forest is then built on the weighted
        core distances (``forest.sample_weight`` holds the weights).  Before any
        train ``data`` is required.  After a ``group=`` train each rank holds
        only its slice, so ``data=None`` raises; given ``data`` is answered on
        its own.  The index is built and closed per call.
        """
        k, r_max = _check_kdist_args(self.min_samples if min_samples is None else min_samples,
                                     self.eps if r_max is None else r_max)
        metric = _native.metric_code(self.metric)
        w = self._query_weights(sample_weight, data, "mutual_reachability_forest")
        weight = None
        if data is None:
            if self._group_trained:
                raise ValueError("mutual_reachability_forest() after a group= train needs data: "
                                 "each rank holds only its slice of the points")
            if self._points is None:
                raise ValueError("mutual_reachability_forest before train needs data")
            X = self._points.X
            weight = self.sample_weight_
        else:
            X = as_points(data, self.device).X
            if w is not None:
                weight = _place_weights(w, X)
        return _mreach_forest(X, k, r_max, metric, squared, weight)

    def hdbscan(self, min_cluster_size, data=None, min_samples=None, r_max=None,
                cluster_selection_method='eom', allow_single_cluster=False, return_tree=False):
        """
        :param min_cluster_size: m >= 2
        :param data: the points, in any form ``train`` takes; None: the
            training points
        :param min_samples: default ``min_cluster_size``, capped at 64 (not the
            model's: HDBSCAN's convention)
        :param r_max: default ``eps``
        :return: as the module-level ``hdbscan(points, min_cluster_size,
            min_samples, r_max, metric, ...)``: ``(labels, probabilities)``,
            with ``return_tree`` also the ``CondensedTree``

        The rules for ``data`` are ``mutual_reachability_forest``'s: before any
        train, and after a ``group=`` train, it is required.  Unweighted, also
        after a train with ``sample_weight``: every row counts once (row
        weights in the condensed tree are not supported yet).
        """
        metric = _native.metric_code(self.metric)
        if data is None:
            if self._group_trained:
                raise ValueError("hdbscan() after a group= train needs data: each rank holds "
                                 "only its slice of the points")
            if self._points is None:
                raise ValueError("hdbscan before train needs data")
            X = self._points.X
        else:
            X = as_points(data, self.device).X
        return _hdbscan(X, min_cluster_size, min_samples, self.eps if r_max is None else r_max,
                        metric, cluster_selection_method, allow_single_cluster, return_tree)

    def radius_neighbors(self, data=None, radius=None, return_distance=True, squared=False,
                         sort_results=False, count_only=False):
        """
        :param data: query points, in any form ``train`` takes; None: the
            training points against themselves
        :param radius: default ``eps``
        :return: as the module-level ``radius_neighbors(points, radius,
            metric, ...)``, whose other parameters these are

        After a train the indexed set is the training points, and with the
        defaults the result is the graph the train clustered: the rows with at
        least ``min_samples`` neighbours are ``core_sample_mask_``, the
        components of the core-core edges are the clusters, and a border point
        carries the smallest label among its core neighbours.  Before any
        train ``data`` is required and is both the indexed set and the
        queries.  After a ``group=`` train each rank holds only its slice, so
        ``data=None`` raises; a given ``data`` is then answered against
        itself.  The index is built and closed per call.
        """
        radius = _check_radius_args(self.eps if radius is None else radius)
        metric = _native.metric_code(self.metric)
        have = self._points is not None and not self._group_trained
        if data is None:
            if self._group_trained:
                raise ValueError("radius_neighbors() after a group= train needs data: each rank "
                                 "holds only its slice of the points")
            if not have:
                raise ValueError("radius_neighbors before train needs data")
            X = q = self._points.X
        elif have:
            X = self._points.X
            q = as_points(data, X.device).X
        else:
            X = q = as_points(data, self.device).X
        return _radius_neighbors(X, q, radius, metric, return_distance, squared, sort_results,
                                 count_only)

    # ------------------------------------------------------------ multi-GPU
    def _sharded_checks(self, points):
        if self.kd_sums != 'exact':
            raise ValueError("kd_sums='sequential' is single-device (the fold order of one "
                             "slice); the multi-GPU train uses the exact sums")
        P = self.max_partitions if self.max_partitions is not None else 4 ** points.d
        return int(P)

    def _set_sharded(self, points, labels, core, res, result, group=None, ops=None):
        ebox = np.ascontiguousarray(res.boxes, np.float64)
        params = {'eps': self.eps, 'min_samples': self.min_samples, 'metric': self.metric}
        if group is not None:
            self.data = _ShardedPartitionRecords(points, res.gid_base, ebox, params, group, ops)
        else:   # one process holds every slice: the single-device records
            self.data = None
        self.labels_ = labels
        self.core_sample_mask_ = core
        self.n_clusters_ = res.n_clusters
        self.bounding_boxes = res.bounding_boxes
        self.expanded_boxes = {L: box.expand(2 * self.eps)
                               for L, box in sorted(res.bounding_boxes.items())}
        self.neighbors = _Neighborhoods(points, self.expanded_boxes)
        if group is None:
            self.data = _PartitionRecords(self.neighbors, params)
        self.result = result
        self.shard = res
        self._points = points
        return self

    def _train_group(self, data, group, metric):
        from . import distributed
        points = as_points(data, self.device)
        P = self._sharded_checks(points)
        res = distributed.train_sharded(points.X, self.eps, self.min_samples, metric=metric,
                                        max_partitions=P, group=group,
                                        keep_owned=self.keep_shard_records)
        result = _ShardedAssignments(points, res.local_labels, res.gid_base, res.n_total, group)
        ops = distributed.NativeOps(points.X.device)
        return self._set_sharded(points, res.local_labels, res.local_core, res, result,
                                 group, ops)

    def _train_devices(self, data, metric):
        from . import distributed
        W = int(self.n_gpus)
        _native.require_gpu()
        if torch.cuda.device_count() < W:
            raise ValueError(f"n_gpus={W} but {torch.cuda.device_count()} GPU(s) are visible")
        points = as_points(data, self.device)
        P = self._sharded_checks(points)
        n = points.n
        cuts = [r * n // W for r in range(W + 1)]
        # a slice moved to another device is a fresh allocation already; one
        # left on its device is a view at an offset, which train_sharded
        # realigns (copies once) when it is not 16-byte aligned — no second
        # full copy of every slice here (transient 2x HBM at C4 scale)
        slices = [points.X[cuts[r]:cuts[r + 1]].to(torch.device("cuda", r)) for r in range(W)]
        torch.cuda.synchronize(points.X.device)
        comms = distributed.device_comms(range(W))
        ops = [distributed.NativeOps(torch.device("cuda", r)) for r in range(W)]
        res = distributed.train_threads(slices, self.eps, self.min_samples, comms, ops,
                                        metric=metric, max_partitions=P,
                                        keep_owned=self.keep_shard_records)
        dev = points.X.device
        labels = torch.cat([r.local_labels.to(dev) for r in res])
        core = torch.cat([r.local_core.to(dev) for r in res])
        return self._set_sharded(points, labels, core, res[0], _Assignments(points, labels))

    def assignments(self):
        """
        :rtype: list
        :return: list of (key, cluster_id), sorted by key
        """
        return self.result.collect()
