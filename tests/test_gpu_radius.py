"""pd_index_radius_count / pd_index_radius_fill / radius_neighbors on the GPU
against the brute-force reference (radius_ref.py).  The order inside a CSR row
is unspecified, so every GPU row is sorted by index on the host first; after
that every comparison is np.array_equal on the offsets, the row numbers and the
raw accumulators: the kernels run the reference's arithmetic, so there is no
tolerance anywhere."""
import numpy as np
import pytest
import torch

import kdist_ref
import radius_ref
from conftest import load_golden
from test_gpu_kdist import R_BLOB, _blob_noise

pytestmark = pytest.mark.gpu

CODE = {"euclidean": 0, "cityblock": 1}
SENTINEL = -77


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _index(X, r_max, metric="euclidean"):
    from pypardis_amd import _native
    return _native.Index.over_rows(_dev(X), r_max, CODE[metric])


def _sorted(indptr, ids, acc=None):
    """Host copies of one GPU result, every row sorted by index."""
    indptr, ids = _np(indptr), _np(ids)
    assert indptr.dtype == np.int64 and ids.dtype == np.int32
    if acc is None:
        return indptr, radius_ref.sort_rows(indptr, ids)[0], None
    acc = _np(acc)
    assert acc.dtype == np.float64
    ids, acc = radius_ref.sort_rows(indptr, ids, acc)
    return indptr, ids, acc


def _equal(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _golden(name):
    g = load_golden(name)
    metric = "cityblock" if str(g["metric"]) == "cityblock" else "euclidean"
    return g, g["X"], float(g["eps"]), int(g["min_samples"]), metric


# ------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8])
def test_blob_and_noise_equal_reference(d, dtype, metric):
    X, Q = _blob_noise(d, dtype)
    r = R_BLOB[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    table = kdist_ref.accumulators(Q, X, metric)
    ix = _index(X, r, metric)
    try:
        dq = _dev(Q)
        for radius in (r, 0.5 * r):
            want = radius_ref.from_accumulators(table, radius, metric)
            if radius == r:      # lanes of one wave see from none to hundreds of hits
                n = np.diff(want[0])
                assert (n == 0).sum() >= 20 and (n >= 65).sum() >= 1
            indptr, ids, acc = ix.radius(dq, radius)
            assert indptr.is_cuda and ids.is_cuda and acc.is_cuda
            assert indptr.shape == (len(Q) + 1,) and ids.shape == acc.shape == (want[0][-1],)
            assert _equal(_sorted(indptr, ids, acc), want), (d, dtype, metric, radius)
            i2, ids2, none = ix.radius(dq, radius, return_acc=False)
            assert none is None and _equal(_sorted(i2, ids2)[:2], want[:2])
            counts, no_ids, no_acc = ix.radius(dq, radius, count_only=True)
            assert no_ids is None and no_acc is None
            assert np.array_equal(_np(counts), want[0])
    finally:
        ix.close()


# ------------------------------------------------------------ 2. goldens
@pytest.mark.parametrize("name", ["b2d_20k", "b3d_20k", "lattice_900", "dup_1d", "ident_40",
                                  "neg_3k", "c0", "c0_p5_cityblock", "c3_5k"])
def test_row_lengths_equal_sklearn_counts(name):
    from pypardis_amd import radius_neighbors
    g, X, eps, _, metric = _golden(name)
    res = radius_neighbors(X, eps, metric, squared=True)
    indptr, ids, acc = _sorted(*res)
    assert np.array_equal(np.diff(indptr), g["sk_counts"])
    assert np.array_equal(_np(radius_neighbors(X, eps, metric, count_only=True)), g["sk_counts"])
    if name == "c3_5k":
        assert len(ids) == 5802                  # the tile path
    if len(X) <= 3000:
        want = radius_ref.radius_neighbors(X, eps, metric)
        assert _equal((indptr, ids, acc), want)
    if name == "lattice_900":                    # pairs at exactly thr are in
        assert (want[2] == kdist_ref.threshold(eps, metric)).sum() == 240
    if name == "ident_40":
        assert np.array_equal(ids.reshape(40, 40), np.tile(np.arange(40, dtype=np.int32), (40, 1)))
        assert not acc.any()


# ------------------------------------------------------------ 3. graph -> labels
@pytest.mark.parametrize("name", ["b2d_20k", "b3d_20k", "c0_p5_cityblock"])
def test_labels_follow_from_the_graph(name):
    from scipy.sparse import csr_matrix
    from pypardis_amd import DBSCAN
    g, X, eps, ms, metric = _golden(name)
    P = int(g["max_partitions"])
    m = DBSCAN(eps=eps, min_samples=ms, metric=metric,
               max_partitions=None if P < 0 else P).train(_dev(X))
    res = m.radius_neighbors(return_distance=False)
    assert res.distances is None
    indptr, ids, _ = _sorted(res.indptr, res.indices)
    labels, core = radius_ref.labels_from_graph(indptr, ids, ms)
    assert core.any() and not core.all()
    assert np.array_equal(core, _np(m.core_sample_mask_).astype(bool))
    assert np.array_equal(labels, _np(m.labels_).astype(np.int64))
    n = len(X)
    A = csr_matrix((np.ones(len(ids), np.int8), ids, indptr), shape=(n, n))
    assert (A != A.T).nnz == 0                   # symmetric
    assert np.array_equal(A.diagonal(), np.ones(n))


# ------------------------------------------------------------ 4. sorted sweep
def test_cell_sorted_and_direct_sweeps_agree(monkeypatch):
    _, X, eps, _, metric = _golden("b2d_20k")
    perm = np.random.default_rng(5).permutation(len(X))[:6000]
    ix = _index(X, eps, metric)
    try:
        monkeypatch.setenv("PD_INDEX_SORT_MIN", str(1 << 40))       # input order
        base = _sorted(*ix.radius(_dev(X[perm]), eps))
        monkeypatch.setenv("PD_INDEX_SORT_MIN", "1")                # cell order
        assert _equal(_sorted(*ix.radius(_dev(X[perm]), eps)), base)
        monkeypatch.delenv("PD_INDEX_SORT_MIN")
        assert _equal(_sorted(*ix.radius(_dev(X[perm]), eps)), base)
        sub = perm[:2500]
        want = radius_ref.radius_neighbors(X[:3000], eps, metric, Q=X[sub])
        assert want[0][-1] > 2500
        ix3 = _index(X[:3000], eps, metric)
        for forced in ("1", str(1 << 40)):
            monkeypatch.setenv("PD_INDEX_SORT_MIN", forced)
            assert _equal(_sorted(*ix3.radius(_dev(X[sub]), eps)), want)
        ix3.close()
    finally:
        ix.close()


# ------------------------------------------------------------ 5. 64-bit cell keys
def test_two_blobs_far_apart_take_64_bit_keys():
    """1e6 apart on both axes at eps 0.01: 1e8 cells per axis (below the 2^28
    at which cells grow), 1e16 in all, so the cell keys are uint64_t."""
    rng = np.random.default_rng(11)
    X = np.concatenate([rng.normal(0.0, 0.02, size=(1500, 2)),
                        rng.normal(0.0, 0.02, size=(1500, 2)) + 1.0e6])
    eps = 0.01
    cells = np.floor((X.max(0) - X.min(0)) / (eps * (1.0 + 2.0 ** -20))) + 1.0
    assert np.all(cells <= 2.0 ** 28) and np.prod(cells) >= 2.0 ** 32
    Q = np.concatenate([X[::2], rng.uniform(4.0e5, 6.0e5, size=(100, 2)),
                        np.array([[1.0e6, 0.0], [-1.0e9, 3.0], [1.0e300, -1.0e300]])])
    table = kdist_ref.accumulators(Q, X)
    ix = _index(X, eps)
    try:
        for radius in (eps, 0.3 * eps):
            want = radius_ref.from_accumulators(table, radius)
            assert want[0][-1] > 3 * len(X) // 2 and np.all(np.diff(want[0])[1500:] == 0)
            assert _equal(_sorted(*ix.radius(_dev(Q), radius)), want)
    finally:
        ix.close()


# ------------------------------------------------------------ 6. totals beyond 2^32
def test_total_beyond_2_to_32_count_only():
    """66,000 copies of one point: 4.356e9 pairs.  The counts are 32-bit, their
    sums and the total 64-bit.  Count only: the pairs themselves are never
    written."""
    n = 66_000
    X = np.full((n, 2), 0.25, np.float32)
    ix = _index(X, 0.5)
    try:
        indptr, total = ix.radius_count(_dev(X), 0.5)
        assert total == n * n and total > 2 ** 32
        assert np.array_equal(_np(indptr), np.arange(n + 1, dtype=np.int64) * n)
    finally:
        ix.close()


# ------------------------------------------------------------ 7. edges and errors
@pytest.mark.parametrize("d", [2, 6])
def test_no_queries_empty_index_and_queries_outside(d):
    from pypardis_amd import _native
    rng = np.random.default_rng(3)
    X = rng.uniform(0.0, 1.0, size=(1500, d)).astype(np.float32)
    r = 0.25 if d == 2 else 0.6
    ix = _index(X, r)
    indptr, ids, acc = ix.radius(torch.empty((0, d), dtype=torch.float32, device="cuda"), r)
    assert _np(indptr).tolist() == [0] and ids.shape == acc.shape == (0,)
    near = X[:300].copy()
    near[:, 0] = -0.5 * r                # outside the box by less than a cell
    far = X[:300].copy()
    far[:, 0] = -2.5 * r                 # by more than one cell
    off = np.full((3, d), 1.0e30, np.float32)
    Q = np.concatenate([near, far, off])
    want = radius_ref.radius_neighbors(X, r, Q=Q)
    assert want[0][300] > 0 and want[0][-1] == want[0][300]
    assert _equal(_sorted(*ix.radius(_dev(Q), r)), want)
    ix.close()
    # no rows at all, and rows none of which the mask admits
    dx = _dev(X)
    for empty in (_native.Index.over_rows(dx[:0], r),
                  _native.Index(dx, torch.zeros(len(X), dtype=torch.uint8, device="cuda"),
                                torch.zeros(len(X), dtype=torch.int32, device="cuda"), r)):
        assert empty.n_core == 0
        indptr, ids, acc = empty.radius(dx, r)
        assert not _np(indptr).any() and indptr.shape == (len(X) + 1,) and ids.shape == (0,)
        bad = indptr.clone()
        bad[4:] += 2                      # a segment for hits that do not exist
        with pytest.raises(_native.PardisError) as e:
            empty.radius_fill(dx, r, bad, torch.zeros(8, dtype=torch.int32, device="cuda"))
        assert e.value.code == _native.PD_EINVAL
        empty.close()


def test_errors_leave_the_index_usable():
    from pypardis_amd import _native
    _, X, eps, _, metric = _golden("neg_3k")
    ix = _index(X, eps, metric)
    want = radius_ref.radius_neighbors(X, eps, metric)
    Q = X[:100].copy()
    Q[37, 1] = np.nan
    for q, radius in ((X, np.nextafter(eps, 1.0)), (X, 2 * eps), (X, 0.0), (X, -eps),
                      (X, float("nan")), (X, float("inf")), (Q, eps),
                      (X.astype(np.float64), eps)):
        with pytest.raises(_native.PardisError) as e:
            ix.radius(_dev(q), radius)
        assert e.value.code == _native.PD_EINVAL, (radius, e.value)
    big = np.repeat(X[:3], 4000, axis=0)
    big[5000, 0] = np.inf
    for forced in ("1", None):                                # the sorted sweep's check too
        with pytest.MonkeyPatch.context() as mp:
            if forced:
                mp.setenv("PD_INDEX_SORT_MIN", forced)
            with pytest.raises(_native.PardisError) as e:
                ix.radius(_dev(big), eps, count_only=True)
            assert e.value.code == _native.PD_EINVAL
    with pytest.raises(ValueError):                           # dimension, as query
        ix.radius(_dev(np.zeros((5, 3), np.float32)), eps)
    assert _equal(_sorted(*ix.radius(_dev(X), eps)), want)
    ix.close()
    with pytest.raises(ValueError):
        ix.radius(_dev(X), eps)


def _segments_mask(off, size, cap):
    """Elements of an array of `size` that some [off[q], min(off[q+1], cap))
    with 0 <= off[q] <= off[q+1] covers: what a fill may touch."""
    mask = np.zeros(size, bool)
    for a, b in zip(off[:-1].tolist(), off[1:].tolist()):
        if 0 <= a <= b:
            mask[a:min(b, cap)] = True
    return mask


@pytest.mark.parametrize("d", [3, 6])
def test_fill_with_foreign_offsets_is_an_error_not_a_store(d):
    """A fill whose offsets are not the count's must end as PD_EINVAL and may
    store only inside the segments those offsets describe, clipped to
    capacity: everything else, the guard band behind capacity included, keeps
    its sentinel.  An ordinary error path: no access leaves the buffers."""
    from pypardis_amd import _native
    rng = np.random.default_rng(6)
    X = rng.normal(0.0, 0.3, size=(900, d)).astype(np.float32)
    r = 0.3 if d == 3 else 0.7
    want = radius_ref.radius_neighbors(X, r)
    ix = _index(X, r)
    try:
        dx = _dev(X)
        indptr, total = ix.radius_count(dx, r)
        assert total == want[0][-1] and total > 5 * len(X)
        guard = 4096
        good = _np(indptr)
        cases = {}
        t = good.copy(); t[300:] -= 3; cases["shifted down"] = t
        t = good.copy(); t[1:] += 5; cases["shifted up, past capacity"] = t
        t = good.copy(); t[5] = 10 ** 12; cases["one huge"] = t
        t = good.copy(); t[7] = -5; cases["one negative"] = t
        t = good.copy(); t[200] = np.iinfo(np.int64).max; t[201] = np.iinfo(np.int64).min
        cases["extremes"] = t
        cases["all zero"] = np.zeros_like(good)
        cases["reversed"] = good[::-1].copy()
        cases["into the guard band"] = good + total + 100
        for what, off in cases.items():
            ids = torch.full((total + guard,), SENTINEL, dtype=torch.int32, device="cuda")
            acc = torch.full((total + guard,), float(SENTINEL), dtype=torch.float64, device="cuda")
            with pytest.raises(_native.PardisError) as e:
                ix.radius_fill(dx, r, _dev(off), ids, acc, capacity=total)
            assert e.value.code == _native.PD_EINVAL, what
            may = _segments_mask(off, total + guard, total)
            assert np.all(_np(ids)[~may] == SENTINEL), what
            assert np.all(_np(acc)[~may] == float(SENTINEL)), what
            assert np.all(_np(ids)[total:] == SENTINEL), what
        # another radius or other queries against the count's offsets
        ids = torch.full((total + guard,), SENTINEL, dtype=torch.int32, device="cuda")
        for q, radius in ((dx, 0.5 * r), (_dev(X[::-1]), r)):
            with pytest.raises(_native.PardisError) as e:
                ix.radius_fill(q, radius, indptr, ids, capacity=total)
            assert e.value.code == _native.PD_EINVAL
            assert np.all(_np(ids)[total:] == SENTINEL)
        # a capacity below the total clips, and says so
        ids.fill_(SENTINEL)
        with pytest.raises(_native.PardisError) as e:
            ix.radius_fill(dx, r, indptr, ids, capacity=total - 1)
        assert e.value.code == _native.PD_EINVAL
        assert np.all(_np(ids)[total - 1:] == SENTINEL)
        # the right offsets into the same over-allocated buffers
        ids.fill_(SENTINEL)
        acc = torch.full((total + guard,), float(SENTINEL), dtype=torch.float64, device="cuda")
        ix.radius_fill(dx, r, indptr, ids, acc, capacity=total)
        assert np.all(_np(ids)[total:] == SENTINEL) and np.all(_np(acc)[total:] == SENTINEL)
        assert _equal(_sorted(indptr, ids[:total], acc[:total]), want)
    finally:
        ix.close()


@pytest.mark.parametrize("d", [2, 7])
def test_ids_of_a_predict_index_are_its_labels(d):
    """The fill writes the index's label of each hit: on an index over the
    cores of a train, the cluster labels of the cores within the radius."""
    from pypardis_amd import _native
    rng = np.random.default_rng(12)
    X = rng.normal(0.0, 0.4, size=(2000, d))
    core = rng.uniform(size=len(X)) < 0.6
    labels = rng.integers(0, 5, size=len(X)).astype(np.int32)
    r = 0.15 if d == 2 else 0.9
    Q = X[:700] + 0.01
    ix = _native.Index(_dev(X), _dev(core.astype(np.uint8)), _dev(labels), r)
    table = kdist_ref.accumulators(Q, X[core])
    try:
        for radius in (r, 0.8 * r):
            indptr, ids, acc = (_np(t) for t in ix.radius(_dev(Q), radius))
            wp, wi, wa = radius_ref.from_accumulators(table, radius)
            assert wp[-1] > len(Q) and (np.diff(wp) == 0).any()
            wl = labels[core][wi]
            rows = np.repeat(np.arange(len(Q)), np.diff(wp))
            assert np.array_equal(indptr, wp)
            o, wo = np.lexsort((ids, acc, rows)), np.lexsort((wl, wa, rows))
            assert np.array_equal(ids[o], wl[wo]) and np.array_equal(acc[o], wa[wo])
            if radius == r:                        # predict = the smallest of them
                best = np.full(len(Q), -1, np.int32)
                have = np.diff(wp) > 0
                best[have] = np.minimum.reduceat(wl, wp[:-1][have])
                assert np.array_equal(_np(ix.query(_dev(Q))), best)
    finally:
        ix.close()


def test_rows_above_944_bytes_are_unsupported():
    from pypardis_amd import _native
    X = np.random.default_rng(1).uniform(size=(80, 119))      # 952 bytes per fp64 row
    ix = _index(X, 4.0)
    with pytest.raises(_native.PardisError) as e:
        ix.radius(_dev(X), 4.0)
    assert e.value.code == -5
    ix.close()
    X = X[:, :118].copy()                                     # 944 bytes: the last that fits
    ix = _index(X, 4.2)
    want = radius_ref.radius_neighbors(X, 4.2)
    assert len(X) < want[0][-1] < len(X) ** 2
    assert _equal(_sorted(*ix.radius(_dev(X), 4.2)), want)
    ix.close()


# ------------------------------------------------------------ 8. Python surface
def test_module_radius_neighbors_inputs_and_options():
    import dbscan
    from pypardis_amd import radius_neighbors
    _, X, eps, _, metric = _golden("neg_3k")
    wp, wi, wa = radius_ref.radius_neighbors(X, eps, metric)
    res = radius_neighbors(X, eps, squared=True)
    assert type(res).__name__ == "RadiusNeighbors" and res.indptr.is_cuda
    assert _equal(_sorted(*res), (wp, wi, wa))
    res = dbscan.radius_neighbors(_dev(X), eps)               # correctly rounded fp64 sqrt
    assert _equal(_sorted(*res), (wp, wi, np.sqrt(wa)))
    recs = [(f"p{i}", X[i]) for i in range(len(X))]           # (key, vector) records
    assert _equal(_sorted(*radius_neighbors(recs, eps, squared=True)), (wp, wi, wa))
    # sort_results: each row by (distance, index), no host sort needed
    rows = np.repeat(np.arange(len(X)), np.diff(wp))
    o = np.lexsort((wi, wa, rows))
    res = radius_neighbors(X, eps, squared=True, sort_results=True)
    assert _equal((_np(res.indptr), _np(res.indices), _np(res.distances)), (wp, wi[o], wa[o]))
    res = radius_neighbors(X, eps, return_distance=False, sort_results=True)
    assert res.distances is None and np.array_equal(_np(res.indices), wi[o])
    # queries= a sample; float64 queries of float32 data are rounded to float32 first
    sub = np.random.default_rng(8).choice(len(X), 500, replace=False)
    Q = X[sub] + np.float32(0.03)
    want = radius_ref.radius_neighbors(X, eps, "cityblock", Q=Q)
    got = radius_neighbors(X, eps, "cityblock", queries=Q.astype(np.float64))
    assert _equal(_sorted(*got), want)                        # cityblock: no sqrt
    counts = radius_neighbors(X, eps, "cityblock", queries=Q, count_only=True)
    assert counts.dtype == torch.int64 and np.array_equal(_np(counts), np.diff(want[0]))
    with pytest.raises(ValueError):
        radius_neighbors(X, eps, queries=np.zeros((4, 3), np.float32))
    bad = X[:50].copy()
    bad[7, 0] = np.nan
    with pytest.raises(ValueError):
        radius_neighbors(X, eps, queries=bad)
    with pytest.raises(ValueError):
        radius_neighbors(bad, eps)


def test_model_radius_neighbors():
    from pypardis_amd import DBSCAN
    _, X, eps, ms, metric = _golden("c0_p5_cityblock")
    fresh = DBSCAN(eps=eps, min_samples=ms, metric=metric)
    with pytest.raises(ValueError):
        fresh.radius_neighbors()
    want = radius_ref.radius_neighbors(X, eps, metric)
    assert _equal(_sorted(*fresh.radius_neighbors(X)), want)  # untrained: data against itself
    assert fresh.labels_ is None
    m = DBSCAN(eps=eps, min_samples=ms, metric=metric, max_partitions=5).train(_dev(X))
    assert _equal(_sorted(*m.radius_neighbors()), want)
    Q = X[:300] + 0.01                                        # new queries, another radius
    want = radius_ref.radius_neighbors(X, 0.5 * eps, metric, Q=Q)
    assert _equal(_sorted(*m.radius_neighbors(_dev(Q), radius=0.5 * eps)), want)
    sub = np.arange(0, len(X), 3)                             # predict's index is untouched
    assert np.array_equal(_np(m.predict(_dev(X[sub]))), _np(m.labels_)[sub])
