"""pd_index_kneighbors / kneighbors on the GPU against the brute-force reference
(knn_ref.py).  The result is ordered by the total order (acc, label), so every
comparison is np.array_equal on the raw ids and accumulators (inf == inf): the
kernels run the reference's arithmetic, so there is no tolerance anywhere."""
import numpy as np
import pytest
import torch

import kdist_ref
import knn_ref
from conftest import load_golden
from test_gpu_kdist import R_BLOB, _blob_noise, _trained

pytestmark = pytest.mark.gpu

# every list tier (registers 4 and 8, LDS at 256 / 128 / 64 lanes) and both sides of each boundary
KS = (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
CODE = {"euclidean": 0, "cityblock": 1}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _index(X, r_max, metric="euclidean"):
    from pypardis_amd import _native
    return _native.Index.over_rows(_dev(X), r_max, CODE[metric])


def _ask(ix, Q, k, return_acc=True):
    """Host copies of one GPU answer, its types and shapes checked."""
    dq = Q if torch.is_tensor(Q) else _dev(Q)
    ids, acc = ix.kneighbors(dq, k, return_acc)
    assert ids.is_cuda and ids.dtype == torch.int32 and ids.shape == (dq.shape[0], k)
    if not return_acc:
        assert acc is None
        return _np(ids), None
    assert acc.is_cuda and acc.dtype == torch.float64 and acc.shape == ids.shape
    return _np(ids), _np(acc)


def _equal(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _agrees(ix, Q, k, want):
    """Both outputs, and the ids alone, equal the reference."""
    dq = Q if torch.is_tensor(Q) else _dev(Q)
    return _equal(_ask(ix, dq, k), want) and np.array_equal(_ask(ix, dq, k, False)[0], want[0])


def _golden(name):
    g = load_golden(name)
    metric = "cityblock" if str(g["metric"]) == "cityblock" else "euclidean"
    return g["X"], float(g["eps"]), int(g["min_samples"]), metric


def _padding(m, k):
    return np.full((m, k), -1, np.int32), np.full((m, k), np.inf)


# ------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8])
def test_blob_and_noise_equal_reference(d, dtype, metric):
    X, Q = _blob_noise(d, dtype)
    r = R_BLOB[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    pairs = knn_ref.smallest_pairs(kdist_ref.accumulators(Q, X, metric), 64)
    ix = _index(X, r, metric)
    try:
        dq = _dev(Q)
        for k in KS:
            want = knn_ref.cut(pairs, k, r, metric)
            if k == 9:
                assert (want[0][:, 8] < 0).sum() > 100       # the noise rows run short
                assert ((want[0][:, 0] >= 0) & (want[0][:, 8] < 0)).sum() > 20    # some partly
            if k == 64:
                assert (want[0][:, 63] >= 0).sum() > 100     # the blob's centre does not
            ids, acc = _ask(ix, dq, k)
            assert _equal((ids, acc), want), (k, int((ids != want[0]).any(axis=1).sum()),
                                              int((acc != want[1]).any(axis=1).sum()))
            assert np.array_equal(_ask(ix, dq, k, return_acc=False)[0], want[0]), k
    finally:
        ix.close()


# ------------------------------------------------------------ 2. ties
@pytest.mark.parametrize("name,ks,mult", [
    ("lattice_900", KS, (1.0, 2.0)),     # the cap sits on a tie; many equal distances per row
    ("dup_1d", (1, 2, 3, 4, 7), (1.0,)),  # every value three times
    ("ident_40", (1, 8, 39, 40, 41, 64), (1.0,)),   # 40 copies of one point
    ("neg_3k", KS, (1.0,)),
])
def test_ties_are_settled_by_row_number(name, ks, mult):
    X, eps, _, metric = _golden(name)
    pairs = knn_ref.smallest_pairs(kdist_ref.accumulators(X, X, metric), 64)
    if name == "lattice_900":             # 742 of the 900 rows hold equal distances among their 9 nearest
        assert (np.diff(pairs[1][:, :9], axis=1) == 0).any(axis=1).sum() > 700
        assert (pairs[1][:, :8] == eps * eps).any()
    for f in mult:
        r = eps * f
        ix = _index(X, r, metric)
        try:
            for k in ks:
                assert _agrees(ix, X, k, knn_ref.cut(pairs, k, r, metric)), (name, f, k)
            if name == "ident_40":
                for k in (8, 40, 41, 64):
                    ids, acc = _ask(ix, X, k)
                    row = np.concatenate([np.arange(min(k, 40)), np.full(max(k - 40, 0), -1)])
                    assert np.array_equal(ids, np.tile(row.astype(np.int32), (40, 1)))
                    assert not acc[:, :min(k, 40)].any() and np.all(np.isinf(acc[:, 40:]))
        finally:
            ix.close()


# ------------------------------------------------------------ 3. identities on trained goldens
def _head_of_sorted_csr(res, k):
    """(ids, acc) (m, k): the first min(k, len) entries of each row of a sorted
    radius_neighbors result, padded with (-1, inf)."""
    indptr, indices, acc = (_np(t) for t in res)
    n = np.diff(indptr)
    t = np.arange(k)[None, :]
    have = t < n[:, None]
    at = np.where(have, indptr[:-1, None] + t, 0)
    ids, out = _padding(len(n), k)
    ids[have] = indices[at[have]]
    out[have] = acc[at[have]]
    return ids, out


@pytest.mark.parametrize("name", ["b2d_20k", "b3d_20k", "c0_p5_cityblock", "c3_5k"])
def test_identities_with_kdist_radius_and_the_core_flags(name):
    from pypardis_amd import radius_neighbors
    m, X, eps, ms, metric = _trained(name)
    core = _np(m.core_sample_mask_).astype(bool)
    assert core.any() and not core.all()
    dx = _dev(X)
    for f in (1.0, 2.0):
        r = eps * f
        ix = _index(X, r, metric)
        try:
            ids, acc = _ask(ix, dx, ms)
            assert np.array_equal(acc[:, ms - 1], _np(ix.kdist(dx, ms)))       # bit for bit, inf too
            counts = np.diff(_np(ix.radius(dx, r, count_only=True)[0]))
            assert np.array_equal((ids >= 0).sum(axis=1), np.minimum(ms, counts))
            assert np.array_equal(ids >= 0, np.isfinite(acc))
        finally:
            ix.close()
        res = radius_neighbors(dx, r, metric, squared=True, sort_results=True)
        assert _equal((ids, acc), _head_of_sorted_csr(res, ms)), (name, f)
        if f == 1.0:
            assert np.array_equal(ids[:, ms - 1] >= 0, core)


# ------------------------------------------------------------ 4. sorted sweep
def test_cell_sorted_and_direct_sweeps_agree(monkeypatch):
    X, eps, ms, metric = _golden("b2d_20k")
    perm = np.random.default_rng(5).permutation(len(X))
    ix = _index(X, eps, metric)
    try:
        for k in (4, ms, 20, 40):
            monkeypatch.setenv("PD_INDEX_SORT_MIN", str(1 << 40))   # input order
            base = _ask(ix, X, k)
            assert (base[0][:, k - 1] >= 0).any() and (base[0][:, k - 1] < 0).any()
            monkeypatch.setenv("PD_INDEX_SORT_MIN", "1")            # cell order
            assert _equal(_ask(ix, X, k), base)
            got = _ask(ix, X[perm], k)
            assert _equal(got, (base[0][perm], base[1][perm]))
            monkeypatch.delenv("PD_INDEX_SORT_MIN")
            assert _equal(_ask(ix, X[perm], k), got)
        sub = perm[:2500]
        ix3 = _index(X[:3000], eps, metric)
        for k in (ms, 20):
            want = knn_ref.kneighbors(X[:3000], k, eps, metric, Q=X[sub])
            for forced in ("1", str(1 << 40)):
                monkeypatch.setenv("PD_INDEX_SORT_MIN", forced)
                assert _equal(_ask(ix3, X[sub], k), want)
        ix3.close()
    finally:
        ix.close()


# ------------------------------------------------------------ 5. row order
@pytest.mark.parametrize("d", [3, 6])
def test_result_does_not_depend_on_the_order_of_the_rows(d):
    """The same points with their rows permuted: the same accumulators, and
    ids that map through the permutation.  No two of a query's k + 1 nearest
    are equally far here, so the row numbers settle nothing."""
    rng = np.random.default_rng(21 + d)
    X = rng.normal(0.0, 0.3, size=(2000, d))
    Q = np.concatenate([X[:700], rng.normal(0.0, 0.3, size=(300, d))])
    r = 0.12 if d == 3 else 0.55
    perm = rng.permutation(len(X))
    Xp = X[perm]                                  # row i of Xp is row perm[i] of X
    pairs = knn_ref.smallest_pairs(kdist_ref.accumulators(Q, X), 41)
    assert not (np.diff(pairs[1], axis=1) == 0).any()
    ix, ixp = _index(X, r), _index(Xp, r)
    try:
        for k in (4, 8, 20, 40):
            want = knn_ref.cut(pairs, k, r)
            assert (want[0][:, k - 1] >= 0).any() and (want[0][:, k - 1] < 0).any()
            assert _equal(_ask(ix, Q, k), want)
            ids, acc = _ask(ixp, Q, k)
            assert np.array_equal(acc, want[1])
            assert np.array_equal(np.where(ids >= 0, perm[np.maximum(ids, 0)], -1), want[0])
    finally:
        ix.close()
        ixp.close()


# ------------------------------------------------------------ 6. edges
@pytest.mark.parametrize("d", [2, 5])
def test_queries_outside_the_box(d):
    rng = np.random.default_rng(9)
    X = rng.uniform(0.0, 1.0, size=(1500, d)).astype(np.float32)
    X[:40, 0] = 0.0                      # rows on the box's face
    r = 0.25 if d == 2 else 0.6
    near = X[:300].copy()
    near[:, 0] = -0.5 * r                # outside by less than a cell
    far = X[:300].copy()
    far[:, 0] = -2.5 * r                 # by more than one cell
    off = np.full((3, d), 1.0e30, np.float32)
    Q = np.concatenate([near, far, off])
    pairs = knn_ref.smallest_pairs(kdist_ref.accumulators(Q, X), 12)
    ix = _index(X, r)
    try:
        for k in (1, 5, 12):
            want = knn_ref.cut(pairs, k, r)
            assert (want[0][:300] >= 0).any() and _equal((want[0][300:], want[1][300:]),
                                                         _padding(303, k))
            assert _agrees(ix, Q, k, want)
    finally:
        ix.close()


def test_no_queries_fewer_rows_than_k_and_an_empty_index():
    from pypardis_amd import _native
    rng = np.random.default_rng(2)
    for d in (3, 6):
        X = rng.uniform(0.0, 1.0, size=(5, d))
        ix = _index(X, 10.0)
        ids, acc = _ask(ix, torch.empty((0, d), dtype=torch.float64, device="cuda"), 3)
        assert ids.shape == acc.shape == (0, 3)
        for k in (5, 8, 40):             # n <= k: the rows there are, then padding
            want = knn_ref.kneighbors(X, k, 10.0)
            assert (want[0][:, :5] >= 0).all() and (want[0][:, 5:] < 0).all()
            assert _agrees(ix, X, k, want)
        ix.close()
        # no rows at all, and rows none of which the mask admits
        dx = _dev(X)
        for empty in (_native.Index.over_rows(dx[:0], 10.0),
                      _native.Index(dx, torch.zeros(5, dtype=torch.uint8, device="cuda"),
                                    torch.zeros(5, dtype=torch.int32, device="cuda"), 10.0)):
            assert empty.n_core == 0
            for k in (2, 20):
                assert _agrees(empty, dx, k, _padding(5, k))
            bad = X.copy()
            bad[3, 1] = np.nan           # the queries are checked all the same
            with pytest.raises(_native.PardisError) as e:
                empty.kneighbors(_dev(bad), 2)
            assert e.value.code == _native.PD_EINVAL
            empty.close()
    # the rows exist but never k of them within the cap
    X = rng.uniform(0.0, 1.0, size=(300, 2))
    want = knn_ref.kneighbors(X, 30, 0.05)
    assert (want[0][:, 0] >= 0).all() and (want[0][:, 29] < 0).all()
    ix = _index(X, 0.05)
    assert _agrees(ix, X, 30, want)
    ix.close()


@pytest.mark.parametrize("gap,r", [(1.0e6, 1.0e-3), (1.0e6, 0.01)])
def test_two_blobs_far_apart(gap, r):
    """1e6 apart on both axes.  At r_max 1e-3 the axes would have 1e9 cells, so
    the cells grow; at 0.01 they have 1e8 (below the 2^28 at which cells grow),
    1e16 in all: 64-bit cell keys."""
    rng = np.random.default_rng(11)
    s = 3.0 * r
    X = np.concatenate([rng.normal(0.0, s, size=(1500, 2)),
                        rng.normal(0.0, s, size=(1500, 2)) + gap])
    Q = np.concatenate([X[::2], rng.uniform(4.0e5, 6.0e5, size=(100, 2)),
                        np.array([[1.0e6, 0.0], [-1.0e9, 3.0], [1.0e300, -1.0e300]])])
    pairs = knn_ref.smallest_pairs(kdist_ref.accumulators(Q, X), 64)
    ix = _index(X, r)
    try:
        for k in (1, 6, 20, 64):
            want = knn_ref.cut(pairs, k, r)
            if k == 20:
                assert (want[0][:1500, 19] >= 0).sum() > 100 and (want[0][:1500, 19] < 0).sum() > 100
            assert np.all(want[0][1500:] < 0)
            assert _agrees(ix, Q, k, want)
    finally:
        ix.close()


def test_dense_tiles_above_64_kib_of_lds():
    """d = 64 fp64 with k = 64: the lanes' rows and pair lists pass the default
    dynamic-LDS limit, the launch that raises it."""
    rng = np.random.default_rng(7)
    X = rng.normal(0.0, 0.1, size=(700, 64))
    r = 1.0                                   # about half the rows have 64 rows that near
    pairs = knn_ref.smallest_pairs(kdist_ref.accumulators(X, X), 64)
    ix = _index(X, r)
    try:
        for k in (1, 33, 64):
            want = knn_ref.cut(pairs, k, r)
            if k == 64:
                assert 50 < (want[0][:, 63] >= 0).sum() < 650
            assert _agrees(ix, X, k, want)
    finally:
        ix.close()


def test_rows_above_944_bytes_are_unsupported():
    from pypardis_amd import _native
    X = np.random.default_rng(1).uniform(size=(80, 119))      # 952 bytes per fp64 row
    ix = _index(X, 1.0)
    with pytest.raises(_native.PardisError) as e:
        ix.kneighbors(_dev(X), 3)
    assert e.value.code == -5
    ix.close()
    X = X[:, :118].copy()                                     # 944 bytes: the last that fits
    pairs = knn_ref.smallest_pairs(kdist_ref.accumulators(X, X), 64)
    for k, r in ((3, 4.0), (64, 4.5)):                        # k = 64: the largest block there is
        ix = _index(X, r)
        assert _agrees(ix, X, k, knn_ref.cut(pairs, k, r))
        ix.close()


@pytest.mark.parametrize("d", [2, 6])
def test_errors_leave_the_index_usable(d):
    from pypardis_amd import _native
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(3000, d)).astype(np.float32)
    r = 0.05 if d == 2 else 0.5
    ix = _index(X, r)
    want = knn_ref.kneighbors(X, 12, r)
    Q = X[:200].copy()
    Q[150, d - 1] = np.nan
    for k, q, code in ((12, Q, _native.PD_EINVAL), (3, Q, _native.PD_EINVAL),
                       (0, X, _native.PD_EINVAL), (-1, X, _native.PD_EINVAL), (65, X, -5),
                       (12, X.astype(np.float64), _native.PD_EINVAL)):      # dtype, as query
        with pytest.raises(_native.PardisError) as e:
            ix.kneighbors(_dev(q), k)
        assert e.value.code == code, (k, e.value)
    big = np.repeat(X[:3], 4000, axis=0)
    big[5000, 0] = np.inf
    for forced in ("1", None):                                # the sorted sweep's check too
        with pytest.MonkeyPatch.context() as mp:
            if forced:
                mp.setenv("PD_INDEX_SORT_MIN", forced)
            with pytest.raises(_native.PardisError) as e:
                ix.kneighbors(_dev(big), 12)
            assert e.value.code == _native.PD_EINVAL
    with pytest.raises(ValueError):                           # dimension, as query
        ix.kneighbors(_dev(np.zeros((5, d + 1), np.float32)), 3)
    assert _agrees(ix, X, 12, want)
    ix.close()
    with pytest.raises(ValueError):
        ix.kneighbors(_dev(X), 3)


# ------------------------------------------------------------ 7. a predict index
@pytest.mark.parametrize("d", [2, 7])
def test_ids_of_a_predict_index_are_its_labels(d):
    """Over the cores of a train the ids are cluster labels ordered by (acc,
    label), and equal pairs — here copies of a core under one label — are each
    kept."""
    from pypardis_amd import _native
    rng = np.random.default_rng(12)
    X = rng.normal(0.0, 0.4, size=(2000, d))
    X[1000:1300] = X[:300]                        # every copy at the same distance of any query
    core = rng.uniform(size=len(X)) < 0.6
    labels = rng.integers(0, 5, size=len(X)).astype(np.int32)
    labels[1000:1150] = labels[:150]              # half of the copies under the same label
    r = 0.15 if d == 2 else 0.9
    Q = np.concatenate([X[:400], X[:300] + 0.01])
    pairs = knn_ref.smallest_pairs(kdist_ref.accumulators(Q, X[core]), 40, labels[core])
    twins = (pairs[0][:, 1:] == pairs[0][:, :-1]) & (pairs[1][:, 1:] == pairs[1][:, :-1])
    assert (twins & (pairs[1][:, 1:] <= r * r)).sum() > 50
    ix = _native.Index(_dev(X), _dev(core.astype(np.uint8)), _dev(labels), r)
    try:
        for k in (3, 8, 12, 40):
            want = knn_ref.cut(pairs, k, r)
            assert (want[0][:, k - 1] >= 0).any() and (want[0] < 0).any()
            assert _agrees(ix, Q, k, want)
    finally:
        ix.close()


# ------------------------------------------------------------ 8. Python surface
def test_model_kneighbors_after_train():
    m, X, eps, ms, metric = _trained("b3d_20k")
    ix = _index(X, eps, metric)
    raw = _ask(ix, X, ms)
    ix.close()
    res = m.kneighbors()
    assert type(res).__name__ == "KNeighbors" and res.indices.is_cuda and res.distances.is_cuda
    assert res.indices.dtype == torch.int32 and res.distances.dtype == torch.float64
    assert np.array_equal(_np(res.indices), raw[0])
    assert np.array_equal(_np(res.distances), np.sqrt(raw[1]))        # correctly rounded fp64 sqrt
    assert _equal([_np(t) for t in m.kneighbors(squared=True)], raw)
    assert np.array_equal(raw[0][:, 0], np.arange(len(X)))            # self first: no duplicates here
    assert np.array_equal(_np(m.core_sample_mask_).astype(bool), raw[0][:, ms - 1] >= 0)
    res = m.kneighbors(return_distance=False)
    assert res.distances is None and np.array_equal(_np(res.indices), raw[0])
    # other k / cap, new queries against the training points
    Q = X[:2000] + np.float32(0.01)
    ix = _index(X, 2 * eps, metric)
    want = _ask(ix, Q, 20)
    ix.close()
    assert _equal([_np(t) for t in m.kneighbors(_dev(Q), k=20, r_max=2 * eps, squared=True)], want)
    sub = np.random.default_rng(3).choice(len(X), 3000, replace=False)
    assert np.array_equal(_np(m.predict(_dev(X[sub]))), _np(m.labels_)[sub])   # predict's index is untouched


def test_model_kneighbors_cityblock_and_before_train():
    from pypardis_amd import DBSCAN
    m, X, eps, ms, metric = _trained("c0_p5_cityblock")
    want = knn_ref.kneighbors(X, ms, eps, metric)
    assert _equal([_np(t) for t in m.kneighbors()], want)             # cityblock: no sqrt
    assert _equal([_np(t) for t in m.kneighbors(squared=True)], want)
    fresh = DBSCAN(eps=eps, min_samples=ms, metric=metric)
    assert _equal([_np(t) for t in fresh.kneighbors(X)], want)        # untrained: data against itself
    assert fresh.labels_ is None
    with pytest.raises(ValueError):
        fresh.kneighbors()


def test_module_kneighbors_inputs_and_options():
    import dbscan
    from pypardis_amd import kneighbors
    X, eps, ms, metric = _golden("neg_3k")
    want = knn_ref.kneighbors(X, ms, eps, metric)
    assert _equal([_np(t) for t in kneighbors(X, ms, eps, squared=True)], want)
    res = dbscan.kneighbors(_dev(X), ms, eps)
    assert np.array_equal(_np(res.indices), want[0])
    assert np.array_equal(_np(res.distances), np.sqrt(want[1]))
    recs = [(f"p{i}", X[i]) for i in range(len(X))]           # (key, vector) records
    assert _equal([_np(t) for t in kneighbors(recs, ms, eps, squared=True)], want)
    # queries= a sample; float64 queries of float32 data are rounded to float32 first
    sub = np.random.default_rng(8).choice(len(X), 500, replace=False)
    got = kneighbors(X, ms, eps, queries=X[sub].astype(np.float64), squared=True)
    assert _equal([_np(t) for t in got], (want[0][sub], want[1][sub]))
    Q = X[sub] + np.float32(0.03)
    got = kneighbors(X, 3, eps, "cityblock", queries=Q)
    assert _equal([_np(t) for t in got], knn_ref.kneighbors(X, 3, eps, "cityblock", Q=Q))
    got = kneighbors(X, 3, eps, queries=Q, return_distance=False)
    assert got.distances is None
    assert np.array_equal(_np(got.indices), knn_ref.kneighbors(X, 3, eps, Q=Q)[0])
    with pytest.raises(ValueError):
        kneighbors(X, ms, eps, queries=np.zeros((4, 3), np.float32))
    bad = X[:50].copy()
    bad[7, 0] = np.nan
    with pytest.raises(ValueError):
        kneighbors(X, ms, eps, queries=bad)
    with pytest.raises(ValueError):
        kneighbors(bad, ms, eps)
