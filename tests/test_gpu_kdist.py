"""pd_index_kdist / k_distances on the GPU against the brute-force reference
(kdist_ref.py).  Every comparison is np.array_equal on the raw accumulators
(inf == inf): the kernels run the reference's arithmetic, so there is no
tolerance anywhere."""
import numpy as np
import pytest
import torch

import kdist_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

KS = (1, 3, 8, 9, 16, 17, 33, 64)     # every list tier and the first k past each boundary
CODE = {"euclidean": 0, "cityblock": 1}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _index(X, r_max, metric="euclidean"):
    from pypardis_amd import _native
    return _native.Index.over_all(_dev(X), r_max, CODE[metric])


def _kdist(X, Q, k, r_max, metric="euclidean"):
    ix = _index(X, r_max, metric)
    try:
        return _np(ix.kdist(_dev(Q), k))
    finally:
        ix.close()


def _golden(name):
    g = load_golden(name)
    metric = "cityblock" if str(g["metric"]) == "cityblock" else "euclidean"
    return g["X"], float(g["eps"]), int(g["min_samples"]), metric


# ------------------------------------------------------------ 1. against the reference
# blob + sparse noise: the lanes of one wave see from none to hundreds of candidates
R_BLOB = {1: 0.02, 2: 0.08, 3: 0.12, 4: 0.2, 5: 0.3, 8: 0.45}


def _blob_noise(d, dtype):
    rng = np.random.default_rng(40 + d)
    X = np.concatenate([rng.normal(0.0, 0.15, size=(2400, d)),
                        rng.uniform(-2.0, 2.0, size=(600, d))]).astype(dtype)
    rng.shuffle(X)
    # queries: rows of X (self at 0), and points near rows / anywhere in the box
    Q = np.concatenate([X[:1800],
                        X[1800:2700] + rng.normal(0.0, 0.05, size=(900, d)).astype(dtype),
                        rng.uniform(-2.2, 2.2, size=(300, d)).astype(dtype)]).astype(dtype)
    return X, Q


@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8])
def test_blob_and_noise_equal_reference(d, dtype, metric):
    X, Q = _blob_noise(d, dtype)
    r = R_BLOB[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    sm = kdist_ref.smallest(X, 64, metric, Q=Q)
    ix = _index(X, r, metric)
    try:
        dq = _dev(Q)
        for k in KS:
            want = kdist_ref.kth_of(sm, k, r, metric)
            got = ix.kdist(dq, k)
            assert got.dtype == torch.float64 and got.is_cuda and got.shape == (len(Q),)
            if k == 9:
                assert np.isinf(want).sum() > 100        # the noise rows run short
            if k == 64:
                assert np.isfinite(want).sum() > 100     # the blob's centre does not
            assert np.array_equal(_np(got), want), (k, int((_np(got) != want).sum()))
    finally:
        ix.close()


@pytest.mark.parametrize("name,ks,mult", [
    ("lattice_900", KS, (1.0, 2.0)),     # r_max exactly a lattice distance: ties, <= thr
    ("dup_1d", (1, 2, 3, 4, 7), (1.0,)),  # every value three times: k below / above it
    ("ident_40", (1, 8, 39, 40, 41, 64), (1.0,)),   # 40 copies of one point
    ("neg_3k", KS, (1.0,)),
])
def test_golden_point_sets_equal_reference(name, ks, mult):
    X, eps, _, metric = _golden(name)
    sm = kdist_ref.smallest(X, 64, metric)
    for f in mult:
        r = eps * f
        ix = _index(X, r, metric)
        try:
            for k in ks:
                want = kdist_ref.kth_of(sm, k, r, metric)
                assert np.array_equal(_np(ix.kdist(_dev(X), k)), want), (name, f, k)
        finally:
            ix.close()
    if name == "ident_40":
        assert np.array_equal(kdist_ref.kth_of(sm, 40, eps, metric), np.zeros(40))
        assert np.all(np.isinf(kdist_ref.kth_of(sm, 41, eps, metric)))
    if name == "lattice_900":     # the cap sits on a tie: rows at exactly thr are counted
        assert (sm[:, :8] == eps * eps).any()


def test_dense_tiles_above_64_kib_of_lds():
    """d = 64 fp64 with k = 64: the lanes' rows and lists pass the default
    dynamic-LDS limit, the launch that raises it."""
    rng = np.random.default_rng(7)
    X = rng.normal(0.0, 0.1, size=(700, 64))
    r = 1.0                                   # about half the rows have 64 rows that near
    sm = kdist_ref.smallest(X, 64)
    for k in (1, 33, 64):
        want = kdist_ref.kth_of(sm, k, r)
        if k == 64:
            assert 50 < np.isfinite(want).sum() < 650
        assert np.array_equal(_kdist(X, X, k, r), want)


# ------------------------------------------------------------ 2. core-flag identity
_TRAINED = {}


def _trained(name):
    if name not in _TRAINED:
        from pypardis_amd import DBSCAN
        X, eps, ms, metric = _golden(name)
        P = int(load_golden(name)["max_partitions"])
        m = DBSCAN(eps=eps, min_samples=ms, metric=metric,
                   max_partitions=None if P < 0 else P).train(_dev(X))
        _TRAINED[name] = (m, X, eps, ms, metric)
    return _TRAINED[name]


@pytest.mark.parametrize("name", ["b2d_20k", "b3d_20k", "c0_p5_cityblock", "c3_5k"])
def test_core_flag_identity(name):
    m, X, eps, ms, metric = _trained(name)
    core = _np(m.core_sample_mask_).astype(bool)
    assert core.any() and not core.all()
    thr = kdist_ref.threshold(eps, metric)
    for f in (1.0, 2.0):
        got = _kdist(X, X, ms, eps * f, metric)
        assert np.array_equal(got <= thr, core), (name, f)


# ------------------------------------------------------------ 3. cap invariance
def test_cap_invariance():
    X, eps, ms, metric = _golden("b3d_20k")
    r1, r2 = eps, 3 * eps
    for k in (ms, 20):                    # 6,367 and 753 of the rows have k rows within r1
        a = _kdist(X, X, k, r1, metric)
        b = _kdist(X, X, k, r2, metric)
        assert np.isfinite(a).any() and np.isinf(a).any()
        assert np.array_equal(a, np.where(b <= r1 * r1, b, np.inf))


# ------------------------------------------------------------ 4. sorted sweep
def test_cell_sorted_and_direct_sweeps_agree(monkeypatch):
    X, eps, ms, metric = _golden("b2d_20k")
    perm = np.random.default_rng(5).permutation(len(X))
    ix = _index(X, eps, metric)
    try:
        for k in (ms, 20):
            monkeypatch.delenv("PD_INDEX_SORT_MIN", raising=False)
            base = _np(ix.kdist(_dev(X), k))                # 20,000 < 2^18: input order
            monkeypatch.setenv("PD_INDEX_SORT_MIN", "1")    # cell order
            assert np.array_equal(_np(ix.kdist(_dev(X), k)), base)
            assert np.array_equal(_np(ix.kdist(_dev(X[perm]), k)), base[perm])
            monkeypatch.delenv("PD_INDEX_SORT_MIN")
            assert np.array_equal(_np(ix.kdist(_dev(X[perm]), k)), base[perm])
        sub = perm[:2500]
        want = kdist_ref.kdist(X[:3000], ms, eps, metric, Q=X[sub])
        ix3 = _index(X[:3000], eps, metric)
        monkeypatch.setenv("PD_INDEX_SORT_MIN", "1")
        assert np.array_equal(_np(ix3.kdist(_dev(X[sub]), ms)), want)
        ix3.close()
    finally:
        ix.close()


# ------------------------------------------------------------ 5. out of sample
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
    for k in (1, 5, 12):
        want = kdist_ref.kdist(X, k, r, Q=Q)
        assert np.isfinite(want[:300]).any() and np.all(np.isinf(want[300:]))
        assert np.array_equal(_kdist(X, Q, k, r), want)


def test_no_queries_and_fewer_rows_than_k():
    rng = np.random.default_rng(2)
    for d in (3, 6):
        X = rng.uniform(0.0, 1.0, size=(7, d))
        ix = _index(X, 10.0)
        out = ix.kdist(torch.empty((0, d), dtype=torch.float64, device="cuda"), 3)
        assert out.shape == (0,) and out.dtype == torch.float64
        assert np.all(np.isinf(_np(ix.kdist(_dev(X), 8))))           # n < k
        assert np.array_equal(_np(ix.kdist(_dev(X), 7)), kdist_ref.kdist(X, 7, 10.0))
        ix.close()
    # the rows exist but never k of them within the cap
    X = rng.uniform(0.0, 1.0, size=(300, 2))
    want = kdist_ref.kdist(X, 30, 0.05)
    assert np.all(np.isinf(want))
    assert np.array_equal(_kdist(X, X, 30, 0.05), want)


# ------------------------------------------------------------ 6. grown cells
def test_two_blobs_far_apart():
    """1e6 apart at r_max 1e-3: 1e9 cells per axis, so the cells grow (exact at
    any width >= r_max) and the directory follows the 3,000 points."""
    rng = np.random.default_rng(11)
    X = np.concatenate([rng.normal(0.0, 0.003, size=(1500, 2)),
                        rng.normal(0.0, 0.003, size=(1500, 2)) + 1.0e6])
    Q = np.concatenate([X[::2], rng.uniform(4.0e5, 6.0e5, size=(100, 2)),
                        np.array([[1.0e6, 0.0], [-1.0e9, 3.0], [1.0e300, -1.0e300]])])
    r = 1.0e-3
    sm = kdist_ref.smallest(X, 64, Q=Q)
    ix = _index(X, r)
    try:
        for k in (1, 6, 20, 64):
            want = kdist_ref.kth_of(sm, k, r)
            if k == 64:
                assert np.isfinite(want).sum() > 100 and np.isinf(want).sum() > 100
            assert np.array_equal(_np(ix.kdist(_dev(Q), k)), want)
    finally:
        ix.close()


# ------------------------------------------------------------ 7. errors
def test_errors_leave_the_index_usable():
    from pypardis_amd import _native
    X, eps, ms, metric = _golden("neg_3k")
    ix = _index(X, eps, metric)
    want = kdist_ref.kdist(X, ms, eps, metric)
    labels = _np(ix.query(_dev(X)))
    assert np.array_equal(labels, np.zeros(len(X)))           # every row is within eps of itself
    Q = X[:100].copy()
    Q[37, 1] = np.nan
    for k, q, code in ((ms, Q, _native.PD_EINVAL), (0, X, _native.PD_EINVAL),
                       (-1, X, _native.PD_EINVAL), (65, X, -5),
                       (ms, X.astype(np.float64), _native.PD_EINVAL)):      # dtype, as query
        with pytest.raises(_native.PardisError) as e:
            ix.kdist(_dev(q), k)
        assert e.value.code == code, (k, e.value)
    big = np.repeat(X[:3], 4000, axis=0)
    big[5000, 0] = np.inf
    for forced in ("1", None):                                # the sorted sweep's check too
        with pytest.MonkeyPatch.context() as mp:
            if forced:
                mp.setenv("PD_INDEX_SORT_MIN", forced)
            with pytest.raises(_native.PardisError) as e:
                ix.kdist(_dev(big), ms)
            assert e.value.code == _native.PD_EINVAL
    with pytest.raises(ValueError):                           # dimension, as query
        ix.kdist(_dev(np.zeros((5, 3), np.float32)), ms)
    assert np.array_equal(_np(ix.kdist(_dev(X), ms)), want)
    assert np.array_equal(_np(ix.query(_dev(X))), labels)
    ix.close()
    with pytest.raises(ValueError):
        ix.kdist(_dev(X), ms)


def test_rows_above_944_bytes_are_unsupported():
    from pypardis_amd import _native
    X = np.random.default_rng(1).uniform(size=(80, 119))      # 952 bytes per fp64 row
    ix = _index(X, 1.0)
    with pytest.raises(_native.PardisError) as e:
        ix.kdist(_dev(X), 3)
    assert e.value.code == -5
    with pytest.raises(_native.PardisError) as e:             # pd_index_query's own limit
        ix.query(_dev(X))
    assert e.value.code == -5
    ix.close()
    X = X[:, :118].copy()                                     # 944 bytes: the last that fits
    assert np.array_equal(_kdist(X, X, 3, 4.0), kdist_ref.kdist(X, 3, 4.0))
    assert np.array_equal(_kdist(X, X, 64, 4.5), kdist_ref.kdist(X, 64, 4.5))


def test_nan_query_on_the_tile_path():
    from pypardis_amd import _native
    X = np.random.default_rng(4).uniform(size=(200, 6)).astype(np.float32)
    Q = X.copy()
    Q[150, 5] = np.nan
    ix = _index(X, 0.5)
    with pytest.raises(_native.PardisError) as e:
        ix.kdist(_dev(Q), 4)
    assert e.value.code == _native.PD_EINVAL
    assert np.array_equal(_np(ix.kdist(_dev(X), 4)), kdist_ref.kdist(X, 4, 0.5))
    ix.close()


# ------------------------------------------------------------ 8. Python surface
def test_model_k_distances_after_train():
    m, X, eps, ms, metric = _trained("b3d_20k")
    raw = _kdist(X, X, ms, eps, metric)
    got = m.k_distances()
    assert got.dtype == torch.float64 and got.is_cuda
    assert np.array_equal(_np(got), np.sqrt(raw))             # correctly rounded fp64 sqrt
    assert np.array_equal(_np(m.k_distances(squared=True)), raw)
    core = _np(m.core_sample_mask_).astype(bool)
    assert np.array_equal(raw <= eps * eps, core)
    # other k / cap, new queries against the training points
    Q = X[:2000] + np.float32(0.01)
    sub = np.random.default_rng(3).choice(len(X), 3000, replace=False)
    assert np.array_equal(_np(m.k_distances(_dev(Q), k=20, r_max=2 * eps, squared=True)),
                          _kdist(X, Q, 20, 2 * eps, metric))
    # predict's index is untouched
    assert np.array_equal(_np(m.predict(_dev(X[sub]))), _np(m.labels_)[sub])


def test_model_k_distances_cityblock_and_before_train():
    from pypardis_amd import DBSCAN
    m, X, eps, ms, metric = _trained("c0_p5_cityblock")
    want = kdist_ref.kdist(X, ms, eps, metric)
    assert np.array_equal(_np(m.k_distances()), want)         # cityblock: no sqrt
    assert np.array_equal(_np(m.k_distances(squared=True)), want)
    fresh = DBSCAN(eps=eps, min_samples=ms, metric=metric)
    assert np.array_equal(_np(fresh.k_distances(X)), want)    # untrained: data against itself
    assert fresh.labels_ is None
    with pytest.raises(ValueError):
        fresh.k_distances()


def test_module_k_distances_inputs():
    import dbscan
    from pypardis_amd import k_distances
    X, eps, ms, metric = _golden("neg_3k")
    want = kdist_ref.kdist(X, ms, eps, metric)
    assert np.array_equal(_np(k_distances(X, ms, eps, squared=True)), want)
    assert np.array_equal(_np(dbscan.k_distances(_dev(X), ms, eps)), np.sqrt(want))
    recs = [(f"p{i}", X[i]) for i in range(len(X))]           # (key, vector) records
    assert np.array_equal(_np(k_distances(recs, ms, eps, squared=True)), want)
    # queries= a sample; float64 queries of float32 data are rounded to float32 first
    sub = np.random.default_rng(8).choice(len(X), 500, replace=False)
    got = k_distances(X, ms, eps, queries=X[sub].astype(np.float64), squared=True)
    assert got.shape == (500,) and np.array_equal(_np(got), want[sub])
    Q = X[sub] + np.float32(0.03)
    assert np.array_equal(_np(k_distances(X, 3, eps, "cityblock", queries=Q, squared=True)),
                          kdist_ref.kdist(X, 3, eps, "cityblock", Q=Q))
    with pytest.raises(ValueError):
        k_distances(X, ms, eps, queries=np.zeros((4, 3), np.float32))
    bad = X[:50].copy()
    bad[7, 0] = np.inf
    with pytest.raises(ValueError):
        k_distances(X, ms, eps, queries=bad)
    with pytest.raises(ValueError):
        k_distances(bad, ms, eps)
