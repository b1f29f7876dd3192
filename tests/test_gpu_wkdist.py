"""pd_index_set_weights / pd_index_kdist_weighted / k_distances(sample_weight=)
on the GPU against the brute-force reference (wkdist_ref.py), the GPU's own
unweighted k_distances and the weighted train.  Every comparison is
np.array_equal on the raw accumulators (inf == inf): no tolerance anywhere."""
import numpy as np
import pytest
import torch

import kdist_ref
import wkdist_ref
from conftest import load_golden
from test_gpu_kdist import R_BLOB, _blob_noise

pytestmark = pytest.mark.gpu

CODE = {"euclidean": 0, "cityblock": 1}
INT03 = ["b2d_20k", "b3d_20k", "lattice_900", "dup_1d", "neg_3k", "ident_40", "c0",
         "c0_p5_cityblock", "blobs4d"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _index(X, r_max, metric="euclidean", weight=None):
    from pypardis_amd import _native
    ix = _native.Index.over_rows(_dev(X), r_max, CODE[metric])
    if weight is not None:
        ix.set_weights(_dev(np.asarray(weight, np.float64)))
    return ix


def _cdw(X, w, Q, k, r_max, metric="euclidean"):
    ix = _index(X, r_max, metric, w)
    try:
        return _np(ix.kdist_weighted(_dev(Q), k))
    finally:
        ix.close()


def _case(name):
    """-> (X, eps, min_samples, metric, weight) of a sw_int03_* golden."""
    if name == "blobs4d":
        from pypardis_amd import synth
        X, eps, ms, metric = synth.blobs_noise(5000, 4), 1.5, 5, "euclidean"
    else:
        g = load_golden(name)
        metric = "cityblock" if str(g["metric"]) == "cityblock" else "euclidean"
        X, eps, ms = g["X"], float(g["eps"]), int(g["min_samples"])
    return X, eps, ms, metric, load_golden(f"int03_{name}", prefix="sw")["weight"]


# ------------------------------------------------------------ 1. random sets
@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8])
def test_blob_and_noise_equal_reference(d, dtype, metric):
    from weighted_ref import fixed_point
    X, Q = _blob_noise(d, dtype)
    w = np.random.default_rng(70 + d).integers(0, 4, size=len(X)).astype(np.float64)
    r = R_BLOB[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    table = wkdist_ref.sorted_table(kdist_ref.accumulators(Q, X, metric), fixed_point(w))
    ix = _index(X, r, metric, w)
    try:
        dq = _dev(Q)
        for k in (1, 3, 8, 9, 33, 64):        # slots = k: every list tier
            want = wkdist_ref.cdw_of_table(None, None, k, r, metric, table=table)
            got = ix.kdist_weighted(dq, k)
            assert got.dtype == torch.float64 and got.is_cuda and got.shape == (len(Q),)
            if k == 9:
                assert np.isinf(want).sum() > 100 and np.isfinite(want).sum() > 100
            assert np.array_equal(_np(got), want), (k, int((_np(got) != want).sum()))
    finally:
        ix.close()


TIERS = [(3, 3.0, 1), (4, 1.0, 4), (5, 1.0, 5), (4, 0.5, 8), (9, 1.0, 9), (8, 0.5, 16),
         (17, 1.0, 17), (8, 0.25, 32), (33, 1.0, 33), (32, 0.5, 64)]


@pytest.mark.parametrize("d", [2, 5])
def test_slot_tiers(d):
    """(min_samples, smallest weight) pairs on both sides of every list tier:
    registers (4, 8 slots) and each LDS block size (16, 32, 64)."""
    from pypardis_amd import _native
    from weighted_ref import fixed_point
    X, Q = _blob_noise(d, np.float32)
    Q = Q[::2]
    r = R_BLOB[d]
    table = kdist_ref.accumulators(Q, X)
    mult = np.random.default_rng(5).integers(0, 4, size=len(X)).astype(np.float64)
    ix = _index(X, r)
    try:
        dq = _dev(Q)
        for k, wmin, slots in TIERS:
            w = mult * wmin
            assert wkdist_ref.slots_needed(w, k) == slots
            ix.set_weights(_dev(w))           # replaces the weights before
            want = wkdist_ref.cdw_of_table(table, fixed_point(w), k, r)
            assert np.isfinite(want).any() and np.isinf(want).any()
            assert np.array_equal(_np(ix.kdist_weighted(dq, k)), want), (k, wmin)
        w = mult * 0.51
        assert wkdist_ref.slots_needed(w, 33) == 65
        ix.set_weights(_dev(w))
        with pytest.raises(_native.PardisError) as e:
            ix.kdist_weighted(dq, 33)
        assert e.value.code == _native.PD_EUNSUPPORTED
        for word in ("min_samples", "33", "sample_weight", "0.51", "64"):
            assert word in str(e.value), str(e.value)
        # the index still answers, weighted and not
        want = wkdist_ref.cdw_of_table(table, fixed_point(w), 32, r)
        assert np.array_equal(_np(ix.kdist_weighted(dq, 32)), want)
        assert np.array_equal(_np(ix.kdist(dq, 6)), kdist_ref.kdist(X, 6, r, Q=Q))
    finally:
        ix.close()
    with pytest.raises(ValueError, match="min_samples"):
        from pypardis_amd import k_distances
        k_distances(X, 33, r, sample_weight=mult * 0.51)


@pytest.mark.parametrize("d", [3, 5])
def test_unit_weights_equal_unweighted(d):
    from pypardis_amd import k_distances
    X, Q = _blob_noise(d, np.float32)
    r = R_BLOB[d]
    for k in (1, 8, 12, 64):
        base = _np(k_distances(X, k, r, queries=Q, squared=True))
        assert np.isinf(base).any() and np.isfinite(base).any()
        got = k_distances(X, k, r, queries=Q, squared=True, sample_weight=np.ones(len(X)))
        assert np.array_equal(_np(got), base), k
    # the square root is taken as in the unweighted call
    a = _np(k_distances(X, 8, r, sample_weight=[1.0] * len(X)))
    assert np.array_equal(a, _np(k_distances(X, 8, r)))


@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("d", [2, 4, 5])
def test_multiplicities_equal_repeated_rows(d, metric):
    """Against the GPU's own unweighted k_distances on the repeated rows."""
    from pypardis_amd import k_distances
    X, _ = _blob_noise(d, np.float64)
    c = np.random.default_rng(d).integers(1, 4, size=len(X))
    c[:20] = 12
    rep = np.repeat(np.arange(len(X)), c)
    r = R_BLOB[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    for k in (5, 10, 20):
        got = _np(k_distances(X, k, r, metric, squared=True, sample_weight=torch.from_numpy(c)))
        want = _np(k_distances(X[rep], k, r, metric, squared=True))
        assert np.array_equal(got[rep], want), k
    # a row of multiplicity >= k is core at 0
    assert np.all(_np(k_distances(X, 12, r, metric, squared=True, sample_weight=c))[:20] == 0.0)


# ------------------------------------------------------------ 2. exact answers
@pytest.mark.parametrize("name", ["lattice_900", "dup_1d"])
def test_ties_and_eviction(name):
    """A lattice whose cap sits on a lattice distance, and a line with every
    value three times: ties at the crossing, at the cap and at the list's end."""
    X, eps, ms, metric, w = _case(name)
    assert set(np.unique(w)) <= {0.0, 1.0, 2.0, 3.0} and (w == 0).any()
    for f in (1.0, 2.0):
        ix = _index(X, eps * f, metric, w)
        try:
            for k in (1, 2, 3, 4, 7, 9, 17, 64):
                want = wkdist_ref.cdw(X, w, k, eps * f, metric)
                assert np.array_equal(_np(ix.kdist_weighted(_dev(X), k)), want), (name, f, k)
        finally:
            ix.close()


def test_one_heavy_row_among_unit_rows():
    rng = np.random.default_rng(11)
    X = rng.uniform(0.0, 1.0, size=(400, 2)).astype(np.float32)
    w = np.ones(len(X))
    w[7] = 30.0
    r, k = 0.08, 30         # no row has 30 rows that near ...
    assert np.all(np.isinf(kdist_ref.kdist(X, k, r)))
    got = _cdw(X, w, X, k, r)
    acc = kdist_ref.accumulators(X, X[7:8])[:, 0]
    near = acc <= r * r
    assert near.sum() > 3
    assert got[7] == 0.0                                   # ... the heavy row is enough alone,
    assert np.array_equal(got[near], acc[near])            # its neighbours cross at it,
    assert np.all(np.isinf(got[~near]))                    # and nobody else crosses
    # fewer rows than min_samples in the whole index: no short cut to inf
    got = _cdw(X[:8], w[:8], X[:8], k, 2.0)
    assert np.array_equal(got, kdist_ref.accumulators(X[:8], X[7:8])[:, 0])


def test_largest_weights_are_clamped():
    rng = np.random.default_rng(12)
    X = rng.uniform(0.0, 1.0, size=(300, 2))
    w = np.full(len(X), 2.0 ** 31)
    assert np.array_equal(_cdw(X, w, X, 64, 0.3), np.zeros(len(X)))
    # every second row weightless: those cross at their nearest weighted row
    w[::2] = 0.0
    got = _cdw(X, w, X, 64, 0.3)
    want = wkdist_ref.cdw(X, w, 64, 0.3)
    assert np.all(want[1::2] == 0.0) and np.all(want[::2] > 0.0)
    assert np.array_equal(got, want)
    # mixed with unit rows the sum of a full 64-slot list passes 32 bits
    w = np.where(rng.uniform(size=len(X)) < 0.5, 1.0, 2.0 ** 31)
    Xc = np.repeat(X[:1], 300, axis=0)                     # all rows tie at 0
    assert np.array_equal(_cdw(Xc, w, Xc, 64, 0.3), np.zeros(300))


@pytest.mark.parametrize("d", [2, 6])
def test_zero_weights(d):
    rng = np.random.default_rng(13)
    X = rng.uniform(0.0, 1.0, size=(500, d))
    r = 0.1 if d == 2 else 0.5
    assert np.all(np.isinf(_cdw(X, np.zeros(len(X)), X, 1, r)))
    w = np.ones(len(X))
    w[:100] = 0.0                                          # zero-weight query rows
    got = _cdw(X, w, X, 3, r)
    want = wkdist_ref.cdw(X, w, 3, r)
    assert np.isfinite(want[:100]).any() and np.all(want[:100][np.isfinite(want[:100])] > 0.0)
    assert np.array_equal(got, want)
    # weightless rows add nothing: the others see only each other
    assert np.array_equal(want[100:], kdist_ref.kdist(X[100:], 3, r, Q=X[100:]))


@pytest.mark.parametrize("d", [2, 5])
def test_queries_outside_the_box(d):
    rng = np.random.default_rng(9)
    X = rng.uniform(0.0, 1.0, size=(1500, d)).astype(np.float32)
    w = rng.integers(0, 4, size=len(X)).astype(np.float64)
    r = 0.25 if d == 2 else 0.6
    near = X[:300].copy()
    near[:, 0] = -0.5 * r
    far = X[:300].copy()
    far[:, 0] = -2.5 * r
    Q = np.concatenate([near, far, np.full((3, d), 1.0e30, np.float32)])
    for k in (1, 5, 12):
        want = wkdist_ref.cdw(X, w, k, r, Q=Q)
        assert np.isfinite(want[:300]).any() and np.all(np.isinf(want[300:]))
        assert np.array_equal(_cdw(X, w, Q, k, r), want)


# ------------------------------------------------------------ 3. shapes and sweeps
@pytest.mark.parametrize("d", [3, 5])
def test_query_shapes(d):
    """queries= of another length than the data, m = 0, and at d = 5 a row
    count that is no multiple of any tile size."""
    from pypardis_amd import k_distances
    rng = np.random.default_rng(14)
    X = rng.normal(0.0, 0.3, size=(1237, d))
    w = rng.integers(0, 4, size=len(X)).astype(np.float64)
    Q = rng.normal(0.0, 0.3, size=(411, d))
    r = 0.3 if d == 3 else 0.6
    got = k_distances(X, 6, r, queries=Q, squared=True, sample_weight=w)
    want = wkdist_ref.cdw(X, w, 6, r, Q=Q)
    assert np.isfinite(want).any() and np.isinf(want).any()
    assert np.array_equal(_np(got), want)
    empty = k_distances(X, 6, r, queries=np.zeros((0, d)), sample_weight=w)
    assert empty.shape == (0,) and empty.dtype == torch.float64
    with pytest.raises(ValueError):
        k_distances(X, 6, r, queries=Q, sample_weight=w[:411])    # one per row of data


def test_cell_sorted_and_direct_sweeps_agree(monkeypatch):
    X, eps, ms, metric, w = _case("b2d_20k")
    perm = np.random.default_rng(5).permutation(len(X))
    ix = _index(X, eps, metric, w)
    try:
        for k in (ms, 20):
            monkeypatch.delenv("PD_INDEX_SORT_MIN", raising=False)
            base = _np(ix.kdist_weighted(_dev(X), k))          # 20,000 < 2^18: input order
            monkeypatch.setenv("PD_INDEX_SORT_MIN", "1")       # cell order
            assert np.array_equal(_np(ix.kdist_weighted(_dev(X), k)), base)
            assert np.array_equal(_np(ix.kdist_weighted(_dev(X[perm]), k)), base[perm])
            monkeypatch.delenv("PD_INDEX_SORT_MIN")
            assert np.array_equal(_np(ix.kdist_weighted(_dev(X[perm]), k)), base[perm])
        sub = perm[:2500]
        want = wkdist_ref.cdw(X[:3000], w[:3000], ms, eps, metric, Q=X[sub])
        ix3 = _index(X[:3000], eps, metric, w[:3000])
        monkeypatch.setenv("PD_INDEX_SORT_MIN", "1")
        assert np.array_equal(_np(ix3.kdist_weighted(_dev(X[sub]), ms)), want)
        ix3.close()
    finally:
        ix.close()


# ------------------------------------------------------------ 4. the train link
@pytest.mark.parametrize("name", INT03)
def test_core_mask_of_the_weighted_train(name):
    from pypardis_amd import DBSCAN, k_distances
    X, eps, ms, metric, w = _case(name)
    thr = kdist_ref.threshold(eps, metric)
    cd = _np(k_distances(X, ms, eps, metric, squared=True, sample_weight=w))
    for P in (1, 8):
        m = DBSCAN(eps=eps, min_samples=ms, metric=metric, max_partitions=P)
        m.train(_dev(X), sample_weight=w)
        core = _np(m.core_sample_mask_).astype(bool)
        assert np.array_equal(cd <= thr, core), (name, P)
        assert m.sample_weight_ is not None and m.sample_weight_.dtype == torch.float64
        assert np.array_equal(_np(m.k_distances(squared=True)), cd)     # the train's weights
    if name in ("b2d_20k", "c0"):
        # a larger cap changes nothing below eps; an unweighted train forgets the weights
        cd2 = _np(m.k_distances(r_max=2 * eps, squared=True))
        assert np.array_equal(cd2 <= thr, core)
        plain = _np(m.train(_dev(X)).k_distances(squared=True))
        assert m.sample_weight_ is None
        assert np.array_equal(plain, _np(k_distances(X, ms, eps, metric, squared=True)))
        assert not np.array_equal(plain, cd)


# ------------------------------------------------------------ 5. errors
def test_errors_leave_the_index_usable():
    from pypardis_amd import DBSCAN, _native, k_distances
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(2000, 2)).astype(np.float32)
    w = rng.integers(0, 4, size=len(X)).astype(np.float64)
    r = 0.05
    want = wkdist_ref.cdw(X, w, 6, r)
    ix = _index(X, r)
    with pytest.raises(_native.PardisError) as e:              # before set_weights
        ix.kdist_weighted(_dev(X), 6)
    assert e.value.code == _native.PD_EINVAL and "pd_index_set_weights" in str(e.value)
    with pytest.raises(_native.PardisError) as e:
        ix.mreach_forest(6, weighted=True)
    assert e.value.code == _native.PD_EINVAL
    for bad in (-1.0, float("nan"), float("inf"), 2.0 ** 31 + 1024.0):
        wb = w.copy()
        wb[1234] = bad
        with pytest.raises(_native.PardisError) as e:
            ix.set_weights(_dev(wb))
        assert e.value.code == _native.PD_EINVAL and "sample_weight" in str(e.value), bad
        with pytest.raises(ValueError, match="sample_weight"):
            k_distances(X, 6, r, sample_weight=wb)
    ix.set_weights(_dev(w))
    assert np.array_equal(_np(ix.kdist_weighted(_dev(X), 6)), want)
    for k, code in ((0, _native.PD_EINVAL), (-2, _native.PD_EINVAL), (65, -5)):
        with pytest.raises(_native.PardisError) as e:
            ix.kdist_weighted(_dev(X), k)
        assert e.value.code == code, k
    with pytest.raises(_native.PardisError) as e:              # the queries' dtype
        ix.kdist_weighted(_dev(X.astype(np.float64)), 6)
    assert e.value.code == _native.PD_EINVAL
    nan = X.copy()
    nan[5, 1] = np.nan
    with pytest.raises(_native.PardisError) as e:
        ix.kdist_weighted(_dev(nan), 6)
    assert e.value.code == _native.PD_EINVAL and "NaN" in str(e.value)
    with pytest.raises((TypeError, ValueError)):
        ix.set_weights(_dev(w[:-1]))
    assert np.array_equal(_np(ix.kdist_weighted(_dev(X), 6)), want)
    assert np.array_equal(_np(ix.kdist(_dev(X), 6)), kdist_ref.kdist(X, 6, r))
    ix.close()
    with pytest.raises(ValueError):
        ix.set_weights(_dev(w))
    # weights on a predict index, and on an index whose labels are no row numbers
    m = DBSCAN(eps=r, min_samples=6).train(_dev(X))
    px = _native.Index(_dev(X), m.core_sample_mask_, m.labels_, r)
    assert 0 < px.n_core < len(X)
    with pytest.raises(_native.PardisError) as e:
        px.set_weights(_dev(w[:px.n_core]))
    assert e.value.code == _native.PD_EINVAL
    assert np.array_equal(_np(px.query(_dev(X))), _np(m.labels_))
    px.close()
    ax = _native.Index.over_all(_dev(X), r)
    with pytest.raises(_native.PardisError) as e:
        ax.set_weights(_dev(w))
    assert e.value.code == _native.PD_EINVAL and "row numbers" in str(e.value)
    assert np.array_equal(_np(ax.kdist(_dev(X), 6)), kdist_ref.kdist(X, 6, r))
    ax.close()
