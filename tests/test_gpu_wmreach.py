"""pd_index_mreach_forest_weighted / mutual_reachability_forest(sample_weight=)
on the GPU against the brute-force reference (wkdist_ref.forest), the weighted
train and the GPU's own unweighted forest of the repeated rows.  Under the
order (w, u, v) the forest is ONE edge list: every comparison is
np.array_equal on the raw row numbers and accumulators."""
import numpy as np
import pytest
import torch

import kdist_ref
import mreach_ref
import wkdist_ref
from test_gpu_kdist import R_BLOB, _blob_noise
from test_gpu_wkdist import INT03, _case, _dev, _index, _np

pytestmark = pytest.mark.gpu


def _ask(ix, k):
    u, v, w, cd, rounds = ix.mreach_forest(k, weighted=True)
    assert u.is_cuda and u.dtype == v.dtype == torch.int32
    assert w.dtype == cd.dtype == torch.float64
    assert u.shape == v.shape == w.shape and cd.shape == (ix.n_core,)
    return (_np(u), _np(v), _np(w), _np(cd))


def _equal(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def _diff(got, want):
    if len(got[0]) != len(want[0]):
        return f"{len(got[0])} edges, the reference has {len(want[0])}"
    return [int((a != b).sum()) for a, b in zip(got, want)]


# ------------------------------------------------------------ 1. edge for edge
@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_forest_equals_reference(d, dtype, metric):
    X, _ = _blob_noise(d, dtype)
    X = X[:2000]
    X[:100] = X[100:200]                       # duplicates: zero edges, ties
    rng = np.random.default_rng(80 + d)
    r = R_BLOB[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    for w, k in ((rng.integers(0, 4, size=len(X)).astype(np.float64), 6),
                 (rng.integers(0, 5, size=len(X)) * 0.5, 4)):        # half weights: 8 slots
        want = wkdist_ref.forest(X, w, k, r, metric)
        assert 0 < len(want[0]) < len(X) - 1 and np.isinf(want[3]).any()
        ix = _index(X, r, metric, w)
        try:
            got = _ask(ix, k)
        finally:
            ix.close()
        assert _equal(got, want), _diff(got, want)


# ------------------------------------------------------------ 2. the train link
@pytest.mark.parametrize("name", INT03)
def test_cuts_equal_the_weighted_train(name):
    """One forest, three eps: each cut is the weighted train at that eps on its
    core rows, -1 elsewhere."""
    from pypardis_amd import DBSCAN, dbscan_labels, mutual_reachability_forest
    from weighted_ref import weighted_dbscan
    X, eps, ms, metric, w = _case(name)
    forest = mutual_reachability_forest(X, ms, eps, metric, sample_weight=w)
    assert forest.sample_weight is not None and forest.sample_weight.dtype == torch.float64
    for f in (1.0, 0.7, 0.4):
        m = DBSCAN(eps=eps * f, min_samples=ms, metric=metric, max_partitions=8 if f == 1.0 else 1)
        m.train(_dev(X), sample_weight=w)
        core = _np(m.core_sample_mask_).astype(bool)
        want = np.where(core, _np(m.labels_), -1)
        # the train ranks the clusters over border rows too, the cut over the
        # member rows: both by smallest core row, so the numbers agree
        got = _np(dbscan_labels(forest, eps * f))
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, f)
        if len(X) <= 3000:
            labels, rcore = weighted_dbscan(X, eps * f, ms, w, metric)
            assert np.array_equal(got, np.where(rcore, labels, -1)), (name, f)
        if f == 1.0:
            mf = m.mutual_reachability_forest()              # the train's weights
            assert mf.sample_weight is m.sample_weight_
            assert all(torch.equal(a, b) for a, b in zip(mf, forest))


# ------------------------------------------------------------ 3. expansion
@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("d", [2, 3])
def test_multiplicities_against_the_repeated_rows(d, metric):
    from pypardis_amd import mutual_reachability_forest
    rng = np.random.default_rng(90 + d)
    X = np.unique(_blob_noise(d, np.float32)[0], axis=0)    # distinct rows
    rng.shuffle(X)
    c = rng.integers(1, 4, size=len(X))
    k = 5
    c[:15] = k + 2                                          # a few rows of weight >= k
    rep = np.repeat(np.arange(len(X)), c)
    r = R_BLOB[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    fw = mutual_reachability_forest(X, k, r, metric, squared=True, sample_weight=c)
    fe = mutual_reachability_forest(X[rep], k, r, metric, squared=True)
    cd = _np(fw.core_distances)
    assert np.array_equal(_np(fe.core_distances), cd[rep])
    extra = np.repeat(cd, c - 1)
    want = np.sort(np.concatenate([_np(fw.distances), extra[np.isfinite(extra)]]))
    assert np.array_equal(_np(fe.distances), want)
    # the heavy rows' copies hang together at 0; distinct rows never do
    assert float(fe.distances[0]) == 0.0 and float(fw.distances[0]) > 0.0


# ------------------------------------------------------------ 4. what a weighted forest refuses
def test_condensed_tree_refuses_a_weighted_forest():
    from pypardis_amd import (DBSCAN, condensed_tree, dbscan_labels, hdbscan_labels,
                              mutual_reachability_forest)
    X, _ = _blob_noise(2, np.float32)
    X = np.unique(X, axis=0)
    w = np.random.default_rng(1).integers(1, 4, size=len(X)).astype(np.float64)
    r = R_BLOB[2]
    fw = mutual_reachability_forest(X, 5, r, sample_weight=w)
    for call in (lambda: condensed_tree(fw, 5), lambda: hdbscan_labels(fw, 5)):
        with pytest.raises(ValueError, match="not supported yet"):
            call()
    assert int(dbscan_labels(fw, r).max()) >= 0             # the cut still works
    labels, prob = hdbscan_labels(mutual_reachability_forest(X, 5, r), 5)   # unweighted: fine
    assert labels.shape == (len(X),)
    # the model's hdbscan builds its own, unweighted forest, also after a weighted train
    m = DBSCAN(eps=r, min_samples=5).train(_dev(X), sample_weight=w)
    ml, mp = m.hdbscan(5, min_samples=5)
    assert torch.equal(ml, labels) and torch.equal(mp, prob)


# ------------------------------------------------------------ 5. errors
def test_errors_leave_the_index_usable():
    from pypardis_amd import _native, mutual_reachability_forest
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(2000, 2)).astype(np.float32)
    w = rng.integers(0, 4, size=len(X)).astype(np.float64)
    r = 0.05
    want = wkdist_ref.forest(X, w, 6, r)
    ix = _index(X, r, weight=w)
    for k, cap, code in ((0, None, _native.PD_EINVAL), (65, None, -5),
                         (6, len(X) - 2, _native.PD_EINVAL)):
        with pytest.raises(_native.PardisError) as e:
            ix.mreach_forest(k, capacity=cap, weighted=True)
        assert e.value.code == code, (k, cap, e.value)
    ix.set_weights(_dev(w * 0.01))                         # 600 slots
    with pytest.raises(_native.PardisError) as e:
        ix.mreach_forest(6, weighted=True)
    assert e.value.code == _native.PD_EUNSUPPORTED and "min_samples" in str(e.value)
    ix.set_weights(_dev(w))
    got = _ask(ix, 6)
    assert _equal(got, want), _diff(got, want)
    # the unweighted forest of the same index is untouched by the weights
    u, v, a, cd, _ = ix.mreach_forest(6)
    assert _equal((_np(u), _np(v), _np(a), _np(cd)), mreach_ref.forest(X, 6, r))
    ix.close()
    # d > 4: unsupported, and the index still answers
    X8 = rng.uniform(size=(500, 8))
    w8 = rng.integers(0, 4, size=len(X8)).astype(np.float64)
    ix = _index(X8, 0.5, weight=w8)
    with pytest.raises(_native.PardisError) as e:
        ix.mreach_forest(3, weighted=True)
    assert e.value.code == -5 and "8" in str(e.value)
    assert np.array_equal(_np(ix.kdist_weighted(_dev(X8), 3)), wkdist_ref.cdw(X8, w8, 3, 0.5))
    assert np.array_equal(_np(ix.kdist(_dev(X8), 3)), kdist_ref.kdist(X8, 3, 0.5))
    ix.close()
    with pytest.raises(ValueError):
        mutual_reachability_forest(X8, 3, 0.5, sample_weight=w8)
    with pytest.raises(ValueError, match="sample_weight"):
        mutual_reachability_forest(X, 6, r, sample_weight=-w)
