"""The weighted core accumulator's reference (wkdist_ref.py) against the other
references, on the CPU: unit weights are kdist_ref, the core mask and the core
labels are weighted_ref's, multiplicities are repeated rows, and the bounded
list a kernel holds gives the unbounded definition's values."""
import numpy as np
import pytest

import kdist_ref
import mreach_ref
import wkdist_ref
from weighted_ref import weighted_dbscan

METRICS = ["euclidean", "cityblock"]


def _set(d, n=320, seed=0):
    rng = np.random.default_rng(100 * d + seed)
    X = np.concatenate([rng.normal(0.0, 0.2, size=(n * 3 // 4, d)),
                        rng.uniform(-1.5, 1.5, size=(n - n * 3 // 4, d))])
    X[: n // 8] = X[n // 8: n // 4]                    # duplicates: ties at 0
    X = np.round(X * 16.0) / 16.0 if d <= 2 else X     # a lattice: ties everywhere
    rng.shuffle(X)
    return X, rng


R = {2: 0.3, 3: 0.45, 8: 1.1}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [2, 3, 8])
def test_unit_weights_equal_kdist(d, metric):
    X, _ = _set(d)
    r = R[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    for k in (1, 4, 9):
        got = wkdist_ref.cdw(X, np.ones(len(X)), k, r, metric)
        assert np.array_equal(got, kdist_ref.kdist(X, k, r, metric))
    assert np.isinf(got).any() and np.isfinite(got).any()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [2, 3, 8])
def test_core_mask_and_core_labels_of_the_weighted_train(d, metric):
    X, rng = _set(d)
    w = rng.integers(0, 4, size=len(X)).astype(np.float64)
    r = R[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    k = 5
    fu, fv, fw, cd = wkdist_ref.forest(X, w, k, r, metric)
    assert (w[np.isfinite(cd)] == 0).any()      # a zero-weight row can be core
    for eps in (r, 0.7 * r, 0.4 * r):
        labels, core = weighted_dbscan(X, eps, k, w, metric)
        assert np.array_equal(cd <= kdist_ref.threshold(eps, metric), core)
        member, cut = mreach_ref.cut((fu, fv, fw), cd, eps, metric)
        assert np.array_equal(member, core)
        # both number the clusters by their smallest core row
        assert np.array_equal(cut, np.where(core, labels, -1))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [2, 3, 8])
def test_multiplicities_are_repeated_rows(d, metric):
    X, rng = _set(d, n=200)
    c = rng.integers(1, 4, size=len(X))
    c[:5] = 7                                           # rows of weight >= k
    r = R[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    k = 6
    rep = np.repeat(np.arange(len(X)), c)
    Xe = X[rep]
    fu, fv, fw, cd = wkdist_ref.forest(X, c.astype(np.float64), k, r, metric)
    eu, ev, ew, ecd = mreach_ref.forest(Xe, k, r, metric)
    assert np.array_equal(ecd, cd[rep])
    extra = np.repeat(cd, c - 1)
    want = np.sort(np.concatenate([fw, extra[np.isfinite(extra)]]))
    assert np.array_equal(np.sort(ew), want)
    # the copies of a heavy row hang together at 0 in the expanded forest only
    assert ew[0] == 0.0 and np.all(cd[:5] == 0.0)


def test_heavy_distinct_rows_give_no_zero_edge():
    rng = np.random.default_rng(3)
    X = rng.uniform(0.0, 1.0, size=(150, 2))
    c = rng.integers(4, 7, size=len(X))
    fu, fv, fw, cd = wkdist_ref.forest(X, c.astype(np.float64), 4, 0.2)
    assert len(fw) and fw[0] > 0.0 and np.all(cd == 0.0)
    ew = mreach_ref.forest(X[np.repeat(np.arange(len(X)), c)], 4, 0.2)[2]
    assert ew[0] == 0.0


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [2, 3, 8])
def test_bounded_list_equals_unbounded(d, metric):
    X, rng = _set(d, n=160)
    r = R[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    Q = np.concatenate([X[:60], X[:30] + 0.01, rng.uniform(-1.6, 1.6, size=(20, d))])
    for w, k in ((rng.integers(0, 4, size=len(X)).astype(np.float64), 5),
                 (rng.choice([0.0, 0.5, 1.0, 2.5], size=len(X)), 7),
                 (rng.choice([0.0, 0.5, 1.0, 2.5], size=len(X)), 32)):
        assert wkdist_ref.slots_needed(w, k) in (5, 14, 64)
        got = wkdist_ref.cdw_bounded(X, w, k, r, metric, Q=Q, rng=rng)
        assert np.array_equal(got, wkdist_ref.cdw(X, w, k, r, metric, Q=Q))
    with pytest.raises(ValueError):
        wkdist_ref.cdw_bounded(X, w, 33, r, metric, Q=Q)    # 66 slots


def test_zero_and_heavy_weights():
    X = np.array([[0.0], [0.1], [0.2], [0.3], [5.0]])
    w = np.array([0.0, 1.0, 3.0, 1.0, 9.0])
    got = wkdist_ref.cdw(X, w, 3, 0.25)
    # row 0 (weight 0) needs rows 1 and 2; row 2 is enough alone; row 4 too
    assert np.array_equal(got, [(0.0 - 0.2) ** 2, (0.1 - 0.2) ** 2, 0.0, (0.3 - 0.2) ** 2, 0.0])
    assert np.all(np.isinf(wkdist_ref.cdw(X, np.zeros(5), 1, 0.25)))
    assert np.array_equal(wkdist_ref.cdw(X, np.full(5, 2.0 ** 31), 64, 0.25), np.zeros(5))


def test_argument_errors_before_any_device_work():
    from pypardis_amd import DBSCAN, k_distances, mutual_reachability_forest
    X = np.zeros((10, 2))
    for bad in (np.ones(9), np.ones((10, 1)), [1.0] * 11):
        with pytest.raises(ValueError):
            k_distances(X, 3, 1.0, sample_weight=bad)
        with pytest.raises(ValueError):
            mutual_reachability_forest(X, 3, 1.0, sample_weight=bad)
        with pytest.raises(ValueError):
            DBSCAN(eps=0.5, min_samples=3).k_distances(X, sample_weight=bad)
    m = DBSCAN(eps=0.5, min_samples=3)
    with pytest.raises(ValueError):
        m.k_distances(sample_weight=np.ones(10))            # explicit weights need data=
    with pytest.raises(ValueError):
        m.mutual_reachability_forest(sample_weight=np.ones(10))
    assert m.sample_weight_ is None
