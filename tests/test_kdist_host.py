"""CPU checks of the k-distance reference (kdist_ref.py) and of the argument
errors of ``k_distances`` that need no GPU."""
import numpy as np
import pytest

import kdist_ref


def _points(d, n=600, seed=0):
    rng = np.random.default_rng(seed + d)
    blob = rng.normal(0.0, 0.2, size=(n - n // 5, d))
    noise = rng.uniform(-2.0, 2.0, size=(n // 5, d))
    return np.concatenate([blob, noise])


@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("d", [1, 2, 3, 5, 8])
def test_reference_equals_sklearn_kd_tree(d, metric):
    """sklearn's kd_tree sums the same per-axis terms in the same order (its
    reduced distance) and takes one sqrt at the end, so the k-th column of
    kneighbors is bit-equal to sqrt(reference): observed difference 0 ulp on
    every case here, asserted as equality."""
    from sklearn.neighbors import NearestNeighbors
    X = _points(d)
    Q = np.concatenate([X[::3], _points(d, 150, seed=50)])
    nn = NearestNeighbors(algorithm="kd_tree", metric=metric).fit(X)
    for k in (1, 4, 10, 33):
        dist, _ = nn.kneighbors(Q, n_neighbors=k)
        acc = kdist_ref.kdist(X, k, 1.0e9, metric, Q=Q)
        want = np.sqrt(acc) if metric == "euclidean" else acc
        assert np.array_equal(want, dist[:, k - 1])


def test_cap_cuts_what_sklearn_finds_beyond_it():
    from sklearn.neighbors import NearestNeighbors
    X = _points(2)
    r = 0.15
    dist, _ = NearestNeighbors(algorithm="kd_tree").fit(X).kneighbors(X, n_neighbors=8)
    got = kdist_ref.kdist(X, 8, r)
    inside = got <= r * r
    assert inside.any() and (~inside).any()
    assert np.all(np.isinf(got[~inside]))
    assert np.array_equal(np.sqrt(got[inside]), dist[inside, 7])
    # nothing the cap cut was within it
    full = kdist_ref.kdist(X, 8, 1.0e9)
    assert np.all(full[~inside] > r * r)


def test_k1_of_self_queries_is_zero_and_n_below_k_is_inf():
    X = _points(3, 200)
    assert np.array_equal(kdist_ref.kdist(X, 1, 0.01), np.zeros(len(X)))
    assert np.all(np.isinf(kdist_ref.kdist(X[:7], 8, 1.0e9)))
    assert np.all(np.isfinite(kdist_ref.kdist(X[:8], 8, 1.0e9)))
    assert kdist_ref.kdist(X, 3, 1.0, Q=X[:0]).shape == (0,)


def test_duplicates_each_count():
    X = np.repeat(np.array([[0.0], [1.0], [5.0]]), 3, axis=0)
    assert np.array_equal(kdist_ref.kdist(X, 3, 10.0), np.zeros(9))
    got = kdist_ref.kdist(X, 4, 10.0)
    assert got.tolist() == [1.0] * 6 + [16.0] * 3
    assert kdist_ref.kdist(X, 4, 10.0, "cityblock").tolist() == [1.0] * 6 + [4.0] * 3


@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
def test_cap_exactly_on_a_lattice_distance(metric):
    """Integer lattice: every accumulator is exact, so a cap equal to a
    lattice distance includes the rows at that distance (<=) and the next
    smaller float excludes them."""
    g = np.arange(7.0)
    X = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    centre = np.array([[3.0, 3.0]])
    # euclidean: 1 + 4 + 4 rows within 2 (0, 1, sqrt 2; then 4 at 2): the 13th is at 2
    # cityblock: 1 + 4 + 8 rows within 2: the 13th is at 2
    at = 4.0 if metric == "euclidean" else 2.0
    assert kdist_ref.kdist(X, 13, 2.0, metric, Q=centre)[0] == at
    assert np.isinf(kdist_ref.kdist(X, 13, np.nextafter(2.0, 0.0), metric, Q=centre)[0])
    k_in = 9 if metric == "euclidean" else 5
    assert np.isfinite(kdist_ref.kdist(X, k_in, np.nextafter(2.0, 0.0), metric, Q=centre)[0])


def test_reference_refuses_more_than_its_cap():
    with pytest.raises(ValueError):
        kdist_ref.kdist(np.zeros((kdist_ref.MAX_N + 1, 2)), 2, 1.0)


@pytest.mark.parametrize("k,r_max", [(0, 1.0), (-3, 1.0), (65, 1.0), (2.5, 1.0), (4, 0.0),
                                     (4, -1.0), (4, float("nan")), (4, float("inf"))])
def test_k_distances_argument_errors(k, r_max):
    """Raised before any device work."""
    from pypardis_amd import DBSCAN, k_distances
    X = np.zeros((10, 2))
    with pytest.raises(ValueError):
        k_distances(X, k, r_max)
    with pytest.raises(ValueError):
        DBSCAN(eps=0.5, min_samples=5).k_distances(X, k=k, r_max=r_max)


def test_k_distances_rejects_other_metrics_and_is_exported_under_both_names():
    import dbscan
    import pypardis_amd
    assert dbscan.k_distances is pypardis_amd.k_distances
    with pytest.raises(ValueError):
        pypardis_amd.k_distances(np.zeros((10, 2)), 3, 1.0, metric="chebyshev")
    m = pypardis_amd.DBSCAN(eps=0.5, min_samples=5)
    with pytest.raises(ValueError):
        m.k_distances()           # before any train, data is required
