"""CPU checks of the radius-neighbour reference (radius_ref.py): against
sklearn's kd_tree, the labels-from-graph derivation against the goldens, and
the argument errors of ``radius_neighbors`` that need no GPU."""
import numpy as np
import pytest

import radius_ref
from conftest import load_golden
from test_kdist_host import _points

RADII = (0.05, 0.15, 0.4, 1.0)
GRAPH_GOLDENS = ["b2d_20k", "b3d_20k", "lattice_900", "dup_1d", "ident_40", "neg_3k", "c0",
                 "c0_p5_cityblock"]


def _golden(name):
    g = load_golden(name)
    metric = "cityblock" if str(g["metric"]) == "cityblock" else "euclidean"
    return g, g["X"], float(g["eps"]), int(g["min_samples"]), metric


@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("d", [1, 2, 3, 5, 8])
def test_reference_equals_sklearn_kd_tree(d, metric):
    """sklearn's kd_tree tests the same per-axis sum against r * r (its reduced
    distance) and takes one sqrt of what it returns: the index sets and the
    distances are equal, row by row, with no tolerance."""
    from sklearn.neighbors import NearestNeighbors
    X = _points(d)
    Q = np.concatenate([X[::3], _points(d, 150, seed=50)])
    nn = NearestNeighbors(algorithm="kd_tree", metric=metric).fit(X)
    for r in RADII:
        dist, ind = nn.radius_neighbors(Q, r, return_distance=True)
        indptr, indices, acc = radius_ref.radius_neighbors(X, r, metric, Q=Q)
        want = np.sqrt(acc) if metric == "euclidean" else acc
        assert indptr[0] == 0 and indptr[-1] == len(indices) == sum(len(i) for i in ind)
        bad = 0
        for q in range(len(Q)):
            o = np.argsort(ind[q], kind="stable")
            s = slice(indptr[q], indptr[q + 1])
            bad += not (np.array_equal(ind[q][o], indices[s]) and
                        np.array_equal(dist[q][o], want[s]))
        assert bad == 0, (d, metric, r, bad)
    assert len(indices) > len(Q)          # the widest radius finds more than the queries themselves


@pytest.mark.parametrize("name", GRAPH_GOLDENS)
def test_labels_from_the_graph_equal_sklearn(name):
    """Core flags, counts and labels of sklearn's DBSCAN follow from the
    brute-force eps-graph alone."""
    g, X, eps, ms, metric = _golden(name)
    if len(X) <= 3000:
        indptr, indices, _ = radius_ref.radius_neighbors(X, eps, metric)
    else:
        indptr, indices, _ = radius_ref.radius_neighbors_blocked(X, eps, metric)
    assert np.array_equal(np.diff(indptr), g["sk_counts"])
    labels, core = radius_ref.labels_from_graph(indptr, indices, ms)
    assert np.array_equal(core, g["sk_core"].astype(bool))
    assert np.array_equal(labels, g["sk_labels"])


def test_blocked_reference_equals_the_plain_one():
    X = _points(3, 700)
    a = radius_ref.radius_neighbors(X, 0.3)
    b = radius_ref.radius_neighbors_blocked(X, 0.3, block=256)
    assert a[0][-1] > len(X)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and np.array_equal(u, v)


def test_ties_duplicates_and_self():
    X = np.repeat(np.array([[0.0], [1.0], [5.0]]), 2, axis=0)
    indptr, indices, acc = radius_ref.radius_neighbors(X, 1.0)      # 1.0 is a tie: in
    assert np.diff(indptr).tolist() == [4, 4, 4, 4, 2, 2]
    assert indices[:4].tolist() == [0, 1, 2, 3] and acc[:4].tolist() == [0.0, 0.0, 1.0, 1.0]
    indptr, _, _ = radius_ref.radius_neighbors(X, np.nextafter(1.0, 0.0))
    assert np.diff(indptr).tolist() == [2] * 6
    indptr, indices, acc = radius_ref.radius_neighbors(X, 4.0, "cityblock", Q=np.array([[3.0]]))
    assert indices.tolist() == [0, 1, 2, 3, 4, 5] and acc.tolist() == [3.0, 3.0, 2.0, 2.0, 2.0, 2.0]
    i2, a2 = radius_ref.sort_rows(indptr, indices[::-1], acc[::-1])
    assert np.array_equal(i2, indices) and np.array_equal(a2, acc)


def test_reference_refuses_more_than_its_cap():
    with pytest.raises(ValueError):
        radius_ref.radius_neighbors(np.zeros((3001, 2)), 1.0)


@pytest.mark.parametrize("radius", [0.0, -1.0, float("nan"), float("inf")])
def test_radius_neighbors_argument_errors(radius):
    """Raised before any device work."""
    from pypardis_amd import DBSCAN, radius_neighbors
    X = np.zeros((10, 2))
    with pytest.raises(ValueError):
        radius_neighbors(X, radius)
    with pytest.raises(ValueError):
        DBSCAN(eps=0.5, min_samples=5).radius_neighbors(X, radius=radius)


def test_radius_neighbors_rejects_other_metrics_and_is_exported_under_both_names():
    import dbscan
    import pypardis_amd
    assert dbscan.radius_neighbors is pypardis_amd.radius_neighbors
    with pytest.raises(ValueError):
        pypardis_amd.radius_neighbors(np.zeros((10, 2)), 1.0, metric="chebyshev")
    m = pypardis_amd.DBSCAN(eps=0.5, min_samples=5)
    with pytest.raises(ValueError):
        m.radius_neighbors()          # before any train, data is required
    assert pypardis_amd.dbscan.RadiusNeighbors._fields == ("indptr", "indices", "distances")


def test_binding_declares_the_count_and_fill_pair():
    from pypardis_amd import _native
    assert "pd_index_radius_count" in _native.EXPORTS
    assert "pd_index_radius_fill" in _native.EXPORTS
    assert hasattr(_native.Index, "radius") and hasattr(_native.Index, "over_rows")
