"""CPU checks of the k-nearest reference (knn_ref.py) against sklearn's
kd_tree, and of the argument errors of ``kneighbors`` that need no GPU."""
import numpy as np
import pytest

import kdist_ref
import knn_ref
from test_gpu_kdist import _blob_noise

K = 64
MAX_TIED_ROWS = 5


@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8])
def test_reference_equals_sklearn_kd_tree(d, dtype, metric):
    """sklearn's kd_tree sums the same per-axis terms in the same order and
    takes one sqrt at the end, so the distances are bit-equal on every row.
    Its order inside a tie is arbitrary, so the indices are compared on the
    rows whose first k + 1 accumulators are all distinct; at most 5 rows per
    case may tie (seen: 2 at d = 1 fp32, 1 at d = 5 fp32 cityblock, else 0)."""
    from sklearn.neighbors import NearestNeighbors
    X, Q = _blob_noise(d, dtype)
    table = kdist_ref.accumulators(Q, X, metric)
    ids, acc = knn_ref.from_accumulators(table, K, np.inf, metric)
    assert ids.dtype == np.int32 and ids.shape == acc.shape == (len(Q), K)
    assert (ids >= 0).all() and np.isfinite(acc).all()        # uncapped: every row is full
    dist, ind = NearestNeighbors(algorithm="kd_tree", metric=metric).fit(X).kneighbors(
        Q, n_neighbors=K)
    want = np.sqrt(acc) if metric == "euclidean" else acc
    assert np.array_equal(want, dist)                         # 0 ulp, every row
    first = np.sort(np.partition(table, K, axis=1)[:, :K + 1], axis=1)
    tied = (np.diff(first, axis=1) == 0).any(axis=1)
    print(f"d={d} {np.dtype(dtype).name} {metric}: {int(tied.sum())} rows with a tie")
    assert tied.sum() <= MAX_TIED_ROWS
    assert np.array_equal(ids[~tied], ind[~tied])
    # the reference is what its definition says: ascending pairs of the table
    rows = np.arange(len(Q))[:, None]
    assert np.array_equal(table[rows, ids], acc)
    assert np.array_equal(acc[:, K - 1], kdist_ref.kth_of(first, K, 1.0e300, metric))


def test_order_is_acc_then_row_and_the_cap_pads():
    X = np.array([[0.0], [1.0], [1.0], [-1.0], [3.0], [0.0]])
    ids, acc = knn_ref.kneighbors(X, 4, 1.0, Q=np.array([[0.0], [3.0], [9.0]]))
    assert ids.tolist() == [[0, 5, 1, 2], [4, -1, -1, -1], [-1, -1, -1, -1]]
    assert acc[0].tolist() == [0.0, 0.0, 1.0, 1.0]            # the tie at thr is in; row 3 lost it
    assert acc[1].tolist() == [0.0] + [np.inf] * 3 and np.isinf(acc[2]).all()
    ids, acc = knn_ref.kneighbors(X, 8, 10.0, Q=X[:1])        # n < k: the rows, then padding
    assert ids.tolist() == [[0, 5, 1, 2, 3, 4, -1, -1]]
    # labels in place of row numbers: ordered by (acc, label), equal pairs each appear
    ids, acc = knn_ref.kneighbors(X, 5, 1.0, Q=X[:1], labels=[7, 2, 2, 0, 1, 7])
    assert ids.tolist() == [[7, 7, 0, 2, 2]] and acc.tolist() == [[0.0, 0.0, 1.0, 1.0, 1.0]]


@pytest.mark.parametrize("k,r_max", [(0, 1.0), (-3, 1.0), (65, 1.0), (2.5, 1.0), (4, 0.0),
                                     (4, -1.0), (4, float("nan")), (4, float("inf"))])
def test_kneighbors_argument_errors(k, r_max):
    """Raised before any device work."""
    from pypardis_amd import DBSCAN, kneighbors
    X = np.zeros((10, 2))
    with pytest.raises(ValueError):
        kneighbors(X, k, r_max)
    with pytest.raises(ValueError):
        DBSCAN(eps=0.5, min_samples=5).kneighbors(X, k=k, r_max=r_max)


def test_kneighbors_rejects_other_metrics_and_is_exported_under_both_names():
    import dbscan
    import pypardis_amd
    assert dbscan.kneighbors is pypardis_amd.kneighbors
    from pypardis_amd.dbscan import KNeighbors
    assert KNeighbors._fields == ("indices", "distances")
    with pytest.raises(ValueError):
        pypardis_amd.kneighbors(np.zeros((10, 2)), 3, 1.0, metric="chebyshev")
    m = pypardis_amd.DBSCAN(eps=0.5, min_samples=5)
    with pytest.raises(ValueError, match="kneighbors before train needs data"):
        m.kneighbors()            # before any train, data is required
    m._points, m._group_trained = object(), True
    with pytest.raises(ValueError, match="after a group= train needs data"):
        m.kneighbors()
