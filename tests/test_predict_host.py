"""CPU-only checks of DBSCAN.predict's boundary: the library exports the index
entry points, predict refuses an untrained model, and the brute-force
reference the GPU tests compare with (predict_ref.py) reproduces sklearn's
labels on every golden — which also pins the semantics claim
``predict(X_train) == labels_`` against reference-generated data."""
import ctypes

import numpy as np
import pytest

from conftest import golden_names, load_golden
from predict_ref import brute_predict, check_query_mix, make_queries, two_runs_1d


def _metric(g):
    m = str(g["metric"])
    return "euclidean" if m == "callable" else m


def test_library_exports_the_index_entry_points():
    from pypardis_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    for s in ("pd_index_build", "pd_index_query", "pd_index_destroy"):
        assert hasattr(lib, s), s


def test_predict_before_train_raises():
    from pypardis_amd import DBSCAN
    with pytest.raises(ValueError):
        DBSCAN(eps=0.3, min_samples=5).predict(np.zeros((4, 2), np.float32))


def test_predict_after_a_group_train_raises():
    """A rank of a group= train holds only its slice: predict says so (the
    model's state after such a train, set by hand: no process group here)."""
    from pypardis_amd import DBSCAN
    m = DBSCAN(eps=0.3, min_samples=5)
    m.labels_ = np.zeros(4, np.int32)
    m._trained = (0.3, 0)
    m._group_trained = True
    with pytest.raises(ValueError, match="group="):
        m.predict(np.zeros((4, 2), np.float32))


@pytest.mark.parametrize("name", golden_names())
def test_brute_force_reproduces_sklearn_labels(name):
    g = load_golden(name)
    X, core, lab = g["X"], g["sk_core"].astype(bool), g["sk_labels"]
    got = brute_predict(X, X[core], lab[core], float(g["eps"]), _metric(g))
    assert np.array_equal(got, lab)


@pytest.mark.parametrize("name", ["b2d_20k", "b3d_20k", "c3_5k", "c0_p5_cityblock"])
def test_out_of_sample_queries_cover_both_outcomes(name):
    """The input conditions of test_gpu_predict's out-of-sample test, checked
    where no GPU is needed (the labels are sklearn's, which the train equals)."""
    g = load_golden(name)
    X, core, lab = g["X"], g["sk_core"].astype(bool), g["sk_labels"]
    Q = make_queries(X, core, float(g["eps"]))
    lo, hi = brute_predict(Q, X[core], lab[core], float(g["eps"]), _metric(g), spread=True)
    check_query_mix(lo, hi)


def test_constructed_case_has_a_query_near_two_labels():
    X, eps, ms, Q = two_runs_1d()
    core = np.ones(len(X), bool)
    lab = (np.arange(len(X)) > 100).astype(np.int64)
    lo, hi = brute_predict(Q, X[core], lab[core], eps, spread=True)
    assert check_query_mix(lo, hi)
