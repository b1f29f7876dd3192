"""CPU checks of the mutual-reachability forest reference (mreach_ref.py)
against sklearn's DBSCAN and scipy's connected components, and of the argument
errors of ``mutual_reachability_forest`` / ``dbscan_labels`` that need no GPU."""
import numpy as np
import pytest

import kdist_ref
import mreach_ref
from conftest import load_golden

# (golden, r_max / its eps).  At its own eps the lattice has 16 core rows and no
# edge (its step is the eps, and fp32 rounds most steps a bit above); at twice
# the eps the diagonals are in and nearly every weight is tied.
CASES = [("lattice_900", 1.0), ("lattice_900", 2.0), ("ident_40", 1.0), ("dup_1d", 1.0),
         ("neg_3k", 1.0)]
_FOREST = {}


def _golden(name):
    g = load_golden(name)
    return g["X"], float(g["eps"]), int(g["min_samples"])


def _forest(name, mult):
    """One reference forest per case, at r_max = mult * the golden's eps."""
    if (name, mult) not in _FOREST:
        X, eps, ms = _golden(name)
        table = kdist_ref.accumulators(X, X)
        _FOREST[name, mult] = (table,) + mreach_ref.forest_of_table(table, ms, mult * eps)
    return _FOREST[name, mult]


@pytest.mark.parametrize("name,mult", CASES)
def test_cut_equals_sklearn_dbscan_on_the_core_rows(name, mult):
    """The forest is built once at r_max; its cut at r_max, at r_max / 2 and
    at a radius that sits exactly on one of its edges gives sklearn's core
    mask and, on the core rows, sklearn's labels.

    kd_tree's leaf test is the train's predicate (exact at a tie) and is asked
    at all three radii.  brute expands |x - y|^2 into x.x - 2 x.y + y.y, which
    is an ulp or so off: on the lattice's fp32 rows (whose products are exact in
    fp64) it still agrees at every radius, ties included, but with a radius
    exactly on an edge of neg_3k it loses one core row (2645: 1295 against
    1296).  So brute is asked at r_max and r_max / 2 everywhere and at the tied
    radius on the lattice."""
    from sklearn.cluster import DBSCAN
    X, eps, ms = _golden(name)
    eps *= mult
    _, u, v, w, cd = _forest(name, mult)
    assert np.all(u < v) and np.all(np.diff(w) >= 0)
    on_edge = mreach_ref.tie_eps(w, eps)
    if (w > 0).any():                          # ident_40: every weight is 0
        assert on_edge * on_edge in w
    if (name, mult) == ("lattice_900", 2.0):
        assert len(w) > 800 and len(np.unique(w)) < 20
    for e in (eps, eps / 2, on_edge):
        member, labels = mreach_ref.cut((u, v, w), cd, e)
        print(f"{name} eps={e!r}: {int(member.sum())} core rows, {labels.max() + 1} clusters")
        assert np.all(labels[~member] == -1)
        # brute on the rows as stored; kd_tree's leaf test is the train's predicate
        tied = e == on_edge and not name.startswith("lattice")
        for algorithm in ("kd_tree",) if tied else ("brute", "kd_tree"):
            sk = DBSCAN(eps=e, min_samples=ms, algorithm=algorithm).fit(X)
            core = np.zeros(len(X), bool)
            core[sk.core_sample_indices_] = True
            assert np.array_equal(member, core), (name, e, algorithm)
            assert np.array_equal(labels[core], sk.labels_[core]), (name, e, algorithm)


@pytest.mark.parametrize("name,mult", CASES)
def test_edge_count_is_n_minus_the_components_of_the_graph(name, mult):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    X, eps, ms = _golden(name)
    eps *= mult
    table, u, v, w, cd = _forest(name, mult)
    n = len(X)
    gu, gv, gw = mreach_ref.graph_edges(table, cd, eps)
    ncomp, _ = connected_components(coo_matrix((np.ones(len(gu)), (gu, gv)), shape=(n, n)),
                                    directed=False)
    assert len(u) == n - ncomp
    assert ncomp >= int(np.isinf(cd).sum())    # a row with cd = inf is isolated
    # the forest's edges are edges of G, each once
    have = set(zip(gu.tolist(), gv.tolist()))
    mine = list(zip(u.tolist(), v.tolist()))
    assert len(set(mine)) == len(mine) and set(mine) <= have


@pytest.mark.parametrize("name,mult", CASES)
def test_scipy_over_ranks_equals_the_kruskal_loop(name, mult):
    """kruskal_pairs (what the 20,000-row GPU identity test uses) against the
    loop, from the pairs in both directions with the self pairs."""
    X, eps, ms = _golden(name)
    eps *= mult
    table, u, v, w, cd = _forest(name, mult)
    thr = kdist_ref.threshold(eps)
    i, j = np.nonzero(table <= thr)
    got = mreach_ref.kruskal_pairs(len(X), i, j, table[i, j], cd, thr)
    assert all(np.array_equal(a, b) for a, b in zip(got, (u, v, w)))


def test_the_order_decides_between_equal_weights():
    """Four points on a line one apart, k = 1 (cd = 0): every edge weighs 1 and
    the order (w, u, v) picks (0, 1), (1, 2), (2, 3) of the rows as numbered."""
    X = np.array([[2.0], [3.0], [1.0], [0.0]])         # the line is rows 3, 2, 0, 1
    u, v, w, cd = mreach_ref.forest(X, 1, 1.0)
    assert cd.tolist() == [0.0] * 4 and w.tolist() == [1.0] * 3
    assert list(zip(u.tolist(), v.tolist())) == [(0, 1), (0, 2), (2, 3)]
    u, v, w, cd = mreach_ref.forest(X, 3, 1.0)          # ends: fewer than 3 rows within 1
    assert np.isinf(cd[[1, 3]]).all() and cd[[0, 2]].tolist() == [1.0, 1.0]
    assert list(zip(u.tolist(), v.tolist())) == [(0, 2)]
    member, labels = mreach_ref.cut((u, v, w), cd, 1.0)
    assert labels.tolist() == [0, -1, 0, -1] and member.tolist() == [True, False, True, False]


@pytest.mark.parametrize("k,r_max", [(0, 1.0), (-3, 1.0), (65, 1.0), (2.5, 1.0), (4, 0.0),
                                     (4, -1.0), (4, float("nan")), (4, float("inf"))])
def test_forest_argument_errors(k, r_max):
    """Raised before any device work."""
    from pypardis_amd import DBSCAN, mutual_reachability_forest
    X = np.zeros((10, 2))
    with pytest.raises(ValueError):
        mutual_reachability_forest(X, k, r_max)
    with pytest.raises(ValueError):
        DBSCAN(eps=0.5, min_samples=5).mutual_reachability_forest(X, min_samples=k, r_max=r_max)


def test_forest_rejects_other_metrics_and_is_exported_under_both_names():
    import dbscan
    import pypardis_amd
    assert dbscan.mutual_reachability_forest is pypardis_amd.mutual_reachability_forest
    assert dbscan.dbscan_labels is pypardis_amd.dbscan_labels
    assert pypardis_amd.ReachabilityForest._fields == ("u", "v", "distances", "core_distances")
    with pytest.raises(ValueError):
        pypardis_amd.mutual_reachability_forest(np.zeros((10, 2)), 3, 1.0, metric="chebyshev")
    m = pypardis_amd.DBSCAN(eps=0.5, min_samples=5)
    with pytest.raises(ValueError, match="before train needs data"):
        m.mutual_reachability_forest()
    m._points, m._group_trained = object(), True
    with pytest.raises(ValueError, match="after a group= train needs data"):
        m.mutual_reachability_forest()


def test_dbscan_labels_refuses_a_radius_above_the_forest_s():
    """The check reads the forest's record of r_max and squared; no device."""
    import torch
    from pypardis_amd import ReachabilityForest, dbscan_labels
    z = torch.zeros(0, dtype=torch.int32)
    acc = torch.tensor([0.25, 1.0], dtype=torch.float64)
    f = ReachabilityForest(z, z, acc, acc, 1.5, 0, False)
    assert f.distances.tolist() == [0.5, 1.0] and f.accumulators is acc and f.r_max == 1.5
    assert ReachabilityForest(z, z, acc, acc, 1.5, 0, True).distances is acc
    assert ReachabilityForest(z, z, acc, acc, 1.5, 1, False).distances is acc    # cityblock
    for eps, squared in ((1.6, False), (2.3, True), (0.0, False), (float("nan"), False)):
        with pytest.raises(ValueError):
            dbscan_labels(f, eps, squared=squared)
    with pytest.raises(ValueError):
        dbscan_labels(ReachabilityForest(z, z, acc, acc, 1.5, 1, False), 1.6)
