"""CPU checks of the HDBSCAN reference (hdbscan_ref.py): the staged
decomposition the GPU runs equals the sequential top-down definition, and the
definition equals sklearn's HDBSCAN where the spanning tree has no ties."""
import numpy as np
import pytest

import hdbscan_ref
import mreach_ref


def _cases():
    rng = np.random.default_rng(2024)
    for i in range(400):
        n = int(rng.integers(2, 121))
        n_comp = 1 if i % 3 else int(rng.integers(1, min(n, 6) + 1))
        yield i, n, hdbscan_ref.random_forest(rng, n, n_comp), int(rng.integers(2, 9))


def test_staged_equals_sequential_on_random_forests():
    """Fall-out edge per row, true-split set, point partition and cluster-tree
    parents, on 400 random forests (n <= 120, m = 2..8, up to 6 components);
    the round count stays within m - 1."""
    splits = clusters = 0
    for i, n, (u, v, w), m in _cases():
        want = hdbscan_ref.sequential(n, u, v, w, m, root=False)
        got = hdbscan_ref.staged(n, u, v, w, m)
        for key in ("fall", "splits", "point_cluster", "parent"):
            assert np.array_equal(got[key], want[key]), (i, n, m, key)
        assert 1 <= got["rounds"] <= m - 1, (i, got["rounds"], m)
        splits += len(want["splits"])
        clusters += len(want["parent"])
    assert splits > 400 and clusters > 1500      # the cases do exercise the tree


def test_tree_invariants_on_random_forests():
    for i, n, (u, v, w), m in _cases():
        if i % 4:
            continue
        r = hdbscan_ref.sequential(n, u, v, w, m, root=False)
        C = len(r["parent"])
        assert np.all((r["parent"] == -1) | (r["parent"] > np.arange(C)))
        assert np.all(r["size"] >= m) and np.all(r["stability"] >= 0)
        assert np.all(r["death"] == r["lambda_max"])
        assert np.all(r["death"] >= r["birth"])
        top = r["parent"] < 0
        assert r["size"][top].sum() == (r["point_cluster"] >= 0).sum()
        assert np.all((r["probabilities"] >= 0) & (r["probabilities"] <= 1))
        assert np.array_equal(r["labels"] >= 0, r["probabilities"] > 0)


def test_selection_rules():
    # one root (2) with two leaves: the root wins only when allowed and heavier
    parent = np.array([2, 2, -1])
    t, margin = hdbscan_ref.select(parent, [1.0, 1.0, 3.0], "eom", False)
    assert t.tolist() == [0, 1, -1] and margin == pytest.approx(1 / 3)
    assert hdbscan_ref.select(parent, [1.0, 1.0, 3.0], "eom", True)[0].tolist() == [2, 2, 2]
    assert hdbscan_ref.select(parent, [1.0, 1.0, 2.0], "eom", True)[0].tolist() == [2, 2, 2]
    assert hdbscan_ref.select(parent, [1.0, 1.5, 2.0], "eom", True)[0].tolist() == [0, 1, -1]
    assert hdbscan_ref.select(parent, [1.0, 1.0, 3.0], "leaf", True)[0].tolist() == [0, 1, -1]
    # a lone leaf root
    assert hdbscan_ref.select(np.array([-1]), [1.0], "eom", False)[0].tolist() == [-1]
    assert hdbscan_ref.select(np.array([-1]), [1.0], "leaf", True)[0].tolist() == [0]
    # two top-level clusters are ordinary candidates
    parent = np.array([3, 3, -1, -1])
    assert hdbscan_ref.select(parent, [1.0, 1.0, 1.0, 5.0], "eom", False)[0].tolist() == \
        [3, 3, 2, 3]


def _blobs_uniform(seed, d):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1.0, 1.0, size=(3, d))
    parts = [c + rng.normal(0.0, s, size=(100, d)) for c, s in zip(centres, (0.05, 0.08, 0.12))]
    return np.concatenate(parts + [rng.uniform(-1.5, 1.5, size=(100, d))])


def same_partition(a, b):
    """Equal noise sets and clusters in bijection."""
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = set(zip(a[a >= 0].tolist(), b[b >= 0].tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


@pytest.mark.parametrize("m", [5, 10, 15])
@pytest.mark.parametrize("d", [2, 3, 4])
def test_sequential_equals_sklearn_without_ties(d, m):
    """min_samples = 1: the mutual-reachability distance is the distance, the
    spanning tree of continuous random rows has no ties, and the clustering is
    then one defined result that sklearn must share."""
    from sklearn.cluster import HDBSCAN
    X = _blobs_uniform(100 * d + m, d)
    assert len(X) == 400
    u, v, w, _ = mreach_ref.forest(X, 1, 100.0)          # r_max above every edge
    assert len(u) == len(X) - 1 and len(np.unique(w)) == len(w) and w[0] > 0
    got = hdbscan_ref.sequential(len(X), u, v, w, m, root=True)
    assert got["margin"] > 1e-6, got["margin"]
    want = HDBSCAN(min_cluster_size=m, min_samples=1, algorithm="brute",
                   copy=True).fit(X).labels_
    assert want.max() >= 1
    assert same_partition(got["labels"], want)


def test_native_selection_equals_reference():
    """pd_condensed_select runs on the host, so it is checked here: on the
    condensed trees of the random forests, every method and flag."""
    from pypardis_amd import _native, build
    build.build(verbose=False)
    compared = 0
    for i, n, (u, v, w), m in _cases():
        if i % 2:
            continue
        r = hdbscan_ref.sequential(n, u, v, w, m, root=False)
        for method in ("eom", "leaf"):
            for single in (False, True):
                want, _ = hdbscan_ref.select(r["parent"], r["stability"], method, single)
                got = _native.condensed_select(r["parent"], r["stability"], method, single)
                assert got.dtype == np.int32 and np.array_equal(got, want), (i, method, single)
                compared += len(want)
    assert compared > 3000
    with pytest.raises(_native.PardisError):
        _native.condensed_select(np.array([0, -1], np.int32), np.ones(2))
    with pytest.raises(ValueError):
        _native.condensed_select(np.array([-1], np.int32), np.ones(1), "best")
