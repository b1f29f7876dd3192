"""pd_index_mreach_forest / mutual_reachability_forest / dbscan_labels on the
GPU against the brute-force reference (mreach_ref.py).  Under the order (w, u,
v) the forest is ONE edge list, so every comparison is np.array_equal on the
raw row numbers and accumulators: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import kdist_ref
import mreach_ref
from conftest import load_golden
from test_gpu_kdist import R_BLOB, _blob_noise, _trained

pytestmark = pytest.mark.gpu

CODE = {"euclidean": 0, "cityblock": 1}
KS = (1, 4, 10, 64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _index(X, r_max, metric="euclidean"):
    from pypardis_amd import _native
    return _native.Index.over_rows(_dev(X), r_max, CODE[metric])


def _ask(ix, k):
    """Host copies of one GPU forest (u, v, w, cd) and its round count, types
    and shapes checked."""
    u, v, w, cd, rounds = ix.mreach_forest(k)
    assert u.is_cuda and u.dtype == v.dtype == torch.int32
    assert w.dtype == cd.dtype == torch.float64
    assert u.shape == v.shape == w.shape and cd.shape == (ix.n_core,)
    return (_np(u), _np(v), _np(w), _np(cd)), rounds


def _forest(X, k, r_max, metric="euclidean"):
    ix = _index(X, r_max, metric)
    try:
        return _ask(ix, k)
    finally:
        ix.close()


def _equal(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def _diff(got, want):
    """What differs, for the assertion message."""
    if len(got[0]) != len(want[0]):
        return f"{len(got[0])} edges, the reference has {len(want[0])}"
    return [int((a != b).sum()) for a, b in zip(got, want)]


def _golden(name):
    g = load_golden(name)
    metric = "cityblock" if str(g["metric"]) == "cityblock" else "euclidean"
    return g["X"], float(g["eps"]), int(g["min_samples"]), metric


# ------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_blob_and_noise_equal_reference(d, dtype, metric):
    X, _ = _blob_noise(d, dtype)
    r = R_BLOB[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    table = kdist_ref.accumulators(X, X, metric)
    pairs = mreach_ref.pairs_within(table, r, metric)
    ix = _index(X, r, metric)
    try:
        for k in KS:
            want = mreach_ref.forest_of_table(table, k, r, metric, pairs)
            if k == 10:
                assert np.isinf(want[3]).sum() > 100       # the noise rows are isolated
                assert len(want[0]) > 1000                 # the blob is a tree
                assert (want[2] == np.maximum(want[3][want[0]], want[3][want[1]])).sum() > 500
            got, rounds = _ask(ix, k)
            assert _equal(got, want), (k, _diff(got, want))
            assert 1 <= rounds <= int(np.ceil(np.log2(len(X)))) + 1
    finally:
        ix.close()


# ------------------------------------------------------------ 2. ties
def _tripled_lattice():
    g = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), indexing="ij"), -1).reshape(-1, 2)
    X = np.repeat(g, 3, axis=0)
    return X[np.random.default_rng(17).permutation(len(X))]


@pytest.mark.parametrize("case", ["lattice_in_order", "lattice_permuted", "ident_40", "dup_1d",
                                  "tripled_lattice"])
def test_ties_are_settled_by_the_row_numbers(case):
    """Sets on which nearly every weight is tied, so every round of the
    Borůvka is decided by (u, v)."""
    if case == "tripled_lattice":
        X, metric = _tripled_lattice(), "euclidean"
        runs = [(1.5, 3), (1.5, 7), (1.0, 4)]              # cd = 0 / 1 / 1; the cap on a tie
    else:
        X, eps, ms, metric = _golden("lattice_900" if case.startswith("lattice") else case)
        if case == "lattice_permuted":
            X = X[np.random.default_rng(3).permutation(len(X))]
        # the lattice's own eps is its step (16 core rows, no edge): also twice that
        runs = [(eps, ms), (2 * eps, ms), (2 * eps, 1)] if case.startswith("lattice") else \
               [(eps, ms), (eps, 1), (eps, 40)]
    table = kdist_ref.accumulators(X, X, metric)
    for r, k in runs:
        want = mreach_ref.forest_of_table(table, k, r, metric)
        if case.startswith("lattice") and r > 0.06 or case == "tripled_lattice":
            assert len(want[0]) > 800 and len(np.unique(want[2])) < 20
        if case == "ident_40":
            assert len(want[0]) == (39 if k <= 40 else 0) and not want[2].any()
        got, _ = _forest(X, k, r, metric)
        assert _equal(got, want), (case, r, k, _diff(got, want))
        if case == "ident_40" and k <= 40:
            assert np.array_equal(got[0], np.zeros(39, np.int32))      # (0, 1), (0, 2), ...
            assert np.array_equal(got[1], np.arange(1, 40, dtype=np.int32))


# ------------------------------------------------------------ 3. the link to train
_FORESTS = {}


def _golden_forest(name):
    """The forest of a trained golden at its own (eps, min_samples), once."""
    if name not in _FORESTS:
        from pypardis_amd import mutual_reachability_forest
        m, X, eps, ms, metric = _trained(name)
        _FORESTS[name] = mutual_reachability_forest(_dev(X), ms, eps, metric, squared=True)
    return _FORESTS[name]


@pytest.mark.parametrize("name", ["b2d_20k", "b3d_20k"])
def test_cuts_are_the_trains_at_every_smaller_eps(name):
    from pypardis_amd import DBSCAN, dbscan_labels, k_distances
    m, X, eps, ms, metric = _trained(name)
    f = _golden_forest(name)
    cd = _np(f.core_distances)
    assert np.array_equal(cd, _np(k_distances(_dev(X), ms, eps, metric, squared=True)))
    w = _np(f.distances)
    assert np.all(_np(f.u) < _np(f.v)) and np.all(np.diff(w) >= 0) and w[-1] <= eps * eps
    for frac in (1.0, 0.7, 0.4):
        e = eps * frac
        model = m if frac == 1.0 else DBSCAN(eps=e, min_samples=ms, metric=metric).train(_dev(X))
        core = _np(model.core_sample_mask_).astype(bool)
        labels = _np(model.labels_)
        assert not core.all() and (core.sum() > 100 or frac == 0.4)   # b3d at 0.4: no core row
        assert np.array_equal(cd <= e * e, core), (name, frac)
        got = dbscan_labels(f, e)
        assert got.is_cuda and got.dtype == torch.int32 and got.shape == (len(X),)
        got = _np(got)
        assert np.array_equal(got[core], labels[core]), (name, frac)
        assert np.all(got[~core] == -1)
        assert np.array_equal(got, _np(dbscan_labels(f, e * e, squared=True)))
        assert got.max() + 1 == model.n_clusters_


@pytest.mark.parametrize("name", ["b2d_20k", "b3d_20k"])
def test_forest_equals_kruskal_over_the_radius_graph(name):
    """20,000 rows are too many for the brute table: the edges come from
    radius_neighbors, the core accumulators from the GPU, Kruskal from scipy."""
    from pypardis_amd import radius_neighbors
    m, X, eps, ms, metric = _trained(name)
    f = _golden_forest(name)
    res = radius_neighbors(_dev(X), eps, metric, squared=True)
    indptr, j, acc = (_np(t) for t in res)
    i = np.repeat(np.arange(len(X)), np.diff(indptr))
    cd = _np(f.core_distances)
    want = mreach_ref.kruskal_pairs(len(X), i, j, acc, cd, eps * eps)
    got = (_np(f.u), _np(f.v), _np(f.distances))
    assert len(want[0]) > 5000
    assert _equal(got, want), _diff(got, want)


# ------------------------------------------------------------ 4. structure
def test_two_blobs_far_apart_are_two_trees():
    """1e6 apart at r_max = 0.01: 1e16 cells, 64-bit cell keys."""
    rng = np.random.default_rng(11)
    r, k = 0.01, 5
    X = np.concatenate([rng.normal(0.0, 0.01, size=(1400, 2)),
                        rng.normal(0.0, 0.01, size=(1400, 2)) + 1.0e6,
                        rng.uniform(4.0e5, 6.0e5, size=(200, 2))])
    X = X[rng.permutation(len(X))]
    want = mreach_ref.forest(X, k, r)
    isolated = int(np.isinf(want[3]).sum())
    assert isolated >= 200
    got, _ = _forest(X, k, r)
    assert _equal(got, want), _diff(got, want)
    # every row with a core distance hangs on one of the two trees
    member, labels = mreach_ref.cut(want[:3], want[3], r)
    if labels.max() == 1:
        assert len(got[0]) == len(X) - 2 - isolated


def test_no_row_with_k_neighbours_no_rows_and_one_row():
    from pypardis_amd import dbscan_labels, mutual_reachability_forest
    rng = np.random.default_rng(2)
    X = rng.uniform(0.0, 1.0, size=(300, 2))
    got, rounds = _forest(X, 30, 0.05)
    assert len(got[0]) == 0 and np.all(np.isinf(got[3])) and rounds == 1
    got, _ = _forest(X[:5], 8, 10.0)                       # fewer rows than k
    assert len(got[0]) == 0 and np.all(np.isinf(got[3]))
    for n in (0, 1):
        f = mutual_reachability_forest(X[:n], 1, 0.5)
        assert f.u.shape == f.v.shape == f.distances.shape == (0,)
        assert _np(f.core_distances).tolist() == [0.0] * n
        assert _np(dbscan_labels(f, 0.5)).tolist() == [0] * n
    f = mutual_reachability_forest(X[:1], 2, 0.5)
    assert np.isinf(_np(f.core_distances)).all() and _np(dbscan_labels(f, 0.5)).tolist() == [-1]


@pytest.mark.parametrize("permuted", [False, True])
def test_a_chain_that_merges_pairwise_takes_log2_rounds(permuted):
    """256 points on a line, the gap after point i growing with the number of
    trailing ones of i: every round merges the components two by two."""
    level = np.array([(~i & (i + 1)).bit_length() - 1 for i in range(255)])
    assert level.max() == 7 and (level == 0).sum() == 128
    x = np.concatenate([[0.0], np.cumsum(1.0 + 0.125 * level)])
    X = x[:, None]
    if permuted:
        X = X[np.random.default_rng(5).permutation(256)]
    want = mreach_ref.forest(X, 1, 2.0)
    assert len(want[0]) == 255 and len(np.unique(want[2])) == 8
    got, rounds = _forest(X, 1, 2.0)
    assert _equal(got, want), _diff(got, want)
    print(f"rounds: {rounds}")
    assert 6 <= rounds <= 9


# ------------------------------------------------------------ 5. order independence
def test_permuted_rows_give_the_same_forest():
    """k = 1: w = acc, no two equal here, so the tree is unique whatever the
    numbering and maps through the permutation.  k = 5: the weights tie at the
    core accumulators, so only what every minimum forest shares is compared: the
    sorted weights, the core accumulators and every cut's partition."""
    rng = np.random.default_rng(23)
    X = rng.normal(0.0, 0.3, size=(2500, 3))
    r = 0.12
    perm = rng.permutation(len(X))                         # row i of X[perm] is row perm[i] of X
    base, _ = _forest(X, 1, r)
    assert len(base[0]) > 1000 and not (np.diff(base[2]) == 0).any()
    got, _ = _forest(X[perm], 1, r)
    a, b = perm[got[0]], perm[got[1]]
    assert np.array_equal(np.minimum(a, b), base[0]) and np.array_equal(np.maximum(a, b), base[1])
    assert np.array_equal(got[2], base[2]) and np.array_equal(got[3], base[3][perm])
    base, _ = _forest(X, 5, r)
    got, _ = _forest(X[perm], 5, r)
    assert np.array_equal(got[2], base[2]) and np.array_equal(got[3], base[3][perm])
    for e in (r, 0.8 * r):
        mb, lb = mreach_ref.cut(base[:3], base[3], e)
        mg, lg = mreach_ref.cut(got[:3], got[3], e)
        assert np.array_equal(mg, mb[perm])
        pair = set(zip(lg[mg].tolist(), lb[perm][mg].tolist()))
        assert len(pair) == lb.max() + 1 == lg.max() + 1   # a bijection of the labels


def test_sweep_order_and_cell_short_cut_change_nothing(monkeypatch):
    X, eps, ms, metric = _golden("b2d_20k")
    ix = _index(X, eps, metric)
    try:
        monkeypatch.setenv("PD_INDEX_SORT_MIN", str(1 << 40))       # input order
        base, rounds = _ask(ix, ms)
        assert len(base[0]) > 10000 and rounds >= 3
        raw = [a.tobytes() for a in base]
        monkeypatch.setenv("PD_INDEX_SORT_MIN", "0")                # cell order
        assert [a.tobytes() for a in _ask(ix, ms)[0]] == raw
        monkeypatch.setenv("PD_MREACH_CELL_SKIP", "0")              # every cell's records read
        got, r2 = _ask(ix, ms)
        assert [a.tobytes() for a in got] == raw and r2 == rounds
        monkeypatch.delenv("PD_INDEX_SORT_MIN")
        assert [a.tobytes() for a in _ask(ix, ms)[0]] == raw
        monkeypatch.delenv("PD_MREACH_CELL_SKIP")
        assert [a.tobytes() for a in _ask(ix, ms)[0]] == raw
    finally:
        ix.close()


# ------------------------------------------------------------ 6. errors
def test_errors_leave_the_index_usable():
    from pypardis_amd import _native, dbscan_labels, mutual_reachability_forest
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(3000, 2)).astype(np.float32)
    r = 0.05
    want = mreach_ref.forest(X, 6, r)
    ix = _index(X, r)
    for k, cap, code in ((0, None, _native.PD_EINVAL), (-1, None, _native.PD_EINVAL),
                         (65, None, -5), (6, len(X) - 2, _native.PD_EINVAL),
                         (6, 0, _native.PD_EINVAL)):
        with pytest.raises(_native.PardisError) as e:
            ix.mreach_forest(k, capacity=cap)
        assert e.value.code == code, (k, cap, e.value)
    got, _ = _ask(ix, 6)
    assert _equal(got, want), _diff(got, want)
    u, v, w, cd, _ = ix.mreach_forest(6, capacity=len(X) + 5)        # more room than needed
    assert _equal((_np(u), _np(v), _np(w), _np(cd)), want)
    # a kdist on the same index still answers
    assert np.array_equal(_np(ix.kdist(_dev(X), 6)), want[3])
    ix.close()
    with pytest.raises(ValueError):
        ix.mreach_forest(6)
    # labels that are not the row numbers
    ix = _native.Index.over_all(_dev(X), r)
    with pytest.raises(_native.PardisError) as e:
        ix.mreach_forest(1)
    assert e.value.code == _native.PD_EINVAL and "row numbers" in str(e.value)
    ix.close()
    # d > 4
    X8 = rng.uniform(size=(500, 8))
    ix = _index(X8, 0.5)
    with pytest.raises(_native.PardisError) as e:
        ix.mreach_forest(3)
    assert e.value.code == -5 and "d" in str(e.value) and "8" in str(e.value)
    assert np.array_equal(_np(ix.kdist(_dev(X8), 3)), kdist_ref.kdist(X8, 3, 0.5))
    ix.close()
    with pytest.raises(ValueError):
        mutual_reachability_forest(X8, 3, 0.5)
    f = mutual_reachability_forest(X, 6, r)
    for eps in (r * 1.01, 2 * r):
        with pytest.raises(ValueError):
            dbscan_labels(f, eps)
    with pytest.raises(ValueError):
        dbscan_labels(f, r * r * 1.01, squared=True)
    member, labels = mreach_ref.cut(want[:3], want[3], r)
    assert np.array_equal(_np(dbscan_labels(f, r)), labels)


def test_forest_labels_takes_any_member_mask():
    """pd_forest_labels on its own: a prefix of a path, members chosen freely —
    numbered by smallest MEMBER row, rows outside the mask -1."""
    from pypardis_amd import _native
    u = _dev(np.array([3, 1, 0, 5], np.int32))
    v = _dev(np.array([4, 2, 1, 6], np.int32))
    member = _dev(np.array([0, 1, 1, 1, 1, 0, 1, 1], np.uint8))
    labels, ncl = _native.forest_labels(u, v, 3, member)          # {0, 1, 2} {3, 4} 5 6 7
    assert _np(labels).tolist() == [-1, 0, 0, 1, 1, -1, 2, 3] and ncl == 4
    labels, ncl = _native.forest_labels(u, v, 4, member.bool())   # ... {5, 6}
    assert _np(labels).tolist() == [-1, 0, 0, 1, 1, -1, 2, 3] and ncl == 4
    labels, ncl = _native.forest_labels(u, v, 0, member)
    assert _np(labels).tolist() == [-1, 0, 1, 2, 3, -1, 4, 5] and ncl == 6
    with pytest.raises(_native.PardisError) as e:
        _native.forest_labels(u, _dev(np.array([4, 2, 8, 6], np.int32)), 4, member)
    assert e.value.code == _native.PD_EINVAL
    with pytest.raises(ValueError):
        _native.forest_labels(u, v, 5, member)


# ------------------------------------------------------------ 7. model methods
def test_model_forest_after_train():
    from pypardis_amd import DBSCAN, ReachabilityForest, dbscan_labels
    m, X, eps, ms, metric = _trained("b3d_20k")
    raw = _golden_forest("b3d_20k")
    f = m.mutual_reachability_forest()
    assert isinstance(f, ReachabilityForest) and f.r_max == eps and not f.squared
    assert all(torch.equal(a, b) for a, b in zip(f[:2], raw[:2]))
    assert np.array_equal(_np(f.distances), np.sqrt(_np(raw.distances)))       # fp64 sqrt
    assert np.array_equal(_np(f.core_distances), np.sqrt(_np(raw.core_distances)))
    assert torch.equal(f.accumulators, raw.distances)
    f2 = m.mutual_reachability_forest(squared=True)
    assert f2.squared and all(torch.equal(a, b) for a, b in zip(f2, raw))
    core = _np(m.core_sample_mask_).astype(bool)
    got = _np(dbscan_labels(f, m.eps))
    assert np.array_equal(got[core], _np(m.labels_)[core]) and np.all(got[~core] == -1)
    # other arguments, other data
    sub = X[:3000]
    want = mreach_ref.forest(sub, 4, 0.8 * eps, metric)
    f3 = m.mutual_reachability_forest(_dev(sub), min_samples=4, r_max=0.8 * eps, squared=True)
    assert _equal([_np(t) for t in f3], want)
    fresh = DBSCAN(eps=0.8 * eps, min_samples=4, metric=metric)
    assert _equal([_np(t) for t in fresh.mutual_reachability_forest(sub, squared=True)], want)
    assert fresh.labels_ is None
    with pytest.raises(ValueError):
        fresh.mutual_reachability_forest()


def test_module_forest_cityblock_and_inputs():
    import dbscan
    X, eps, ms, metric = _golden("neg_3k")
    want = mreach_ref.forest(X, ms, eps, "cityblock")
    f = dbscan.mutual_reachability_forest(X, ms, eps, "cityblock")     # numpy in, no sqrt
    assert _equal([_np(t) for t in f], want)
    recs = [(f"p{i}", X[i]) for i in range(len(X))]                    # (key, vector) records
    assert _equal([_np(t) for t in dbscan.mutual_reachability_forest(recs, ms, eps, "manhattan")],
                  want)
    for e in (eps, 0.6 * eps):
        member, labels = mreach_ref.cut(want[:3], want[3], e, "cityblock")
        assert np.array_equal(_np(dbscan.dbscan_labels(f, e)), labels)
    bad = X[:50].copy()
    bad[7, 0] = np.nan
    with pytest.raises(ValueError):
        dbscan.mutual_reachability_forest(bad, ms, eps)
