"""condensed_tree / hdbscan_labels / hdbscan on the GPU against the sequential
top-down definition (hdbscan_ref.sequential) run on the GPU's own forest.  The
result is one defined tree, so everything is compared with np.array_equal —
cluster numbers included — except the stabilities, whose bound is derived: any
summation order of t non-negative fp64 terms errs by at most (t - 1) * 2^-53 of
their sum, the reference sums with math.fsum, so |got - want| <= terms * 2^-52
* want."""
import json

import numpy as np
import pytest
import torch

import hdbscan_ref
from test_gpu_kdist import R_BLOB, _blob_noise, _golden

pytestmark = pytest.mark.gpu

VARIANTS = [("eom", False), ("eom", True), ("leaf", False), ("leaf", True)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _forest(X, k, r_max, metric="euclidean"):
    from pypardis_amd import mutual_reachability_forest
    return mutual_reachability_forest(_dev(X), k, r_max, metric, squared=True)


def _edges(f):
    return _np(f.u), _np(f.v), _np(f.accumulators)


def _reference(f, m):
    u, v, w = _edges(f)
    n = f.core_accumulators.shape[0]
    return hdbscan_ref.sequential(n, u, v, w, m, root=f.metric == 0)


def _check_tree(tree, ref, ctx):
    """The GPU's CondensedTree against the reference's, every array."""
    assert tree.point_cluster.is_cuda and tree.point_cluster.dtype == torch.int32, ctx
    assert tree.point_lambda.is_cuda and tree.point_lambda.dtype == torch.float64, ctx
    assert all(isinstance(a, np.ndarray) for a in tree[:6]), ctx
    assert np.array_equal(_np(tree.point_cluster), ref["point_cluster"]), ctx
    assert np.array_equal(_np(tree.point_lambda), ref["point_lambda"]), ctx
    assert np.array_equal(tree.parent, ref["parent"]), ctx
    assert np.array_equal(tree.birth_lambda, ref["birth"]), ctx
    assert np.array_equal(tree.death_lambda, ref["death"]), ctx
    assert np.array_equal(tree.lambda_max, ref["lambda_max"]), ctx
    assert np.array_equal(tree.size, ref["size"]), ctx
    err = np.abs(tree.stability - ref["stability"])
    bound = ref["terms"] * 2.0 ** -52 * ref["stability"]
    assert np.all(err <= bound), (ctx, float(err.max()), int(np.argmax(err - bound)))
    assert 1 <= tree.rounds <= max(tree.min_cluster_size - 1, 1), (ctx, tree.rounds)


def _check_labels(f, m, ref, ctx, variants=VARIANTS):
    """Labels and probabilities of every selection variant.  The selection is
    replayed in the reference on the GPU's own stabilities (so a decision
    inside the stability bound cannot differ); where the reference's own
    decisions are further than 1e-6 from a tie, its labels must be equal too.
    -> the number of variants compared that second way."""
    from pypardis_amd import hdbscan_labels
    firm = 0
    for method, single in variants:
        labels, prob, tree = hdbscan_labels(f, m, method, single, return_tree=True)
        assert labels.is_cuda and labels.dtype == torch.int32, ctx
        assert prob.is_cuda and prob.dtype == torch.float64, ctx
        target, _ = hdbscan_ref.select(ref["parent"], tree.stability, method, single)
        want_l, want_p = hdbscan_ref.labels_of(ref["point_cluster"], ref["point_lambda"], target,
                                               ref["lambda_max"])
        assert np.array_equal(_np(labels), want_l), (ctx, method, single)
        assert np.array_equal(_np(prob), want_p), (ctx, method, single)
        target, margin = hdbscan_ref.select(ref["parent"], ref["stability"], method, single)
        if margin > 1e-6:
            firm += 1
            own_l, own_p = hdbscan_ref.labels_of(ref["point_cluster"], ref["point_lambda"],
                                                 target, ref["lambda_max"])
            assert np.array_equal(_np(labels), own_l), (ctx, method, single, margin)
            assert np.array_equal(_np(prob), own_p), (ctx, method, single, margin)
    return firm


def _check(f, m, ctx, variants=VARIANTS):
    """Everything, for one forest and one m.  A forest whose lightest edge
    weighs 0 must be refused instead.  -> (reference, firm variants)."""
    from pypardis_amd import condensed_tree
    if f.accumulators.shape[0] and float(f.accumulators[0]) == 0.0:
        with pytest.raises(ValueError, match="weight 0"):
            condensed_tree(f, m)
        return None, 0
    ref = _reference(f, m)
    _check_tree(condensed_tree(f, m), ref, ctx)
    return ref, _check_labels(f, m, ref, ctx, variants)


# ------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("metric", ["euclidean", "cityblock"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_blob_and_noise_equal_reference(d, dtype, metric):
    X, _ = _blob_noise(d, dtype)
    r = R_BLOB[d] * (1.0 if metric == "euclidean" else np.sqrt(d))
    clusters = firm = 0
    for k in (1, 10):
        f = _forest(X, k, r, metric)
        for m in (2, 5, 15, 64):
            ref, nf = _check(f, m, (d, dtype.__name__, metric, k, m))
            if ref is not None:
                clusters += len(ref["parent"])
                firm += nf
    assert clusters > 50 and firm >= 8, (clusters, firm)


@pytest.mark.parametrize("factor", [1, 4])
@pytest.mark.parametrize("name", ["b2d_20k", "b3d_20k"])
def test_goldens_of_20k_rows(name, factor):
    """r_max = eps: many components, top-level clusters beside small-component
    noise; 4 eps: few components and deep trees."""
    X, eps, ms, metric = _golden(name)
    f = _forest(X, ms, factor * eps, metric)
    assert float(f.accumulators[0]) > 0.0
    clusters = 0
    for m in (5, 50):
        ref, firm = _check(f, m, (name, factor, m), variants=[("eom", False), ("leaf", True)])
        tops = int((ref["parent"] < 0).sum())
        print(f"{name} x{factor} m={m}: clusters {len(ref['parent'])}, top-level {tops}, "
              f"splits {len(ref['splits'])}, noise {int((ref['point_cluster'] < 0).sum())}, "
              f"margin-firm variants {firm}")
        clusters += len(ref["parent"])
    assert clusters >= 3
    from pypardis_amd import hdbscan_labels
    a = hdbscan_labels(f, 5, return_tree=True)
    b = hdbscan_labels(f, 5, return_tree=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].stability.tobytes() == b[2].stability.tobytes()


def test_two_calls_are_bit_equal():
    X, _ = _blob_noise(3, np.float32)
    f = _forest(X, 10, R_BLOB[3])
    from pypardis_amd import hdbscan_labels
    for m in (5, 15):
        a = hdbscan_labels(f, m, return_tree=True)
        b = hdbscan_labels(f, m, return_tree=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert a[2].stability.tobytes() == b[2].stability.tobytes()
        assert torch.equal(a[2].point_cluster, b[2].point_cluster)


# ------------------------------------------------------------ 2. the deepest rounds
def test_caterpillar_chain(tmp_path, monkeypatch):
    """x_i = 1.1^i: every merge adds one row to the chain, so a small subtree
    of s rows takes s - 1 rounds."""
    from pypardis_amd import condensed_tree, hdbscan_labels
    n = 200
    X = (1.1 ** np.arange(n))[:, None]
    f = _forest(X, 1, 1.0e9)
    assert f.u.shape[0] == n - 1
    for m in (2, 3, 33):
        ref, _ = _check(f, m, ("caterpillar", m))
        rounds = condensed_tree(f, m).rounds
        assert rounds <= m - 1
        if m == 33:
            assert rounds > 2
            assert rounds == 32          # 31 rounds add a row each, the last merges nothing
    # m = n: the root is the only cluster
    ref, _ = _check(f, n, ("caterpillar", n))
    assert len(ref["parent"]) == 1 and ref["size"][0] == n
    labels, prob = hdbscan_labels(f, n)
    assert np.all(_np(labels) == -1) and not _np(prob).any()
    labels, prob = hdbscan_labels(f, n, allow_single_cluster=True)
    assert np.all(_np(labels) == 0) and np.all(_np(prob) > 0) and _np(prob).max() == 1.0
    # m > n: nothing reaches m rows
    tree = condensed_tree(f, n + 1)
    assert len(tree.parent) == 0 and np.all(_np(tree.point_cluster) == -1)
    labels, prob = hdbscan_labels(f, n + 1, allow_single_cluster=True)
    assert np.all(_np(labels) == -1) and not _np(prob).any()
    # the trace: one line per round
    path = tmp_path / "trace.jsonl"
    monkeypatch.setenv("PD_HDBSCAN_TRACE", str(path))
    rounds = condensed_tree(f, 6).rounds
    monkeypatch.delenv("PD_HDBSCAN_TRACE")
    lines = [json.loads(s) for s in path.read_text().splitlines()]
    assert [t["round"] for t in lines] == list(range(1, rounds + 1))
    assert [t["merges"] for t in lines] == [1] * (rounds - 1) + [0]


# ------------------------------------------------------------ 3. ties, duplicates
def test_lattice_every_weight_ties():
    """The order of the merges is decided by (u, v) alone."""
    X, eps, ms, metric = _golden("lattice_900")
    for r, k in ((2 * eps, ms), (2 * eps, 1)):
        f = _forest(X, k, r, metric)
        w = _np(f.accumulators)
        assert len(w) > 800 and len(np.unique(w)) < 20
        for m in (2, 5, 15):
            _check(f, m, ("lattice", r, k, m))


def test_duplicate_rows_are_refused():
    from pypardis_amd import _native, condensed_tree, hdbscan, hdbscan_labels
    rng = np.random.default_rng(8)
    X = rng.uniform(size=(500, 2))
    X[100:104] = X[100]                                   # 4 identical rows
    f = _forest(X, 4, 0.3)
    assert float(f.accumulators[0]) == 0.0
    for call in (lambda: condensed_tree(f, 5), lambda: hdbscan_labels(f, 5),
                 lambda: hdbscan(X, 5, min_samples=4, r_max=0.3)):
        with pytest.raises(ValueError, match="sample_weight"):
            call()
    u, v, w = f.u, f.v, f.accumulators
    with pytest.raises(_native.PardisError) as e:
        _native.forest_condense(len(X), u, v, w, True, 5)
    assert e.value.code == _native.PD_EINVAL
    # the same four rows at k = 5: their core distance is positive, no edge weighs 0
    f = _forest(X, 5, 0.3)
    assert float(f.accumulators[0]) > 0.0
    _check(f, 5, "dups below k")
    # min_samples = 1 without duplicates: core distance 0, but no edge of weight 0
    Y = rng.uniform(size=(500, 2))
    _check(_forest(Y, 1, 0.3), 5, "k = 1")


# ------------------------------------------------------------ 4. order independence
def test_permuted_rows_give_the_same_partition():
    """k = 1, random floats: no ties, so the clustering is unique whatever the
    numbering of the rows."""
    from pypardis_amd import hdbscan_labels
    from test_hdbscan_host import same_partition
    rng = np.random.default_rng(31)
    X = np.concatenate([rng.normal(0.0, 0.1, size=(1200, 2)),
                        rng.normal(1.0, 0.2, size=(800, 2)),
                        rng.uniform(-1.0, 2.0, size=(500, 2))])
    perm = rng.permutation(len(X))
    fa, fb = _forest(X, 1, 0.5), _forest(X[perm], 1, 0.5)
    assert not (np.diff(_np(fa.accumulators)) == 0).any()
    for m in (5, 25):
        assert hdbscan_ref.eom_margin(*[_reference(fa, m)[key] for key in ("parent", "stability")]) \
            > 1e-6
        for method in ("eom", "leaf"):
            la, pa = hdbscan_labels(fa, m, method)
            lb, pb = hdbscan_labels(fb, m, method)
            la, lb = _np(la), _np(lb)
            assert la.max() >= 1
            assert same_partition(la[perm], lb)
            assert np.array_equal(_np(pa)[perm], _np(pb))


# ------------------------------------------------------------ 5. errors
def test_malformed_input_leaves_the_context_usable():
    from pypardis_amd import _native, condensed_tree
    rng = np.random.default_rng(12)
    X = rng.uniform(size=(2000, 2))
    f = _forest(X, 3, 0.2)
    n, (u, v, w) = len(X), _edges(f)
    assert len(u) > 1500
    ref = _reference(f, 5)
    need = len(ref["parent"])
    assert need >= 4

    def run(u_, v_, w_, **kw):
        return _native.forest_condense(n, _dev(u_), _dev(v_), _dev(w_), True, 5, **kw)

    def refused(u_, v_, w_, word, **kw):
        with pytest.raises(_native.PardisError) as e:
            run(u_, v_, w_, **kw)
        assert e.value.code == _native.PD_EINVAL and word in str(e.value), e.value
        _check_tree(condensed_tree(f, 5), ref, word)       # the context still works

    bad = u.copy()
    bad[700] = n
    refused(bad, v, w, "endpoint")
    bad = v.copy()
    bad[3] = -1
    refused(u, bad, w, "endpoint")
    cyc = v.copy()                                         # edge 900 repeats edge 10: a cycle
    cu = u.copy()
    cu[900], cyc[900] = u[10], v[10]
    refused(cu, cyc, w, "cycle")
    uns = w.copy()
    uns[[400, 1200]] = uns[[1200, 400]]
    assert uns[400] != uns[1200]
    refused(u, v, uns, "ascending")
    nan = w.copy()
    nan[50] = np.nan
    refused(u, v, nan, "ascending")
    refused(u, v, w, "capacity", capacity=need - 1)
    refused(u, v, w, "capacity", capacity=0)
    assert len(run(u, v, w, capacity=need)["parent"]) == need
    with pytest.raises(_native.PardisError) as e:          # more edges than a forest has
        _native.forest_condense(len(u), _dev(u), _dev(v), _dev(w), True, 5)
    assert e.value.code == _native.PD_EINVAL
    with pytest.raises(_native.PardisError) as e:
        _native.forest_condense(n, _dev(u), _dev(v), _dev(w), True, 1)
    assert e.value.code == _native.PD_EINVAL
    # the selection and the labels check their arrays too
    with pytest.raises(_native.PardisError):
        _native.condensed_select(np.array([0, -1], np.int32), np.ones(2))     # parent[x] <= x
    with pytest.raises(ValueError):
        _native.condensed_select(ref["parent"], ref["stability"], "best")
    tree = condensed_tree(f, 5)
    target = _native.condensed_select(tree.parent, tree.stability)
    wrong = tree.point_cluster.clone()
    wrong[17] = need
    with pytest.raises(_native.PardisError) as e:
        _native.condensed_labels(wrong, tree.point_lambda, target, tree.lambda_max)
    assert e.value.code == _native.PD_EINVAL
    labels, prob, nsel = _native.condensed_labels(tree.point_cluster, tree.point_lambda, target,
                                                  tree.lambda_max)
    want = hdbscan_ref.labels_of(ref["point_cluster"], ref["point_lambda"],
                                 hdbscan_ref.select(ref["parent"], tree.stability)[0],
                                 ref["lambda_max"])
    assert np.array_equal(_np(labels), want[0]) and nsel == want[0].max() + 1


# ------------------------------------------------------------ 6. the Python surface
def test_module_and_model_calls():
    import dbscan
    from pypardis_amd import DBSCAN, CondensedTree, hdbscan, hdbscan_labels
    X, _ = _blob_noise(2, np.float64)
    r = R_BLOB[2]
    f = _forest(X, 15, r)
    want = hdbscan_labels(f, 15)
    got = hdbscan(X, 15, r_max=r)                          # min_samples defaults to m
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert _np(got[0]).max() >= 0 and (_np(got[0]) == -1).any()
    got = dbscan.hdbscan(_dev(X), 15, min_samples=15, r_max=r, return_tree=True)
    assert len(got) == 3 and isinstance(got[2], CondensedTree)
    assert torch.equal(got[0], want[0])
    want = hdbscan_labels(_forest(X, 64, r), 100, "leaf", True)   # min_samples capped at 64
    got = hdbscan(X, 100, r_max=r, cluster_selection_method="leaf", allow_single_cluster=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    model = DBSCAN(eps=r, min_samples=10)
    want = hdbscan_labels(_forest(X, 7, r), 7)
    got = model.hdbscan(7, X)                              # before any train: data needed
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError):
        model.hdbscan(7)
    model.train(_dev(X))
    got = model.hdbscan(7)                                 # the training points, r_max = eps
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got = model.hdbscan(7, min_samples=3, r_max=0.5 * r, cluster_selection_method="leaf")
    want = hdbscan_labels(_forest(X, 3, 0.5 * r), 7, "leaf")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for bad in (lambda: hdbscan(X, 1, r_max=r), lambda: hdbscan(X, 2.5, r_max=r),
                lambda: hdbscan(X, 5), lambda: hdbscan(X, 5, r_max=r, min_samples=65),
                lambda: hdbscan(X, 5, r_max=r, cluster_selection_method="best"),
                lambda: hdbscan_labels(f, 5, "best"), lambda: dbscan.condensed_tree(f, 0)):
        with pytest.raises(ValueError):
            bad()
    # no rows, one row
    for n in (0, 1):
        labels, prob = hdbscan(X[:n], 2, r_max=r)
        assert _np(labels).tolist() == [-1] * n and _np(prob).tolist() == [0.0] * n
