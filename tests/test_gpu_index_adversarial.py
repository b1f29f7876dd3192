"""The index queries (csrc/assign.hip) on row and query sets whose neighbour
decisions sit at the edge of the index's own grid, walk, fp32 screen and
k-lists (tests/index_adversarial.py; the generators' claims are pinned on the
CPU in tests/test_index_adversarial_host.py).  Every expected value comes from
the brute-force references (kdist_ref, knn_ref, radius_ref, predict_ref,
mreach_ref, wkdist_ref) and is compared with np.array_equal: no tolerance
anywhere.  Every family runs all the query kinds (``_all_kinds``) in both sweep
orders (PD_INDEX_SORT_MIN = 1 and 2^40), and the public functions on one set
(DESIGN.md section 19)."""
import numpy as np
import pytest
import torch

import grid_adversarial as ga
import index_adversarial as ia
import knn_ref
import radius_ref
import wkdist_ref

pytestmark = pytest.mark.gpu

CODE = {"euclidean": 0, "cityblock": 1}
SORTS = ("1", str(1 << 40))
DTYPES = ("float64", "float32")
METRICS = ("euclidean", "cityblock")


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()     # (a copy: the shared cases are read-only)


def _np(t):
    return t.cpu().numpy()


def _rows_index(X, r_max, metric):
    from pypardis_amd import _native
    return _native.Index.over_rows(_dev(X), r_max, CODE[metric])


def _label_index(X, r_max, metric):
    """Every row a core under its own number: query() is then the smallest row
    number of an accepted pair."""
    from pypardis_amd import _native
    n = len(X)
    return _native.Index(_dev(X), torch.ones(n, dtype=torch.uint8, device="cuda"),
                         torch.arange(n, dtype=torch.int32, device="cuda"), r_max, CODE[metric])


def _knn_equal(ix, dq, k, want, tag):
    ids, acc = ix.kneighbors(dq, k)
    assert np.array_equal(_np(ids), want[0]), (tag, "kneighbors ids", k)
    assert np.array_equal(_np(acc), want[1]), (tag, "kneighbors acc", k)
    ids, acc = ix.kneighbors(dq, k, False)
    assert acc is None and np.array_equal(_np(ids), want[0]), (tag, "kneighbors ids alone", k)


def _radius_equal(ix, dq, radius, want, tag):
    indptr, ids, acc = want
    got = ix.radius(dq, radius, count_only=True)[0]
    assert np.array_equal(_np(got), indptr), (tag, "radius count", radius)
    p, i, a = ix.radius(dq, radius, return_acc=False)
    assert a is None and np.array_equal(_np(p), indptr)
    assert np.array_equal(radius_ref.sort_rows(_np(p), _np(i))[0], ids), (tag, "radius fill", radius)
    p, i, a = ix.radius(dq, radius)
    si, sa = radius_ref.sort_rows(_np(p), _np(i), _np(a))
    assert np.array_equal(si, ids) and np.array_equal(sa, acc), (tag, "radius fill + acc", radius)


def _all_kinds(case, monkeypatch, r_max=None, radii=None, ks=None, forest=True, predict=True):
    """All the query kinds on Index.over_rows(X, r_max), in both sweep orders:
    kdist at k; kneighbors at k and k + 1, ids + accumulators and ids alone;
    radius as count, fill, and fill with accumulators, at every radius of
    `radii`; kdist_weighted with unit weights (== kdist bit for bit);
    mreach_forest at k (d <= 4); query() on the index labelled by row number.
    -> the reference."""
    X, Q, metric = case["X"], case["Q"], case["metric"]
    r_max = case["r_max"] if r_max is None else r_max
    radii = (r_max,) if radii is None else tuple(radii)
    ks = (case["k"],) if ks is None else tuple(ks)
    d = X.shape[1]
    forest = forest and d <= 4
    ref = ia.reference(case, radii, r_max, kmax=max(ks) + 1, forest_k=ks[0])
    dq = _dev(Q)
    for sort in SORTS:
        monkeypatch.setenv("PD_INDEX_SORT_MIN", sort)
        tag = (case["key"], r_max, sort)
        ix = _rows_index(X, r_max, metric)
        try:
            assert ix.n_core == len(X)
            ix.set_weights(torch.ones(len(X), dtype=torch.float64, device="cuda"))
            for k in ks:
                kd = _np(ix.kdist(dq, k))
                assert np.array_equal(kd, ia.kdist_of(ref["pairs"], k, r_max, metric)), (tag, "kdist", k)
                assert np.array_equal(_np(ix.kdist_weighted(dq, k)), kd), (tag, "kdist_weighted", k)
                for kk in (k, k + 1):
                    if kk <= 64:
                        _knn_equal(ix, dq, kk, knn_ref.cut(ref["pairs"], kk, r_max, metric), tag)
            for radius in radii:
                _radius_equal(ix, dq, radius, ref["csr"][radius], tag)
            if forest:
                u, v, w, cd, _ = ix.mreach_forest(ks[0])
                fu, fv, fw, fcd = ref["forest"]
                assert np.array_equal(_np(cd), fcd), (tag, "forest cd")
                assert np.array_equal(_np(u), fu) and np.array_equal(_np(v), fv), (tag, "forest u v")
                assert np.array_equal(_np(w), fw), (tag, "forest w")
        finally:
            ix.close()
        if predict:
            ix = _label_index(X, r_max, metric)
            try:
                assert np.array_equal(_np(ix.query(dq)).astype(np.int64), ref["predict"]), (tag, "query")
            finally:
                ix.close()
    monkeypatch.delenv("PD_INDEX_SORT_MIN")
    return ref


def _public_queries(case, ref, k=None):
    """k_distances, kneighbors and radius_neighbors on a case whose rows are
    its queries, against the same reference."""
    from pypardis_amd import k_distances, kneighbors, radius_neighbors
    X, metric, r = case["X"], case["metric"], case["r_max"]
    k = case["k"] if k is None else k
    assert case["Q"] is X
    dx = _dev(X)
    want = knn_ref.cut(ref["pairs"], k, r, metric)
    assert np.array_equal(_np(k_distances(dx, k, r, metric, squared=True)), want[1][:, k - 1])
    res = kneighbors(dx, k, r, metric, squared=True)
    assert np.array_equal(_np(res.indices), want[0]) and np.array_equal(_np(res.distances), want[1])
    cnt = radius_neighbors(dx, r, metric, count_only=True)
    assert np.array_equal(_np(cnt), np.diff(ref["csr"][r][0]))
    indptr, ids, acc = ref["csr"][r]
    res = radius_neighbors(dx, r, metric, squared=True, sort_results=False)
    si, sa = radius_ref.sort_rows(_np(res.indptr), _np(res.indices), _np(res.distances))
    assert np.array_equal(_np(res.indptr), indptr)
    assert np.array_equal(si, ids) and np.array_equal(sa, acc)
    return dx


def _public(case, ref, ms=2):
    """The public functions on a case whose rows are its queries, against the
    same reference: k_distances, kneighbors, radius_neighbors,
    mutual_reachability_forest, and DBSCAN.train(...).predict."""
    from pypardis_amd import DBSCAN, mutual_reachability_forest
    X, metric, r, k = case["X"], case["metric"], case["r_max"], case["k"]
    dx = _public_queries(case, ref)
    if X.shape[1] <= 4:
        f = mutual_reachability_forest(dx, k, r, metric, squared=True)
        fu, fv, fw, fcd = ref["forest"]
        got = [_np(t) for t in (f.u, f.v, f.distances, f.core_distances)]
        assert np.array_equal(got[0], fu) and np.array_equal(got[1], fv)
        assert np.array_equal(got[2], fw) and np.array_equal(got[3], fcd)
    m = DBSCAN(eps=r, min_samples=ms, metric=metric).train(dx)
    assert np.array_equal(_np(m.predict(dx)), _np(m.labels_))
    assert np.array_equal(_np(m.core_sample_mask_).astype(bool), np.diff(ref["csr"][r][0]) >= ms)
    return m


def _triple_expectations(case, ref, tag):
    """What a straddling family expects of its groups, read off the REFERENCE:
    counts (2, 3, 2), the twin absent from the query's row, kneighbors(k = 3)
    of the query ending in (-1, inf), the forest joining each triple by two
    edges."""
    role, groups, r = case["role"], case["groups"], case["r_max"]
    cnt = np.diff(ref["csr"][r][0])[:len(role)]
    assert (cnt[role == 0] == 2).all() and (cnt[role == 1] == 3).all(), tag
    assert (cnt[role == 2] == 2).all() and (cnt[role == 3] == 1).all(), tag
    ids, acc = knn_ref.cut(ref["pairs"], 3, r, case["metric"])
    qrows = np.flatnonzero(role == 0)
    assert (ids[qrows, 2] == -1).all() and np.isinf(acc[qrows, 2]).all(), tag
    assert (role[ids[qrows, 1]] == 1).all() and (groups[ids[qrows, 1]] == groups[qrows]).all(), tag
    if "forest" in ref:
        fu, fv, _, _ = ref["forest"]
        assert len(fu) == 2 * len(qrows) and (groups[fu] == groups[fv]).all(), tag


# ------------------------------------------------------------ a. cell edge
CELL = [(dt, d, m, off) for dt in DTYPES for d in (2, 3, 4) for m in METRICS
        for off in (0.0, 2.0 ** 20)]


@pytest.mark.parametrize("dtype,d,metric,offset", CELL)
def test_cell_edge(monkeypatch, dtype, d, metric, offset):
    """Neighbours in the next row of the INDEX's cells at the last offset the
    predicate accepts, and twins one step further."""
    case = ia.cell_edge(dtype, d, metric, offset)
    ref = _all_kinds(case, monkeypatch)
    _triple_expectations(case, ref, case["key"])
    if offset == 0.0 and dtype == "float64":
        _public(case, ref)


@pytest.mark.parametrize("dtype,d,metric", [(dt, d, m) for dt in DTYPES for d in (2, 3, 4)
                                            for m in METRICS])
def test_cell_edge_off_grid_thresholds(monkeypatch, dtype, d, metric):
    """The same sets under indexes of r_max = 2 eps and 1.37 eps, asked at
    radius = eps: the pairs no longer sit at boundaries of these cells, the
    threshold still does; and (kdist(k = 2) <= fl(eps^2)) == (count >= 2)."""
    case = ia.cell_edge(dtype, d, metric, 0.0 if d != 3 else 2.0 ** 20)
    eps = case["r_max"]
    X = case["X"]
    for f in (2.0, 1.37):
        r_max = f * eps
        ref = _all_kinds(case, monkeypatch, r_max=r_max, radii=(eps, r_max), forest=False,
                         predict=False)
        ix = _rows_index(X, r_max, metric)
        try:
            kd = _np(ix.kdist(_dev(X), 2))
            cnt = np.diff(_np(ix.radius(_dev(X), eps, count_only=True)[0]))
        finally:
            ix.close()
        assert np.array_equal(kd <= ga.threshold(eps, metric), cnt >= 2)
        assert np.array_equal(cnt, np.diff(ref["csr"][eps][0]))
        role = case["role"]
        assert (cnt[role == 0] == 2).all() and (cnt[role == 1] == 3).all() and (cnt[role == 2] == 2).all()


# ------------------------------------------------------------ b. cap edge
CAP = [(d, axis, over) for d in (2, 3, 4) for axis in range(d) for over in (False, True)]


@pytest.mark.parametrize("d,axis,over", CAP)
def test_cap_edge(monkeypatch, d, axis, over):
    """One axis of exactly 2^28 cells, and one cell more (the cells double)."""
    case = ia.cap_edge(d, axis, over)
    ref = _all_kinds(case, monkeypatch)
    _triple_expectations(case, ref, case["key"])
    if axis == d - 1:
        _public(case, ref)
    if d == 2:
        _all_kinds(ia.cap_edge(d, axis, over, "cityblock"), monkeypatch)


SLACK = [(d, a, m) for d, a in ((1, 0), (2, 0), (2, 1), (3, 2), (4, 3)) for m in METRICS]


@pytest.mark.parametrize("d,axis,metric", SLACK)
def test_slack_edge(monkeypatch, d, axis, metric):
    """Pairs within eps that a cell width of eps itself, without the factor
    1 + 2^-20, would put two cells apart: a walk of +-1 cell finds them only
    because of the slack."""
    case = ia.slack_edge(d, axis, metric)
    ref = _all_kinds(case, monkeypatch)
    cnt = np.diff(ref["csr"][case["r_max"]][0])
    assert (cnt[case["role"] != 3] == 2).all() and (cnt[case["role"] == 3] == 1).all()


# ------------------------------------------------------------ c. key width
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", sorted(ia.KEY_SHAPES))
def test_key_width(monkeypatch, shape, dtype):
    """Grids on both sides of the 4 / 8-byte key boundary, groups at keys near
    0, near G - 1 and 2^32 apart; queries one cell outside the far faces."""
    case = ia.key_width(shape, dtype)
    ref = _all_kinds(case, monkeypatch)
    _triple_expectations(case, ref, case["key"])
    if dtype == "float64":
        rows_only = dict(case, Q=case["X"], key=case["key"] + ("rows",))
        _public(rows_only, ia.reference(rows_only))
        _all_kinds(ia.key_width(shape, dtype, "cityblock"), monkeypatch)


# ------------------------------------------------------------ d. faces
FACES = [(dt, d, m, kind) for dt in DTYPES for d in (1, 2, 3, 4) for m in METRICS
         for kind in ia.FACE_KINDS if not (kind == "plane" and d < 2)]


@pytest.mark.parametrize("dtype,d,metric,kind", FACES)
def test_faces(monkeypatch, dtype, d, metric, kind):
    """Queries outside the box: less than a cell, at the last accepted
    distance and one step on either side of it, at the corners, and more than
    a cell out."""
    case = ia.faces(dtype, d, metric, kind)
    ks = (1, 2) if kind in ("twins", "plane") else (1,)
    ref = _all_kinds(case, monkeypatch, ks=ks, forest=False)
    cnt = np.diff(ref["csr"][case["r_max"]][0])
    assert (cnt[case["expect_none"]] == 0).all()
    lv = case["level"]
    assert (cnt[lv == 2] >= 1).all() and (cnt[lv == 0] >= 1).all()
    if kind in ("single", "twins"):
        n = len(case["X"])
        assert (cnt[lv <= 2] == n).all() and (cnt[lv == 3] == 0).all()
    if kind == "box" and dtype == "float64" and metric == "euclidean":
        from pypardis_amd import k_distances, kneighbors, radius_neighbors
        dx, dq, r = _dev(case["X"]), _dev(case["Q"]), case["r_max"]
        want = knn_ref.cut(ref["pairs"], 1, r, metric)
        assert np.array_equal(_np(k_distances(dx, 1, r, metric, queries=dq, squared=True)), want[1][:, 0])
        assert np.array_equal(_np(kneighbors(dx, 1, r, metric, queries=dq).indices), want[0])
        assert np.array_equal(_np(radius_neighbors(dx, r, metric, queries=dq, count_only=True)), cnt)


# ------------------------------------------------------------ e. k shell
@pytest.mark.parametrize("dtype,d,metric", [(dt, d, m) for dt in DTYPES for d in (2, 4)
                                            for m in METRICS])
def test_k_shell(monkeypatch, dtype, d, metric):
    """A k-list filled exactly to the cap: with the query itself exactly k rows
    qualify, each at the last accepted offset; k - 1 twins one step out."""
    case = ia.k_shell(dtype, d, metric)
    r = case["r_max"]
    ref = _all_kinds(case, monkeypatch, ks=ia.KS, forest=False)
    thr = ga.threshold(r, metric)
    cnt = np.diff(ref["csr"][r][0])
    for k, iq, ins, outs in case["shell"]:
        assert cnt[iq] == k
        kd = ia.kdist_of(ref["pairs"], k, r, metric)[iq]
        assert np.isfinite(kd) and kd <= thr
        if k < 64:
            assert np.isinf(ia.kdist_of(ref["pairs"], k + 1, r, metric)[iq])
            ids, acc = knn_ref.cut(ref["pairs"], k + 1, r, metric)
            assert ids[iq, k] == -1 and np.isinf(acc[iq, k]) and ids[iq, k - 1] >= 0
            assert set(ids[iq, :k].tolist()) == set([iq] + ins.tolist())
    # the forest at k = 2 (every shell is one tree: its twins hang on the in rows)
    _all_kinds(case, monkeypatch, ks=(2,), predict=False)
    if dtype == "float64" and metric == "euclidean":
        _public(case, ia.reference(case, (r,), r, kmax=3, forest_k=2))


@pytest.mark.parametrize("dtype,d,metric", [(dt, d, m) for dt in DTYPES for d in (2, 4)
                                            for m in METRICS])
def test_k_shell_weighted(monkeypatch, dtype, d, metric):
    """Dyadic weights whose running sum reaches min_samples exactly on the last
    in row of a shell; the twins carry a weight that would cross at once."""
    case = ia.k_shell(dtype, d, metric, ia.KS[:-1])
    X, r = case["X"], case["r_max"]
    w, ms_of = ia.shell_weights(case)
    thr = ga.threshold(r, metric)
    want = {k: wkdist_ref.cdw(X, w, ms, r, metric) for k, ms in ms_of.items()}
    for k, iq, ins, outs in case["shell"]:
        cd = want[k][iq]
        assert np.isfinite(cd) and cd <= thr
        assert np.isinf(wkdist_ref.cdw(X[[iq] + ins.tolist()], w[[iq] + ins.tolist()],
                                       ms_of[k] + 1, r, metric)[0])
    dx = _dev(X)
    for sort in SORTS:
        monkeypatch.setenv("PD_INDEX_SORT_MIN", sort)
        ix = _rows_index(X, r, metric)
        try:
            ix.set_weights(_dev(w))
            for k, ms in ms_of.items():
                assert np.array_equal(_np(ix.kdist_weighted(dx, ms)), want[k]), (sort, k, ms)
        finally:
            ix.close()
    from pypardis_amd import k_distances
    k, ms = 9, ms_of[9]
    got = k_distances(dx, ms, r, metric, squared=True, sample_weight=_dev(w))
    assert np.array_equal(_np(got), want[k])


# ------------------------------------------------------------ f. screen band
@pytest.mark.parametrize("d,metric", [(d, m) for d in (1, 2, 3, 4) for m in METRICS])
def test_screen_band(monkeypatch, d, metric):
    """The fp32 misdecision and band-edge pairs through query_kernel's screen:
    the expected label is the smaller row number of an accepted pair, or the
    row's own, so a pair wrongly accepted or rejected shows on one row."""
    case = ia.screen(d, metric)
    ref = _all_kinds(case, monkeypatch)
    n = len(case["X"])
    assert (ref["predict"] <= np.arange(n)).all() and (ref["predict"] < np.arange(n)).any()
    _public(case, ref)


# ------------------------------------------------------------ g. scaled goldens
def _ask_golden(r, X, eps, monkeypatch, sort):
    """kdist, kneighbors ids + acc, radius counts, the forest (d <= 4) and
    query() on the golden's own cores and labels."""
    from pypardis_amd import _native
    metric, ms = r["metric"], r["min_samples"]
    d = X.shape[1]
    monkeypatch.setenv("PD_INDEX_SORT_MIN", sort)
    dx = _dev(X)
    out = {}
    ix = _rows_index(X, eps, metric)
    try:
        out["kdist"] = _np(ix.kdist(dx, ms))
        ids, acc = ix.kneighbors(dx, min(ms, 64))
        out["ids"], out["acc"] = _np(ids), _np(acc)
        out["counts"] = np.diff(_np(ix.radius(dx, eps, count_only=True)[0]))
        if d <= 4:
            u, v, w, cd, _ = ix.mreach_forest(ms)
            out["forest"] = (_np(u), _np(v), _np(w), _np(cd))
    finally:
        ix.close()
    lab = r["labels"].astype(np.int32)
    ix = _native.Index(dx, _dev(r["core"].astype(np.uint8)), _dev(np.maximum(lab, 0)), eps,
                       CODE[metric])
    try:
        out["query"] = _np(ix.query(dx)).astype(np.int64)
    finally:
        ix.close()
    return out


_UNSCALED = {}


@pytest.mark.parametrize("name,dtype,s", ga.scaled_cases())
def test_scaled_golden(monkeypatch, name, dtype, s):
    """A golden times 2^s asks the same questions: accumulators scaled by
    2^(2 s) (cityblock 2^s), the same ids, counts, forest edges and labels.
    The index keeps its geometry in fp64, so every exponent of the family runs,
    also those outside the train's eps range and on both sides of the fp32
    screen's gate (float(thr) = 0 or inf for float32 rows)."""
    r = ia.scaled(name, dtype, s)
    e = 2 * s if r["metric"] == "euclidean" else s
    if (name, dtype) not in _UNSCALED:
        _UNSCALED[name, dtype] = _ask_golden(r, r["X0"], r["eps0"], monkeypatch, SORTS[1])
    base = _UNSCALED[name, dtype]
    assert np.array_equal(base["counts"], r["counts"])
    assert np.array_equal(base["query"], r["labels"])
    for sort in SORTS:
        got = _ask_golden(r, r["X"], r["eps"], monkeypatch, sort)
        assert np.array_equal(got["counts"], r["counts"]), sort
        assert np.array_equal(got["query"], r["labels"]), sort
        assert np.array_equal(got["kdist"], np.ldexp(base["kdist"], e)), sort
        assert np.array_equal(got["ids"], base["ids"]), sort
        assert np.array_equal(got["acc"], np.ldexp(base["acc"], e)), sort
        if "forest" in base:
            for a, b, scaled in zip(got["forest"], base["forest"], (False, False, True, True)):
                assert np.array_equal(a, np.ldexp(b, e) if scaled else b), sort


# (name, dtype, s, whether eps is inside the train's range: test_gpu_grid_adversarial.eps_supported)
PUBLIC_SCALED = [("b2d_20k", "float32", -64, True),      # float(thr) underflows: the gate is shut
                 ("b2d_20k", "float32", 100, False),     # float(thr) = inf
                 ("b3d_20k", "float64", -80, True),
                 ("b3d_20k", "float64", 480, False)]


@pytest.mark.parametrize("name,dtype,s,train_ok", PUBLIC_SCALED)
def test_scaled_golden_public(monkeypatch, name, dtype, s, train_ok):
    """The public functions on scaled goldens, two per dtype: k_distances,
    kneighbors, radius_neighbors and mutual_reachability_forest against the
    unscaled set's answers scaled exactly, the golden's counts and labels.
    DBSCAN.train(...).predict runs where eps is inside the train's range; on
    (b2d_20k, float32, 100) and (b3d_20k, float64, 480) it is outside
    (the fp32 cell geometry of the d <= 4 train), so the
    train is not run there — the index queries are."""
    from pypardis_amd import (DBSCAN, k_distances, kneighbors, mutual_reachability_forest,
                              radius_neighbors)
    r = ia.scaled(name, dtype, s)
    metric, ms, eps = r["metric"], r["min_samples"], r["eps"]
    e = 2 * s if metric == "euclidean" else s
    if (name, dtype) not in _UNSCALED:
        _UNSCALED[name, dtype] = _ask_golden(r, r["X0"], r["eps0"], monkeypatch, SORTS[1])
        monkeypatch.delenv("PD_INDEX_SORT_MIN")
    base = _UNSCALED[name, dtype]
    dx = _dev(r["X"])
    assert np.array_equal(_np(k_distances(dx, ms, eps, metric, squared=True)),
                          np.ldexp(base["kdist"], e))
    res = kneighbors(dx, ms, eps, metric, squared=True)
    assert np.array_equal(_np(res.indices), base["ids"])
    assert np.array_equal(_np(res.distances), np.ldexp(base["acc"], e))
    assert np.array_equal(_np(radius_neighbors(dx, eps, metric, count_only=True)), r["counts"])
    f = mutual_reachability_forest(dx, ms, eps, metric, squared=True)
    u, v, w, cd = base["forest"]
    assert np.array_equal(_np(f.u), u) and np.array_equal(_np(f.v), v)
    assert np.array_equal(_np(f.distances), np.ldexp(w, e))
    assert np.array_equal(_np(f.core_distances), np.ldexp(cd, e))
    if train_ok:
        m = DBSCAN(eps=eps, min_samples=ms, metric=metric).train(dx)
        assert np.array_equal(_np(m.labels_).astype(np.int64), r["labels"])
        assert np.array_equal(_np(m.predict(dx)).astype(np.int64), r["labels"])


# ------------------------------------------------------------ h. the tile kernels (d > 4)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [8, 64])
def test_tile_ties(monkeypatch, d, dtype):
    """Accumulators of exactly 9 and exactly 10 against thr = 9: the axis loop
    breaks at the first partial sum ABOVE the bound, never at it.  (No d = 5:
    dense_adversarial.tie_islands needs d >= 8 for its axes; at d = 5 the ties
    at acc == thr are those of test_tile_row_and_query_counts.)  The public
    k_distances, kneighbors and radius_neighbors run on every set here and in
    test_tile_shell; the forest is d <= 4, and predict on these sets runs in
    test_gpu_dense_band."""
    case = ia.tile_ties(d, dtype)
    ref = _all_kinds(case, monkeypatch, ks=(1, 2, 16, 17), forest=False)
    acc = ref["csr"][3.0][2]
    assert (acc == 9.0).any() and (ref["pairs"][1] == 10.0).any()
    _public_queries(case, ref, k=16)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [5, 8, 64])
def test_tile_shell(monkeypatch, d, dtype):
    """Partners at eps (1 +- 2^-k), k = 4 .. 52."""
    case = ia.tile_shell(d, dtype)
    ref = _all_kinds(case, monkeypatch, forest=False)
    cnt = np.diff(ref["csr"][case["r_max"]][0])
    assert (cnt == 1).sum() > 100 and (cnt == 2).sum() > 100
    _public_queries(case, ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [5, 8, 64])
def test_tile_row_and_query_counts(monkeypatch, d, dtype):
    """Row counts around the tile (the LAST row is the only neighbour, at
    acc == thr) and query counts around the block sizes."""
    for n_rows in (1, 63, 64, 65, 129):
        for n_q in ((255, 256, 257) if n_rows in (1, 65) else (63, 65, 127, 129)):
            case = ia.tile_counts(d, dtype, n_rows, n_q)
            ref = _all_kinds(case, monkeypatch, ks=(1,), forest=False)
            ids, acc = knn_ref.cut(ref["pairs"], 1, 3.0, "euclidean")
            assert (ids[0::2, 0] == n_rows - 1).all() and (acc[0::2, 0] == 9.0).all()
            assert (ids[1::2, 0] == -1).all()


# ------------------------------------------------------------ far cells (grid_adversarial)
FAR = [(d, axis) for d in (2, 3, 4) for axis in range(1, d)]


@pytest.mark.parametrize("d,axis", FAR)
def test_far_cell_index_all_kinds(monkeypatch, d, axis):
    """grid_adversarial.far_cell (pairs two rows apart at index ~2^34 under the
    ungrown formula): the index grows its cells, and every kind finds them."""
    r = ga.far_cell_detail("float64", d, axis)
    role = np.where(r["groups"] == r["anchor"], 3, 0)
    case = ia._case("far_cell", ("float64", d, axis), r["X"], r["groups"], role, r["eps"],
                    r["metric"], k=2)
    assert case["grow"] > 1.0
    ref = _all_kinds(case, monkeypatch)
    cnt = np.diff(ref["csr"][r["eps"]][0])
    assert (cnt[role == 0] == 2).all() and (cnt[role == 3] == 1).all()
