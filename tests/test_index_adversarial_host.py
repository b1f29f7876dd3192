"""The generators of tests/index_adversarial.py produce what they claim: every
condition below is what makes a set adversarial for the index queries of
csrc/assign.hip (tests/test_gpu_index_adversarial.py runs them on the GPU).
CPU only.  The grid model (index_grid) places points; the asserted nc, grow, G
and key width are the model's, on both sides of every grid decision."""
import numpy as np
import pytest

import grid_adversarial as ga
import index_adversarial as ia
import kdist_ref
import wkdist_ref

DTYPES = ("float64", "float32")
METRICS = ("euclidean", "cityblock")


def _isolated(case):
    X = case["X"]
    assert len(X) <= 20_000 and len(case["Q"]) <= 20_000
    sep = ga.group_min_separation(X, case["groups"], case["metric"])
    assert sep >= 4.0 * case["r_max"], sep


def _triples(case, min_keep=0.9):
    """acc(in) <= thr < acc(twin); twin and neighbour adjacent representable
    values; the straddling pair in different cells of index_grid; >= 90 % of
    the enumerated combinations kept."""
    q, n_in, n_out = case["q"], case["n_in"], case["n_out"]
    metric, thr = case["metric"], ga.threshold(case["r_max"], case["metric"])
    print(case["key"], "kept", len(q), "of", case["enumerated"])
    assert len(q) >= min_keep * case["enumerated"]
    assert (ga.pair_acc(q, n_in, metric) <= thr).all() and (ga.pair_acc(q, n_out, metric) > thr).all()
    diff = n_in != n_out
    assert (diff.sum(axis=1) == 1).all()
    a, b = n_in[diff], n_out[diff]
    assert (np.nextafter(a, b) == b).all()
    cq = ia.row_cells(q, case["lo"], case["inv"])
    cn = ia.row_cells(n_in, case["lo"], case["inv"])
    assert (cq != cn).any(axis=1).all()
    assert np.abs(cq - cn).max() == 1
    return cq, cn


# ------------------------------------------------------------ the grid model
def test_index_grid_follows_the_documented_formula():
    X = np.array([[0.0, 0.0], [1.0, 0.26]])
    lo, inv, nc, grow, G, kb = ia.index_grid(X, 0.05)
    cw = 0.05 * (1.0 + 2.0 ** -20) * 1.0
    assert inv == 1.0 / cw and grow == 1.0 and list(nc) == [20, 6] and G == 120 and kb == 4
    # an axis of more than 2^28 cells doubles the cells until it fits
    X = np.array([[0.0], [0.05 * 2.0 ** 30]])
    lo, inv, nc, grow, G, kb = ia.index_grid(X, 0.05)
    assert grow == 4.0 and 2 ** 28 - 512 < nc[0] <= 2 ** 28 and kb == 4
    # G < 4e18 with every axis below the cap
    X = np.array([[0.0] * 3, [0.05 * 2.0 ** 27] * 3])
    lo, inv, nc, grow, G, kb = ia.index_grid(X, 0.05)    # (2^27 / 64)^3 = 2^63 > 4e18 > 2^60
    assert grow == 128.0 and G < 4.0e18 < 8 * G and kb == 8
    # the key width switches at G = 2^32 - 1
    assert ia.KEY4_BELOW == 2 ** 32 - 1


# ------------------------------------------------------------ a. cell edge
@pytest.mark.parametrize("offset", [0.0, 2.0 ** 20])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cell_edge_is_at_the_indexes_own_boundaries(dtype, d, metric, offset):
    case = ia.cell_edge(dtype, d, metric, offset)
    r = ga.chord_edge_detail(dtype, d, metric, 1, 1.0, offset)
    # the index's tight box and cells are the generator's
    assert np.array_equal(case["lo"], r["lo"]) and case["inv"] == r["inv"][1] == r["inv"][0]
    assert case["grow"] == 1.0 and case["key_bytes"] == 4
    assert np.array_equal(case["X"].max(axis=0).astype(np.float64), r["hi"])
    # euclidean: all 360 / 1080 / 1440 combinations survive, 1082 / 3242 / 4322 rows;
    # cityblock: two rows crossed at half a cell each are further than eps (1040, 1360)
    want = {2: 360, 3: 1080, 4: 1440}[d]
    kept = want if metric == "euclidean" else {2: 360, 3: 1040, 4: 1360}[d]
    assert case["enumerated"] == want and len(case["q"]) == kept and len(case["X"]) == 3 * kept + 2
    cq, cn = _triples(case)
    for j in range(1, d):
        assert np.array_equal((cn - cq)[:, j], case["side"][:, j])
    _isolated(case)


# ------------------------------------------------------------ b. cap edge
@pytest.mark.parametrize("d,axis", [(d, a) for d in (2, 3, 4) for a in range(d)])
def test_cap_edge_sits_on_both_sides_of_the_cap(d, axis):
    a, b = ia.cap_edge(d, axis, False), ia.cap_edge(d, axis, True)
    assert a["grow"] == 1.0 and a["nc"][axis] == 2 ** 28
    assert b["grow"] == 2.0 and b["nc"][axis] == 2 ** 27 + 1
    for c in (a, b):
        assert c["X"].dtype == np.float64
        assert all(c["nc"][j] <= 4 for j in range(d) if j != axis)
        assert c["G"] == int(np.prod([int(v) for v in c["nc"]]))
        assert c["key_bytes"] == (4 if c["G"] < 2 ** 32 - 1 else 8)
        assert len(c["q"]) >= 96
        cq, cn = _triples(c)
        # both ends of the long axis; across it and across a short one
        assert cq[:, axis].min() <= 16 and cq[:, axis].max() >= c["nc"][axis] - 17
        crossed_long = (cq != cn)[:, axis]
        for end in (cq[:, axis] < 2 ** 20, cq[:, axis] > 2 ** 20):
            assert (crossed_long & end).sum() >= 20
            if d > 1:
                assert ((cq != cn)[:, [j for j in range(d) if j != axis]].any(axis=1) & end).sum() >= 20
        _isolated(c)
    if d == 2:
        _triples(ia.cap_edge(d, axis, False, "cityblock"))
        _triples(ia.cap_edge(d, axis, True, "cityblock"))


def test_cap_edge_is_float64_only():
    """float32 cannot resolve 2^28 cells of an axis: with 24 significant bits
    the values at the far end of an extent of 2^28 cells are 2^(28 - 24) = 16
    cells apart, so no float32 row can be placed relative to a cell there."""
    cw = ga.cell_width(ia.EPS)
    assert np.spacing(np.float32(2.0 ** 28 * cw)) >= 16.0 * cw * (1.0 - 2.0 ** -20)


def test_far_cell_search_under_the_cap_finds_no_pair(monkeypatch):
    """grid_adversarial.far_cell's search with the pairs' cells starting at
    index 2^28 instead of 2^34 (lo moved accordingly) finds no pair within eps
    whose cells differ by 2: under the cap the reference's counts are reachable
    by a walk of +-1 cell.  (The same search at 2^27, 2^28 - 70000, 2^30 and
    2^32 finds none either; a search result, not a proof.)"""
    monkeypatch.setattr(ga, "FAR_INDEX", 2 ** 28)
    r = ga.far_cell_detail("float64", 2, 1, 1, 96, 8, 0.05, -(2.0 ** 28 * 0.05) - 7.25)
    assert len(r["pairs"]) == 0 and len(r["control"]) == 8
    c = np.floor((r["X"][:, 1] - r["lo"]) * r["inv"])
    assert c.max() >= 2 ** 28


SLACK = [(d, a, m) for d, a in ((1, 0), (2, 0), (2, 1), (3, 2), (4, 3)) for m in METRICS]


@pytest.mark.parametrize("d,axis,metric", SLACK)
def test_slack_edge_pairs_need_the_slack(d, axis, metric):
    """Within eps, two cells apart under cw = eps, one cell apart under the
    real width eps (1 + 2^-20)."""
    c = ia.slack_edge(d, axis, metric)
    a1, a2, lo = c["a1"], c["a2"], float(c["lo"][axis])
    print(c["key"], "hits", c["hits"], "of", c["candidates"], "candidates")
    assert len(a1) >= 96 and lo == -1000.1 and c["grow"] == 1.0
    assert (ga.pair_acc(a1[:, None], a2[:, None], metric) <= ga.threshold(c["r_max"], metric)).all()
    assert c["inv_no_slack"] == 1.0 / c["r_max"]
    narrow = ga.cells(a2, lo, c["inv_no_slack"]) - ga.cells(a1, lo, c["inv_no_slack"])
    real = ga.cells(a2, lo, c["inv"]) - ga.cells(a1, lo, c["inv"])
    assert (narrow == 2).all() and (real == 1).all()
    X, role = c["X"], c["role"]
    for j in range(d):
        if j != axis:
            assert (ga.cells(X[:, j], float(c["lo"][j]), c["inv"]) == 0).all()
    cnt = ga.brute_counts(X, c["r_max"], metric)
    assert (cnt[role != 3] == 2).all() and (cnt[role == 3] == 1).all()
    _isolated(c)


# ------------------------------------------------------------ c. key width
@pytest.mark.parametrize("dtype", DTYPES)
def test_key_width_grids_sit_on_both_sides_of_the_boundary(dtype):
    want = {"2d_below": (2 ** 32 - 65536, 4), "2d_first8": (2 ** 32 - 1, 8), "2d_pow": (2 ** 32, 8),
            "2d_over": (2 ** 32 + 2 ** 20, 8), "3d_first8": (2 ** 32 - 1, 8)}
    for shape, (G, kb) in want.items():
        for metric in METRICS:
            c = ia.key_width(shape, dtype, metric)
            assert tuple(c["nc"]) == ia.KEY_SHAPES[shape] and c["grow"] == 1.0
            assert c["G"] == G and c["key_bytes"] == kb
            cq, cn = _triples(c)
            kq = np.array(ia.cell_keys(cq, c["nc"]), dtype=object)
            kn = np.array(ia.cell_keys(cn, c["nc"]), dtype=object)
            assert min(kq.min(), kn.min()) < 2 ** 17           # the first rows of cells
            assert max(kq.max(), kn.max()) > G - 2 ** 17       # and the last
            if shape == "2d_over":
                # rows of cells whose keys differ only above bit 31
                low = {int(k) for k in kq if k < 2 ** 32} | {int(k) for k in kn if k < 2 ** 32}
                high = [int(k) for k in list(kq) + list(kn) if k >= 2 ** 32]
                assert sum(k - 2 ** 32 in low for k in high) >= 12
            # the query twins lie one cell outside a far face
            Q = c["Q"][len(c["X"]):]
            s = (Q.astype(np.float64) - c["lo"]) * c["inv"]
            out = s >= c["nc"]
            assert out.any(axis=1).all() and (s < c["nc"] + 1.0).all() and (s >= 0).all()
            assert len(Q) >= len(c["nc"]) * 6
            _isolated(c)


# ------------------------------------------------------------ d. faces
@pytest.mark.parametrize("dtype,d,metric,kind",
                         [(dt, d, m, k) for dt in DTYPES for d in (1, 2, 3, 4) for m in METRICS
                          for k in ia.FACE_KINDS if not (k == "plane" and d < 2)])
def test_faces_queries_sit_at_the_last_accepted_distance(dtype, d, metric, kind):
    c = ia.faces(dtype, d, metric, kind)
    X, Q, lv, src, ax = c["X"], c["Q"], c["level"], c["src"], c["axis"]
    thr = ga.threshold(c["r_max"], metric)
    assert c["found"] and X.dtype == Q.dtype == np.dtype(dtype)
    near = lv < 4
    acc = ga.pair_acc(Q[near], X[src[near]], metric)
    assert (acc[lv[near] <= 2] <= thr).all() and (acc[lv[near] == 3] > thr).all()
    # below / at / above are three neighbouring values of the walked coordinate
    for a, b in ((1, 2), (2, 3)):
        va, vb = Q[lv == a, ax[lv == a]], Q[lv == b, ax[lv == b]]
        assert ((np.nextafter(va, vb) == vb) & (va != vb)).all()
    # every such query lies outside the box, by less than a cell
    s = (Q.astype(np.float64) - c["lo"]) * c["inv"]
    outside = (Q < X.min(axis=0)) | (Q > X.max(axis=0))
    off = near & (ax == 0) if kind == "plane" else near      # (a plane: also queries inside it)
    assert outside[off].any(axis=1).all() and off.sum() >= 8
    ok = lv <= 2        # (the rejected query one step on may be more than a cell out)
    assert ((s[ok] >= -1.0) & (s[ok] < c["nc"] + 1.0)).all()
    if kind == "box":
        # outside on every axis at once, at both corners
        allout = outside[near].all(axis=1)
        assert (allout & (lv[near] == 2)).sum() >= 2
        assert (c["nc"] == 6).all()
        # every face has a row on it, and a query beyond it
        for j in range(d):
            assert (Q[near][:, j] < X[:, j].min()).any() and (Q[near][:, j] > X[:, j].max()).any()
    if kind == "plane":
        assert c["nc"][0] == 1 and (X[:, 0] == X[0, 0]).all()
    if kind in ("single", "twins"):
        assert (c["nc"] == 1).all() and len(X) == (1 if kind == "single" else 2)
    # the far queries: more than one cell outside on their axis, nothing within eps
    far = ~near
    assert far.sum() >= 4 * d
    sj = s[far, ax[far]]
    assert ((sj < -1.0) | (sj >= c["nc"][ax[far]] + 1.0)).all()
    assert (kdist_ref.accumulators(Q[far], X, metric) > thr).all()
    assert np.array_equal(c["expect_none"], far)


# ------------------------------------------------------------ e. k shell
@pytest.mark.parametrize("dtype,d,metric", [(dt, d, m) for dt in DTYPES for d in (2, 4)
                                            for m in METRICS])
def test_k_shell_fills_the_list_exactly(dtype, d, metric):
    c = ia.k_shell(dtype, d, metric)
    X = c["X"]
    thr = ga.threshold(c["r_max"], metric)
    assert c["found"] and sorted({s[0] for s in c["shell"]}) == sorted(ia.KS)
    cc = ia.row_cells(X, c["lo"], c["inv"])
    reach = 2 * d if metric == "cityblock" else {2: 6, 4: 38}[d]
    for k, iq, ins, outs in c["shell"]:
        assert len(ins) == len(outs) == k - 1
        if k == 1:
            continue
        q = np.repeat(X[iq][None, :], k - 1, axis=0)
        assert (ga.pair_acc(q, X[ins], metric) <= thr).all()
        assert (ga.pair_acc(q, X[outs], metric) > thr).all()
        assert (X[ins][:, :-1] == X[outs][:, :-1]).all()
        a, b = X[ins][:, -1], X[outs][:, -1]
        assert ((np.nextafter(a, b) == b) & (a != b)).all()
        # every in row in another cell than the query's, in as many different
        # cells as k - 1 rows within eps of a cell's middle can reach
        assert (cc[ins] != cc[iq]).any(axis=1).all()
        assert len({tuple(v) for v in cc[ins].tolist()}) >= 0.75 * min(k - 1, reach)
    _isolated(c)
    # the weighted variant: the sum reaches ms exactly on the last in row
    cw = ia.k_shell(dtype, d, metric, ia.KS[:-1])
    w, ms_of = ia.shell_weights(cw)
    assert wkdist_ref.slots_needed(w, max(ms_of.values())) <= wkdist_ref.MAX_SLOTS
    for k, iq, ins, outs in cw["shell"]:
        rows = [iq] + ins.tolist()
        assert w[rows].sum() == ms_of[k]
        sub = cw["X"][rows]
        assert np.isfinite(wkdist_ref.cdw(sub, w[rows], ms_of[k], cw["r_max"], metric)[0])
        assert np.isinf(wkdist_ref.cdw(sub, w[rows], ms_of[k] + 1, cw["r_max"], metric)[0])
        if k > 1:
            drop = [iq] + ins.tolist()[1:]
            assert np.isinf(wkdist_ref.cdw(cw["X"][drop], w[drop], ms_of[k], cw["r_max"], metric)[0])


# ------------------------------------------------------------ f. screen band
@pytest.mark.parametrize("d,metric", [(d, m) for d in (1, 2, 3, 4) for m in METRICS])
def test_screen_holds_both_kinds_of_misdecision(d, metric):
    c = ia.screen(d, metric)
    X, m = c["X"], c["mis"]
    thr = ga.threshold(c["r_max"], metric)
    assert X.dtype == np.float32 and 1e-30 < thr < 1e30      # query_kernel's gate is open
    a32 = ga.screen_acc32(X[m[:, 0]], X[m[:, 1]], metric)
    exact = ga.pair_acc(X[m[:, 0]], X[m[:, 1]], metric) <= thr
    assert len(m) >= 64 and ((a32 <= np.float32(thr)) != exact).all()
    print(c["key"], "wrongly rejected", int(exact.sum()), "wrongly accepted", int((~exact).sum()),
          "band edge", len(c["edge"]))
    assert len(c["edge"]) >= 1                               # both kinds: misdecided and band-edge
    # the expected label of query(): the smaller row of an accepted pair, else its own
    ref = ia.reference(c)
    want = np.arange(len(X))
    hit = m[exact]
    want[hit.max(axis=1)] = hit.min(axis=1)
    e = c["edge"]
    ein = ga.pair_acc(X[e[:, 0]], X[e[:, 1]], metric) <= thr
    want[e[ein].max(axis=1)] = e[ein].min(axis=1)
    assert np.array_equal(ref["predict"], want)
    _isolated(c)


def test_screen_sets_hold_both_directions():
    """Over the eight sets: pairs the bare fp32 test rejects and the exact one
    accepts, and pairs it accepts and the exact one rejects (the search finds
    the first kind only at d >= 3)."""
    rejected = accepted = 0
    for d in (1, 2, 3, 4):
        for metric in METRICS:
            c = ia.screen(d, metric)
            X, m = c["X"], c["mis"]
            exact = ga.pair_acc(X[m[:, 0]], X[m[:, 1]], metric) <= ga.threshold(c["r_max"], metric)
            rejected += int(exact.sum())
            accepted += int((~exact).sum())
    assert rejected >= 10 and accepted >= 500


# ------------------------------------------------------------ g. scaled goldens
def test_scaling_is_exact_for_every_case():
    """The numpy reference on 1500 rows of each golden: within the threshold
    every accumulator scales exactly and nothing leaves the normal range, at
    every exponent of the family — so all of them run on the GPU, also those
    outside the train's eps range.  Cases where it is not exact, by name:"""
    inexact = [c for c in ga.scaled_cases() if not ia.scaling_is_exact(*c)]
    assert inexact == []
    # float(thr) = 0 and inf for float32 rows, and both sides of the screen's gate
    thr = [ga.threshold(ia.scaled("b2d_20k", "float32", s)["eps"], "euclidean")
           for s in ga.SCALE_EXPONENTS["float32"]]
    with np.errstate(over="ignore", under="ignore"):
        f = [float(np.float32(t)) for t in thr]
    assert 0.0 in f and np.inf in f
    assert any(t <= 1e-30 for t in thr) and any(t >= 1e30 for t in thr)
    assert any(1e-30 < t < 1e30 for t in thr)


# ------------------------------------------------------------ h. the tile kernels
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_sets(dtype):
    for d in (8, 64):
        c = ia.tile_ties(d, dtype)
        acc = kdist_ref.accumulators(c["X"], c["X"])
        assert (acc == 9.0).any() and (acc == 10.0).any() and len(c["X"]) <= 4000
        assert ga.threshold(c["r_max"], "euclidean") == 9.0
    for d in (5, 8, 64):
        c = ia.tile_shell(d, dtype)
        assert len(c["X"]) <= 4000 and c["X"].shape[1] == d
    for n_rows in (1, 63, 64, 65, 129):
        c = ia.tile_counts(5, dtype, n_rows, 257)
        acc = kdist_ref.accumulators(c["Q"], c["X"])
        assert (acc[0::2, -1] == 9.0).all() and (acc[1::2, -1] == 10.0).all()
        assert (acc[:, :-1] >= 100.0).all() and acc.shape == (257, n_rows)


def test_reference_tiles_are_the_untiled_table():
    c = ia.cell_edge("float32", 3, "cityblock", 0.0)
    X = c["X"]
    assert len(X) > kdist_ref.MAX_N
    t = ia.table(X, X, "cityblock")
    rows = np.array([0, 2999, 3000, len(X) - 1])
    assert np.array_equal(t[rows], np.stack([ga.pair_acc(X[i][None, :], X, "cityblock")
                                             for i in rows]))
