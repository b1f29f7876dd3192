"""Pins the CPU oracle (oracle/) to the reference before anything is checked
against it: sklearn's own known-answer tests, global sklearn DBSCAN outputs,
and the stage outputs of the reference pipeline run under an RDD stand-in
(tests/golden/make_golden.py)."""
import numpy as np
import pytest

import oracle
from conftest import GOLDEN, golden_names, load_golden, rotation_names

NAMES = golden_names()
ROT = rotation_names()


@pytest.mark.parametrize("name", ROT)
def test_rotation_partition_matches_reference(name):
    """split_method='rotation' (median_search_split, R:dbscan/partition.py:8-30):
    medians, split sizes, boxes and owner labels equal the reference's."""
    g = load_golden(name, "rot")
    kd = oracle.kd_partition(g["X"], int(g["max_partitions"]), split_method="rotation")
    sp = np.array([[s[0], s[1], s[2], s[4], s[5]] for s in kd["splits"]], np.int64)
    assert np.array_equal(sp, g["splits"])
    assert np.array_equal(np.array([s[8] for s in kd["splits"]]), g["medians"])
    assert np.array_equal(kd["box_lo"], g["box_lo"])
    assert np.array_equal(kd["box_hi"], g["box_hi"])
    assert np.array_equal(kd["owner"], g["owner"])


def _metric(g):
    m = str(g["metric"])
    return "euclidean" if m == "callable" else m


def _P(g):
    P = int(g["max_partitions"])
    return None if P < 0 else P


def test_sklearn_kats():
    z = np.load(f"{GOLDEN}/sklearn_kat.npz")
    for ms in (1, 2, 3, 4):
        lab, core, _, _ = oracle.dbscan(z["toy_X"], 1.0, ms)
        assert np.array_equal(lab, z[f"toy_ms{ms}_labels"])
        assert np.array_equal(np.nonzero(core)[0], z[f"toy_ms{ms}_core"])
    # eps inclusive, min_samples counts the point itself (SK test_boundaries)
    assert np.array_equal(np.nonzero(oracle.dbscan(z["bnd_a_X"], 2, 2)[1])[0], z["bnd_a_core"])
    assert np.array_equal(np.nonzero(oracle.dbscan(z["bnd_b_X"], 1, 2)[1])[0], z["bnd_b_core_eps1"])
    assert np.array_equal(np.nonzero(oracle.dbscan(z["bnd_b_X"], 0.99, 2)[1])[0],
                          z["bnd_b_core_eps099"])
    lab, core, _, _ = oracle.dbscan(z["clustered_X"], 0.8, 10)
    assert np.array_equal(lab, z["clustered_labels"])
    assert np.array_equal(np.nonzero(core)[0], z["clustered_core"])
    lab, core, _, nc = oracle.dbscan(z["nocore_X"], 0.5, 6)
    assert nc == 0 and core.sum() == 0 and np.all(lab == -1)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_global_sklearn(name):
    g = load_golden(name)
    lab, core, cnt, _ = oracle.dbscan(g["X"], float(g["eps"]), int(g["min_samples"]), _metric(g))
    assert np.array_equal(cnt, g["sk_counts"])
    assert np.array_equal(core, g["sk_core"])
    assert np.array_equal(lab, g["sk_labels"])


@pytest.mark.parametrize("name", NAMES)
def test_kd_partition_matches_reference(name):
    g = load_golden(name)
    kd = oracle.kd_partition(g["X"], _P(g))
    sp = np.array([s[:6] for s in kd["splits"]], np.int64).reshape(-1, 6)
    sf = np.array([s[6:] for s in kd["splits"]], np.float64).reshape(-1, 3)
    assert np.array_equal(sp, g["splits"])
    assert np.array_equal(sf, g["split_f"])          # bit-exact mean/var/boundary
    assert np.array_equal(kd["box_lo"], g["box_lo"])
    assert np.array_equal(kd["box_hi"], g["box_hi"])
    assert np.array_equal(kd["owner"], g["owner"])


@pytest.mark.parametrize("name", NAMES)
def test_halo_matches_reference(name):
    g = load_golden(name)
    elo, ehi, members = oracle.halo(g["X"], g["box_lo"], g["box_hi"], float(g["eps"]))
    assert np.array_equal(elo, g["ebox_lo"]) and np.array_equal(ehi, g["ebox_hi"])
    pairs = np.array(sorted((L, int(i)) for L, m in enumerate(members) for i in m),
                     np.int64).reshape(-1, 2)
    assert np.array_equal(pairs, g["halo"])


@pytest.mark.parametrize("name", NAMES)
def test_partition_dbscan_matches_reference(name):
    """dbscan_partition (R:dbscan/dbscan.py:12-34) per neighbourhood: local
    labels and core flags, record for record."""
    g = load_golden(name)
    X, eps, ms = g["X"], float(g["eps"]), int(g["min_samples"])
    po = g["part_out"]
    for L in range(int(g["P"])):
        rows = po[po[:, 0] == L]
        keys = rows[:, 1]
        lab, core, _, _ = oracle.dbscan(X[keys], eps, ms, _metric(g))
        assert np.array_equal(lab, rows[:, 2]), L
        assert np.array_equal(core, rows[:, 3].astype(np.uint8)), L


@pytest.mark.parametrize("name", NAMES)
def test_pipeline_equals_global_dbscan(name):
    """Owner-rule merge of the per-neighbourhood results == global sklearn."""
    g = load_golden(name)
    out = oracle.pipeline(g["X"], float(g["eps"]), int(g["min_samples"]), _P(g), _metric(g))
    assert np.array_equal(out["core"], g["sk_core"])
    assert np.array_equal(out["labels"], g["sk_labels"])


# Datasets whose reference split decisions are decided by round-off:
#  - C0 is StandardScaler output: both axes have variance 1 in exact
#    arithmetic, the sequential fold's last bits pick the axis;
#  - ident_40 is 40 copies of one point: variance 0 in exact arithmetic, the
#    fold leaves +4.4e-16 and moves the boundary below the points.
TIES = {"c0": "equal variances", "c0_callable": "equal variances",
        "c0_p3": "equal variances", "c0_p5_cityblock": "equal variances",
        "ident_40": "zero variance"}


@pytest.mark.parametrize("name", NAMES)
def test_exact_sums_agree_with_reference_except_ties(name):
    g = load_golden(name)
    ex = oracle.kd_partition(g["X"], _P(g), sums="exact")
    sp = np.array([s[:6] for s in ex["splits"]], np.int64).reshape(-1, 6)
    if name in TIES:
        # the tie is real: within the sequential fold's error bound
        mom = oracle.min_var_moments(g["X"], "exact")
        var = mom[2] / mom[0] - (mom[1] / mom[0]) ** 2
        bound = 64 * len(g["X"]) * np.finfo(float).eps * max(1.0, float(np.max(np.abs(mom[2] / mom[0]))))
        if TIES[name] == "equal variances":
            assert abs(var[0] - var[1]) <= bound
        else:
            assert np.all(np.abs(var) <= bound)
        return
    assert np.array_equal(sp, g["splits"])
    assert np.array_equal(ex["owner"], g["owner"])
    np.testing.assert_allclose(ex["box_lo"], g["box_lo"], rtol=1e-12)
    np.testing.assert_allclose(ex["box_hi"], g["box_hi"], rtol=1e-12, atol=1e-300)


# ---------------------------------------------------------------------------
# Link-stage topologies (tests/topologies.py): the preconditions that
# tests/test_gpu_link_topology.py relies on, checked with the oracle alone.
# ---------------------------------------------------------------------------
import topologies as topo  # noqa: E402

DTYPES = ["float32", "float64"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,m", [(3, 30), (4, 13)])
def test_super_eps_lattice_preconditions(d, m, dtype):
    """Every point a cluster of its own, and enough neighbouring cell pairs
    that the cell verify must overflow its 1024-pair block buffer and the
    pair list (min(records, 64 Mi) entries)."""
    X, _ = topo.points("super_eps_lattice", (d, m), dtype)
    lab, core, cnt, nc = topo.reference("super_eps_lattice", (d, m), 1, dtype)
    n = m ** d
    assert X.shape == (n, d) and X.dtype == np.dtype(dtype) and X.flags.c_contiguous
    assert nc == n and cnt.max() == 1 and core.all()
    assert np.array_equal(lab, np.arange(n))
    cells = len(topo.occupied_cells(X)[0])
    pairs = topo.neighbour_cell_pairs(X)
    assert cells == n          # one record per cell: every cell its own root
    assert pairs == {3: 319_492, 4: 922_800}[d]
    F = topo.forward_cells(d)
    assert F == {3: 22, 4: 67}[d]
    # some block of 256 cells defers more than its buffer holds (pigeonhole)
    assert pairs > 1024 * -(-cells // 256)
    # a block stages min(l, 1024) >= l * 1024 / (256 F) of its l pairs: the
    # staged pairs exceed the list's capacity
    assert pairs * 1024 // (256 * F) > min(n, 64 << 20)


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_cell_clumps_preconditions(dtype):
    """Both clumps of a pair share one grid cell, are separate clusters, and
    the mixed cells cover every size tier of the cell-root kernels."""
    X, pair = topo.points("same_cell_clumps", (), dtype)
    lab, core, cnt, nc = topo.reference("same_cell_clumps", (), 5, dtype)
    assert len(X) == 14_429 and X.dtype == np.dtype(dtype) and X.flags.c_contiguous
    assert np.array_equal(X[0], [0, 0]) and (X >= 0).all()      # the anchor is the grid origin
    assert nc == 56 and int((lab < 0).sum()) == 9
    cc = topo.cell_coords(X)
    tiers = set()
    for k, (na, nb) in enumerate(topo.CLUMP_SIZES):
        m = pair == k
        assert int(m.sum()) == na + nb
        assert (cc[m] == np.array(topo.clump_cell(k))).all(), k     # one cell
        assert int((cc == np.array(topo.clump_cell(k))).all(axis=1).sum()) == na + nb
        pa, pb = X[m][:na].astype(np.float64), X[m][na:].astype(np.float64)
        gap = np.sqrt(((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1)).min()
        assert gap >= 1.011 * topo.EPS
        if min(na, nb) >= 5:
            la, lb = np.unique(lab[m][:na]), np.unique(lab[m][na:])
            assert len(la) == 1 and len(lb) == 1 and la[0] != lb[0] and la[0] >= 0 and lb[0] >= 0
            assert core[m].all()
            tiers.add("small" if na + nb <= 16 else "mid" if na + nb <= 1024 else "big")
            if (na, nb) == (5, 5):
                assert na + nb <= 16
            elif (na, nb) == (20, 20):
                assert 16 < na + nb <= 1024
            else:
                assert na + nb > 1024
    assert tiers == {"small", "mid", "big"}


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_cell_clumps_bridged_preconditions(dtype):
    """The chains join the two components of every bridged pair — one cluster
    less per bridged pair — through records that lie outside the shared cell."""
    kw = (("bridged", True),)
    X, pair = topo.points("same_cell_clumps", (), dtype)
    Xb, pairb = topo.points("same_cell_clumps", (), dtype, None, kw)
    bridged = topo.bridged_pairs()
    assert len(bridged) == 14 and len(Xb) == len(X) + 5 * len(bridged)
    assert np.array_equal(Xb[:len(X)], X)
    nc = topo.reference("same_cell_clumps", (), 3, dtype)[3]
    lab_b, core_b, _, nc_b = topo.reference("same_cell_clumps", (), 3, dtype, None, kw)
    assert nc == 56 and nc_b == nc - len(bridged)
    assert core_b[len(X):].all()
    cc = topo.cell_coords(Xb)
    clump_cells = {topo.clump_cell(k) for k in range(len(topo.CLUMP_SIZES))}
    assert not any(tuple(c) in clump_cells for c in cc[len(X):])
    for k in range(len(topo.CLUMP_SIZES)):
        if min(topo.CLUMP_SIZES[k]) >= 3:
            assert len(np.unique(lab_b[pairb == k])) == (1 if k in bridged else 2), k
    chain = Xb[len(X):].astype(np.float64).reshape(len(bridged), 5, 2)
    step = np.sqrt((np.diff(chain, axis=1) ** 2).sum(-1)) / topo.EPS
    assert np.abs(step - 0.8).max() < 1e-4


@pytest.mark.parametrize("dtype", DTYPES)
def test_snake_preconditions(dtype):
    """One cluster in which every point has only its predecessor and its
    successor: every edge a bridge (deleting one point gives two clusters)."""
    args = (120, 300)
    X, _ = topo.points("snake", args, dtype)
    n = len(X)
    assert n == 36_119 and X.dtype == np.dtype(dtype) and X.flags.c_contiguous
    for ms in (2, 3):
        lab, core, cnt, nc = topo.reference("snake", args, ms, dtype)
        assert nc == 1 and (lab == 0).all()
        assert set(np.unique(cnt)) == {2, 3}
        assert np.array_equal(np.nonzero(core == 0)[0], [0, n - 1] if ms == 3 else [])
        assert topo.reference("snake", args, ms, dtype, None, (("cut", True),))[3] == 2
        assert topo.reference("snake", args, ms, dtype, 7)[3] == 1      # permuted order
    assert len(topo.points("snake", args, dtype, None, (("cut", True),))[0]) == n - 1
    assert topo.reference("snake", (60, 150), 3, dtype)[3] == 1


@pytest.mark.parametrize("d,rows,cols", [(3, 120, 300), (4, 120, 300), (8, 40, 200)])
def test_snake_nd_preconditions(d, rows, cols):
    args = (d, rows, cols)
    X, _ = topo.points("snake_nd", args)
    assert X.shape == (rows * cols + rows - 1, d) and X.flags.c_contiguous
    step = np.linalg.norm(np.diff(X.astype(np.float64), axis=0), axis=1) / topo.EPS
    assert 0.7499 < step.min() and step.max() < 0.9001
    for ms in (2, 3):
        lab, core, cnt, nc = topo.reference("snake_nd", args, ms)
        assert nc == 1 and set(np.unique(cnt)) == {2, 3}
        assert topo.reference("snake_nd", args, ms, "float32", None, (("cut", True),))[3] == 2


@pytest.mark.parametrize("ms", [1, 2, 3])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_percolation_regime(d, ms):
    """The tortuous regime: more than 1000 clusters, the largest holding
    between 2 % and 80 % of the points."""
    n = 30_000 if d == 4 else 60_000
    X, _ = topo.points("percolation", (d, n))
    assert X.shape == (n, d) and X.flags.c_contiguous
    lab, _, _, nc = topo.reference("percolation", (d, n), ms)
    largest = int(np.bincount(lab[lab >= 0]).max())
    assert nc > 1000
    assert 0.02 * n <= largest <= 0.80 * n


@pytest.mark.parametrize("dtype", DTYPES)
def test_comb_preconditions(dtype):
    """Every midpoint is a labelled border point with 17 neighbours that lies
    within eps of core points of exactly two clusters."""
    X, mid = topo.points("comb", (), dtype)
    lab, core, cnt, nc = topo.reference("comb", (), 20, dtype)
    assert len(X) == 24_936 and int(mid.sum()) == 936 and X.flags.c_contiguous
    assert nc == 40
    assert not core[mid].any() and (cnt[mid] == 17).all() and (lab[mid] >= 0).all()
    off, nbr = oracle.neighbors(X, topo.EPS)
    for i in np.nonzero(mid)[0]:
        js = nbr[off[i]:off[i + 1]]
        adj = np.unique(lab[js[core[js] == 1]])
        assert len(adj) == 2 and lab[i] == adj.min(), i
    # a permuted order keeps the adjacency but not "the lower line wins"
    labp = topo.reference("comb", (), 20, dtype, 11)[0]
    _, midp = topo.points("comb", (), dtype, 11)
    assert topo.reference("comb", (), 20, dtype, 11)[3] == 40 and (labp[midp] >= 0).all()
