"""Link stage on point sets where every edge matters (tests/topologies.py):
the HIP path against the oracle on bridge-only clusters, many-root grids,
cells that hold two components and border points with a choice of cluster.
Labels, core flags and neighbour counts are compared bit for bit; the
generators' preconditions are pinned on the CPU in tests/test_oracle.py.

What notices what (checked once against builds of engine.hip that drop link
work): without pair_kernel the snakes, the bridged clumps at window 2 and
every 2-D..4-D percolation case fail; without the in-place resolution of the
cell verify's overflowing pairs the partitioned snake trains and percolation
fail (a partitioned snake defers ~43 000 - 59 000 cell pairs, more than its
records, so the pair list overflows with unions still to make; the lattice
only proves those branches run and unite nothing they should not); with
mixed cells treated as uniform in pair_block, or without a mixed cell's own
pair, percolation (and the 4-D snake) fail."""
import contextlib

import numpy as np
import pytest
import torch

import topologies as topo

pytestmark = pytest.mark.gpu

EPS = topo.EPS


def _dev(X):
    return torch.from_numpy(np.array(X, order="C")).cuda()   # (a copy: the shared cases are read-only)


@pytest.fixture(scope="module")
def native():
    from pypardis_amd import _native
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _native.load()
    return _native


def _cluster(native, X, eps, ms, metric="euclidean"):
    """pd_cluster with full counts: (labels, core, n_clusters, counts)."""
    ctx = native.context()
    ctx.set_option(native.PD_OPT_FULL_COUNTS, 1)
    try:
        lab, core, cnt, ncl = native.cluster(_dev(X), eps, ms, native.metric_code(metric),
                                             want_counts=True)
    finally:
        ctx.set_option(native.PD_OPT_FULL_COUNTS, 0)
    return (lab.cpu().numpy().astype(np.int64), core.cpu().numpy(), ncl,
            cnt.cpu().numpy().astype(np.int64))


def _train(X, eps, ms, P, metric="euclidean"):
    from pypardis_amd import DBSCAN
    m = DBSCAN(eps=eps, min_samples=ms, metric=metric, max_partitions=P).train(_dev(X))
    return (m.labels_.cpu().numpy().astype(np.int64), m.core_sample_mask_.cpu().numpy(),
            m.n_clusters_)


@contextlib.contextmanager
def _options(native, *opts):
    """opts: (option, value, default) — set for the block, restored after it."""
    ctx = native.context()
    try:
        for opt, val, _ in opts:
            ctx.set_option(opt, val)
        yield ctx
    finally:
        for opt, _, default in opts:
            ctx.set_option(opt, default)


def _assert_cluster(native, X, ref, eps, ms, metric="euclidean"):
    lab_o, core_o, cnt_o, nc_o = ref
    lab, core, ncl, cnt = _cluster(native, X, eps, ms, metric)
    assert np.array_equal(cnt, cnt_o)
    assert np.array_equal(core, core_o)
    assert np.array_equal(lab, lab_o)
    assert ncl == nc_o


def _assert_train(X, ref, eps, ms, P, metric="euclidean"):
    lab_o, core_o, _, nc_o = ref
    lab, core, ncl = _train(X, eps, ms, P, metric)
    assert np.array_equal(core, core_o), P
    assert np.array_equal(lab, lab_o), P
    assert ncl == nc_o, P


# ------------------------------------------------------------ 1. n clusters = n
LATTICE = [(3, 30, 0, 0, "float32"), (3, 30, 0, 1, "float32"), (3, 30, 1, 0, "float32"),
           (3, 30, 1, 1, "float32"), (4, 13, 0, 0, "float32"), (4, 13, 0, 1, "float32"),
           (4, 13, 1, 0, "float32"), (4, 13, 1, 1, "float32"), (3, 30, 0, 0, "float64"),
           (4, 13, 0, 0, "float64")]


@pytest.mark.parametrize("d,m,stats,fused,dtype", LATTICE)
def test_super_eps_lattice_every_point_alone(native, d, m, stats, fused, dtype):
    """min_samples = 1 on a lattice of spacing 1.03 eps: n clusters numbered in
    input order, every cell its own root.  The cell verify defers a pair for
    every neighbouring cell pair: under PD_OPT_SWEEP_STATS the device's own
    counters prove that a block deferred more than its 1024-pair LDS buffer
    (resolved in place by pair_block) and that the staged pairs exceeded the
    pair list (lbase + k >= pcap, also resolved in place)."""
    X, _ = topo.points("super_eps_lattice", (d, m), dtype)
    n = len(X)
    ref = topo.reference("super_eps_lattice", (d, m), 1, dtype)
    assert ref[3] == n
    with _options(native, (native.PD_OPT_SWEEP_STATS, stats, 0),
                  (native.PD_OPT_VERIFY_FUSED, fused, 0)) as ctx:
        lab, core, ncl, cnt = _cluster(native, X, EPS, 1)
        t = ctx.timings()
        assert ncl == n
        # spacing 1.03 eps exceeds every cell width: no two points share a cell
        assert int(t["cells_n"]) == n
        assert np.array_equal(cnt, ref[2]) and np.array_equal(core, ref[1])
        assert np.array_equal(lab, np.arange(n)) and np.array_equal(lab, ref[0])
        if stats:
            pairs, cells, R = int(t["s_verify_pairs"]), int(t["cells_n"]), int(t["records"])
            F = topo.forward_cells(d)
            print(f"\nsuper_eps_lattice d={d} fused={fused}: s_verify_pairs={pairs} "
                  f"cells_n={cells} records={R} cpu_pairs={topo.neighbour_cell_pairs(X)}")
            assert pairs > 1024 * -(-cells // 256)
            assert pairs * 1024 // (256 * F) > min(R, 64 << 20)
        Xp, _ = topo.points("super_eps_lattice", (d, m), dtype, 3)
        _assert_cluster(native, Xp, topo.reference("super_eps_lattice", (d, m), 1, dtype, 3),
                        EPS, 1)
        _assert_train(X, ref, EPS, 1, 8)


# ------------------------------------------------------------ 2. mixed cells
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("window", [-1, 2, 64])
@pytest.mark.parametrize("bridged", [False, True])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_same_cell_clumps(native, dtype, bridged, window, fused):
    """Two components in one grid cell (kMixed), in cells of <= 16, <= 1024
    and > 1024 records: they stay two clusters — or, bridged, become one
    through records of other cells only — whatever the window union's length
    and the form of the cell verify."""
    kw = (("bridged", True),) if bridged else ()
    ms = 3 if bridged else 5
    X, _ = topo.points("same_cell_clumps", (), dtype, None, kw)
    ref = topo.reference("same_cell_clumps", (), ms, dtype, None, kw)
    assert ref[3] == (42 if bridged else 56)
    with _options(native, (native.PD_OPT_CENTRE_WINDOW, window, -1),
                  (native.PD_OPT_VERIFY_FUSED, fused, 0)):
        _assert_cluster(native, X, ref, EPS, ms)
        _assert_train(X, ref, EPS, ms, 4)


# ------------------------------------------------------------ 3. one record wide
SNAKE = (120, 300)


@pytest.mark.parametrize("ms", [2, 3])
@pytest.mark.parametrize("setting", ["cluster", "P1", "P8", "P64", "permuted", "cut", "float64"])
def test_snake(native, setting, ms):
    """One cluster in which every edge is a bridge, crossing every KD
    partition boundary hundreds of times: one lost union or merge splits it."""
    dtype = "float64" if setting == "float64" else "float32"
    perm = 5 if setting == "permuted" else None
    kw = (("cut", True),) if setting == "cut" else ()
    X, _ = topo.points("snake", SNAKE, dtype, perm, kw)
    ref = topo.reference("snake", SNAKE, ms, dtype, perm, kw)
    assert ref[3] == (2 if setting == "cut" else 1)
    if setting[0] == "P":
        _assert_train(X, ref, EPS, ms, int(setting[1:]))
    else:
        _assert_cluster(native, X, ref, EPS, ms)
        if setting != "cluster":
            _assert_train(X, ref, EPS, ms, 8)


def test_snake_sharded(native, tmp_path):
    """Two ranks, eight partitions: the one cluster crosses every rank and
    partition boundary many times, so every halo export and merge pair counts."""
    from dist_worker import run_world
    X, _ = topo.points("snake", (60, 150))
    lab_o, core_o, _, nc_o = topo.reference("snake", (60, 150), 3)
    assert nc_o == 1
    out = run_world(2, np.array(X), EPS, 3, 0, 8, str(tmp_path), native=True)
    assert (out["seen"] == 1).all()
    assert out["exports"] > 0
    np.testing.assert_array_equal(out["labels"], lab_o)
    np.testing.assert_array_equal(out["core"], core_o)
    np.testing.assert_array_equal(out["loc_labels"], lab_o)
    np.testing.assert_array_equal(out["loc_core"], core_o)
    assert out["ncl"] == {1}


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("d", [3, 4])
def test_snake_nd_grid(native, d, cut):
    """The snake rotated into 3-D and 4-D: the grid path's wider forward
    neighbourhoods, no axis aligned with the chain."""
    kw = (("cut", True),) if cut else ()
    args = (d,) + SNAKE
    X, _ = topo.points("snake_nd", args, "float32", None, kw)
    ref = topo.reference("snake_nd", args, 3, "float32", None, kw)
    assert ref[3] == (2 if cut else 1)
    _assert_cluster(native, X, ref, EPS, 3)
    _assert_train(X, ref, EPS, 3, 8)


@pytest.mark.parametrize("screen", [1, 0])
@pytest.mark.parametrize("cut", [False, True])
def test_snake_nd_dense(native, cut, screen):
    """The snake in 8-D: the dense path's forest (pd_dense_link) on a cluster
    with no redundant edge, under both count screens."""
    kw = (("cut", True),) if cut else ()
    args = (8, 40, 200)
    X, _ = topo.points("snake_nd", args, "float32", None, kw)
    assert X.shape[1] == 8
    with _options(native, (native.PD_OPT_DENSE_SCREEN, screen, 1)):
        for ms in (2, 3):
            ref = topo.reference("snake_nd", args, ms, "float32", None, kw)
            assert ref[3] == (2 if cut else 1)
            _assert_cluster(native, X, ref, EPS, ms)
            _assert_train(X, ref, EPS, ms, 1)


# ------------------------------------------------------------ 4. percolation
PERC = [(d, ms, "euclidean") for d in (1, 2, 3, 4) for ms in (1, 2, 3)] + \
       [(2, ms, "cityblock") for ms in (1, 2, 3)]


@pytest.mark.parametrize("d,ms,metric", PERC)
def test_percolation(native, d, ms, metric):
    """Uniform points near the connectivity threshold (1-D: a density ramp,
    see topologies.percolation): thousands of tortuous clusters, most cells
    holding several roots."""
    n = 30_000 if d == 4 else 60_000
    X, _ = topo.points("percolation", (d, n))
    ref = topo.reference("percolation", (d, n), ms, "float32", None, (), metric)
    assert ref[3] > 1000
    _assert_cluster(native, X, ref, EPS, ms, metric)
    _assert_train(X, ref, EPS, ms, 8, metric)


# ------------------------------------------------------------ 5. contested borders
@pytest.mark.parametrize("setting", ["cluster", "cluster64", "P2", "P8", "P13", "permuted"])
def test_comb_border_takes_smaller_label(native, setting):
    """Every midpoint is a border point within eps of core points of two
    clusters and takes the smaller label (sklearn's first-discovered rule) —
    also when the partition boundaries run through the comb and when the
    input order decides which of the two lines has the smaller label."""
    dtype = "float64" if setting == "cluster64" else "float32"
    perm = 11 if setting == "permuted" else None
    X, mid = topo.points("comb", (), dtype, perm)
    ref = topo.reference("comb", (), 20, dtype, perm)
    assert ref[3] == 40 and (ref[0][mid] >= 0).all() and not ref[1][mid].any()
    if setting[0] == "P":
        _assert_train(X, ref, EPS, 20, int(setting[1:]))
    else:
        _assert_cluster(native, X, ref, EPS, 20)
        if perm is not None:
            _assert_train(X, ref, EPS, 20, 8)
