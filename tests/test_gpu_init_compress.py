"""The initial forest compressed per record tile (link step 1, init_kernel): a
block stages the parents of its TILE consecutive records in LDS and jumps
pointers there until every record points at its first ancestor outside the
tile, or at its chain's root inside it.  The forest only saves the later steps
work, so a lost hop costs time; a wrong one (a non-core parent, a parent above
its child or in another tree, a changed root, a lane that misses a barrier at
the end of the records) changes labels.  The record counts sit around the
multiples of the tile, the chains are as long as the tile allows, and every
case compares labels, core flags and n_clusters with the oracle bit for bit
(tests/topologies.py)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import topologies as topo
from weighted_ref import weighted_dbscan

pytestmark = pytest.mark.gpu

EPS = topo.EPS
SHIPPED_TILE = 4096                               # kInitSub * kBlock (engine.hip)
TILES = tuple(sorted({1024, SHIPPED_TILE}))


def _edge_sizes(T):
    return (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 4 * T + 1)


def _dev(X):
    return torch.from_numpy(np.array(X, order="C")).cuda()   # (a copy: the shared cases are read-only)


@pytest.fixture(scope="module")
def native():
    from pypardis_amd import _native
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _native.load()
    return _native


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


def _assert_cluster(native, X, ref, ms, what):
    """pd_cluster (no halo: records = points)."""
    lab_o, core_o, _, nc_o = ref
    lab, core, _, ncl = native.cluster(_dev(X), EPS, ms, native.metric_code("euclidean"))
    assert np.array_equal(core.cpu().numpy().astype(bool), core_o), what
    assert np.array_equal(lab.cpu().numpy().astype(np.int64), lab_o), what
    assert ncl == nc_o, what


def _assert_train(X, ref, ms, P, what):
    from pypardis_amd import DBSCAN
    lab_o, core_o, _, nc_o = ref
    m = DBSCAN(eps=EPS, min_samples=ms, max_partitions=P).train(_dev(X))
    assert np.array_equal(m.core_sample_mask_.cpu().numpy(), core_o), what
    assert np.array_equal(m.labels_.cpu().numpy().astype(np.int64), lab_o), what
    assert m.n_clusters_ == nc_o, what


@functools.lru_cache(maxsize=None)
def _reference(key, ms):
    """The oracle's result for a point set of this module (built once)."""
    import oracle
    lab, core, cnt, nc = oracle.dbscan(_points(key), EPS, ms)
    for a in (lab, core, cnt):
        a.setflags(write=False)
    return lab, core, cnt, nc


# ------------------------------------------------ the point sets of this module
def _line(n, gap_after=None, d=2, dtype="float32"):
    """n points 0.6 eps apart along axis 0 (one per eps/2 sub-cell, so record
    order = order along the line whatever the input order).  With
    min_samples = 3 every inner point is core with the record before as its
    only smaller neighbour: one chain through every tile.  gap_after = g: the
    spacing between points g and g + 1 is 1.5 eps, so both are non-core and
    the line is two clusters."""
    step = np.full(n, 0.6)
    step[0] = 0.0
    if gap_after is not None:
        step[gap_after + 1] = 1.5
    X = np.zeros((n, d))
    X[:, 0] = np.cumsum(step) * EPS
    return np.ascontiguousarray(X.astype(dtype))


def _empty_tile(T):
    """A chain of T / 2 + 3 points, then 2 T + 9 points 3 eps apart (noise:
    at least one whole tile without a core record), then a chain of T + 5."""
    steps = np.r_[0.0, np.full(T // 2 + 2, 0.6), np.full(2 * T + 9, 3.0), 3.0, np.full(T + 4, 0.6)]
    X = np.zeros((len(steps), 2))
    X[:, 0] = np.cumsum(steps) * EPS
    return np.ascontiguousarray(X.astype(np.float32))


def _clumps(T):
    """T + 3 clumps of three points (within 0.02 eps) 3 eps apart on a line:
    at min_samples = 3 every clump is a root and two records that point at
    it, at min_samples = 4 nothing is core."""
    k = T + 3
    X = np.zeros((k, 3, 2))
    X[:, :, 0] = (3.0 * np.arange(k)[:, None] + np.array([0.0, 0.01, 0.02])) * EPS
    X[:, :, 1] = np.array([0.0, 0.01, 0.0]) * EPS
    return np.ascontiguousarray(X.reshape(-1, 2).astype(np.float32))


def _interleaved_rows(T):
    """Two rows 0.95 eps apart in one row of cells, points 0.9 eps apart, the
    second row shifted by 0.45 eps: no point of one row is within eps of the
    other (1.05 eps), and in key order the records of the two rows
    interleave (one or two of a row at a time).  Two chains whose parents lie
    two or three records back: both cross every tile edge side by side."""
    m = (3 * T + 5) // 2
    a = np.stack([0.9 * np.arange(m), np.zeros(m)], -1)
    b = np.stack([0.9 * np.arange(m) + 0.45, np.full(m, 0.95)], -1)
    return np.ascontiguousarray((np.concatenate([a, b]) * EPS).astype(np.float32))


def _stacked_rows(T):
    """Two rows of T + 9 points 0.6 eps apart, 0.06 cells apart on either side
    of a cell-row boundary (an anchor at the origin pins the grid).  At
    min_samples = 4 the count sweep has to leave a point's own row, so the
    second row's parents lie in the first, more than a tile back: every
    chain of its tiles leaves the tile at once."""
    m = T + 9
    cw = topo.cell_width() / EPS
    x = 1.0 + 0.6 * np.arange(m)
    a = np.stack([x, np.full(m, 0.97 * cw)], -1)
    b = np.stack([x, np.full(m, 1.03 * cw)], -1)
    return np.ascontiguousarray((np.concatenate([np.zeros((1, 2)), a, b]) * EPS).astype(np.float32))


_MAKERS = {"line": _line, "empty_tile": _empty_tile, "clumps": _clumps,
           "interleaved": _interleaved_rows, "stacked": _stacked_rows}


@functools.lru_cache(maxsize=None)
def _points(key):
    X = _MAKERS[key[0]](*key[1:])
    X.setflags(write=False)
    return X


# ------------------------------------------------ 1. tile edges
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_tile_edges(native, d, dtype):
    """Record counts T - 1, T, T + 1, 2 T - 1, 2 T + 1 and 4 T + 1: the last
    block's partial tile (lanes past R still vote), a tile of one record, and
    under max_partitions = 2 and 8 the halo duplicates that shift every
    edge."""
    for T in TILES:
        for n in _edge_sizes(T):
            X, _ = topo.points("percolation", (d, n), dtype)
            ref = topo.reference("percolation", (d, n), 3, dtype)
            _assert_cluster(native, X, ref, 3, (T, n, "cluster"))
            _assert_train(X, ref, 3, 2, (T, n, "P2"))
            _assert_train(X, ref, 3, 8, (T, n, "P8"))


def test_edge_cases_hold_chains_and_roots():
    """The generator at the smallest edge size (CPU): core and non-core
    records and several clusters, so chains, roots and kNone slots all occur
    in one tile."""
    lab, core, _, nc = topo.reference("percolation", (3, 1023), 3)
    assert nc == 43 and int(core.sum()) == 767 and int((lab < 0).sum()) == 143


# ------------------------------------------------ 2. the longest chain in a tile
@pytest.mark.parametrize("T", TILES)
@pytest.mark.parametrize("d,dtype", [(1, "float32"), (2, "float32"), (2, "float64")])
def test_line_one_chain_through_every_tile(native, T, d, dtype):
    """5 T + 7 points on a line at min_samples = 3: every parent is the record
    before, so a tile holds one chain of T records (log2(T) jumping rounds)
    and hands it to the tile before."""
    key = ("line", 5 * T + 7, None, d, dtype)
    ref = _reference(key, 3)
    assert ref[3] == 1 and int(ref[1].sum()) == 5 * T + 5
    _assert_cluster(native, _points(key), ref, 3, "cluster")
    _assert_train(_points(key), ref, 3, 8, "P8")


@pytest.mark.parametrize("T", TILES)
@pytest.mark.parametrize("where", [-2, -1, 0])
def test_line_gap_at_a_tile_edge(native, T, where):
    """The same line with two non-core records just before, on and just
    after the edge between the second and third tile: the chain ends there
    and a new root starts, two clusters."""
    key = ("line", 5 * T + 7, 2 * T + where, 2, "float32")
    ref = _reference(key, 3)
    assert ref[3] == 2 and not ref[1][2 * T + where] and not ref[1][2 * T + where + 1]
    _assert_cluster(native, _points(key), ref, 3, "cluster")
    _assert_train(_points(key), ref, 3, 2, "P2")


# ------------------------------------------------ 3. particular tiles
@pytest.mark.parametrize("T", TILES)
def test_tile_without_a_core_record(native, T):
    key = ("empty_tile", T)
    ref = _reference(key, 3)
    assert ref[3] == 2 and not ref[1][T // 2 + 3:T // 2 + 3 + 2 * T + 9].any()
    _assert_cluster(native, _points(key), ref, 3, "cluster")
    _assert_train(_points(key), ref, 3, 8, "P8")


@pytest.mark.parametrize("T", TILES)
def test_tiles_of_roots(native, T):
    """Every record a root (a lattice of lone points at min_samples = 1, as
    many clusters as points), then clumps of a root and two records that
    already point at it (nothing moves), then the clumps with nothing core."""
    m = int(np.ceil(np.sqrt(2 * T + 1)))
    X, _ = topo.points("super_eps_lattice", (2, m))
    ref = topo.reference("super_eps_lattice", (2, m), 1)
    assert ref[3] == len(X) >= 2 * T + 1
    _assert_cluster(native, X, ref, 1, "lattice")
    key = ("clumps", T)
    for ms, nc in ((3, T + 3), (4, 0)):
        ref = _reference(key, ms)
        assert ref[3] == nc
        _assert_cluster(native, _points(key), ref, ms, ("clumps", ms))
        _assert_train(_points(key), ref, ms, 8, ("clumps P8", ms))


@pytest.mark.parametrize("T", TILES)
def test_chains_that_leave_their_tile(native, T):
    """Two interleaved rows (two chains cross every tile edge side by side)
    and two stacked rows (the second row's parents lie more than a tile
    back)."""
    key = ("interleaved", T)
    ref = _reference(key, 3)
    assert ref[3] == 2
    _assert_cluster(native, _points(key), ref, 3, "interleaved")
    _assert_train(_points(key), ref, 3, 2, "interleaved P2")
    key = ("stacked", T)
    ref = _reference(key, 4)
    assert ref[3] == 1 and int(ref[1].sum()) == 2 * (T + 9)
    _assert_cluster(native, _points(key), ref, 4, "stacked")
    _assert_train(_points(key), ref, 4, 8, "stacked P8")


# ------------------------------------------------ 4. the link topologies, every window class
TOPOLOGIES = [("snake", (120, 300), 3, ()), ("super_eps_lattice", (3, 30), 1, ()),
              ("same_cell_clumps", (), 5, ()), ("same_cell_clumps", (), 3, (("bridged", True),)),
              ("comb", (), 20, ())]


@pytest.mark.parametrize("window", [2, 8, 64])
@pytest.mark.parametrize("name,args,ms,kw", TOPOLOGIES)
def test_link_topologies(native, name, args, ms, kw, window):
    """Bridge-only, many-root, two-components-in-a-cell and contested-border
    point sets: the window union and the cell roots walk the compressed
    forest at each window length."""
    X, _ = topo.points(name, args, "float32", None, kw)
    ref = topo.reference(name, args, ms, "float32", None, kw)
    with _options(native, (native.PD_OPT_CENTRE_WINDOW, window, -1)):
        _assert_cluster(native, X, ref, ms, "cluster")
        _assert_train(X, ref, ms, 8, "P8")


# ------------------------------------------------ 5. the other builds of the link stage
def test_weighted(native):
    """sample_weight launches the same init_kernel on weighted core flags:
    integer weights 0..3 on 2 * 1024 + 1 points against the brute-force
    weighted reference, and unit weights at 2 T + 1 against the oracle."""
    n = 2 * 1024 + 1
    X, _ = topo.points("percolation", (2, n))
    w = np.random.default_rng(11).integers(0, 4, n).astype(np.float64)
    lab_r, core_r = weighted_dbscan(X, EPS, 4, w)
    assert 200 < int(core_r.sum()) < n - 200
    lab, core, _, _ = native.cluster(_dev(X), EPS, 4, sample_weight=_dev(w))
    assert np.array_equal(core.cpu().numpy().astype(bool), core_r)
    assert np.array_equal(lab.cpu().numpy().astype(np.int64), lab_r)
    n = 2 * SHIPPED_TILE + 1
    X, _ = topo.points("percolation", (3, n))
    lab_o, core_o, _, nc_o = topo.reference("percolation", (3, n), 3)
    lab, core, _, ncl = native.cluster(_dev(X), EPS, 3, sample_weight=_dev(np.ones(n)))
    assert np.array_equal(core.cpu().numpy().astype(bool), core_o)
    assert np.array_equal(lab.cpu().numpy().astype(np.int64), lab_o)
    assert ncl == nc_o


def test_sweep_stats_build(native):
    """PD_OPT_SWEEP_STATS selects the tallying instantiations of the count
    sweep and the window union around the same init_kernel."""
    T = SHIPPED_TILE
    key = ("line", 5 * T + 7, 2 * T - 1, 2, "float32")
    with _options(native, (native.PD_OPT_SWEEP_STATS, 1, 0)):
        _assert_cluster(native, _points(key), _reference(key, 3), 3, "line")
        n = 4 * T + 1
        X, _ = topo.points("percolation", (3, n))
        _assert_cluster(native, X, topo.reference("percolation", (3, n), 3), 3, "percolation")
