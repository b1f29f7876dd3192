"""The window union with several 64-record groups per wave (link step 2,
window_uf_kernel): a wave covers 64 K records plus the W look-ahead ones, K a
function of the row size and the window (1..8), so the record counts here sit
around every multiple of 64 K and around 64 K + W, at the windows of the three
LDS classes (2, 8, 64).  The window union only saves the cell verify work, so
a lost union costs time; a wrong one (a non-core record, a pair farther apart
than eps, a parent above its child) changes labels.  Every case compares
labels, core flags and counts with the oracle bit for bit
(tests/topologies.py)."""
import contextlib

import numpy as np
import pytest
import torch

import topologies as topo

pytestmark = pytest.mark.gpu

EPS = topo.EPS
SIZES = (1, 2, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257, 258, 264, 320, 511, 512, 513,
         514, 520, 576, 1023, 1024, 1025, 1088)
SIZES64 = (65, 258, 513, 1025)
WINDOWS = (2, 8, 64)


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


def _window(native, window):
    return _options(native, (native.PD_OPT_CENTRE_WINDOW, window, -1),
                    (native.PD_OPT_FULL_COUNTS, 1, 0))


def _assert_cluster(native, X, ref, ms, what):
    """pd_cluster (no halo: records = points) with full counts."""
    lab_o, core_o, cnt_o, nc_o = ref
    lab, core, cnt, ncl = native.cluster(_dev(X), EPS, ms, native.metric_code("euclidean"),
                                         want_counts=True)
    assert np.array_equal(cnt.cpu().numpy().astype(np.int64), cnt_o), what
    assert np.array_equal(core.cpu().numpy(), core_o), what
    assert np.array_equal(lab.cpu().numpy().astype(np.int64), lab_o), what
    assert ncl == nc_o, what


def _assert_train(X, ref, ms, P, what):
    from pypardis_amd import DBSCAN
    lab_o, core_o, _, nc_o = ref
    m = DBSCAN(eps=EPS, min_samples=ms, max_partitions=P).train(_dev(X))
    assert np.array_equal(m.core_sample_mask_.cpu().numpy(), core_o), what
    assert np.array_equal(m.labels_.cpu().numpy().astype(np.int64), lab_o), what
    assert m.n_clusters_ == nc_o, what


# ------------------------------------------------ 1. group and tail boundaries
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("d", [2, 3])
def test_group_and_tail_boundaries(native, d, window, dtype):
    """Record counts around every multiple of 64 K (K <= 8) and around
    64 K + W: the last wave's partial groups, a look-ahead that ends at R,
    and the grid's last block."""
    with _window(native, window):
        for n in (SIZES if dtype == "float32" else SIZES64):
            X, _ = topo.points("percolation", (d, n), dtype)
            for ms in (1, 3):
                ref = topo.reference("percolation", (d, n), ms, dtype)
                _assert_cluster(native, X, ref, ms, (n, ms))


def test_boundary_cases_hold_every_kind_of_neighbour():
    """The generator at these sizes (CPU): 3-D n = 1025 with min_samples 3
    has several clusters, non-core and noise records, so neighbouring records
    of different clusters and non-core records between core ones occur."""
    lab, core, _, nc = topo.reference("percolation", (3, 1025), 3)
    assert nc == 41 and int(core.sum()) == 770 and int((lab < 0).sum()) == 143


# ------------------------------------------------ 2. many groups, records != points
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("d", [2, 3])
def test_many_groups_and_halo_records(native, d, window):
    """Hundreds of waves; under max_partitions = 8 the halo records make
    R != n and partition starts fall inside groups."""
    X, _ = topo.points("percolation", (d, 20000))
    ref = topo.reference("percolation", (d, 20000), 3)
    with _window(native, window):
        _assert_cluster(native, X, ref, 3, "cluster")
        _assert_train(X, ref, 3, 8, "P8")


# ------------------------------------------------ 3. mixed cells, contested borders
@pytest.mark.parametrize("window", [8, 64])
@pytest.mark.parametrize("bridged", [False, True])
def test_same_cell_clumps_long_windows(native, bridged, window):
    """Two components in one grid cell, now inside one wave's span of up to
    576 records: they stay two clusters, or become one through the bridge."""
    kw = (("bridged", True),) if bridged else ()
    ms = 3 if bridged else 5
    X, _ = topo.points("same_cell_clumps", (), "float32", None, kw)
    ref = topo.reference("same_cell_clumps", (), ms, "float32", None, kw)
    assert ref[3] == (42 if bridged else 56)
    with _window(native, window):
        _assert_train(X, ref, ms, 4, "P4")
        _assert_train(X, ref, ms, 8, "P8")


@pytest.mark.parametrize("window", [8, 64])
def test_comb_long_windows(native, window):
    """No union through a non-core midpoint: the lines stay 40 clusters and
    each midpoint takes the smaller label."""
    X, mid = topo.points("comb", ())
    ref = topo.reference("comb", (), 20)
    assert ref[3] == 40 and not ref[1][mid].any()
    with _window(native, window):
        _assert_train(X, ref, 20, 4, "P4")
        _assert_train(X, ref, 20, 8, "P8")


# ------------------------------------------------ 4. the instrumented instantiation
def test_sweep_stats_instantiation(native):
    """PD_OPT_SWEEP_STATS selects the tallying instantiation: same labels,
    and its counters nest (a union needs a hit, a hit a candidate)."""
    X, _ = topo.points("percolation", (3, 20000))
    ref = topo.reference("percolation", (3, 20000), 3)
    with _window(native, 2), _options(native, (native.PD_OPT_SWEEP_STATS, 1, 0)) as ctx:
        _assert_cluster(native, X, ref, 3, "stats")
        t = ctx.timings()
        cand, hit, unions = (int(t[k]) for k in ("s_link_cand", "s_link_hit", "s_link_unions"))
        print(f"\ns_link_cand={cand} s_link_hit={hit} s_link_unions={unions}")
        assert hit > 0
        assert unions <= hit <= cand
