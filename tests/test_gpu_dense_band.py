"""The d > 4 path (csrc/dense.hip, and csrc/assign.hip's d > 4 tiles) on point
sets whose neighbour decisions sit at the edge of its low-precision
arithmetic (tests/dense_adversarial.py; their preconditions are pinned on the
CPU in tests/test_dense_adversarial_host.py).  Every comparison is with the
oracle (or predict_ref) and exact: full neighbour counts, core flags, labels
and the number of clusters by np.array_equal — no tolerance anywhere.

What notices what (checked once against builds of dense.hip with one constant
or term changed): with kBandC = 2^-16 the 16 mantissa="bf16" cases of
test_shell_pairs_aligned_rounding fail and nothing else does — on random
mantissas the split product is within 2^-17 of the norms, so no random set
can tell 2^-16 from 2^-13; with tile_kernel's fp64 recheck stubbed to false,
and with bi lacking its max_j |x_j|^2 term, every test that reaches the MFMA
tiles fails (all but d = 129, the k >= 49 outlier sets, which take the exact
VALU tile, and the row-size limit of pd_index_query)."""
import contextlib

import numpy as np
import pytest
import torch

import dense_adversarial as da
from predict_ref import brute_predict
from test_gpu_parity import _dense_stages

pytestmark = pytest.mark.gpu

SHELL_D = (5, 16, 17, 32, 33, 64, 65, 127, 128, 129)
SHELL_R = {"float32": (-2, -8, -14), "float64": (-2, -8, -14, -20)}
SHELL = [(d, dt, r) for dt in ("float32", "float64") for d in SHELL_D for r in SHELL_R[dt]]
TIE = [(d, off, dt) for d in (8, 17, 64, 65, 128)
       for off, dt in ((0, "float32"), (2 ** 20, "float32"), (2 ** 40, "float64"))]


def _dev(X):
    return torch.from_numpy(np.array(X, order="C")).cuda()   # (a copy: the shared cases are read-only)


def _np(t):
    return t.cpu().numpy().astype(np.int64)


@pytest.fixture(scope="module")
def native():
    from pypardis_amd import _native
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    _native.load()
    return _native


def _cluster(native, X, eps, ms):
    """pd_cluster with full counts: (labels, core, n_clusters, counts)."""
    ctx = native.context()
    ctx.set_option(native.PD_OPT_FULL_COUNTS, 1)
    try:
        lab, core, cnt, ncl = native.cluster(_dev(X), eps, ms, native.PD_EUCLIDEAN,
                                             want_counts=True)
    finally:
        ctx.set_option(native.PD_OPT_FULL_COUNTS, 0)
    return _np(lab), core.cpu().numpy(), ncl, _np(cnt)


def _train(X, eps, ms, P):
    from pypardis_amd import DBSCAN
    return DBSCAN(eps=eps, min_samples=ms, max_partitions=P).train(_dev(X))


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


def _screen(native, v):
    return (native.PD_OPT_DENSE_SCREEN, v, 1)


def _prune(native, v):
    return (native.PD_OPT_DENSE_PRUNE, v, 1)


def _assert_cluster(native, X, ref, eps, ms, tag=None):
    lab_o, core_o, cnt_o, nc_o = ref
    lab, core, ncl, cnt = _cluster(native, X, eps, ms)
    assert np.array_equal(cnt, cnt_o), tag
    assert np.array_equal(core, core_o), tag
    assert np.array_equal(lab, lab_o), tag
    assert ncl == nc_o, tag


def _assert_train(X, ref, eps, ms, P, tag=None):
    lab_o, core_o, _, nc_o = ref
    m = _train(X, eps, ms, P)
    assert np.array_equal(m.core_sample_mask_.cpu().numpy(), core_o), (tag, P)
    assert np.array_equal(_np(m.labels_), lab_o), (tag, P)
    assert m.n_clusters_ == nc_o, (tag, P)


# ------------------------------------------------------------ 1. the band
@pytest.mark.parametrize("d,dtype,r", SHELL)
def test_shell_pairs_band(native, d, dtype, r):
    """min_samples = 2 on pairs at eps (1 +- 2^-k): the partner decides each
    anchor's core flag and cluster.  Each side of every k-step class (d <= 16 /
    32 / 64 / 128), the second e4m3 k8-step (d > 64) and, at d = 129, the same
    data through the exact VALU tile; both count screens; at d = 5 / 65 / 128
    every pruning mode; at d = 5 / 64 / 128 also pairs that differ in one
    coordinate only."""
    for direction in (("dense", "axis") if d in (5, 64, 128) else ("dense",)):
        X, eps, ref = da.shell_case(d, dtype, r, 1024, direction)
        assert 0 < int(ref[1].sum()) < len(X)
        for screen in (1, 0):
            for prune in ((1, 0, 2) if d in (5, 65, 128) else (1,)):
                with _options(native, _screen(native, screen), _prune(native, prune)):
                    _assert_cluster(native, X, ref, eps, 2, (direction, screen, prune))


@pytest.mark.parametrize("mantissa", ["bf16", "e4m3"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("d", [16, 17, 32, 33, 64, 65, 127, 128])
def test_shell_pairs_aligned_rounding(native, d, dtype, mantissa):
    """Pairs whose coordinates all round the same way, so the errors of the
    low-precision products add up: "bf16" puts the split product ~1.5 2^-16
    of |a|^2 + |b|^2 off (random mantissas: < 2^-17; the band is 2^-13) and
    the hi.hi screen 0.98 of its worst case, "e4m3" puts the e4m3 screen
    0.86 of its band off.  min_samples = 2 as above."""
    for r in (-8, -14):
        X, eps, ref = da.shell_case(d, dtype, r, 1024, "dense", mantissa)
        assert 0 < int(ref[1].sum()) < len(X)
        for screen in (1, 0):
            with _options(native, _screen(native, screen)):
                _assert_cluster(native, X, ref, eps, 2, (r, screen))


# ------------------------------------------------------------ 2. ties link and border
@pytest.mark.parametrize("d,offset,dtype", TIE)
def test_tie_islands_link_and_border(native, d, offset, dtype):
    """Integer islands at eps = 3: consecutive islands are one cluster through
    pairs at d^2 = 9 exactly and two clusters at d^2 = 10, so the link and the
    border stage each depend on ties (far from the origin too: offset 2^20 in
    float32, 2^40 in float64).  The number of clusters is the closed form."""
    Z, X, joined, probes, ref = da.tie_case(d, 120, offset, dtype)
    isl = da.island_labels(joined)
    want = {"border": isl[probes["border"][1]], "noise": -1,
            "contested": isl[probes["contested"][1]]}
    assert ref[3] == 1 + int((~joined).sum())
    for screen in (1, 0):
        with _options(native, _screen(native, screen)):
            lab, core, ncl, cnt = _cluster(native, X, da.TIE_EPS, da.TIE_MIN_SAMPLES)
            assert np.array_equal(cnt, ref[2]), screen
            assert np.array_equal(core, ref[1]), screen
            assert np.array_equal(lab, ref[0]), screen
            assert ncl == 1 + int((~joined).sum()), screen
            for kind, (row, _) in probes.items():
                assert lab[row] == want[kind], (kind, screen)
            for P in (1, 3):
                _assert_train(X, ref, da.TIE_EPS, da.TIE_MIN_SAMPLES, P, screen)


# ------------------------------------------------------------ 3. ties at the window edge
def test_tie_islands_at_projection_window_edge(native):
    """8003 rows (four sub-bands of 2048): the ties lie exactly eps apart along
    the three widest axes, the ones the count pass prunes by.  Every pruning
    mode, and three simulated ranks (pd_dense_*), give the oracle's answer."""
    Z, X, joined, probes, ref = da.tie_case(16, 500, 2 ** 20, "float32")
    for prune in (1, 0, 2):
        for screen in (1, 0):
            with _options(native, _prune(native, prune), _screen(native, screen)):
                _assert_cluster(native, X, ref, da.TIE_EPS, da.TIE_MIN_SAMPLES, (prune, screen))
    (lab, core, cnt, ncl), parts = _dense_stages(native, _dev(X), da.TIE_EPS, da.TIE_MIN_SAMPLES,
                                                 native.PD_EUCLIDEAN, 3, full=True)
    assert np.array_equal(_np(cnt), ref[2])
    assert np.array_equal(core.cpu().numpy(), ref[1])
    assert np.array_equal(_np(lab), ref[0]) and ncl == ref[3]
    for p in parts:   # every rank computed some rows
        assert int((p > 0).sum()) > 0


# ------------------------------------------------------------ 4. tile and pad edges
def test_shell_pairs_tile_and_pad_edges(native):
    """n on both sides of the 32-row fragment group, the 64-row tile, the
    128-row pad (kPadNorm rows) and the 256-row block."""
    for d in (5, 128):
        for dtype, r in (("float32", -8), ("float64", -2)):
            for n_pairs in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129):
                X, eps, ref = da.shell_case(d, dtype, r, n_pairs)
                for screen in (1, 0):
                    with _options(native, _screen(native, screen)):
                        _assert_cluster(native, X, ref, eps, 2, (d, dtype, n_pairs, screen))


# ------------------------------------------------------------ 5. scale dispatch
@pytest.mark.parametrize("d,k", [(8, 40), (8, 48), (8, 49), (8, 60), (64, 48), (64, 49)])
def test_outlier_scale_dispatch(native, d, k):
    """eps^2 scale^2 on both sides of 1e-30 (k = 48: MFMA tiles on norms of
    ~1e-30; k = 49: the exact VALU tile): the same answer.  d = 64 has no pair
    within eps (min_samples = 1: n clusters in row order)."""
    ms = da.OUTLIER_MIN_SAMPLES if d == 8 else 1
    X, eps, ref = da.outlier_case(d, k, "float32", ms)
    for screen in (1, 0):
        with _options(native, _screen(native, screen)):
            _assert_cluster(native, X, ref, eps, ms, screen)
            _assert_train(X, ref, eps, ms, 1, screen)


# ------------------------------------------------------------ 6. predict
def test_predict_on_tie_islands():
    Z, X, joined, probes, ref = da.tie_case(64, 120, 2 ** 20, "float32")
    m = _train(X, da.TIE_EPS, da.TIE_MIN_SAMPLES, 1)
    assert np.array_equal(_np(m.labels_), ref[0])
    assert np.array_equal(_np(m.predict(_dev(X))), _np(m.labels_))
    # the probes against a model trained without them
    n = len(X) - 3
    m = _train(X[:n], da.TIE_EPS, da.TIE_MIN_SAMPLES, 1)
    core = m.core_sample_mask_.cpu().numpy().astype(bool)
    want = brute_predict(X[n:], X[:n][core], _np(m.labels_)[core], da.TIE_EPS)
    isl = da.island_labels(joined)
    assert want.tolist() == [isl[probes["border"][1]], -1, isl[probes["contested"][1]]]
    assert np.array_equal(_np(m.predict(_dev(X[n:]))), want)


def test_predict_on_shell_pairs():
    X, eps, ref = da.shell_case(128, "float32", -8)
    m = _train(X, eps, 2, 1)
    assert np.array_equal(_np(m.labels_), ref[0])
    assert np.array_equal(_np(m.predict(_dev(X))), _np(m.labels_))


ROW_LIMIT = [("float32", 236), ("float64", 118)]


def _index_case(dtype, d, seed):
    """~500 points, a few dozen queries around eps = 1 of the cores."""
    rng = np.random.default_rng(seed)
    n = 500
    X = rng.uniform(-1.0, 1.0, size=(n, d)).astype(dtype)
    core = rng.uniform(size=n) < 0.6
    lab = np.where(core, rng.integers(0, 6, size=n), -1).astype(np.int32)
    src = X[core][rng.integers(0, int(core.sum()), size=32)].astype(np.float64)
    f = rng.uniform(0.5, 1.5, size=(32, 1))          # |jitter| ~ f eps
    Q = np.concatenate([src + rng.normal(0.0, 1.0 / np.sqrt(d), size=(32, d)) * f,
                        X[rng.integers(0, n, size=8)],
                        rng.uniform(-1.0, 1.0, size=(8, d))]).astype(dtype)
    return X, core, lab, np.ascontiguousarray(Q)


@pytest.mark.parametrize("dtype,d", ROW_LIMIT)
def test_index_query_at_the_row_size_limit(native, dtype, d):
    """d * itemsize = 944 bytes is the largest row pd_index_query's tile
    kernel stages (64 query rows and one core row in LDS): it answers as the
    brute force does."""
    X, core, lab, Q = _index_case(dtype, d, 900 + d)
    ix = native.Index(_dev(X), _dev(core.astype(np.uint8)), _dev(lab), 1.0, native.PD_EUCLIDEAN)
    want = brute_predict(Q, X[core], lab[core], 1.0)
    assert (want >= 0).sum() >= 8 and (want == -1).sum() >= 8
    assert np.array_equal(_np(ix.query(_dev(Q))), want)
    ix.close()


@pytest.mark.parametrize("dtype,d", [(t, d + 1) for t, d in ROW_LIMIT])
def test_index_query_past_the_row_size_limit(native, dtype, d):
    X, core, lab, Q = _index_case(dtype, d, 900 + d)
    ix = native.Index(_dev(X), _dev(core.astype(np.uint8)), _dev(lab), 1.0, native.PD_EUCLIDEAN)
    with pytest.raises(native.PardisError) as e:
        ix.query(_dev(Q))
    assert e.value.code == native.PD_EUNSUPPORTED
    ix.close()
