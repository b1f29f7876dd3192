"""Preconditions of the dense path's adversarial point sets
(tests/dense_adversarial.py), on the CPU: conditions on the inputs that
tests/test_gpu_dense_band.py relies on, so a generator that stops being
adversarial fails here and not silently on the GPU."""
import numpy as np
import pytest

import dense_adversarial as da

SHELL_D = (5, 16, 17, 32, 33, 64, 65, 127, 128, 129)
SHELL_R = {"float32": (-2, -8, -14), "float64": (-2, -8, -14, -20)}
SHELL = [(d, dt, r) for dt in ("float32", "float64") for d in SHELL_D for r in SHELL_R[dt]]
TIE = [(d, off, dt) for d in (8, 17, 64, 65, 128)
       for off, dt in ((0, "float32"), (2 ** 20, "float32"), (2 ** 40, "float64"))]


# ---------------------------------------------------------------- shell pairs
@pytest.mark.parametrize("d,dtype,r", SHELL)
def test_shell_pairs_straddle_eps_and_defeat_fp32(d, dtype, r):
    X, eps = da.shell_pairs(d, dtype, r)
    assert X.dtype == np.dtype(dtype) and X.shape == (2048, d) and X.flags.c_contiguous
    assert eps == np.sqrt(float(d)) * 2.0 ** r
    inside = da.pair_d2_exact(X) <= np.longdouble(eps) * np.longdouble(eps)
    frac = float(inside.mean())
    wrong = int((da.gram32_pair_within(X, eps) != inside).sum())
    ratio = da.pair_band_ratio(X, eps)
    in_band = int(((ratio >= 2.0 ** -22) & (ratio <= 2.0 ** -13)).sum())
    print(f"\nshell_pairs d={d} {dtype} r={r}: within={frac:.3f} gram32_wrong={wrong} "
          f"band={in_band} of {len(inside)}")
    # both sides of eps, by distances far more precise than the predicate's
    assert 0.40 <= frac <= 0.60
    # a plain fp32 Gram evaluation gets them wrong: without the exact recheck
    # the GPU test cannot pass
    assert wrong >= 0.20 * len(inside)
    # pairs outside the band c = 2^-13 but within 2^9 of it, which the MFMA
    # product decides on its own: a narrower band decides them wrongly
    if r in (-2, -8):
        assert in_band >= 0.03 * len(inside)


@pytest.mark.parametrize("d", [5, 64, 128])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_shell_pairs_axis_direction(d, dtype):
    """direction="axis": the pair differs in one coordinate, so the rounding
    of that coordinate to dtype decides the side of the small |delta|.  The
    sign of delta decides where eps 2^-k exceeds half an ulp of a coordinate
    below 2 (2^-24 in float32): at r = -14 that is k < 10 + log2(sqrt(d)), 7
    or more of the 49 values of k, so >= 7 % of the pairs fall on each side in
    expectation, 4 % with 3.8 sigma to spare at 960 pairs."""
    for r in SHELL_R[dtype]:
        X, eps = da.shell_pairs(d, dtype, r, direction="axis")
        t = X[0::2].astype(np.float64) - X[1::2].astype(np.float64)
        assert ((t != 0).sum(axis=1) == 1).all()
        frac = float((da.pair_d2_exact(X) <= np.longdouble(eps) * np.longdouble(eps)).mean())
        print(f"\nshell_pairs axis d={d} {dtype} r={r}: within={frac:.3f}")
        assert 0.04 <= frac <= 0.96


ALIGNED_D = (16, 17, 32, 33, 64, 65, 127, 128)
# what the number formats alone can cost, relative to |a|^2 + |b|^2 (the
# derivations are in dense.hip's header and screen comments): with u = 2^-8 /
# (1 + 2^-8) the largest relative rounding of a bf16, u8 = 2^-4 / (1 + 2^-4)
# that of an e4m3
U16, U8 = 2.0 ** -8 / (1.0 + 2.0 ** -8), 2.0 ** -4 / (1.0 + 2.0 ** -4)
SPLIT_BOUND = 3.01 * 2.0 ** -16
HI_BOUND = 2.0 * U16 + U16 * U16
E4M3_BOUND = 2.0 * U8 + U8 * U8


@pytest.mark.parametrize("d", ALIGNED_D)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_shell_pairs_aligned_bf16_defeat_a_narrow_band(d, dtype):
    """mantissa="bf16" at r = -14: every coordinate of a pair rounds the same
    way, so the split product's error is ~1.5 2^-16 of |a|^2 + |b|^2 (lo.lo'
    ~ 2^-16 and the anchor's residual ~ 2^-17 of each product, doubled in
    d2, over x.y ~ half the norms) where random mantissas give < 2^-17: a
    band of 2^-16 rejects the pairs within eps without a recheck (all of
    them in expectation, half the pairs; the floor is the 20 % of the other
    sets).  The hi.hi product alone is off by ~0.98 of the most a bf16 can be."""
    X, eps = da.shell_pairs(d, dtype, -14, mantissa="bf16")
    inside = da.pair_d2_exact(X) <= np.longdouble(eps) * np.longdouble(eps)
    assert 0.40 <= inside.mean() <= 0.60
    ratio = da.pair_band_ratio(X, eps)
    split = da.pair_low_precision_excess(X, eps, "split")
    hi = da.pair_low_precision_excess(X, eps, "hi")
    rejected = inside & (split - ratio - 2.0 ** -16 > 2.0 ** -19)
    print(f"\naligned bf16 d={d} {dtype}: split excess {split.min():.3g}..{split.max():.3g} "
          f"hi.hi excess {hi.min():.3g}..{hi.max():.3g} rejected by 2^-16: {int(rejected.sum())}")
    assert rejected.sum() >= 0.20 * len(inside)
    assert (split > 2.0 ** -16).all() and (split <= SPLIT_BOUND).all()
    assert (hi >= 0.95 * HI_BOUND).all() and (hi <= HI_BOUND).all()


@pytest.mark.parametrize("d", ALIGNED_D)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_shell_pairs_aligned_e4m3_near_the_screen_bound(d, dtype):
    """mantissa="e4m3" at r = -14: every coordinate is rounded by 1 / 17 of
    itself, the most e4m3 can, so the screen's d2 is off by (2 u8 - u8^2) of
    2 x.y ~ 0.114 (|a|^2 + |b|^2), 0.86 of the band c8 = 2^-3 + 2^-7."""
    X, eps = da.shell_pairs(d, dtype, -14, mantissa="e4m3")
    inside = da.pair_d2_exact(X) <= np.longdouble(eps) * np.longdouble(eps)
    assert 0.40 <= inside.mean() <= 0.60
    e8 = da.pair_low_precision_excess(X, eps, "e4m3")
    print(f"\naligned e4m3 d={d} {dtype}: e4m3 excess {e8.min():.4f}..{e8.max():.4f}")
    assert (e8 >= 0.11).all() and (e8 <= E4M3_BOUND).all()


@pytest.mark.parametrize("d,dtype,r", [c for c in SHELL if c[0] <= 128])
def test_low_precision_products_stay_inside_their_bounds(d, dtype, r):
    """The bounds the bands of dense.hip are derived from, on every shell set
    the MFMA tiles see (d > 128 takes the exact VALU tile)."""
    for mantissa in ("uniform", "bf16", "e4m3"):
        if mantissa != "uniform" and d < 16:
            continue
        X, eps = da.shell_pairs(d, dtype, r, mantissa=mantissa)
        assert np.abs(da.pair_low_precision_excess(X, eps, "split")).max() <= SPLIT_BOUND
        assert np.abs(da.pair_low_precision_excess(X, eps, "hi")).max() <= HI_BOUND


def test_shell_pairs_are_deterministic_and_seeded():
    a, _ = da.shell_pairs(17, "float32", -8, n_pairs=64)
    b, _ = da.shell_pairs(17, "float32", -8, n_pairs=64)
    c, _ = da.shell_pairs(17, "float32", -8, n_pairs=64, seed=1)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert (np.abs(a[0::2]) >= 0.5).all() and (np.abs(a[0::2]) <= 1.0).all()


# ---------------------------------------------------------------- tie islands
def _check_ties(d, n_islands, offset, dtype):
    Z, X, joined, probes, ref = da.tie_case(d, n_islands, offset, dtype)
    lab, core, cnt, ncl = ref
    n = 16 * n_islands
    assert X.dtype == np.dtype(dtype) and len(X) == n + 3
    # integer valued, exactly
    assert np.array_equal(X.astype(np.longdouble) - np.longdouble(offset),
                          Z.astype(np.longdouble))
    # the oracle's counts by an integer reference that shares nothing with it
    assert np.array_equal(cnt, da.int_counts(Z, 9))
    # every island point is core; clusters in closed form
    assert core[:n].all() and not core[n:].any()
    assert ncl == 1 + int((~joined).sum())
    isl = da.island_labels(joined)
    assert np.array_equal(lab[:n], np.repeat(isl, 16))
    assert int(joined.sum()) >= 20 and int((~joined).sum()) >= 20
    # the probes: border through one tie, noise at d^2 = 10, the smaller of two labels
    c9, c10 = da.int_counts(Z, 9), da.int_counts(Z, 10)
    rb, ib = probes["border"]
    assert c9[rb] == 2 and lab[rb] == isl[ib]
    rn, _ = probes["noise"]
    assert c9[rn] == 1 and c10[rn] == 2 and lab[rn] == -1
    rc, g = probes["contested"]
    assert c9[rc] == 3 and not joined[g] and isl[g + 1] == isl[g] + 1 and lab[rc] == isl[g]
    zc = Z[rc] - Z[:n]
    tied = np.nonzero((zc * zc).sum(axis=1) == 9)[0]
    assert sorted(tied // 16) == [g, g + 1]


@pytest.mark.parametrize("d,offset,dtype", TIE)
def test_tie_islands(d, offset, dtype):
    _check_ties(d, 120, offset, dtype)


def test_tie_islands_window_edge_set():
    """The 8000-point set of the projection-window test: the three widest axes
    are advance axes, along which the ties are exactly eps apart."""
    _check_ties(16, 500, 2 ** 20, "float32")
    Z, X, joined, _, _ = da.tie_case(16, 500, 2 ** 20, "float32")
    width = X.max(axis=0).astype(np.float64) - X.min(axis=0)
    assert set(np.argsort(-width, kind="stable")[:3]) <= {0, 4, 8, 15}
    assert len(X) > 3 * 2048          # four sub-bands of 2048 rows


def test_int_counts_small():
    Z = np.array([[0, 0], [3, 0], [0, 3], [3, 3], [2, 2]])
    assert da.int_counts(Z, 9).tolist() == [4, 4, 4, 4, 5]
    assert da.int_counts(Z + 2 ** 40, 9, chunk=2).tolist() == [4, 4, 4, 4, 5]


# ---------------------------------------------------------------- outlier scale
def test_outlier_scale_straddles_the_mfma_switch():
    for d in (8, 64):
        vals = {}
        for k in (40, 48, 49, 60):
            X, eps = da.outlier_scale(d, k)
            assert X.dtype == np.float32 and eps == 2.0 ** -10
            vals[k] = da.eps2_scaled(X, eps)
            assert vals[k] == 2.0 ** -(2 * k + 2)
        assert vals[40] > vals[48] > 1e-30 > vals[49] > vals[60] > 0.0
        assert vals[48] < 4e-30 and vals[49] > 7e-31     # next to the switch


@pytest.mark.parametrize("k", [40, 48, 49, 60])
def test_outlier_scale_has_core_border_and_noise(k):
    X, eps, (lab, core, cnt, ncl) = da.outlier_case(8, k)
    border = (lab >= 0) & (core == 0)
    print(f"\noutlier_scale d=8 k={k}: core={int(core.sum())} border={int(border.sum())} "
          f"noise={int((lab < 0).sum())} clusters={ncl}")
    assert core.sum() >= 50 and border.sum() >= 50 and (lab < 0).sum() >= 50 and ncl >= 1
    # the cloud is the same for every k: so is the answer
    assert np.array_equal(cnt, da.outlier_case(8, 40)[2][2])


def test_outlier_scale_d64_every_point_alone():
    """At d = 64 the cloud's pairs lie ~2.3 eps apart (5.12 eps^2 chi2_64 / 64):
    no point has a neighbour, so min_samples = 1 makes n clusters in row order."""
    for k in (48, 49):
        X, eps, (lab, core, cnt, ncl) = da.outlier_case(64, k, "float32", 1)
        assert (cnt == 1).all() and ncl == len(X) and np.array_equal(lab, np.arange(len(X)))
