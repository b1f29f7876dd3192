"""Point sets on which the d > 4 path (csrc/dense.hip) must take neighbour
decisions at the edge of what its low-precision arithmetic can tell apart
(tests/test_gpu_dense_band.py; the generators' preconditions are pinned on the
CPU in tests/test_dense_adversarial_host.py).

Blobs and embeddings put every pair orders of magnitude away from eps in
units of the MFMA error, so a band that is too narrow, a norm that drifts from
the fragments or a threshold rounded the wrong way never changes a count.
Here the pairs sit where those matter:

* ``shell_pairs``   — anchors with full mantissas and norms as large as the
  scaled box allows, each with one partner at eps (1 + delta), delta = +-2^-k
  for k = 4 .. 52 (and 0): from well outside the band c = 2^-13 to below the
  rounding of the coordinates.
* ``tie_islands``   — integer points whose clusters are joined, or kept
  apart, by squared distances of exactly eps^2 = 9 or of 10; the number of
  clusters is known in closed form, and ``int_counts`` is an integer
  reference that shares nothing with the oracle.
* ``outlier_scale`` — a cloud of diameter ~ eps with two outliers at
  +-eps 2^k that set the power-of-two scale: eps^2 scale^2 falls on either
  side of the 1e-30 below which the exact VALU tile replaces the MFMA.

Pure numpy; every generator is deterministic from its arguments.  Not a
conftest and not a test module.
"""
import functools

import numpy as np

TIE_EPS = 3.0          # tie_islands: eps^2 = 9
TIE_MIN_SAMPLES = 16   # every island point is core (16 points within 2 of each other)
OUTLIER_EPS = 2.0 ** -10
OUTLIER_MIN_SAMPLES = 8


# ---------------------------------------------------------------- 1. shell pairs
# |coordinate| of the anchors whose rounding errors all point the same way:
# bf16: 0.5 (1 + 2^-8 - 3 2^-17) splits into hi = 0.5 (the largest rounding a
#       bf16 can make, 2^-8 of the value), lo = 0.5 (2^-8 - 2^-15) (a tie, to
#       even) and a residual of 0.5 2^-17 that the split drops;
# e4m3: 0.5 (1 + 2^-4) is 136 at the screen's 2^8 scale, a tie that rounds to
#       128 (the largest rounding e4m3 can make, 1 / 17 of the value).
ALIGNED = {"bf16": 0.5 * (1.0 + 2.0 ** -8 - 3.0 * 2.0 ** -17), "e4m3": 0.5 * (1.0 + 2.0 ** -4)}


def shell_pairs(d, dtype, r_log2, n_pairs=1024, seed=0, direction="dense", mantissa="uniform"):
    """-> (X (2 n_pairs, d) in dtype, eps).  Anchors a = U(0.5, 1)^d with random
    signs; eps = sqrt(d) 2^r_log2; partner b_i = a_i + eps (1 + delta_i) u_i in
    fp64, then rounded to dtype, with u_i a random unit vector ("dense") or a
    random signed axis ("axis") and delta_i = +-2^-k, k uniform in 4 .. 52
    (0 for every 16th pair).  Rows interleaved: X[0::2] = a, X[1::2] = b.

    mantissa = "bf16" / "e4m3": every anchor coordinate is +-ALIGNED[mantissa]
    and u_i points towards the origin on every axis, so that (for eps small
    against the coordinates) a and b round the same way in every coordinate
    and the errors of the low-precision dot product add up instead of
    averaging out — the case the error bounds of dense.hip are written for."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng([seed, d, dtype.itemsize, int(r_log2) % 4096, n_pairs,
                                 0 if direction == "dense" else 1,
                                 ["uniform", "bf16", "e4m3"].index(mantissa)])
    a = rng.uniform(0.5, 1.0, size=(n_pairs, d)) * rng.choice([-1.0, 1.0], size=(n_pairs, d))
    if mantissa != "uniform":
        a = np.sign(a) * ALIGNED[mantissa]
    a = a.astype(dtype).astype(np.float64)
    eps = float(np.sqrt(float(d)) * 2.0 ** r_log2)
    if direction == "dense":
        u = rng.normal(size=(n_pairs, d))
        if mantissa != "uniform":
            u = -np.abs(u) * np.sign(a)
        u /= np.sqrt((u * u).sum(axis=1))[:, None]
    elif direction == "axis" and mantissa == "uniform":
        u = np.zeros((n_pairs, d))
        u[np.arange(n_pairs), rng.integers(0, d, size=n_pairs)] = rng.choice([-1.0, 1.0],
                                                                            size=n_pairs)
    else:
        raise ValueError(direction)
    delta = rng.choice([-1.0, 1.0], size=n_pairs) * 2.0 ** -rng.integers(4, 53, size=n_pairs)
    delta[::16] = 0.0
    b = a + (eps * (1.0 + delta))[:, None] * u
    X = np.empty((2 * n_pairs, d), dtype)
    X[0::2] = a
    X[1::2] = b
    return np.ascontiguousarray(X), eps


def pair_d2_exact(X):
    """|a_i - b_i|^2 of the interleaved pairs in np.longdouble (64-bit
    mantissa on x86: the fp64 / fp32 coordinates' differences are exact and the
    sum over d <= 129 squares carries ~2^-57 relative error)."""
    L = np.asarray(X).astype(np.longdouble)
    t = L[0::2] - L[1::2]
    return (t * t).sum(axis=1)


def centre_and_scale(X):
    """The geometry count_stage derives from the data box: the bbox midpoint
    0.5 lo + 0.5 hi per axis (fp64) and the power of two 2^-e2 with
    frexp(largest half-span) = (m, e2) — scaled coordinates in [-1, 1]."""
    X64 = np.asarray(X, np.float64)
    lo, hi = X64.min(axis=0), X64.max(axis=0)
    c = 0.5 * lo + 0.5 * hi
    span = float(np.maximum(np.abs(lo - c), np.abs(hi - c)).max())
    e2 = int(np.frexp(span)[1]) if span > 0.0 else 0
    return c, float(np.ldexp(1.0, -e2))


def gram32_pair_within(X, eps):
    """What a plain fp32 Gram evaluation says of the pairs, with no error band
    and no recheck: coordinates centred on the bbox midpoint in fp64 and cast
    to float32, |a|^2 + |b|^2 - 2 a.b with float32 sums, against float32(eps^2)."""
    c, _ = centre_and_scale(X)
    C = (np.asarray(X, np.float64) - c).astype(np.float32)
    a, b = C[0::2], C[1::2]
    na = (a * a).sum(axis=1, dtype=np.float32)
    nb = (b * b).sum(axis=1, dtype=np.float32)
    ab = (a * b).sum(axis=1, dtype=np.float32)
    d2 = (na + nb) - np.float32(2.0) * ab
    return d2 <= np.float32(eps * eps)


def pair_band_ratio(X, eps):
    """|d^2 - eps^2| / (|a|^2 + |b|^2) of the pairs on centred coordinates:
    the quantity the error band c bounds (scale-free)."""
    c, _ = centre_and_scale(X)
    C = np.asarray(X, np.float64) - c
    s = (C[0::2] ** 2).sum(axis=1) + (C[1::2] ** 2).sum(axis=1)
    e2 = np.longdouble(eps) * np.longdouble(eps)
    return np.abs(pair_d2_exact(X) - e2).astype(np.float64) / s


def round_bf16(v):
    """float32 -> nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def round_e4m3(v):
    """-> nearest OCP e4m3 value (ties to even, subnormals of 2^-9 kept), for
    |v| <= 448, as float64."""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(v)                       # v = m 2^e, 0.5 <= |m| < 1
    q = np.ldexp(np.round(m * 16.0) / 16.0, e)      # 4 significant bits (np.round: half to even)
    sub = np.abs(v) < 2.0 ** -6
    return np.where(sub, np.round(v * 512.0) / 512.0, q)


def pair_low_precision_excess(X, eps, kind):
    """(d2~ - d2) / (|a|^2 + |b|^2) of the pairs, with d2~ from the dot product
    the device forms, evaluated here without any further rounding
    (np.longdouble sums) on count_stage's centred, scaled float32 coordinates:
    kind = "split": hi.hi + hi.lo + lo.hi of the bf16 split (the band c);
    kind = "hi":    hi.hi alone (the bf16 screen c');
    kind = "e4m3":  coordinates x 2^8 rounded to e4m3 (the e4m3 screen c8).
    What remains is the error of the number formats alone, which the bands
    must cover whatever the accumulation adds."""
    c, scale = centre_and_scale(X)
    V = ((np.asarray(X, np.float64) - c) * scale).astype(np.float32)
    L = V.astype(np.longdouble)
    a, b = L[0::2], L[1::2]
    s = (a * a).sum(axis=1) + (b * b).sum(axis=1)
    if kind == "e4m3":
        Q = (round_e4m3(V.astype(np.float64) * 256.0) / 256.0).astype(np.longdouble)
        dot = (Q[0::2] * Q[1::2]).sum(axis=1)
    else:
        H = round_bf16(V)
        lo = round_bf16(V - H).astype(np.longdouble)
        H = H.astype(np.longdouble)
        dot = (H[0::2] * H[1::2]).sum(axis=1)
        if kind == "split":
            dot = dot + (H[0::2] * lo[1::2]).sum(axis=1) + (lo[0::2] * H[1::2]).sum(axis=1)
    d2 = ((a - b) ** 2).sum(axis=1)
    return ((s - 2 * dot - d2) / s).astype(np.float64)


# ---------------------------------------------------------------- 2. tie islands
def _tie_axes(d):
    """(advance axes by i % 4, the axis of a non-joining gap's extra step, the
    probes' axis): the last two lie outside the islands' axes 0..3 and are no
    advance axis."""
    adv = [0, 4, d // 2, d - 1]
    free = [k for k in range(5, d) if k not in adv]
    return adv, free[0], free[1]


def tie_islands(d, n_islands, offset, dtype, seed=0):
    """-> (Z int64 (n, d), X = Z + offset in dtype, joined bool (n_islands - 1),
    probes).  Island i: the 16 points of {0, 1}^4 on axes 0..3 at an integer
    origin; island i + 1's origin advances along axis [0, 4, d // 2, d - 1][i % 4]
    so that the nearest faces are 3 apart — a tie at eps = 3, the islands join
    (joined[i]) — or 3 apart and 1 along another axis (d^2 = 10, they do not);
    a seeded coin decides.  The last three rows are the probes,
    ``probes[kind] = (row, island)``:
      border     d^2 = 9 from one point of `island`, >= 10 from every other
      noise      d^2 = 10 from its nearest point
      contested  d^2 = 9 from one point each of `island` and `island + 1`,
                 which a d^2 = 10 gap separates (different labels)."""
    if d < 8:
        raise ValueError("tie_islands needs d >= 8")
    rng = np.random.default_rng([seed, d, n_islands])
    adv, extra, pax = _tie_axes(d)
    joined = rng.integers(0, 2, size=n_islands - 1).astype(bool)
    side = rng.choice([-1, 1], size=n_islands - 1)
    cube = np.array([[(c >> b) & 1 for b in range(4)] for c in range(16)], np.int64)
    origins = np.zeros((n_islands, d), np.int64)
    for i in range(n_islands - 1):
        a = adv[i % 4]
        origins[i + 1] = origins[i]
        origins[i + 1, a] += 4 if a < 4 else 3    # the island is 1 wide on its own axes
        if not joined[i]:
            origins[i + 1, extra] += side[i]
    Z = np.zeros((16 * n_islands + 3, d), np.int64)
    for i in range(n_islands):
        Z[16 * i:16 * i + 16] = origins[i]
        Z[16 * i:16 * i + 16, :4] += cube
    n = 16 * n_islands
    # border: 3 along the probes' axis from island 0's origin point
    Z[n] = origins[0]
    Z[n, pax] += 3
    # noise: 3 along the probes' axis and 1 beyond the last island's far face
    Z[n + 1] = origins[-1]
    Z[n + 1, 0] += 2
    Z[n + 1, pax] += 3
    # contested: across the first non-joining gap g (g >= 2, advance axis a not
    # an island axis).  With v = e_a + 2 s e_extra + 2 e_pax from p = origin g
    # and p' = p + 3 e_a + s e_extra (origin g + 1): |v|^2 = 9 and
    # |v - (p' - p)|^2 = |(-2, s, 2)|^2 = 9.
    cand = [g for g in range(2, n_islands - 1) if not joined[g] and g % 4 != 0]
    if not cand:
        raise ValueError("no d^2 = 10 gap for the contested probe: more islands or another seed")
    g = cand[0]
    Z[n + 2] = origins[g]
    Z[n + 2, adv[g % 4]] += 1
    Z[n + 2, extra] += 2 * side[g]
    Z[n + 2, pax] += 2
    probes = {"border": (n, 0), "noise": (n + 1, n_islands - 1), "contested": (n + 2, g)}
    X = np.ascontiguousarray((Z + np.int64(offset)).astype(dtype))
    return Z, X, joined, probes


def island_labels(joined):
    """Label of each island: the number of d^2 = 10 gaps before it (clusters
    are numbered by their first core point, the islands come in row order)."""
    return np.concatenate([[0], np.cumsum(~np.asarray(joined))]).astype(np.int64)


def int_counts(Z, e2, chunk=1024):
    """Neighbour counts (self included) of integer points in int64 alone:
    d2 = |z_i|^2 + |z_j|^2 - 2 z_i.z_j, d2 <= e2.  Coordinates are taken
    relative to the per-axis minimum so every product stays far below 2^63."""
    Z = np.asarray(Z, np.int64)
    Z = Z - Z.min(axis=0)
    nrm = (Z * Z).sum(axis=1)
    out = np.zeros(len(Z), np.int64)
    for s in range(0, len(Z), chunk):
        d2 = nrm[s:s + chunk, None] + nrm[None, :] - 2 * (Z[s:s + chunk] @ Z.T)
        out[s:s + chunk] = (d2 <= int(e2)).sum(axis=1)
    return out


# ---------------------------------------------------------------- 3. outlier scale
def outlier_scale(d, k, dtype=np.float32, n=1500, seed=0):
    """-> (X (n, d), eps = 2^-10): n - 2 points of N(0, (1.6 eps / sqrt(d))^2)
    and two outliers at +-eps 2^k on axis 0, which set count_stage's scale to
    2^-(k - 9): eps^2 scale^2 = 2^-(2 k + 2).  The cloud does not depend on k."""
    eps = OUTLIER_EPS
    rng = np.random.default_rng([seed, d, n])
    X = rng.normal(0.0, 1.6 * eps / np.sqrt(float(d)), size=(n, d))
    X[n // 3] = 0.0
    X[n // 3, 0] = eps * 2.0 ** k
    X[2 * n // 3] = 0.0
    X[2 * n // 3, 0] = -eps * 2.0 ** k
    return np.ascontiguousarray(X.astype(dtype)), eps


def eps2_scaled(X, eps):
    """eps^2 scale^2 as count_stage computes it (compared there with 1e-30:
    above it the MFMA tiles run, at or below it the exact VALU tile)."""
    _, scale = centre_and_scale(X)
    return eps * eps * scale * scale


# ---------------------------------------------------------------- shared cases
@functools.lru_cache(maxsize=None)
def shell_case(d, dtype, r_log2, n_pairs=1024, direction="dense", mantissa="uniform",
               perm_seed=1):
    """(X, eps, reference): the shell pairs in a seeded permutation of the rows
    (what the GPU tests feed) and the oracle's (labels, core, counts,
    n_clusters) at min_samples = 2, computed once and read-only."""
    import oracle
    X, eps = shell_pairs(d, dtype, r_log2, n_pairs, 0, direction, mantissa)
    X = np.ascontiguousarray(X[np.random.default_rng(perm_seed).permutation(len(X))])
    ref = oracle.dbscan(X, eps, 2)
    return _frozen(X), eps, _freeze_ref(ref)


@functools.lru_cache(maxsize=None)
def tie_case(d, n_islands, offset, dtype, seed=0):
    """(Z, X, joined, probes, reference at eps = 3, min_samples = 16)."""
    import oracle
    Z, X, joined, probes = tie_islands(d, n_islands, offset, dtype, seed)
    ref = oracle.dbscan(X, TIE_EPS, TIE_MIN_SAMPLES)
    return _frozen(Z), _frozen(X), _frozen(joined), probes, _freeze_ref(ref)


@functools.lru_cache(maxsize=None)
def outlier_case(d, k, dtype="float32", min_samples=OUTLIER_MIN_SAMPLES):
    """(X, eps, reference at min_samples)."""
    import oracle
    X, eps = outlier_scale(d, k, dtype)
    return _frozen(X), eps, _freeze_ref(oracle.dbscan(X, eps, min_samples))


def _frozen(a):
    a.setflags(write=False)
    return a


def _freeze_ref(ref):
    lab, core, cnt, nc = ref
    return _frozen(lab), _frozen(core), _frozen(cnt), nc
