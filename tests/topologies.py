"""Point sets whose clusters are connected as thinly as possible, for the link
stage (tests/test_gpu_link_topology.py; preconditions in tests/test_oracle.py).

Blobs and full lattices connect every cluster many times over, so a link bug
that drops one edge never changes a label.  Here every edge matters:

* ``super_eps_lattice`` — every point alone (n clusters), every cell its own
  root: the cell verify defers a pair for every neighbouring cell pair, past
  its block buffer and past the pair list.
* ``same_cell_clumps``  — two components inside one grid cell (kMixed cells)
  in every size tier of the cell-root kernels.
* ``snake`` / ``snake_nd`` — one cluster, one record wide: every edge a bridge.
* ``percolation``       — uniform points near the connectivity threshold.
* ``comb``              — border points within eps of two clusters.

Every generator takes a seed and a dtype and returns a C-contiguous (n, d)
array.  Not a conftest and not a test module.
"""
import functools

import numpy as np

EPS = 0.05


def _out(X, dtype):
    return np.ascontiguousarray(np.asarray(X, np.float64).astype(dtype))


# ---------------------------------------------------------------- the grid
def cell_width(eps=EPS):
    """pd_cluster's cell width on axes 1..d-1 (half of it on axis 0 at the
    default xsub = 2)."""
    return eps * (1.0 + 2.0 ** -20)


def cell_coords(X, eps=EPS):
    """Integer cell coordinates of every point in the grid pd_cluster builds:
    origin at the data minimum, cells ``cell_width(eps)`` wide, halved on
    axis 0."""
    X = np.asarray(X, np.float64)
    cw = cell_width(eps)
    inv = np.full(X.shape[1], 1.0 / cw)
    inv[0] = 2.0 / cw
    return np.floor((X - X.min(axis=0)) * inv).astype(np.int64)


def occupied_cells(X, eps=EPS):
    """Sorted unique cell coordinates and the number of points in each."""
    return np.unique(cell_coords(X, eps), axis=0, return_counts=True)


def forward_cells(d):
    """Cells a cell looks forward to in the cell verify at xsub = 2: 2 in its
    own row, 5 in each of the (3**(d-1) - 1) / 2 rows after it."""
    return 2 + 5 * (3 ** (d - 1) - 1) // 2


def neighbour_cell_pairs(X, eps=EPS):
    """Unordered pairs of occupied cells with |delta| <= 2 on axis 0 and <= 1
    on every other axis.  When every cell holds its own root (no two points
    within eps) this is the number of pairs the cell verify must defer."""
    cells, _ = occupied_cells(X, eps)
    d = cells.shape[1]
    pad = np.array([2] + [1] * (d - 1), np.int64)
    dims = cells.max(axis=0) + 1 + 2 * pad
    stride = np.ones(d, np.int64)
    for j in range(1, d):
        stride[j] = stride[j - 1] * dims[j - 1]
    keys = np.sort((cells + pad) @ stride)
    total = 0
    for off in np.ndindex(*([5] + [3] * (d - 1))):
        o = np.array(off, np.int64) - pad
        if tuple(o[::-1]) <= (0,) * d:      # forward half only (last axis leads)
            continue
        q = keys + int(o @ stride)
        pos = np.searchsorted(keys, q)
        pos[pos == len(keys)] = 0
        total += int(np.count_nonzero(keys[pos] == q))
    return total


# ---------------------------------------------------------------- 1. lattice
def super_eps_lattice(d, m, eps=EPS, seed=0, dtype=np.float32):
    """m**d lattice with spacing 1.03 eps and a jitter uniform in +-0.01 eps
    per axis: nearest neighbours are >= 1.01 eps apart, so with min_samples = 1
    every point is a cluster of its own, in input order."""
    rng = np.random.default_rng(seed)
    g = np.arange(m, dtype=np.float64) * (1.03 * eps)
    X = np.stack(np.meshgrid(*([g] * d), indexing="ij"), -1).reshape(-1, d)
    X = X + rng.uniform(-0.01 * eps, 0.01 * eps, X.shape)
    return _out(X, dtype)


# ---------------------------------------------------------------- 2. clumps
CLUMP_SIZES = [(5, 5)] * 8 + [(20, 20)] * 8 + [(600, 600)] * 8 + [(5, 1100)] * 4 + [(1, 1)] * 4


def clump_cell(k):
    """Grid cell (axis-0 half cells, axis-1 cells) that holds pair k."""
    return 8 * (k % 8) + 4, 4 * (k // 8) + 2


def bridged_pairs(sizes=None, min_samples=3):
    """Pairs that ``same_cell_clumps(bridged=True)`` joins: every second pair
    whose two clumps are both core at ``min_samples`` (a chain between two
    single points would add a cluster, not remove one)."""
    sizes = CLUMP_SIZES if sizes is None else sizes
    return [k for k, (na, nb) in enumerate(sizes)
            if k % 2 == 0 and min(na, nb) >= min_samples]


def same_cell_clumps(sizes=None, bridged=False, eps=EPS, seed=0, dtype=np.float32):
    """2-D.  An anchor at (0, 0) pins the grid origin.  Pair k lives in cell
    ``clump_cell(k)`` with origin o: clump A is ``na`` points around
    o + (0.03, 0.03) eps, clump B ``nb`` points around o + (0.47, 0.97) eps,
    each uniform in +-0.01 eps.  The two clumps share one cell and are
    >= 1.011 eps apart: two components in one cell.

    Returns (X, pair) with pair[i] = the pair index of point i (-1 for the
    anchor and for chain points).

    bridged=True adds, for every pair of ``bridged_pairs()``, a chain of five
    points 0.8 eps apart that leaves clump A to the left of the cell, climbs
    past it and comes down on clump B from above: the cell's two components
    become one cluster (min_samples = 3) joined only by records of other
    cells."""
    sizes = CLUMP_SIZES if sizes is None else sizes
    rng = np.random.default_rng(seed)
    cw = cell_width(eps)
    pts, pair = [np.zeros((1, 2))], [np.full(1, -1, np.int64)]
    chains = []
    for k, (na, nb) in enumerate(sizes):
        i, j = clump_cell(k)
        o = np.array([i * cw / 2, j * cw])
        a_c = o + np.array([0.03, 0.03]) * eps
        b_c = o + np.array([0.47, 0.97]) * eps
        pts.append(a_c + rng.uniform(-0.01 * eps, 0.01 * eps, (na, 2)))
        pts.append(b_c + rng.uniform(-0.01 * eps, 0.01 * eps, (nb, 2)))
        pair.append(np.full(na + nb, k, np.int64))
        if bridged and k in bridged_pairs(sizes):
            s = 0.8 * eps
            p1 = a_c + np.array([-s, 0.0])
            p2 = p1 + np.array([0.0, s])
            p3 = p2 + np.array([0.0, s])
            t = b_c + np.array([0.0, s])
            # the elbow: 0.8 eps from p3 and from t, on the far side of the cell
            mid, v = (p3 + t) / 2, t - p3
            half = np.hypot(*v) / 2
            perp = np.array([-v[1], v[0]]) / (2 * half)
            e = mid + perp * np.sqrt(s * s - half * half)
            chains.append(np.stack([p1, p2, p3, e, t]))
    if chains:
        pts.append(np.concatenate(chains))
        pair.append(np.full(5 * len(chains), -1, np.int64))
    return _out(np.concatenate(pts), dtype), np.concatenate(pair)


# ---------------------------------------------------------------- 3. snake
def snake(rows, cols, eps=EPS, seed=0, dtype=np.float32, cut=False):
    """2-D boustrophedon in walking order: rows 1.5 eps apart with points
    0.9 eps apart, consecutive rows joined at alternating ends by one
    connector 0.75 eps from each.  rows * cols + rows - 1 points, every one
    with its predecessor and successor as its only neighbours: one cluster,
    one record wide.  The geometry is fixed (``seed`` is unused; ``snake_nd``
    uses it).  cut=True deletes point n // 2: two clusters."""
    pts = []
    for r in range(rows):
        x = np.arange(cols, dtype=np.float64) * 0.9
        if r % 2:
            x = x[::-1]
        pts.append(np.stack([x, np.full(cols, r * 1.5)], -1))
        if r + 1 < rows:
            pts.append(np.array([[x[-1], r * 1.5 + 0.75]]))
    X = np.concatenate(pts) * eps
    if cut:
        X = np.delete(X, len(X) // 2, axis=0)
    return _out(X, dtype)


def snake_nd(d, rows, cols, eps=EPS, seed=0, dtype=np.float32, cut=False):
    """The 2-D snake padded with zeros and rotated into d-D by a fixed
    orthonormal matrix (QR of a seeded normal matrix)."""
    X2 = snake(rows, cols, eps, seed, np.float64, cut)
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(d, d)))
    X = np.zeros((len(X2), d))
    X[:, :2] = X2
    return _out(X @ q.T, dtype)


# ---------------------------------------------------------------- 4. percolation
# points per eps**d near the connectivity threshold of each dimension
PERCOLATION_DENSITY = {1: 4.5, 2: 1.3, 3: 0.75, 4: 0.45}


def percolation(d, n, density=None, eps=EPS, seed=0, dtype=np.float32):
    """n uniform points in a cube holding ``density`` points per eps**d
    (default ``PERCOLATION_DENSITY[d]``: 1.3, 0.75 and 0.45 for d = 2..4).
    At these densities min_samples 1..3 give thousands of clusters with a
    largest one of a few to some tens of per cent of the points: tortuous
    clusters full of bridges.

    d = 1 has no connectivity threshold: on a uniform line a cluster ends at
    every gap > eps, cluster sizes are geometric with mean exp(density), and
    the largest of N of them is about exp(density) * ln N points.  More than
    1000 clusters in 60 000 points bound the mean by 60, hence the largest by
    ~420 points (0.7 %): no uniform density gives "more than 1000 clusters
    and a largest one of >= 2 %" (density 1.6 gave 7 687 - 12 117 clusters,
    the largest 49 points).  The 1-D case therefore ramps its local density
    linearly along the line from 0.25 to 1.75 times ``density`` (mean 4.5:
    1.125 to 7.875 points per eps), which passes through every regime from
    dust to runs of thousands of points; the points come in random order
    like the uniform cases'."""
    density = PERCOLATION_DENSITY[d] if density is None else density
    rng = np.random.default_rng(seed)
    if d == 1:
        lam = np.linspace(0.25, 1.75, n) * density
        x = np.cumsum(rng.exponential(1.0, n) / lam) * eps
        return _out(rng.permutation(x)[:, None], dtype)
    side = (n / density) ** (1.0 / d) * eps
    return _out(rng.uniform(0.0, side, (n, d)), dtype)


# ---------------------------------------------------------------- 5. comb
def comb(rows=40, cols=600, eps=EPS, seed=0, dtype=np.float32):
    """2-D.  ``rows`` horizontal lines 1.8 eps apart of ``cols`` points at
    0.1 eps spacing, and between consecutive lines a midpoint every 25 columns
    (from column 12, so that each has its eight neighbours on both lines and
    all of them are core) at (c * 0.1 + 0.05, r * 1.8 + 0.9) eps.  With min_samples = 20 every line
    is a cluster and every midpoint a border point (17 neighbours) within eps
    of core points of exactly two clusters.  The geometry is fixed (``seed``
    is unused).

    Returns (X, is_mid)."""
    c = np.arange(cols, dtype=np.float64) * 0.1
    lines = np.stack([np.tile(c, rows), np.repeat(np.arange(rows) * 1.8, cols)], -1)
    cm = np.arange(12, cols, 25, dtype=np.float64) * 0.1 + 0.05
    mids = np.stack([np.tile(cm, rows - 1), np.repeat(np.arange(rows - 1) * 1.8 + 0.9, len(cm))], -1)
    X = np.concatenate([lines, mids]) * eps
    is_mid = np.zeros(len(X), bool)
    is_mid[len(lines):] = True
    return _out(X, dtype), is_mid


# ---------------------------------------------------------------- shared cases
GENERATORS = {"super_eps_lattice": super_eps_lattice, "same_cell_clumps": same_cell_clumps,
              "snake": snake, "snake_nd": snake_nd, "percolation": percolation, "comb": comb}


def _frozen(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def points(name, args=(), dtype="float32", perm=None, kw=()):
    """(X, aux) of ``GENERATORS[name](*args, dtype=dtype, **dict(kw))``, built
    once and read-only; aux is the generator's second return value (or None).
    perm: seed of a random permutation of the input order (applied to both)."""
    out = GENERATORS[name](*args, dtype=np.dtype(dtype).type, **dict(kw))
    X, aux = out if isinstance(out, tuple) else (out, None)
    if perm is not None:
        p = np.random.default_rng(perm).permutation(len(X))
        X = np.ascontiguousarray(X[p])
        aux = None if aux is None else aux[p]
    return _frozen(X), _frozen(aux)


@functools.lru_cache(maxsize=None)
def reference(name, args, min_samples, dtype="float32", perm=None, kw=(), metric="euclidean",
              eps=EPS):
    """The oracle's (labels, core, counts, n_clusters) for ``points(...)``,
    computed once and read-only."""
    import oracle
    X, _ = points(name, args, dtype, perm, kw)
    lab, core, cnt, nc = oracle.dbscan(X, eps, min_samples, metric)
    return _frozen(lab), _frozen(core), _frozen(cnt), nc
