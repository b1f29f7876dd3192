"""Row and query sets on which the index queries (csrc/assign.hip: predict,
kdist, kneighbors, radius, weighted kdist and the mutual-reachability forest)
must take neighbour decisions at the edge of what the index's own grid, walk,
fp32 screen and k-lists can tell apart (tests/test_gpu_index_adversarial.py; the
generators' claims are pinned on the CPU in tests/test_index_adversarial_host.py).

The index shares no geometry with the train: its box is the tight bounding box
of its rows, its cells are r_max (1 + 2^-20) grow wide with grow doubled until
every axis has <= 2^28 cells (size_grid), its keys are 4 bytes wide below
G = 2^32 - 1 cells and 8 from there on, and a query may lie up to one cell
outside the box.  ``index_grid`` models that in numpy, operation by operation.
The model only places points: every expected answer comes from the brute-force
references (``reference``), none from the model.

* ``cell_edge``  — grid_adversarial.chord_edge at xsub = 1, grow = 1: its two
  anchors are rows, so the index's box and cells are the generator's.
* ``cap_edge``   — one axis of exactly 2^28 cells (grow 1) or 2^28 + 1 (grow
  2), straddling groups at both ends.
* ``slack_edge`` — pairs two cells apart if the cell width were eps itself.
* ``key_width``  — grids of 2^32 - 65536, 2^32 - 1, 2^32 and 2^32 + 2^20 cells.
* ``faces``      — queries that are not rows, outside every face and corner.
* ``k_shell``    — a k-list filled exactly to the cap.
* ``screen``     — grid_adversarial.screen_band's fp32 misdecision pairs.
* ``scaled``     — the goldens times 2^s (grid_adversarial.scaled_cases).
* ``tile_*``     — dense_adversarial's ties and shells, and row / query counts
  around the tile and block sizes, for the d > 4 tile kernels.

Every family returns a dict: X (rows), Q (queries; X itself where the rows are
the queries), r_max, metric, k, groups (of the rows), and what its host test
pins.  Pure numpy; deterministic from the arguments.  Not a conftest and not a
test module.
"""
import functools

import numpy as np

import dense_adversarial as da
import grid_adversarial as ga
import kdist_ref
import knn_ref
import mreach_ref
import predict_ref
import radius_ref
from grid_adversarial import (_step, _walk_largest, cells, chord_edge_detail, pair_acc,
                              scaled_golden_detail, screen_band_detail, threshold)

MAX_AXIS_CELLS = 1 << 28          # size_grid's cap per axis
KEY4_BELOW = 0xFFFFFFFF           # G below this: 4-byte keys
KS = (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)     # test_gpu_knn.KS: both sides of every list tier
EPS = 0.05


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- the grid model
def index_grid(rows, r_max):
    """size_grid over the tight box of `rows`: -> (lo, inv, nc, grow, G,
    key_bytes).  cw = r_max (1 + 2^-20) grow left to right, inv = 1 / cw,
    nc_j = floor((hi_j - lo_j) inv) + 1, each operation rounded in fp64; grow
    doubles until every nc_j <= 2^28 and G < 4e18."""
    X = np.asarray(rows).astype(np.float64)
    lo, hi = X.min(axis=0), X.max(axis=0)
    grow = 1.0
    for _ in range(2200):
        cw = ga.cell_width(r_max, grow)
        inv = 1.0 / cw
        nc = np.floor((hi - lo) * np.float64(inv)) + 1.0
        G = 1
        for v in nc:
            G *= int(v)
        if np.isfinite(cw) and inv > 0.0 and (nc >= 1).all() and (nc <= MAX_AXIS_CELLS).all() \
                and G < 4.0e18:
            return lo, inv, nc.astype(np.int64), grow, G, (4 if G < KEY4_BELOW else 8)
        grow *= 2.0
    raise ValueError("no cell size fits")


def row_cells(a, lo, inv):
    """Cell coordinates of rows a (n, d) under index_grid's lo / inv."""
    a = np.asarray(a)
    return np.stack([cells(a[:, j], lo[j], inv) for j in range(a.shape[1])], axis=1)


def cell_keys(c, nc):
    """Keys of cell coordinates c (n, d): axis 0 has stride 1 (Python ints)."""
    out = []
    for row in np.asarray(c).tolist():
        k, st = 0, 1
        for j, v in enumerate(row):
            k += int(v) * st
            st *= int(nc[j])
        out.append(k)
    return out


# ---------------------------------------------------------------- straddling groups
def straddle(dtype, metric, eps, lo, inv, want, cross, side, free, sgn, delta):
    """Groups of three around a cell boundary, as grid_adversarial.chord_edge
    builds them but at any cell: per group the query q in cell want (in-cell
    fraction 1/2; on axis `cross` the fraction delta from the boundary on
    `side`), its neighbour — on `cross` the representable value of the next
    cell nearest to q's, along `free` (direction sgn) the largest offset the
    exact predicate accepts — and the neighbour's twin one step further along
    `free`, which it rejects.  cross == free: the offset along that axis is
    itself what crosses (direction side).  cross < 0: nothing is crossed on
    purpose.  -> (q, nb, twin, ok); ok: the searches ended on two adjacent
    values and q, nb lie in the cells aimed at."""
    dtype = np.dtype(dtype)
    want = np.asarray(want, np.int64)
    G, d = want.shape
    ar = np.arange(G)
    cross, side, free, sgn = (np.broadcast_to(np.asarray(v, np.int64), (G,)).copy()
                              for v in (cross, side, free, sgn))
    delta = np.broadcast_to(np.asarray(delta, np.float64), (G,))
    lo = np.asarray(lo, np.float64)
    thr = threshold(eps, metric)
    has = cross >= 0
    sgn = np.where(has & (cross == free), side, sgn)
    fr = np.full((G, d), 0.5)
    fr[ar[has], cross[has]] = np.where(side[has] > 0, 1.0 - delta[has], delta[has])
    q = (lo[None, :] + (want + fr) / inv).astype(dtype)
    for j in range(d):
        for _ in range(8):
            c = cells(q[:, j], lo[j], inv)
            q[:, j] = np.where(c > want[:, j], _step(q[:, j], False),
                               np.where(c < want[:, j], _step(q[:, j], True), q[:, j]))
    ok = np.all([cells(q[:, j], lo[j], inv) == want[:, j] for j in range(d)], axis=0)
    nb = q.copy()
    for j in range(d):
        m = has & (cross == j) & (free != j)
        if not m.any():
            continue
        tgt = want[m, j] + side[m]
        start = (lo[j] + (want[m, j] + (side[m] > 0)) / inv).astype(dtype)
        v, f = _walk_largest(start, lambda x, j=j, tgt=tgt: cells(x, lo[j], inv) == tgt,
                             side[m] < 0)
        nb[m, j] = v
        ok[m] &= f
    rest = pair_acc(q, nb, metric)
    ok &= rest <= thr
    room = np.maximum(thr - rest, 0.0)
    dx = np.sqrt(room) if metric == "euclidean" else room
    start = (q[ar, free].astype(np.float64) + sgn * dx).astype(dtype)

    def accepted(v):
        t = nb.copy()
        t[ar, free] = v
        return pair_acc(q, t, metric) <= thr

    v, f = _walk_largest(start, accepted, sgn > 0)
    ok &= f
    nb[ar, free] = v
    twin = nb.copy()
    twin[ar, free] = _step(v, sgn > 0)
    ok &= (twin[ar, free] != nb[ar, free]) & (nb[ar, free] != q[ar, free])
    cq = np.stack([cells(q[:, j], lo[j], inv) for j in range(d)], axis=1)
    cn = np.stack([cells(nb[:, j], lo[j], inv) for j in range(d)], axis=1)
    ok &= ~has | ((cn - cq)[ar, np.maximum(cross, 0)] == side)
    return q, nb, twin, ok


def _assemble(dtype, anchors, q, nb, twin, keep, seed):
    """Rows: the anchors (role 3, groups 0 ..), then per kept group q (role 0),
    nb (1), twin (2); shuffled by a seeded permutation."""
    rows = [np.asarray(a) for a in anchors]
    groups = list(range(len(rows)))
    role = [3] * len(rows)
    g = len(rows)
    for i in keep:
        rows += [q[i], nb[i], twin[i]]
        groups += [g] * 3
        role += [0, 1, 2]
        g += 1
    X = np.array(rows, np.dtype(dtype))
    perm = np.random.default_rng(seed).permutation(len(X))
    return (_frozen(np.ascontiguousarray(X[perm])), _frozen(np.array(groups, np.int64)[perm]),
            _frozen(np.array(role, np.int64)[perm]))


def _box(dtype, lo, ncells, eps, grow=1.0, frac=0.5):
    """(lo, hi) in dtype whose index grid has `ncells` cells per axis: hi at
    in-cell fraction `frac` of the last cell."""
    cw = ga.cell_width(eps, grow)
    lo = np.asarray(lo, np.float64).astype(dtype)
    hi = (lo.astype(np.float64) + (np.asarray(ncells, np.float64) - 1.0 + frac) * cw).astype(dtype)
    return lo, hi


def _case(fam, key, X, groups, role, eps, metric, k=2, Q=None, **more):
    out = dict(family=fam, key=(fam,) + tuple(key), X=X, Q=X if Q is None else _frozen(Q),
               groups=groups, role=role, r_max=float(eps), metric=metric, k=k)
    lo, inv, nc, grow, G, kb = index_grid(X, eps)
    out.update(lo=lo, inv=inv, nc=nc, grow=grow, G=G, key_bytes=kb)
    out.update(more)
    return out


# ---------------------------------------------------------------- a. cell edge
@functools.lru_cache(maxsize=None)
def cell_edge(dtype, d, metric, offset=0.0):
    """chord_edge at xsub = 1, grow = 1: the anchors are rows, so the index's
    tight box is the generator's and its cells are floor((a - lo) inv) with
    the same cw.  r_max = eps; the rows are the queries."""
    r = chord_edge_detail(np.dtype(dtype).name, d, metric, 1, 1.0, float(offset))
    return _case("cell_edge", (np.dtype(dtype).name, d, metric, float(offset)), r["X"],
                 r["groups"], r["role"], r["eps"], metric, k=2, q=r["q"], n_in=r["n_in"],
                 n_out=r["n_out"], side=r["side"], enumerated=_chord_enumerated(d))


def _chord_enumerated(d):
    return len(ga._chord_axes(d)) * 2 * len(ga.CHORD_DELTAS) * len(ga.chord_f0(1)) * 2 * 2


# ---------------------------------------------------------------- b. cap edge
@functools.lru_cache(maxsize=None)
def cap_edge(d, axis, over, metric="euclidean", per=24):
    """fp64.  Axis `axis` has exactly 2^28 cells (over = False: grow 1) or an
    extent worth 2^28 + 1 (over = True: size_grid doubles the cells, 2^27 + 1
    of them, and the groups are placed relative to the doubled cells); the
    other axes have 4.  4 x `per` groups: at the first and the last cells of
    the long axis, crossing the long axis itself (the offset along it crosses)
    and crossing a short axis with the offset along the long one."""
    dtype = np.dtype("float64")
    eps = EPS
    grow = 2.0 if over else 1.0
    long_cells = MAX_AXIS_CELLS + (1 if over else 0)
    n_un = np.full(d, 4.0 * grow)            # in ungrown cells
    n_un[axis] = long_cells
    lo, hi = _box(dtype, np.full(d, -3.25), n_un, eps, 1.0, 0.5)
    nc_long = long_cells if not over else long_cells // 2 + 1
    inv = ga.cell_inv(eps, grow)
    short = [j for j in range(d) if j != axis]
    want, cross, side, free, sgn, delta = [], [], [], [], [], []
    deltas = ga.CHORD_DELTAS
    for end in (0, 1):
        for kind in (0, 1):                   # 0: across the long axis, 1: across a short one
            for i in range(per):
                w = np.ones(d, np.int64)
                step = 8 * (2 * i + kind + 1)
                w[axis] = step if end == 0 else nc_long - 1 - step
                if kind == 0 or not short:
                    cr, sd = axis, (1 if i % 2 == 0 else -1)
                else:
                    cr = short[i % len(short)]
                    sd = 1 if (i // len(short)) % 2 == 0 else -1
                    w[cr] = 1 if sd > 0 else 2
                want.append(w)
                cross.append(cr)
                side.append(sd)
                free.append(axis)
                sgn.append(1 if (i // 2) % 2 == 0 else -1)
                delta.append(deltas[i % len(deltas)] / grow)
    q, nb, twin, ok = straddle(dtype, metric, eps, lo, inv, np.array(want), cross, side, free,
                               sgn, delta)
    keep = np.flatnonzero(ok)
    X, groups, role = _assemble(dtype, [lo, hi], q, nb, twin, keep, [31, d, axis, int(over)])
    return _case("cap_edge", (d, axis, bool(over), metric), X, groups, role, eps, metric, k=2,
                 q=_frozen(q[keep]), n_in=_frozen(nb[keep]), n_out=_frozen(twin[keep]),
                 cross=np.array(cross)[keep], side1=np.array(side)[keep], enumerated=len(ok),
                 want=np.array(want)[keep])


# ---------------------------------------------------------------- b'. the 2^-20 slack
@functools.lru_cache(maxsize=None)
def slack_edge(d, axis, metric="euclidean", n_pairs=96):
    """fp64 pairs within eps whose cells would differ by 2 on `axis` if the cell
    width were eps itself, without the factor 1 + 2^-20: for 2^14 consecutive
    candidate cells k of that narrower grid, a1 is the largest value below the
    boundary lo + k eps and a2 the largest value the exact predicate accepts
    from a1; the pair is kept when floor((a - lo) (1 / eps)) puts them in cells
    k - 1 and k + 1 — the rounding of a - lo (lo = -1000.1 is on a coarser
    lattice than the rows at 3 .. 800) and of the product alone does that, for
    nearly one candidate in two; the kept pairs are thinned to 8 cells apart.
    Under the real width the two are one cell apart.  One anchor row fixes lo;
    the other coordinates stay inside one cell."""
    dtype = np.dtype("float64")
    eps = EPS
    thr = threshold(eps, metric)
    lo = -1000.1
    inv0 = 1.0 / eps
    k = int(np.ceil(-lo * inv0)) + 64 + np.arange(1 << 14, dtype=np.int64)
    b = (lo + k.astype(np.float64) / inv0).astype(dtype)
    a1, f1 = _walk_largest(b, lambda v: cells(v, lo, inv0) < k, True)
    a2, f2 = _walk_largest((a1 + eps).astype(dtype),
                           lambda v: pair_acc(a1[:, None], v[:, None], metric) <= thr, True)
    hit = f1 & f2 & (cells(a1, lo, inv0) == k - 1) & (cells(a2, lo, inv0) == k + 1)
    hits, last = [], -8
    for i in np.flatnonzero(hit):
        if i - last >= 8 and len(hits) < n_pairs:
            hits.append(i)
            last = i
    hits = np.array(hits, np.int64)
    rows, groups, role = [], [], []

    def point(v, g, r):
        p = np.array([eps * 0.05 * ((g + 3 * j) % 4) for j in range(d)])
        p[axis] = v
        rows.append(p)
        groups.append(g)
        role.append(r)

    anchor = np.zeros(d)
    anchor[axis] = lo
    rows.append(anchor)
    groups.append(0)
    role.append(3)
    for g, i in enumerate(hits):
        point(a1[i], g + 1, 0)
        point(a2[i], g + 1, 1)
    X = np.array(rows, dtype)
    perm = np.random.default_rng([53, d, axis]).permutation(len(X))
    return _case("slack_edge", (d, axis, metric), _frozen(np.ascontiguousarray(X[perm])),
                 _frozen(np.array(groups)[perm]), _frozen(np.array(role)[perm]), eps, metric, k=2,
                 a1=_frozen(a1[hits]), a2=_frozen(a2[hits]), candidates=len(k), hits=int(hit.sum()),
                 inv_no_slack=inv0, axis=axis)


# ---------------------------------------------------------------- c. key width
KEY_SHAPES = {
    "2d_below": (65536, 65535),            # G = 2^32 - 65536: 4-byte keys
    "2d_first8": (65535, 65537),           # G = 2^32 - 1: the first value with 8-byte keys
    "2d_pow": (65536, 65536),              # G = 2^32
    "2d_over": (65536, 65552),             # sixteen rows of cells whose keys pass bit 31
    "3d_first8": (255, 257, 65537),        # G = 2^32 - 1
}


@functools.lru_cache(maxsize=None)
def key_width(shape, dtype="float64", metric="euclidean", per=6):
    """A grid of exactly KEY_SHAPES[shape] cells.  Straddling groups in the
    first and the last rows of cells (keys near 0 and near G - 1), in the
    middle, and — 2d_over — in rows c and c + 65536 of the last axis at the
    same other coordinates, whose keys differ by exactly 2^32.  Q: the rows,
    and twins of the far-face rows one cell outside the far faces."""
    dtype = np.dtype(dtype)
    ncw = np.array(KEY_SHAPES[shape], np.int64)
    d = len(ncw)
    eps = EPS
    lo, hi = _box(dtype, np.full(d, 1.5), ncw, eps, 1.0, 0.5)
    inv = ga.cell_inv(eps, 1.0)
    L = d - 1                                 # the axis with the largest stride
    want, cross, side, sgn, delta = [], [], [], [], []
    # (row of cells on the last axis, side crossed, at the far end of axis 0)
    rows_L = [(0, 1, False), (int(ncw[L]) - 1, -1, True), (int(ncw[L]) // 2, 1, False)]
    if shape == "2d_over":
        rows_L = [(0, 1, False), (65536, 1, False), (9, -1, False), (65536 + 9, -1, False),
                  (int(ncw[L]) - 1, -1, True), (int(ncw[L]) // 2, 1, False)]
    for cL, sd, far_end in rows_L:
        for i in range(per):
            w = np.ones(d, np.int64)
            w[0] = int(ncw[0]) - 6 - 8 * i if far_end else 5 + 8 * i
            w[L] = cL
            want.append(w)
            cross.append(L)
            side.append(sd)
            sgn.append(1 if i % 2 == 0 else -1)
            delta.append(ga.CHORD_DELTAS[(3 * i) % len(ga.CHORD_DELTAS)])
    q, nb, twin, ok = straddle(dtype, metric, eps, lo, inv, np.array(want), cross, side, 0, sgn,
                               delta)
    keep = np.flatnonzero(ok)
    X, groups, role = _assemble(dtype, [lo, hi], q, nb, twin, keep,
                                [37, sorted(KEY_SHAPES).index(shape), dtype.itemsize])
    # query twins one cell outside the far faces: the rows of the last row of cells
    cw = ga.cell_width(eps)
    far = X[(row_cells(X, lo.astype(np.float64), inv)[:, L] == ncw[L] - 1) & (role != 3)]
    outs = []
    for j in range(d):
        t = far.astype(np.float64).copy()
        t[:, j] = float(hi[j]) + (0.75 + 0.5 * (np.arange(len(t)) % 2)) * cw
        outs.append(t.astype(dtype))
    Q = np.concatenate([X] + outs)
    return _case("key_width", (shape, dtype.name, metric), X, groups, role, eps, metric, k=2, Q=Q,
                 q=_frozen(q[keep]), n_in=_frozen(nb[keep]), n_out=_frozen(twin[keep]),
                 enumerated=len(ok), want=np.array(want)[keep], shape=tuple(int(v) for v in ncw))


# ---------------------------------------------------------------- d. faces
FACE_LEVELS = ("near", "below", "at", "above")


def _outward(dtype, metric, eps, row, base, axis, out_sign):
    """Queries outside the box along `axis` of face row `row` (base: the other
    coordinates, already displaced): half a radius out, and the largest
    distance at which `row` is still accepted with one step less and one more.
    -> (4, d) in FACE_LEVELS order, found."""
    dtype = np.dtype(dtype)
    thr = threshold(eps, metric)
    b = np.array(base, dtype)[None, :]
    r = np.array(row, dtype)[None, :]
    rest = float(pair_acc(np.where(np.arange(b.shape[1]) == axis, r, b), r, metric)[0])
    room = max(thr - rest, 0.0)
    dx = np.sqrt(room) if metric == "euclidean" else room
    start = np.array([float(r[0, axis]) + out_sign * dx]).astype(dtype)

    def accepted(v):
        t = b.copy()
        t[0, axis] = v[0]
        return pair_acc(t, r, metric) <= thr

    v, f = _walk_largest(start, accepted, np.array([out_sign > 0]))
    up = np.array([out_sign > 0])
    vals = [np.array([float(r[0, axis]) + out_sign * 0.5 * dx]).astype(dtype)[0],
            _step(v, ~up)[0], v[0], _step(v, up)[0]]
    out = np.repeat(b, 4, axis=0)
    out[:, axis] = vals
    return out, bool(f[0]) and rest <= thr


@functools.lru_cache(maxsize=None)
def faces(dtype, d, metric, kind="box"):
    """Queries that are not rows.  kind = "box": rows on every face of a box of
    6 cells per axis (its two corners among them) and a few inside; queries
    outside each face along its axis, and outside the two corners on every
    axis at once, at the four FACE_LEVELS; and queries more than one cell out,
    which must get nothing.  "plane": every row shares coordinate 0 (one cell
    on that axis), queries off the plane on both sides.  "single": one row.
    "twins": two identical rows."""
    dtype = np.dtype(dtype)
    eps = EPS
    cw = ga.cell_width(eps)
    rng = np.random.default_rng([41, d, dtype.itemsize, 0 if metric == "euclidean" else 1,
                                 FACE_KINDS.index(kind)])
    if kind == "box":
        lo, hi = _box(dtype, np.full(d, 3.75), np.full(d, 6), eps, 1.0, 1.0 - 2.0 ** -22)
    else:
        lo, hi = _box(dtype, np.full(d, 3.75), np.full(d, 6), eps, 1.0, 0.5)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    rows, Q, level, expect_none, src, axis_of = [], [], [], [], [], []
    if kind == "box":
        rows += [lo, hi]
        for j in range(d):
            for sd, face in ((-1, lo64[j]), (1, hi64[j])):
                for _ in range(2 if d > 1 else 0):
                    p = lo64 + rng.uniform(0.2, 0.8, size=d) * (hi64 - lo64)
                    p[j] = face
                    rows.append(p.astype(dtype))
        for _ in range(4):
            rows.append((lo64 + rng.uniform(0.3, 0.7, size=d) * (hi64 - lo64)).astype(dtype))
    elif kind == "plane":
        if d < 2:
            raise ValueError("a plane needs d >= 2")
        for i in range(12):
            p = lo64 + rng.uniform(0.0, 1.0, size=d) * (hi64 - lo64)
            p[0] = lo64[0]
            rows.append(p.astype(dtype))
    elif kind == "single":
        rows.append(lo)
    elif kind == "twins":
        rows += [lo, lo.copy()]
    else:
        raise ValueError(kind)
    rows = np.array(rows, dtype)
    found = True
    for ri, r in enumerate(rows):
        for j in range(d):
            for sd in (-1, 1):
                on_face = (kind != "box") or (sd < 0 and r[j] == lo[j]) or (sd > 0 and r[j] == hi[j])
                if not on_face:
                    continue
                qs, f = _outward(dtype, metric, eps, r, r, j, sd)
                found &= f
                Q += list(qs)
                level += list(range(4))
                expect_none += [False, False, False, False]
                src += [ri] * 4
                axis_of += [j] * 4
    if kind == "box":
        # the corners: outside on every axis at once, the last axis walked
        for ri, (r, sd) in enumerate(((lo, -1), (hi, 1))):
            for rep in range(3):
                base = r.astype(np.float64) + sd * eps * rng.uniform(0.05, 0.45, size=d) / max(1, d - 1)
                qs, f = _outward(dtype, metric, eps, r, base.astype(dtype), d - 1, sd)
                found &= f
                Q += list(qs)
                level += list(range(4))
                expect_none += [False] * 4
                src += [ri] * 4
                axis_of += [d - 1] * 4
    # far queries: more than one cell outside (s < -1, s >= nc + 1)
    for r in rows[:8]:
        for j in range(d):
            for sd, far in ((-1, 1.0 + 2.0 ** -10), (-1, 2.5), (1, 1.0 + 2.0 ** -10), (1, 2.5)):
                t = r.astype(np.float64).copy()
                t[j] = (lo64[j] - far * cw) if sd < 0 else \
                    (rows[:, j].astype(np.float64).max() + far * cw)
                # (beyond the last cell's end, not only beyond the last row)
                if sd > 0:
                    t[j] += cw
                Q.append(t.astype(dtype))
                level.append(4)
                expect_none.append(True)
                src.append(-1)
                axis_of.append(j)
    Q = np.array(Q, dtype)
    X = _frozen(np.ascontiguousarray(rows))
    return _case("faces", (dtype.name, d, metric, kind), X, _frozen(np.arange(len(X))),
                 _frozen(np.full(len(X), 3)), eps, metric, k=1, Q=Q, level=np.array(level),
                 expect_none=np.array(expect_none), found=found, src=np.array(src),
                 axis=np.array(axis_of))


FACE_KINDS = ("box", "plane", "single", "twins")


# ---------------------------------------------------------------- e. k shell
def _neighbour_cells(d):
    """The 3^d - 1 offsets to the neighbour cells, in a fixed order."""
    out = []
    for c in range(3 ** d):
        o = [(c // 3 ** j) % 3 - 1 for j in range(d)]
        if any(o):
            out.append(o)
    return out


@functools.lru_cache(maxsize=None)
def k_shell(dtype, d, metric, ks=KS, reps=2):
    """Per k of `ks`, `reps` queries each with k - 1 rows at the largest offset
    the predicate accepts (spread over the query's neighbour cells, as many
    different ones as the dimension has) and their k - 1 twins one step out:
    with the query itself exactly k rows qualify.  Row i of a shell is displaced
    on the axes j < d - 1 by a fixed fraction of eps towards its cell and walked
    along the last axis.  -> case; shell[g] = (k, query row, in rows, out rows)."""
    dtype = np.dtype(dtype)
    eps = EPS
    thr = threshold(eps, metric)
    cw = ga.cell_width(eps)
    # the neighbour cells a row within eps of a query at its cell's middle can be
    # in: half a cell on every crossed axis (cityblock: one axis; euclidean: two
    # before the last, which leaves 0.66 of a cell for the last)
    ncell = [o for o in _neighbour_cells(d)
             if (sum(map(abs, o)) <= 1 if metric == "cityblock" else sum(map(abs, o[:-1])) <= 2)]
    n_sh = len(ks) * reps
    per_row = 8
    span = np.full(d, 8.0)
    span[0] = 8.0 * (min(n_sh, per_row) + 1)
    if d > 1:
        span[1] = 8.0 * ((n_sh + per_row - 1) // per_row + 1)
    lo, hi = _box(dtype, np.full(d, -2.25), span, eps, 1.0, 0.5)
    lo64 = lo.astype(np.float64)
    rows, groups, role = [lo, hi], [0, 1], [3, 3]
    shell = []
    found = True
    rng = np.random.default_rng([43, d, dtype.itemsize, 0 if metric == "euclidean" else 1])
    for s in range(n_sh):
        k = ks[s // reps]
        cq = np.full(d, 4, np.int64)
        cq[0] = 4 + 8 * (s % per_row)
        if d > 1:
            cq[1] = 4 + 8 * (s // per_row)
        q = (lo64 + (cq + 0.5) * cw).astype(dtype)
        iq = len(rows)
        rows.append(q)
        groups.append(s + 2)
        role.append(0)
        ins, outs = [], []
        G = k - 1
        if G:
            off = np.array([ncell[i % len(ncell)] for i in range(G)], np.float64)
            base = np.repeat(q[None, :].astype(np.float64), G, axis=0)
            # the axes before the last: 0.51 .. 0.53 of a cell towards the cell where
            # it is another one (q sits at the middle of its own, so the row leaves
            # it), a small fraction of a cell otherwise
            fr = np.where(off[:, :-1] != 0, 0.51 + 0.02 * rng.uniform(size=(G, d - 1)),
                          0.0) * off[:, :-1] + \
                np.where(off[:, :-1] == 0, 0.03 * rng.uniform(-1, 1, size=(G, d - 1)), 0.0)
            base[:, :-1] += fr * cw
            nb = base.astype(dtype)
            qq = np.repeat(q[None, :], G, axis=0)
            rest = pair_acc(np.concatenate([nb[:, :-1], qq[:, -1:]], axis=1), qq, metric)
            room = np.maximum(thr - rest, 0.0)
            dx = np.sqrt(room) if metric == "euclidean" else room
            sg = np.where(off[:, -1] != 0, off[:, -1], np.where(np.arange(G) % 2 == 0, 1.0, -1.0))
            start = (qq[:, -1].astype(np.float64) + sg * dx).astype(dtype)

            def accepted(v, nb=nb, qq=qq):
                t = nb.copy()
                t[:, -1] = v
                return pair_acc(qq, t, metric) <= thr

            v, f = _walk_largest(start, accepted, sg > 0)
            found &= bool(f.all()) and bool((rest <= thr).all())
            nb[:, -1] = v
            tw = nb.copy()
            tw[:, -1] = _step(v, sg > 0)
            for i in range(G):
                ins.append(len(rows))
                rows.append(nb[i])
                outs.append(len(rows))
                rows.append(tw[i])
                groups += [s + 2, s + 2]
                role += [1, 2]
        shell.append((k, iq, np.array(ins, np.int64), np.array(outs, np.int64)))
    X = np.array(rows, dtype)
    perm = np.random.default_rng([47, d]).permutation(len(X))
    inv_perm = np.argsort(perm)
    shell = [(k, int(inv_perm[iq]), inv_perm[ins], inv_perm[outs]) for k, iq, ins, outs in shell]
    return _case("k_shell", (dtype.name, d, metric, tuple(ks), reps),
                 _frozen(np.ascontiguousarray(X[perm])), _frozen(np.array(groups)[perm]),
                 _frozen(np.array(role)[perm]), eps, metric, k=2, shell=shell, found=found)


def shell_weights(case, heavy=8.0):
    """Dyadic weights for the weighted variant: the query 1, its in rows 1/2
    (one of them 1 where their number is odd), the twins `heavy`: taken
    nearest first the running sum reaches ms(k) = 1 + ceil((k - 1) / 2) exactly
    on the last in row.  -> (weights, {k: ms})."""
    w = np.ones(len(case["X"]))
    ms = {}
    for k, iq, ins, outs in case["shell"]:
        w[ins] = 0.5
        if len(ins) % 2:
            w[ins[0]] = 1.0
        w[outs] = heavy
        ms[k] = 1 + (k - 1 + 1) // 2
    return w, ms


# ---------------------------------------------------------------- f. screen band
@functools.lru_cache(maxsize=None)
def screen(d, metric):
    r = screen_band_detail(d, metric)
    role = np.zeros(len(r["X"]), np.int64)
    return _case("screen", (d, metric), r["X"], r["groups"], _frozen(role), r["eps"], metric, k=2,
                 mis=r["mis"], edge=r["edge"])


# ---------------------------------------------------------------- g. scaled goldens
def scaled(name, dtype, s):
    """(X, X0, eps, eps0, metric, min_samples, labels, core, counts) of the
    golden times 2^s."""
    return scaled_golden_detail(name, int(s), np.dtype(dtype).name)


def scaling_is_exact(name, dtype, s, sample=1500):
    """The numpy reference on a seeded sample of the rows: every accumulator
    within the unscaled threshold scales to ldexp(acc, 2 s) (cityblock: s)
    exactly, every other one stays beyond the scaled threshold, and the scaled
    threshold is a normal number."""
    r = scaled(name, dtype, s)
    n = len(r["X"])
    pick = np.sort(np.random.default_rng(5).choice(n, min(n, sample), replace=False))
    e = 2 * s if r["metric"] == "euclidean" else s
    a0 = kdist_ref.accumulators(r["X0"][pick], r["X0"][pick], r["metric"])
    a1 = kdist_ref.accumulators(r["X"][pick], r["X"][pick], r["metric"])
    t0, t1 = threshold(r["eps0"], r["metric"]), threshold(r["eps"], r["metric"])
    inside = a0 <= t0
    tiny = np.finfo(np.float64).tiny
    return bool(np.isfinite(t1) and t1 >= tiny and t1 == np.ldexp(t0, e)
                and np.array_equal(a1[inside], np.ldexp(a0[inside], e))
                and (a1[~inside] > t1).all()
                and ((a1[inside] == 0) | (a1[inside] >= tiny)).all())


# ---------------------------------------------------------------- h. the tile kernels
@functools.lru_cache(maxsize=None)
def tile_ties(d, dtype, n_islands=12, offset=0):
    """dense_adversarial.tie_islands (accumulators of exactly 9 and exactly 10)
    as an index over its rows at r_max = 3."""
    Z, X, joined, probes = da.tie_islands(d, n_islands, offset, dtype)
    return _case_dense("tile_ties", (d, np.dtype(dtype).name, n_islands, offset), X, da.TIE_EPS,
                       k=da.TIE_MIN_SAMPLES)


@functools.lru_cache(maxsize=None)
def tile_shell(d, dtype, r_log2=-3, n_pairs=600):
    """dense_adversarial.shell_pairs: partners at eps (1 +- 2^-k)."""
    X, eps = da.shell_pairs(d, dtype, r_log2, n_pairs)
    return _case_dense("tile_shell", (d, np.dtype(dtype).name, r_log2, n_pairs), X, eps, k=2)


@functools.lru_cache(maxsize=None)
def tile_counts(d, dtype, n_rows, n_queries):
    """n_rows integer rows of which only the LAST lies near the queries, at an
    accumulator of exactly 9 = thr (r_max = 3) from every even query and of 10
    from every odd one; the others are >= 100 away.  Row counts around the tile
    (64 rows), query counts around the block (64 / 128 / 256 lanes)."""
    X = np.zeros((n_rows, d), np.float64)
    i = np.arange(n_rows - 1)
    X[:-1, 1] = 100.0 + 10.0 * i
    X[:-1, d - 1] = -50.0 - (i % 7)
    X[-1, 0] = 3.0
    Q = np.zeros((n_queries, d), np.float64)
    Q[1::2, d - 2] = 1.0
    X, Q = X.astype(dtype), Q.astype(dtype)
    return _case_dense("tile_counts", (d, np.dtype(dtype).name, n_rows, n_queries), X, 3.0, k=1,
                       Q=Q)


def _case_dense(fam, key, X, eps, k, Q=None, metric="euclidean"):
    X = _frozen(np.ascontiguousarray(X))
    return dict(family=fam, key=(fam,) + tuple(key), X=X, Q=X if Q is None else _frozen(Q),
                groups=None, role=None, r_max=float(eps), metric=metric, k=k)


# ---------------------------------------------------------------- the references
def table(Q, X, metric):
    """kdist_ref.accumulators over tiles within its cap: the full m x n table."""
    T = kdist_ref.MAX_N
    out = np.empty((len(Q), len(X)))
    for q0 in range(0, len(Q), T):
        for x0 in range(0, len(X), T):
            out[q0:q0 + T, x0:x0 + T] = kdist_ref.accumulators(Q[q0:q0 + T], X[x0:x0 + T], metric)
    return out


_REF = {}


def reference(case, radii=(), r_max=None, kmax=None, forest_k=None):
    """The brute-force answers of a case, computed once per (case, r_max) and
    read-only: pairs (knn_ref.smallest_pairs, uncapped, kmax columns),
    csr[radius] (radius_ref.from_accumulators), predict (brute_predict over
    the rows labelled by their numbers), forest (mreach_ref, rows only, d <= 4,
    at forest_k or the case's k)."""
    r_max = case["r_max"] if r_max is None else float(r_max)
    kmax = min(65, kmax or max(case["k"] + 1, 3))
    fk = case["k"] if forest_k is None else forest_k
    key = (case["key"], r_max, kmax, tuple(radii), fk)
    if key in _REF:
        return _REF[key]
    X, Q, metric = case["X"], case["Q"], case["metric"]
    acc = table(Q, X, metric)
    out = dict(pairs=tuple(_frozen(a) for a in knn_ref.smallest_pairs(acc, kmax)), csr={})
    for r in set(radii) | {r_max}:
        out["csr"][r] = tuple(_frozen(a) for a in radius_ref.from_accumulators(acc, r, metric))
    out["predict"] = _frozen(predict_ref.brute_predict(Q, X, np.arange(len(X)), r_max, metric))
    if X.shape[1] <= 4:
        xx = acc if Q is X else table(X, X, metric)
        out["forest"] = tuple(_frozen(np.asarray(a))
                              for a in mreach_ref.forest_of_table(xx, fk, r_max, metric))
    _REF[key] = out
    return out


def kdist_of(pairs, k, r_max, metric):
    """kdist from the pairs table: column k - 1 of knn_ref.cut."""
    return knn_ref.cut(pairs, k, r_max, metric)[1][:, k - 1]
