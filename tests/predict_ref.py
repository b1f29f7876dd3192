"""Brute-force reference of DBSCAN.predict and the query sets its tests use
(shared by test_predict_host.py, which pins the reference against the goldens
on the CPU, and test_gpu_predict.py).

    predict(q) = min { label(c) : c core, dist(q, c) <= eps }     (-1: none)

The distance is the train's predicate restated in numpy: fp64, one axis at a
time in axis order, the product and the sum rounded separately, compared with
``eps * eps`` (cityblock: ``eps``).  No ``np.sum(axis)`` / ``np.linalg.norm``:
their summation order is not the predicate's.
"""
import numpy as np

NO_LABEL = np.iinfo(np.int64).max


def brute_predict(Q, C, L, eps, metric="euclidean", chunk=256, spread=False):
    """Q (m, d) queries, C (k, d) core points, L (k,) their labels (>= 0).
    Returns int64 (m,): the smallest label among the cores within eps, -1 if
    none.  spread=True: also the largest such label (-1 if none)."""
    Q = np.asarray(Q, np.float64)
    C = np.asarray(C, np.float64)
    L = np.asarray(L, np.int64)
    if Q.ndim == 1:
        Q = Q.reshape(-1, 1)
    if C.ndim == 1:
        C = C.reshape(-1, 1)
    m, d = Q.shape
    eps = float(eps)
    thr = eps if metric == "cityblock" else eps * eps
    lo = np.full(m, -1, np.int64)
    hi = np.full(m, -1, np.int64)
    if len(C) == 0 or m == 0:
        return (lo, hi) if spread else lo
    for s in range(0, m, chunk):
        q = Q[s:s + chunk]
        acc = np.zeros((len(q), len(C)), np.float64)
        with np.errstate(over="ignore"):      # a far query's square may reach inf: no hit
            for j in range(d):
                t = q[:, j][:, None] - C[:, j][None, :]
                if metric == "cityblock":
                    acc = acc + np.abs(t)
                else:
                    acc = acc + t * t
        hit = acc <= thr
        mn = np.where(hit, L[None, :], NO_LABEL).min(axis=1)
        mx = np.where(hit, L[None, :], -1).max(axis=1)
        lo[s:s + chunk] = np.where(mn == NO_LABEL, -1, mn)
        hi[s:s + chunk] = mx
    return (lo, hi) if spread else lo


def make_queries(X, core, eps, m=4096, seed=7):
    """m queries in X's dtype, three kinds in equal parts (shuffled): uniform
    over the data box grown by 3 eps (some outside the cores' box), training
    points jittered by N(0, eps / 2), exact copies of core points."""
    X = np.asarray(X)
    rng = np.random.default_rng(seed)
    n, d = X.shape
    lo = X.min(axis=0).astype(np.float64) - 3.0 * eps
    hi = X.max(axis=0).astype(np.float64) + 3.0 * eps
    k = m // 3
    uni = rng.uniform(lo, hi, size=(m - 2 * k, d))
    jit = X[rng.integers(0, n, size=k)].astype(np.float64) + rng.normal(0.0, eps / 2.0, size=(k, d))
    cid = np.nonzero(np.asarray(core))[0]
    cop = X[cid[rng.integers(0, len(cid), size=k)]].astype(np.float64) if len(cid) else \
        rng.uniform(lo, hi, size=(k, d))
    Q = np.concatenate([uni, jit, cop]).astype(X.dtype)
    return np.ascontiguousarray(Q[rng.permutation(len(Q))])


def two_runs_1d():
    """Two 1-D runs 0..1 and 1.5..2.5 in steps of 0.01, eps 0.3: queries in
    [1.2, 1.3] lie within eps of both.  -> (X, eps, min_samples, Q)."""
    a = np.arange(0, 101) * 0.01
    b = 1.5 + np.arange(0, 101) * 0.01
    X = np.concatenate([a, b]).reshape(-1, 1)
    Q = np.concatenate([np.linspace(1.2, 1.3, 41), np.linspace(-1.0, 3.5, 200)]).reshape(-1, 1)
    return X, 0.3, 5, Q


def check_query_mix(lo, hi):
    """The conditions the out-of-sample tests put on their inputs: >= 5 % of
    the queries unassigned, >= 5 % assigned, one near two labels."""
    m = len(lo)
    assert (lo == -1).sum() >= 0.05 * m, ((lo == -1).sum(), m)
    assert (lo >= 0).sum() >= 0.05 * m, ((lo >= 0).sum(), m)
    return bool(((lo >= 0) & (hi != lo)).any())
