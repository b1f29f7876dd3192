#!/usr/bin/env python3
"""Generate the sample_weight fixtures tests/golden/sw_<case>.npz.

scikit-learn 1.7.2, DBSCAN(algorithm='kd_tree').fit(X, sample_weight=w) on the
fp64 upcast of each point set, as make_golden.py does for the unweighted
goldens.  X, eps, min_samples and metric come from the existing
ref_<name>.npz (blobs4d: synth.blobs_noise(5000, 4), eps 1.5, min_samples 5).
Each file holds the weights, sklearn's labels_ and its core mask.

Cases
  int03_<set>   integer weights 0..3, default_rng(7)
  dyadic_<set>  multiples of 1/8 in [0, 2.5], default_rng(11)
  frac_<set>    default_rng(0).uniform(0, 2, n): not multiples of 2^-20.  The
                script asserts that no point's weighted sum lies within 1e-4
                of min_samples (the fixed-point rule then provably agrees
                with sklearn: its bound is k * 2^-21, k neighbours) and that
                the fixed-point core set equals sklearn's.

The "sw_" prefix keeps the files out of golden_names() ("ref_*").

Usage:  python tests/golden/make_golden_weighted.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

INT03 = ["b2d_20k", "b3d_20k", "lattice_900", "dup_1d", "neg_3k", "ident_40", "c0",
         "c0_p5_cityblock", "blobs4d"]
DYADIC = ["b2d_20k", "b3d_20k"]
FRAC = ["b2d_20k", "b3d_20k"]
BLOBS4D = dict(n=5000, d=4, eps=1.5, min_samples=5, metric="euclidean")


def point_set(name):
    if name == "blobs4d":
        from pypardis_amd import synth
        c = BLOBS4D
        return synth.blobs_noise(c["n"], c["d"]), c["eps"], c["min_samples"], c["metric"]
    z = np.load(os.path.join(HERE, f"ref_{name}.npz"))
    return z["X"], float(z["eps"]), int(z["min_samples"]), str(z["metric"])


def weights(kind, n):
    if kind == "int03":
        return np.random.default_rng(7).integers(0, 4, n).astype(np.float64)
    if kind == "dyadic":
        return np.random.default_rng(11).integers(0, 21, n).astype(np.float64) / 8.0
    if kind == "frac":
        return np.random.default_rng(0).uniform(0.0, 2.0, n)
    raise ValueError(kind)


def main():
    import sklearn
    from sklearn.cluster import DBSCAN
    from sklearn.neighbors import NearestNeighbors
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    for kind, names in (("int03", INT03), ("dyadic", DYADIC), ("frac", FRAC)):
        for name in names:
            X, eps, ms, metric = point_set(name)
            X64 = np.asarray(X, np.float64)
            w = weights(kind, len(X64))
            m = DBSCAN(eps=eps, min_samples=ms, metric=metric, algorithm="kd_tree")
            m.fit(X64, sample_weight=w)
            core = np.zeros(len(X64), np.uint8)
            core[m.core_sample_indices_] = 1
            note = ""
            if kind == "frac":
                nn = NearestNeighbors(radius=eps, metric=metric, algorithm="kd_tree").fit(X64)
                nb = nn.radius_neighbors(X64, return_distance=False)
                sums = np.array([w[i].sum() for i in nb])
                gap = np.abs(sums - ms).min()
                assert gap > 1e-4, (name, gap)
                W = np.rint(w * 2.0 ** 20).astype(np.uint64)
                fx = np.array([W[i].sum(dtype=np.uint64) for i in nb]) >= np.uint64(ms << 20)
                assert np.array_equal(fx, core.astype(bool)), name
                note = f"  min |sum - min_samples| = {gap:.3g}"
            out = os.path.join(HERE, f"sw_{kind}_{name}.npz")
            np.savez_compressed(out, weight=w, sk_labels=m.labels_.astype(np.int64),
                                sk_core=core, eps=eps, min_samples=ms, metric=metric)
            print(f"{os.path.basename(out)}: n={len(X64)} clusters={m.labels_.max() + 1} "
                  f"core={int(core.sum())} zero-weight core={int((core.astype(bool) & (w == 0)).sum())}"
                  f"{note}")


if __name__ == "__main__":
    main()
