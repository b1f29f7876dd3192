"""sample_weight, the parts that need no GPU: the brute-force reference
(weighted_ref.py) against scikit-learn's weighted fit on the small fixtures,
the C ABI's three weighted entry points, and the argument checks that run
before the first device call."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from weighted_ref import fixed_point, weighted_dbscan

SMALL = ["lattice_900", "dup_1d", "neg_3k", "ident_40", "c0", "c0_p5_cityblock"]
WEIGHTED = ["pd_cluster_weighted", "pd_train_weighted", "pd_train_tree_weighted"]


@pytest.mark.parametrize("name", SMALL)
def test_reference_equals_sklearn(name):
    g = load_golden(name)
    f = load_golden(f"int03_{name}", prefix="sw")
    metric = "cityblock" if str(g["metric"]) == "cityblock" else "euclidean"
    assert float(f["eps"]) == float(g["eps"]) and int(f["min_samples"]) == int(g["min_samples"])
    lab, core = weighted_dbscan(g["X"], float(g["eps"]), int(g["min_samples"]), f["weight"],
                                metric)
    assert np.array_equal(core, f["sk_core"].astype(bool))
    assert np.array_equal(lab, f["sk_labels"])
    # the fixture tells weighted from unweighted
    assert not np.array_equal(f["sk_core"], g["sk_core"]) or name == "ident_40"


def test_fixed_point_rule():
    u = 2.0 ** -20
    w = np.array([0.0, u / 2, 1.5 * u, 2.5 * u, 1.0, 1 - u, 2.0 ** 31, 0.3])
    assert fixed_point(w).tolist() == [0, 0, 2, 2, 1 << 20, (1 << 20) - 1, 1 << 51,
                                       int(np.rint(0.3 * 2 ** 20))]
    for bad in (-1e-300, np.nan, np.inf, 2.0 ** 31 * (1 + 2.0 ** -52)):
        with pytest.raises(ValueError):
            fixed_point(np.array([1.0, bad]))


def test_fixture_files_keep_out_of_the_unweighted_goldens():
    from conftest import golden_names, rotation_names
    assert not [n for n in golden_names() + rotation_names() if "int03" in n or "frac" in n]
    assert len([f for f in os.listdir(os.path.join(REPO, "tests", "golden"))
                if f.startswith("sw_")]) >= 13


# ------------------------------------------------------------ C ABI
def _declared():
    txt = open(os.path.join(REPO, "include", "pardis.h")).read()
    return sorted(set(re.findall(r"^\w[\w\s\*]*?\b(pd_\w+)\s*\(", txt, re.M)))


def test_header_and_binding_cover_the_weighted_entry_points():
    from pypardis_amd import _native
    syms = _declared()
    for s in WEIGHTED:
        assert s in syms and s in _native.EXPORTS
    assert sorted(_native.EXPORTS) == syms
    txt = open(os.path.join(REPO, "include", "pardis.h")).read()
    assert re.search(r"#define\s+PD_ABI_VERSION\s+3\b", txt)


def test_library_exports_the_weighted_entry_points():
    from pypardis_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    for s in WEIGHTED:
        assert hasattr(lib, s), s


def test_weighted_twins_take_the_unweighted_arguments():
    """Same argument list as the unweighted twin: `const double* weight` stands
    where `uint32_t* counts` stood (a pointer for a pointer)."""
    txt = open(os.path.join(REPO, "include", "pardis.h")).read()

    def args(name):
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, txt)
        return [" ".join(a.split()) for a in m.group(1).split(",")]

    for s in WEIGHTED:
        a, b = args(s[:-len("_weighted")]), args(s)
        assert len(a) == len(b)
        diff = [(x, y) for x, y in zip(a, b) if x != y]
        assert diff == [("uint32_t* counts", "const double* weight")], (s, diff)


# ------------------------------------------------------------ argument checks
def test_multi_device_trains_reject_weights_before_any_device_work():
    from pypardis_amd import DBSCAN
    X = np.zeros((10, 2), np.float32)
    w = np.ones(10)
    with pytest.raises(ValueError, match="n_gpus"):
        DBSCAN(eps=0.1, n_gpus=2).train(X, sample_weight=w)
    with pytest.raises(ValueError, match="group"):
        DBSCAN(eps=0.1, group="world").fit_predict(X, sample_weight=w)


def test_native_rejects_host_weights():
    """The binding takes device tensors only: a host tensor raises before
    the library is entered."""
    import torch
    from pypardis_amd import _native

    class FakeX:   # stands in for a device tensor: _check_weight reads no more
        device = torch.device("cpu")
        shape = (10, 2)

    with pytest.raises(TypeError):
        _native._check_weight(torch.ones(10, dtype=torch.float64), FakeX(), False)
    with pytest.raises(TypeError):
        _native._check_weight(np.ones(10), FakeX(), False)
