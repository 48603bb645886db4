"""CPU: the restatement of the classifier fit (tests/logreg_cpu.py) against the coefficients the reference ships, against
sklearn where it imports, its own optimality conditions, and the C-ABI additions (symbols, struct layout, defaults).

Bounds are ten times the value measured with this file (EXPERIMENTS.md "Fitting the classifiers"): the shipped numbers
carry six significant digits and the residual of the L-BFGS run that made them, so agreement cannot be exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import logreg_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP = np.load(os.path.join(ROOT, "tests", "golden", "model_parameters.npz"))
NEW = ["cfear_logreg_params_default", "cfear_logreg_fit_batch"]
FULL_ROWS = "/root/reference/tbv_slam/model_parameters/combined.txt"
SHIPPED_LOOP_BOUND = 4.8e-4          # measured 4.79e-5
SHIPPED_ALIGN_BOUND = 4.1e-2         # measured 4.02e-3, on a coefficient of -15.2
SKLEARN_COEF_BOUND = 1.7e-8          # measured 1.63e-9 (sklearn 1.7.2 lbfgs, tol 1e-12, on the well-scaled set)
KKT_BOUND = 7.5e-8                   # measured 7.47e-9 (combined_head; 2.2e-11 loop_rows, 1.5e-13 synthetic): |gradient| / largest term of its sums


def _xy(rows):
    return rows[:, 1:], rows[:, 0]


def _vec(c):
    return np.concatenate([[c["intercept"]], c["coef"]])


def _sets():
    return {"loop_rows": _xy(MP["loop_rows"]), "combined_head": _xy(MP["combined_head"]), "synthetic": R.synthetic(11, 3000, 4)}


def test_loop_rows_land_on_the_shipped_loop_classifier():
    c = R.fit(*_xy(MP["loop_rows"]))
    d = np.abs(_vec(c) - MP["loop"]).max()
    print("restatement vs trained_loop_classifier.txt: %.3e after %d iterations" % (d, c["iterations"]))
    assert c["status"] == R.OK and d <= SHIPPED_LOOP_BOUND


@pytest.mark.skipif(not os.path.exists(FULL_ROWS), reason="the reference's 58 071 training rows are not on this machine")
def test_full_alignment_rows_land_on_the_shipped_alignment_classifier():
    rows = np.array([[float(t) for t in ln.split(",")] for ln in open(FULL_ROWS) if ln.strip()])
    assert rows.shape == (int(MP["combined_rows"][0]), 7)
    c = R.fit(*_xy(rows))
    d = np.abs(_vec(c) - MP["align"]).max()
    print("restatement vs trained_alignment_classifier.txt: %.3e after %d iterations" % (d, c["iterations"]))
    assert c["status"] == R.OK and d <= SHIPPED_ALIGN_BOUND


@pytest.mark.parametrize("name", ["loop_rows", "combined_head", "synthetic"])
def test_objective_is_not_above_sklearns(name):
    """The restatement is the minimiser, so F at its coefficients cannot exceed F at anybody else's, up to the rounding of F
    itself: a sum of n non-negative terms, 4 n eps relative."""
    sk = pytest.importorskip("sklearn.linear_model")
    X, y = _sets()[name]
    c = R.fit(X, y)
    clf = sk.LogisticRegression(class_weight="balanced", max_iter=1000).fit(X, y)
    F_sk = R.objective(X, y, np.asarray(clf.coef_[0], np.float64), float(clf.intercept_[0]))
    print("%s: F restatement %.15g, F sklearn %.15g, coefficient distance %.3e" %
          (name, c["objective"], F_sk, np.abs(_vec(c) - np.concatenate([clf.intercept_, clf.coef_[0]])).max()))
    assert c["status"] == R.OK and c["objective"] <= F_sk * (1.0 + 4 * X.shape[0] * np.finfo(np.float64).eps)


def test_coefficients_agree_with_a_tightened_sklearn_on_well_scaled_rows():
    sk = pytest.importorskip("sklearn.linear_model")
    X, y = _sets()["synthetic"]
    c = R.fit(X, y)
    clf = sk.LogisticRegression(class_weight="balanced", max_iter=10000, tol=1e-12).fit(X, y)
    d = np.abs(_vec(c) - np.concatenate([clf.intercept_, clf.coef_[0]])).max()
    print("restatement vs sklearn (tol 1e-12): %.3e" % d)
    assert d <= SKLEARN_COEF_BOUND


@pytest.mark.parametrize("name", ["loop_rows", "combined_head", "synthetic"])
def test_gradient_vanishes_at_the_result(name):
    X, y = _sets()[name]
    c = R.fit(X, y)
    g, scale = R.gradient(X, y, c["coef"], c["intercept"], dtype=np.longdouble)
    print("%s: |gradient| %.3e, largest term %.3e, ratio %.3e" % (name, float(np.abs(g).max()), scale, float(np.abs(g).max()) / scale))
    assert float(np.abs(g).max()) <= KKT_BOUND * scale
    assert abs(c["grad_inf"] - float(np.abs(g).max())) <= 1e-13 * X.shape[0] * scale


def test_refusals_and_options_of_the_restatement():
    X, y = R.synthetic(5, 200, 3)
    assert R.fit(X, np.ones(200))["status"] == R.ERR_INVALID_ARGUMENT
    assert R.fit(X[:0], y[:0])["status"] == R.ERR_INVALID_ARGUMENT
    bad = y.copy()
    bad[3] = 2.0
    assert R.fit(X, bad)["status"] == R.ERR_INVALID_ARGUMENT
    Xn = X.copy()
    Xn[0, 0] = np.inf
    assert R.fit(Xn, y)["status"] == R.ERR_INVALID_ARGUMENT
    assert R.fit(X, y, max_iterations=1)["status"] == R.ERR_SOLVER
    c = R.fit(X, y, fit_intercept=False, balanced=False, C=0.25)
    assert c["status"] == R.OK and c["intercept"] == 0.0
    g, scale = R.gradient(X, y, c["coef"], 0.0, C=0.25, balanced=False, fit_intercept=False, dtype=np.longdouble)
    assert float(np.abs(g).max()) <= KKT_BOUND * scale
    z = np.array([-800.0, -30.0, 0.0, 30.0, 800.0])
    assert np.isfinite(R.softplus(z)).all() and R.softplus(z)[0] == 0.0 and R.softplus(z)[4] == 800.0
    assert (R.sigmoid(z) == [0.0, R.sigmoid(z)[1], 0.5, R.sigmoid(z)[3], 1.0]).all()


def test_the_ragged_batch_covers_what_it_says():
    sets = R.ragged_batch()
    assert len(sets) == 256 and {X.shape[1] for X, _ in sets} == set(range(1, 9))
    n = [X.shape[0] for X, _ in sets]
    assert min(n) == 50 and max(n) == 20000
    X, y = sets[2]                                             # separable: some w splits the classes
    c = R.fit(X, y)
    assert c["status"] == R.OK and c["confusion"][1] == 0 and c["confusion"][2] == 0
    X, y = sets[6]                                             # near-degenerate: two columns nearly equal
    assert np.corrcoef(X[:, 0], X[:, 1])[0, 1] > 0.999 and R.fit(X, y)["status"] == R.OK


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_built_and_struct_layout():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
    assert C.sizeof(L.LogregParams) == 24 and L.LogregParams.max_iterations.offset == 16
    assert C.sizeof(L.LogregJob) == 48 and L.LogregJob.n_rows.offset == 32 and L.LogregJob.n_features.offset == 44
    d = L.LOGREG_RESULT_DTYPE
    assert d.itemsize == 152 and [d.fields[k][1] for k in ("intercept", "coef", "objective", "grad_inf", "balanced_accuracy", "n_used",
                                                            "n_pos", "confusion", "iterations", "status")] == [0, 8, 72, 80, 88, 96, 104, 112, 144, 148]
    assert "} cfear_logreg_result;                  /* 152 bytes */" in hdr and "#define CFEAR_LOGREG_MAX_FEATURES 8" in hdr
    assert lib.cfear_abi_version() == 1


def test_defaults_are_the_reference_settings():
    from tbv_slam_public_amd import _lib as L, api
    p = L.LogregParams(C=9.0, class_weight_balanced=9, fit_intercept=9, max_iterations=9, pad=9)
    L.lib().cfear_logreg_params_default(C.byref(p))
    assert (p.C, p.class_weight_balanced, p.fit_intercept, p.max_iterations, p.pad) == (1.0, 1, 1, 100, 0)
    assert api.logreg_params(max_iterations=7).max_iterations == 7
    with pytest.raises(KeyError):
        api.logreg_params(nonsense=1)
    assert all(hasattr(api.LogisticRegression, m) for m in ("fit", "fit_device"))
    assert all(hasattr(api.ScanLearningInterface, m) for m in ("FitModels", "FitModelsDevice", "AddTrainingData", "AddTrainingDataBatch"))


def test_cpp_mirror_compiles_with_and_without_the_standins(tmp_path):
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    for name, extra in (("plain", []), ("standin", ["-I", os.path.join(ROOT, "tests", "cpp", "standin")])):
        exe = str(tmp_path / ("logreg_signature_" + name))
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + extra +
                              [os.path.join(ROOT, "tests", "cpp", "logreg_signature.cpp"), "-o", exe, "-L", so_dir,
                               "-lcfear_hip", "-Wl,-rpath," + so_dir])
        assert os.path.exists(exe)
