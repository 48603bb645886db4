"""GPU: cfear_logreg_fit_batch and the mirrors over it against the NumPy restatement (tests/logreg_cpu.py).

Every comparison of coefficients is max |device - restatement| over (intercept, coef), bounded per set by ten times the first
deviation measured on an MI355X (BOUND; EXPERIMENTS.md "Fitting the classifiers" records the measurements).  The two
sides minimise the same strictly convex F with the same iteration; they differ in the order of the row sums, so the
deviation is the rounding of the sums pushed through the inverse Hessian -- largest where F has a nearly flat direction."""
import os
import subprocess

import numpy as np
import pytest

from tests import logreg_cpu as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP = np.load(os.path.join(ROOT, "tests", "golden", "model_parameters.npz"))
SHIPPED_LOOP_BOUND = 4.8e-4          # tests/test_logreg_cpu.py: ten times the restatement's 4.8e-5 against the shipped file
# ten times the first measured max |device - restatement|: 1.243e-14, 1.457e-13 (the six-feature model; 5.3e-15 and 8.0e-14 for
# columns 1-3 and 4-6), 1.510e-8 (model 101 of the ragged batch, 424 x 6 with 3 % positives).  The folds are held to the bound
# of the rows they are cut from (measured 7.1e-15); the large-logit set is of the ragged batch's family (R.synthetic, plain)
# and is held to that batch's bound (measured 1.4e-17).
BOUND = {"loop_rows": 1.3e-13, "combined_head": 1.5e-12, "ragged": 1.6e-7}
BOUND["folds"], BOUND["large_logits"] = BOUND["loop_rows"], BOUND["ragged"]
HEAD_COLUMNS = ([1, 2, 3, 4, 5, 6], [1, 2, 3], [4, 5, 6])          # combined, CorAl, CFEAR: column 0 of a row is y


def _vec(r, d):
    return np.concatenate([[r["intercept"]], r["coef"][:d]])


def _cpu_vec(c):
    return np.concatenate([[c["intercept"]], c["coef"]])


def _dev(jobs, **kw):
    from tbv_slam_public_amd import api
    return api.logreg_fit_batch(jobs, **kw)


def _xy(rows):
    return np.ascontiguousarray(rows[:, 1:]), np.ascontiguousarray(rows[:, 0])


def _check(name, dev, cpu):
    print("max |device - restatement| %s: %.3e (bound %.3e)" % (name, dev, BOUND[name]))
    assert cpu >= 0 and dev <= BOUND[name], (name, dev, BOUND[name])


def test_loop_rows_against_the_restatement_and_the_shipped_coefficients():
    X, y = _xy(MP["loop_rows"])
    r = _dev([(X, y)])[0]
    c = R.fit(X, y)
    assert r["status"] == 0 and c["status"] == 0
    _check("loop_rows", np.abs(_vec(r, 3) - _cpu_vec(c)).max(), 0)
    shipped = np.abs(_vec(r, 3) - MP["loop"]).max()
    print("max |device - shipped trained_loop_classifier.txt|: %.3e" % shipped)
    assert shipped <= SHIPPED_LOOP_BOUND


def test_combined_head_as_three_models_through_columns():
    """One upload of the 1300 x 7 table, three models over its columns.  F of the six-feature model is nearly flat along
    one direction (the classes of these 1300 rows are separable), so this is the loosest set."""
    rows = np.ascontiguousarray(MP["combined_head"])
    y = np.ascontiguousarray(rows[:, 0])
    out = _dev([dict(X=rows, y=y, columns=c) for c in HEAD_COLUMNS])
    worst = 0.0
    for r, cols in zip(out, HEAD_COLUMNS):
        c = R.fit(rows[:, cols], y)
        assert r["status"] == 0 and c["status"] == 0 and (r["coef"][len(cols):] == 0).all()
        dev = np.abs(_vec(r, len(cols)) - _cpu_vec(c)).max()
        print("combined_head columns %s: %.3e, iterations %d / %d" % (cols, dev, r["iterations"], c["iterations"]))
        worst = max(worst, dev)
    _check("combined_head", worst, 0)
    alone = _dev([(np.ascontiguousarray(rows[:, 1:4]), y)])[0]                   # compact columns: the same rows, the same bits
    assert alone.tobytes() == out[1].tobytes()


@pytest.fixture(scope="module")
def ragged():
    sets = R.ragged_batch()
    return sets, _dev(sets)


def test_ragged_batch_of_256_models(ragged):
    sets, out = ragged
    assert len(sets) == 256 and sorted({X.shape[1] for X, _ in sets}) == list(range(1, 9))
    assert min(X.shape[0] for X, _ in sets) == 50 and max(X.shape[0] for X, _ in sets) == 20000
    worst, where = 0.0, -1
    for m, ((X, y), r) in enumerate(zip(sets, out)):
        c = R.fit(X, y)
        assert r["status"] == 0 and c["status"] == 0, (m, r["status"], c["status"])
        dev = np.abs(_vec(r, X.shape[1]) - _cpu_vec(c)).max()
        if dev > worst:
            worst, where = dev, m
    print("worst model %d (%d x %d)" % (where, sets[where][0].shape[0], sets[where][0].shape[1]))
    _check("ragged", worst, 0)


def _record_checks(X, y, r, c, max_iterations=100):
    """objective: non-negative terms summed in chains of at most n / 512 + 9 additions, each term a few ulp of exp and log1p:
    1e-12 relative is a hundred times that.  grad_inf: signed terms, so the sums' rounding is absolute, at most
    (n / 512 + 9) eps times the sum of |terms| <= n * largest term; 1e-13 n * largest term leaves a factor of twenty."""
    d = X.shape[1]
    w, b = r["coef"][:d], float(r["intercept"])
    assert r["n_used"] == X.shape[0] and r["n_pos"] == int((y == 1).sum())
    F = R.objective(X, y, w, b)
    print("objective device %.17g host %.17g" % (r["objective"], F))
    assert abs(r["objective"] - F) <= 1e-12 * abs(F)
    g, scale = R.gradient(X, y, w, b, dtype=np.longdouble)
    ginf = float(np.abs(g).max())
    print("grad_inf device %.3e longdouble %.3e (largest term %.3e)" % (r["grad_inf"], ginf, scale))
    assert abs(r["grad_inf"] - ginf) <= 1e-13 * X.shape[0] * scale
    # quadratic convergence: the decrement falls from ~1e-8 to ~1e-16 in a step, so only the last test can flip under rounding
    assert 0 < r["iterations"] <= max_iterations and abs(int(r["iterations"]) - c["iterations"]) <= 1
    margin = R.margin_rows(X, w, b)
    conf, bacc = R.confusion(X, y, w, b)
    print("margin rows %d of %d" % (margin.sum(), X.shape[0]))
    assert margin.sum() <= 0.001 * X.shape[0]
    assert np.abs(r["confusion"] - conf).max() <= margin.sum() and r["confusion"].sum() == X.shape[0]
    tn, fp, fn, tp = [float(v) for v in r["confusion"]]
    assert r["balanced_accuracy"] == 0.5 * (tp / (fn + tp) + tn / (tn + fp))
    if margin.sum() == 0:
        assert r["balanced_accuracy"] == bacc


def test_record_fields_are_consistent_with_the_host(ragged):
    for rows in (MP["loop_rows"], MP["combined_head"]):
        X, y = _xy(rows)
        c = R.fit(X, y)
        assert R.margin_rows(X, c["coef"], c["intercept"]).sum() == 0         # the fixtures have no row on the boundary
        _record_checks(X, y, _dev([(X, y)])[0], c)
    sets, out = ragged
    for m in (0, 1, 2, 6, 21, 255):
        _record_checks(sets[m][0], sets[m][1], out[m], R.fit(*sets[m]))


def test_a_record_is_bit_identical_at_any_batch_position_and_from_host_or_device(ragged):
    import torch
    sets, out = ragged
    X, y = _xy(MP["loop_rows"])
    alone = _dev([(X, y)])[0].tobytes()
    others = [sets[m] for m in (3, 1, 40, 7, 100)]
    assert _dev([(X, y)] + others)[0].tobytes() == alone
    assert _dev(others + [(X, y)])[-1].tobytes() == alone
    mid = _dev(others[:2] + [(X, y)] + others[2:])
    assert mid[2].tobytes() == alone
    for k, m in zip((0, 1, 3, 4), (3, 1, 40, 7)):
        assert mid[k].tobytes() == out[m].tobytes()
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    assert _dev([(Xd, yd)])[0].tobytes() == alone
    assert _dev([(Xd, y), (X, yd)])[1].tobytes() == alone                        # mixed
    md = torch.ones(X.shape[0], dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert _dev([dict(X=Xd, y=yd, row_mask=md)])[0].tobytes() == alone


def test_row_mask_folds_equal_fits_of_the_compacted_rows():
    X, y = _xy(MP["loop_rows"])
    fold = np.arange(X.shape[0]) % 5
    masks = [np.ascontiguousarray((fold != k).astype(np.uint8)) for k in range(5)]
    masked = _dev([dict(X=X, y=y, row_mask=m) for m in masks])
    compact = _dev([(np.ascontiguousarray(X[m > 0]), np.ascontiguousarray(y[m > 0])) for m in masks])
    worst = 0.0
    for k in range(5):
        assert masked[k]["status"] == 0 and masked[k]["n_used"] == int(masks[k].sum()) == compact[k]["n_used"]
        assert masked[k]["n_pos"] == compact[k]["n_pos"] and (masked[k]["confusion"] == compact[k]["confusion"]).all()
        c = R.fit(X[masks[k] > 0], y[masks[k] > 0])
        worst = max(worst, np.abs(_vec(masked[k], 3) - _vec(compact[k], 3)).max(), np.abs(_vec(masked[k], 3) - _cpu_vec(c)).max())
    _check("folds", worst, 0)


def test_large_logits_stay_finite():
    """Rows 3000 times further out than the rest, on the right side: |z| > 700 at the minimiser, where exp(z) overflows."""
    X, y = R.synthetic(99, 4000, 3)
    c0 = R.fit(X, y)
    far = 3000.0 * c0["coef"] / np.linalg.norm(c0["coef"])
    X = np.vstack([X, np.outer([1.0, 1.0, -1.0, -1.0], far)])
    y = np.concatenate([y, [1.0, 1.0, 0.0, 0.0]])
    r = _dev([(X, y)])[0]
    c = R.fit(X, y)
    z = X @ r["coef"][:3] + r["intercept"]
    print("largest |z| %.1f" % np.abs(z).max())
    assert np.abs(z).max() > 700 and r["status"] == 0 and c["status"] == 0
    assert np.isfinite(_vec(r, 3)).all() and np.isfinite(r["objective"]) and np.isfinite(r["grad_inf"])
    _check("large_logits", np.abs(_vec(r, 3) - _cpu_vec(c)).max(), 0)
    assert abs(r["objective"] - R.objective(X, y, r["coef"][:3], float(r["intercept"]))) <= 1e-12 * r["objective"]


def test_a_failing_job_gets_its_status_and_leaves_its_neighbours_alone(ragged):
    from tbv_slam_public_amd import _lib as L
    sets, out = ragged
    A, B = sets[3], sets[12]
    X, y = R.synthetic(5, 300, 4)
    one_class = (X, np.ones(300))
    Xn = X.copy()
    Xn[17, 2] = np.nan
    y2 = y.copy()
    y2[5] = 2.0
    none = dict(X=X, y=y, row_mask=np.zeros(300, np.uint8))
    got = _dev([A, one_class, B, (Xn, y), (X, y2), none, A, (np.zeros((0, 4)), np.zeros(0))])
    assert [int(s) for s in got["status"]] == [0, L.ERR_INVALID_ARGUMENT, 0, L.ERR_INVALID_ARGUMENT, L.ERR_INVALID_ARGUMENT,
                                               L.ERR_INVALID_ARGUMENT, 0, L.ERR_INVALID_ARGUMENT]
    assert got[0].tobytes() == out[3].tobytes() == got[6].tobytes() and got[2].tobytes() == out[12].tobytes()
    assert got[1]["n_used"] == 300 and got[1]["n_pos"] == 300 and got[5]["n_used"] == 0 and (got[1]["coef"] == 0).all()
    # a NaN or a bad label in a row the mask leaves out is not a used value
    keep = np.ones(300, np.uint8)
    keep[17] = keep[5] = 0
    ok = _dev([dict(X=Xn, y=y2, row_mask=keep)])[0]
    assert ok["status"] == 0 and ok["n_used"] == 298
    # not converged within max_iterations: CFEAR_ERR_SOLVER, the record holds the last iterate
    short = _dev([A, sets[2]], max_iterations=1)
    assert (short["status"] == L.ERR_SOLVER).all() and (short["iterations"] == 1).all() and np.isfinite(short["coef"]).all()


def test_refused_at_entry():
    from tbv_slam_public_amd import _lib as L, api
    X, y = R.synthetic(5, 100, 3)
    for job in (dict(X=X, y=y, columns=[]), (np.zeros((100, 9)), y), dict(X=X, y=y, columns=[0, 5]), dict(X=X, y=y, columns=[0, -1])):
        with pytest.raises(L.CfearError) as e:
            _dev([(X, y), job])
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "job 1" in str(e.value)
    with pytest.raises(L.CfearError):
        _dev([(X, y)], C=0.0)
    assert _dev([]).shape == (0,)
    ctx = api.default_context()
    assert ctx._lib.cfear_logreg_fit_batch(ctx.h, None, -1, None, None) == L.ERR_INVALID_ARGUMENT
    # parameters other than the defaults reach the kernel
    r = _dev([(X, y)], C=0.25, class_weight_balanced=0, fit_intercept=0)[0]
    c = R.fit(X, y, C=0.25, balanced=False, fit_intercept=False)
    assert r["status"] == 0 and r["intercept"] == 0.0 and np.abs(_vec(r, 3) - _cpu_vec(c)).max() <= BOUND["ragged"]


@pytest.fixture(scope="module")
def scans():
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api, synth
    imgs, gt, sc = synth.scene_v1(3, 6)
    rr = float(sc.range_res)
    out = []
    for f in range(6):
        sr, si, cnt = O.kstrongest(imgs[f], 40, 60)
        pk = O.peaks(imgs[f], 40, sr, cnt)
        cells = O.surface_points(O.kstrongest_cloud(sr, si, cnt, rr, 2.5), 3.0, 1.0, weight_intensity=True)
        out.append(dict(T=gt[f], cldPeaks=O.kstrongest_cloud(sr, si, cnt, rr, 2.5, mask=pk), CFEAR=api.MapPointNormal(cells=cells)))
    out.insert(3, dict(out[2], T=out[2]["T"] + np.array([0.1, 0.0, 0.0])))      # closer than min_dist_btw_scans_: skipped
    return out


@pytest.mark.parametrize("combined", [True, False])
def test_training_end_to_end_on_synthetic_scans(scans, combined, tmp_path):
    from tbv_slam_public_amd import api
    loop, batch = api.ScanLearningInterface(combined), api.ScanLearningInterface(combined)
    for s in scans:
        loop.AddTrainingData(s)
    batch.AddTrainingDataBatch(scans[:2])                                       # two calls: prev_ carries over
    batch.AddTrainingDataBatch(scans[2:])
    assert loop.frame_ == batch.frame_ == len(scans) and loop.prev_ is batch.prev_ is scans[-1]
    for a, b in zip((loop.combined_class, loop.coral_class, loop.cfear_class), (batch.combined_class, batch.coral_class, batch.cfear_class)):
        assert a.X_.shape == b.X_.shape and a.X_.tobytes() == b.X_.tobytes() and a.y_.tobytes() == b.y_.tobytes()
    models = [batch.combined_class] if combined else [batch.coral_class, batch.cfear_class]
    assert all(m.X_.shape == (5 * 13, 6 if combined else 3) and m.y_.sum() == 5 for m in models)
    recs = batch.FitModelsDevice()
    for m, rec in zip(models, recs):
        single = api.LogisticRegression()
        single.AddDataPoint(m.X_, m.y_)
        r = single.fit_device()
        assert r.tobytes() == rec.tobytes() and m.IsFit()
        assert (single.coef_ == m.coef_).all() and single.intercept_ == m.intercept_ and len(m.coef_) == m.X_.shape[1]
        c = R.fit(m.X_, m.y_)
        print("synthetic scans, %d features: |device - restatement| %.3e" % (m.X_.shape[1], np.abs(_vec(rec, m.X_.shape[1]) - _cpu_vec(c)).max()))
    batch.SaveCoefficients(tmp_path)
    other = api.ScanLearningInterface(combined)
    other.LoadCoefficients(str(tmp_path) + "/")
    for a, b in zip(models, [other.combined_class] if combined else [other.coral_class, other.cfear_class]):
        np.testing.assert_allclose(b.coef_, a.coef_, rtol=1e-5)                 # %g: six significant digits
        np.testing.assert_allclose(b.intercept_, a.intercept_, rtol=1e-5)
    if combined:
        par = other.verify_params()
        np.testing.assert_allclose(list(par.align_coef), batch.combined_class.coef_, rtol=1e-5)
        np.testing.assert_allclose(par.align_intercept, batch.combined_class.intercept_, rtol=1e-5)
        q, _, _ = batch.PredAlignment(scans[5], scans[4])
        assert np.isfinite(q[api.COMBINED_COST])


def test_invalid_training_data_raises_like_fit():
    from tbv_slam_public_amd import api
    clf = api.LogisticRegression()
    with pytest.raises(ValueError):
        clf.fit_device()
    clf.AddDataPoint(np.random.RandomState(0).randn(20, 2), np.ones(20))
    with pytest.raises(ValueError):
        clf.fit_device()
    assert not clf.IsFit()


def test_cpp_mirror_fits_the_rows_savedata_wrote(tmp_path):
    from tbv_slam_public_amd import api
    exe = str(tmp_path / "logreg_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "logreg_signature.cpp"), "-o", exe, "-L", so_dir,
                           "-lcfear_hip", "-Wl,-rpath," + so_dir])
    clf = api.LogisticRegression()
    clf.AddDataPoint(MP["loop_rows"][:, 1:], MP["loop_rows"][:, 0])
    clf.SaveData(tmp_path / "rows.txt")
    back = api.LogisticRegression()
    back.LoadData(tmp_path / "rows.txt")
    rec = back.fit_device()
    r = subprocess.run([exe, str(tmp_path / "rows.txt"), str(tmp_path / "coef.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert [float(v) for v in lines[0]] == [back.intercept_] + list(back.coef_)             # the same kernel on the same rows
    assert float(lines[1][0]) == rec["objective"] and float(lines[1][1]) == rec["balanced_accuracy"] and int(lines[1][2]) == rec["iterations"]
    assert [int(v) for v in lines[2]] == [int(v) for v in rec["confusion"]]
    loaded = api.LogisticRegression()
    loaded.LoadCoefficients(tmp_path / "coef.txt")                                           # written by the C++ mirror
    np.testing.assert_allclose(np.concatenate([[loaded.intercept_], loaded.coef_]), _vec(rec, 3), rtol=1e-5)
    assert float(lines[3][0]) == pytest.approx(loaded.intercept_ + loaded.coef_.sum(), rel=1e-12) and int(lines[3][1]) == 1
    assert np.abs(_vec(rec, 3) - MP["loop"]).max() <= SHIPPED_LOOP_BOUND
