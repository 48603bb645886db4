"""CPU: what the loop-evaluation calls (cfear_loop_stats_batch, cfear_loop_curves_batch, csrc/loopeval.hip) need no device
for -- the NumPy models the GPU results are compared with (tests/loopeval_cpu.py) against a literal transcription of the
reference's per-candidate loop and against sklearn, the inputs the GPU tests use, the ABI, the defaults, the refusals (made
before a context is needed), LoopClosureEval's marshalling, the CSV round trip and the signature program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import loopeval_cpu as M
from tbv_slam_public_amd import _lib as L
from tbv_slam_public_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stats_model_equals_the_transcription():
    off, gt, has, cands, ties = M.stats_cases()
    a, b = M.loop_stats_model(off, gt, has, cands), M.loop_stats_transcription(off, gt, has, cands)
    assert a.tobytes() == b.tobytes()
    for par in (dict(min_index_gap=0), dict(min_index_gap=3, max_distance=1.0), dict(no_loop_distance=4.0)):
        assert M.loop_stats_model(off, gt, has, cands, **par).tobytes() == M.loop_stats_transcription(off, gt, has, cands, **par).tobytes()


def test_stats_cases_cover_what_they_claim():
    off, gt, has, cands, ties = M.stats_cases()
    r = M.loop_stats_model(off, gt, has, cands)
    assert {0, 10, 11, 12} <= set(cands["from"].tolist()) and {0, 1, 75, 76, 77} <= set(np.diff(off).tolist())
    for i, want in ties.items():
        assert r["id_close"][i] == want and r["closest_loop_distance"][i] == 5.0
    for n in (75, 76, 77):                                       # the nearest is the last eligible node: lanes 63, 0 and 1
        i = [k for k, c in enumerate(cands) if np.diff(off)[c["graph"]] == n][0]
        assert r["id_close"][i] == n - 12 and cands["from"][i] == n - 1
    # from = 0, 10: nothing eligible; from = 11, 12: node 0 / nodes 0, 1
    first = {int(c["from"]): r[i] for i, c in enumerate(cands) if c["graph"] == 0 and c["from"] <= 12}
    assert first[0]["closest_loop_distance"] == first[10]["closest_loop_distance"] == 100000.0 and first[10]["id_close"] == 10
    assert first[11]["id_close"] == 0 and first[12]["id_close"] in (0, 1) and first[12]["closest_loop_distance"] < 100000.0
    no_from = [i for i, c in enumerate(cands) if not has[off[c["graph"]] + c["from"]]]
    no_to = [i for i, c in enumerate(cands) if has[off[c["graph"]] + c["from"]] and not has[off[c["graph"]] + c["to"]]]
    assert no_from and no_to and (r["candidate_loop_distance"][no_from + no_to] == -1.0).all()
    assert (r["closest_loop_distance"][no_from] == 100000.0).all() and (r["closest_loop_distance"][no_to] < 100000.0).all()
    assert np.abs(r["diff"][no_from]).max() > 0.0               # Terror is computed whatever has_gt says
    same = [i for i, c in enumerate(cands) if c["from"] == c["to"] and not c["guess_xyt"].any()]
    assert same and np.abs(r["diff"][same]).max() == 0.0
    g3 = [i for i, c in enumerate(cands) if c["graph"] == 0 and c["from"] == 140]
    assert cands["guess_nr"][g3].tolist() == [0, 1, 2] and len(set(r["closest_loop_distance"][g3])) == 1
    assert r["candidate_close"][g3].tolist() == [1, 0, 0] and r["is_loop"][g3].all()
    # every flag of every case is decided with a margin no device rounding reaches
    assert np.abs(r["closest_loop_distance"] - 6.0).min() > 1e-9 and np.abs(r["transl_error"] - 4.0).min() > 1e-9
    assert np.abs(r["rot_error"] - 2.5).min() > 1e-9
    assert 0 < r["is_loop"].sum() < len(r) and 0 < r["prediction_pos_ok"].sum() < len(r)


CURVE_CASES = M.CURVE_CASES


@pytest.mark.parametrize("n,mode", CURVE_CASES)
def test_curves_model_equals_sklearn(n, mode):
    metrics = pytest.importorskip("sklearn.metrics")
    y, s, ok = M.curve_case(n, mode)
    for drop in (1, 0):
        got, rec = M.curves_one(y, s, ok, drop_intermediate=drop, reference_endpoints=0)
        fpr, tpr, thr = metrics.roc_curve(y, s, drop_intermediate=bool(drop))
        p, r, pt = metrics.precision_recall_curve(y, s)
        for a, b in ((got["roc_fpr"], fpr), (got["roc_tpr"], tpr), (got["roc_thr"], thr), (got["pr_precision"], p), (got["pr_recall"], r),
                     (got["pr_thr"], pt)):
            assert a.shape == b.shape and np.array_equal(a, b)
            assert (a + 0.0).tobytes() == (np.asarray(b, np.float64) + 0.0).tobytes()      # bitwise, -0.0 read as 0.0
        assert rec["auc"] == metrics.auc(fpr, tpr)
        # the curves as the reference's scripts plot and integrate them (3_loop_closure.py:156-165)
        got1, rec1 = M.curves_one(y, s, ok, drop_intermediate=drop, reference_endpoints=1)
        tpr[-1] = tpr[-2]
        r[0] = r[1]
        p[0] = p[1]
        assert np.array_equal(got1["roc_tpr"], tpr) and np.array_equal(got1["pr_recall"], r) and np.array_equal(got1["pr_precision"], p)
        assert rec1["auc"] == metrics.auc(fpr, tpr)
    pred = (s >= 0.9).astype(int)
    yc = y.copy()
    yc[(y == 1) & (pred == 1) & (ok == 0)] = 0                                             # CorrectLabelForPosition on a copy
    if len(set(yc)) == 2 or len(set(pred)) == 2:
        assert tuple(metrics.confusion_matrix(yc, pred, labels=[0, 1]).ravel()) == rec["confusion"]
    assert rec["accuracy"] == metrics.accuracy_score(yc, pred)
    assert rec["precision"] == metrics.precision_score(yc, pred, zero_division=0) and rec["recall"] == metrics.recall_score(yc, pred, zero_division=0)


def test_curve_cases_cover_what_they_claim():
    y, s, ok = M.curve_case(257, "masked")
    assert (s == 0.0).sum() > 100 and np.signbit(s[s == 0.0]).any() and not np.signbit(s[s == 0.0]).all() and (s == 0.9).any()
    assert np.unique(M.curve_case(65, "equal")[1]).size == 1 and np.unique(M.curve_case(257, "decimal")[1]).size <= 11
    assert M.curves_one(*M.curve_case(65, "equal"))[1]["n_thresholds"] == 1
    for bad in ((np.array([1, 1], np.uint8), np.array([0.1, 0.2])), (np.array([1, 0], np.uint8), np.array([np.nan, 0.2])),
                (np.array([2, 0, 1], np.uint8), np.array([0.1, 0.2, 0.3])), (np.zeros(0, np.uint8), np.zeros(0))):
        assert M.curves_one(*bad) is None
    cases = [M.curve_case(5, "distinct"), (np.ones(3, np.uint8), np.ones(3), np.ones(3, np.uint8)), M.curve_case(64, "decimal")]
    arrays, rec = M.loop_curves_model(*M.curve_batch(cases))
    assert rec["status"].tolist() == [L.OK, L.ERR_INVALID_ARGUMENT, L.OK] and rec["n_roc"][1] == 0
    sl = api.loop_curve_slices(arrays, rec, M.curve_batch(cases)[0])
    assert sl[1]["roc_fpr"].size == 0 and sl[2]["pr_thr"].size == rec["n_pr"][2] - 1 and np.isfinite(sl[2]["pr_recall"]).all()
    assert np.isnan(arrays["roc_fpr"][5 + 1:5 + 1 + 4]).all()


def test_abi_names_the_calls_and_their_structs():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_[a-z0-9_]+)\s*\(", hdr))
    names = {"cfear_loop_stats_params_default", "cfear_loop_stats_batch", "cfear_loop_curves_params_default", "cfear_loop_curves_batch"}
    assert names <= declared & set(L.EXPORTS) and all(hasattr(lib, n) for n in names) and lib.cfear_abi_version() == 1
    assert int(re.search(r"#define CFEAR_LOOPEVAL_LDS_ROWS (\d+)", hdr).group(1)) == L.LOOPEVAL_LDS_ROWS == 16384
    assert C.sizeof(L.LoopStatsParams) == 40 and C.sizeof(L.LoopCurvesParams) == 16
    assert [(f, getattr(L.LoopStatsParams, f).offset) for f, _ in L.LoopStatsParams._fields_] == [
        ("max_distance", 0), ("max_registration_translation", 8), ("max_registration_rotation_deg", 16), ("no_loop_distance", 24),
        ("min_index_gap", 32), ("pad", 36)]
    assert [(f, getattr(L.LoopCurvesParams, f).offset) for f, _ in L.LoopCurvesParams._fields_] == [
        ("p_threshold", 0), ("drop_intermediate", 8), ("reference_endpoints", 12)]
    off = lambda dt: [(k, dt.fields[k][1]) for k in dt.names]
    assert L.LOOP_CANDIDATE_DTYPE.itemsize == 40 and off(L.LOOP_CANDIDATE_DTYPE) == [("graph", 0), ("from", 4), ("to", 8), ("guess_nr", 12), ("guess_xyt", 16)]
    assert L.LOOP_ROW_DTYPE.itemsize == 88 and off(L.LOOP_ROW_DTYPE) == [
        ("diff", 0), ("closest_loop_distance", 24), ("candidate_loop_distance", 32), ("transl_error", 40), ("rot_error", 48), ("close_xy", 56),
        ("id_close", 72), ("is_loop", 76), ("candidate_close", 80), ("prediction_pos_ok", 84)]
    assert L.LOOP_CURVES_RESULT_DTYPE.itemsize == 96 and off(L.LOOP_CURVES_RESULT_DTYPE) == [
        ("auc", 0), ("accuracy", 8), ("precision", 16), ("recall", 24), ("n_pos", 32), ("n_neg", 40), ("confusion", 48), ("n_thresholds", 80),
        ("n_roc", 84), ("n_pr", 88), ("status", 92)]


def test_defaults_follow_the_reference():
    p = api.loop_stats_params()
    assert (p.max_distance, p.max_registration_translation, p.max_registration_rotation_deg) == (6.0, 4.0, 2.5)   # EvaluationManager.cpp:14-16
    assert (p.no_loop_distance, p.min_index_gap) == (100000.0, 10) == (M.STATS_DEFAULTS["no_loop_distance"], M.STATS_DEFAULTS["min_index_gap"])
    c = api.loop_curves_params()
    assert (c.p_threshold, c.drop_intermediate, c.reference_endpoints) == (0.9, 1, 1)
    assert api.loop_stats_params(min_index_gap=3).min_index_gap == 3 and api.loop_curves_params(p_threshold=0.8).p_threshold == 0.8
    for bad in (lambda: api.loop_stats_params(pad=1), lambda: api.loop_curves_params(no_such_field=1)):
        with pytest.raises(L.CfearError):
            bad()


def _stats_call(off, gt, has, cands, par, n_nodes=None):
    rows = np.full(len(cands), 7, L.LOOP_ROW_DTYPE)
    bad = C.c_int64(5)
    rc = L.lib().cfear_loop_stats_batch(None, off.ctypes.data, gt.ctypes.data, has.ctypes.data, len(has) if n_nodes is None else n_nodes,
                                        len(off) - 1, cands.ctypes.data, len(cands), C.byref(par), rows.ctypes.data, C.byref(bad))
    return rc, bad.value, rows


def test_stats_refusals_need_no_device():
    """Every check of host buffers is made before a context is asked for: the refusals name the candidate, nothing is written."""
    off, gt, has, cands, _ = M.stats_cases()
    par = api.loop_stats_params()
    untouched = np.full(len(cands), 7, L.LOOP_ROW_DTYPE).tobytes()
    rc, bad, rows = _stats_call(off, gt, has, cands, par)
    assert (rc, bad) == (L.ERR_INVALID_ARGUMENT, -1) and rows.tobytes() == untouched             # valid: only the context is missing

    def cand(i, **kw):
        c = cands.copy()
        for k, v in kw.items():
            c[k][i] = v
        return c

    def edited(arr, idx, v):
        a = arr.copy()
        a[idx] = v
        return a
    one_node = [i for i, c in enumerate(cands) if np.diff(off)[c["graph"]] == 1][0]
    has_hole = [i for i, c in enumerate(cands) if not has[off[c["graph"]] + c["from"]]][0]
    node = int(off[cands["graph"][has_hole]] + cands["from"][has_hole])
    cases = [(off, gt, has, cand(3, graph=len(off) - 1), par, 3), (off, gt, has, cand(3, graph=-1), par, 3), (off, gt, has, cand(4, to=150), par, 4),
             (off, gt, has, cand(2, **{"from": -1}), par, 2), (off, gt, has, cand(one_node, to=1), par, one_node),
             (off, gt, has, cand(5, graph=1), par, 5),                                            # the graph of 0 nodes
             (off, gt, has, cand(6, guess_nr=-1), par, 6), (off, gt, has, cand(7, guess_xyt=(0.0, np.nan, 0.0)), par, 7),
             (off, gt, has, cand(1, guess_xyt=(np.inf, 0.0, 0.0)), par, 1),
             (off, edited(gt, (node, 2), np.nan), has, cands, par, has_hole),                      # a pose a candidate reads, without has_gt
             (off, edited(gt, (5, 0), np.inf), has, cands, par, -1),                              # a node with has_gt
             (edited(off, 0, 1), gt, has, cands, par, -1), (edited(off, 3, 100), gt, has, cands, par, -1),
             (edited(off, len(off) - 1, off[-1] - 1), gt, has, cands, par, -1),
             (off, gt, has, cands, api.loop_stats_params(max_distance=np.nan), -1), (off, gt, has, cands, api.loop_stats_params(min_index_gap=-1), -1)]
    for k, (o_, g_, h_, c_, p_, want) in enumerate(cases):
        rc, bad, rows = _stats_call(o_, g_, h_, c_, p_)
        assert (rc, bad) == (L.ERR_INVALID_ARGUMENT, want), k
        assert rows.tobytes() == untouched, k
    # a pose without has_gt that no candidate reads may hold anything
    free = np.flatnonzero(has == 0)
    free = [k for k in free if k not in set((off[cands["graph"]] + cands["from"]).tolist()) | set((off[cands["graph"]] + cands["to"]).tolist())][0]
    assert _stats_call(off, edited(gt, (free, 0), np.nan), has, cands, par)[:2] == (L.ERR_INVALID_ARGUMENT, -1)
    with pytest.raises(L.CfearError):
        api.loop_stats([(np.zeros((3, 3)), np.ones(2))], [])


def _curves_call(off, y, s, ok, par, n_rows=None):
    n_rows = len(s) if n_rows is None else n_rows
    arrays = [np.full(len(s) + len(off) - 1, 7.0) for _ in range(6)]
    rec = np.full(len(off) - 1, 7, L.LOOP_CURVES_RESULT_DTYPE)
    bad = C.c_int32(5)
    rc = L.lib().cfear_loop_curves_batch(None, off.ctypes.data, y.ctypes.data, s.ctypes.data, None if ok is None else ok.ctypes.data, n_rows,
                                         len(off) - 1, C.byref(par), *[a.ctypes.data for a in arrays], rec.ctypes.data, C.byref(bad))
    return rc, bad.value, all((a == 7.0).all() for a in arrays) and rec.tobytes() == np.full(len(off) - 1, 7, L.LOOP_CURVES_RESULT_DTYPE).tobytes()


def test_curves_refusals_need_no_device():
    off, y, s, ok = M.curve_batch([M.curve_case(5, "distinct"), M.curve_case(0, "equal") if False else (np.zeros(0), np.zeros(0), np.zeros(0)),
                                   M.curve_case(64, "decimal")])
    par = api.loop_curves_params()
    assert _curves_call(off, y, s, ok, par) == (L.ERR_INVALID_ARGUMENT, -1, True)                 # valid: only the context is missing
    assert _curves_call(off, y, s, None, par) == (L.ERR_INVALID_ARGUMENT, -1, True)
    o1, o2, o3 = off.copy(), off.copy(), off.copy()
    o1[0], o2[2], o3[3] = 1, 3, off[3] + 1
    for k, (o_, p_, want) in enumerate(((o1, par, 0), (o2, par, 1), (o3, par, 2), (off, api.loop_curves_params(p_threshold=np.nan), -1))):
        assert _curves_call(o_, y, s, ok, p_) == (L.ERR_INVALID_ARGUMENT, want, True), k
    with pytest.raises(L.CfearError):
        api.loop_curves([(y[:5], s[:5], ok[:5]), (y[5:], s[5:])])
    assert api.loop_curves([]) == []


def test_loop_closure_eval_marshalling_and_names():
    E = api.LoopClosureEval
    assert E.settings_name() == ["1) Radar Scan Context", "2) Aggregated point cloud map", "3) Origin augmentation",
                                 "4) Alignment loop verification", "5) Odometry decoupled", "6) Odometry coupled", "7) Cascaded classifier",
                                 "8) Multiple candidate selection"]
    full = ["odom-bounds", "sc-sim", "alignment_quality"]
    assert E.settings_name(["sc-sim"], guess0=True, radar_raw=1, augment=0, odometry_coupled=0) == "1) Radar Scan Context"
    assert E.settings_name(full, guess0=False, radar_raw=0, augment=1, odometry_coupled=1) == "8) Multiple candidate selection"
    assert E.settings_name(full, radar_raw=0, augment=1, odometry_coupled=1, cascaded=True) == "7) Cascaded classifier"
    assert E.settings_name(["odom-bounds", "sc-sim"], radar_raw=0, augment=1) == "" and E.settings_name(full, guess0=False, radar_raw=1) == ""
    t = M.synthetic_table()
    ev = E(t)
    st = ev.settings()
    assert sorted(s["name"] for s in st) == E.settings_name()
    tb = ev.table
    lim = 2.5 * np.pi / 180.0                                    # the script's own form of the rotation limit
    assert (tb["candidate close"] == ((np.sqrt(tb["diff.x"] ** 2 + tb["diff.y"] ** 2) < 4.0) & (np.fabs(tb["diff.z"]) < lim))).all()
    assert (tb["prediction pos ok"] == ((tb["is loop"] == 0) | tb["candidate close"])).all() and 0 < tb["prediction pos ok"].sum() < len(tb["is loop"])
    for s in st:
        assert (tb["guess_nr"][s["train"]] == 0).all() and (tb["prediction pos ok"][s["train"]] == 1).all()
        assert (tb["id_from"][s["train"]] != tb["id_to"][s["train"]]).all() and len(s["train"]) < len(s["guess0_rows"])
    jobs, where = ev.model_jobs(st)
    assert len(jobs) == 9 and sorted(k for _, k in where) == ["align", "sc"] + ["single"] * 7
    assert [j["X"].shape[1] for j, (s, k) in zip(jobs, where) if st[s]["name"].startswith("7)")] == [2, 1]
    # scores with hand-made models: the first maximum wins, the cascade multiplies predict() into the probability
    models = np.zeros(len(jobs), L.LOGREG_RESULT_DTYPE)
    models["coef"][:, 0] = -1.0
    models["intercept"] = 0.5
    sc = ev.scores(st, models, where)
    for s, (y, p, ok, rows) in zip(st, sc):
        X0 = np.asarray(tb[{"sc": "odom-bounds"}.get("x", s["feature_cols"][0])], np.float64)
        assert (y == tb["is loop"][rows]).all() and (ok == tb["candidate close"][rows]).all()
        if s["guess0"] and not s["cascaded"]:
            assert (rows == s["guess0_rows"]).all()
            assert np.array_equal(p, 1.0 / (1.0 + np.exp(-(X0[rows] * -1.0 + 0.5))) * tb["prediction pos ok"][rows])
        elif not s["guess0"]:
            z = (0.5 - X0[s["rows"]]).reshape(-1, 3)
            assert (rows == s["rows"].reshape(-1, 3)[np.arange(len(z)), np.argmax(z, 1)]).all() and len(rows) == len(s["guess0_rows"])
        else:
            z_sc = 0.5 - tb["odom-bounds"][rows]
            z_al = 0.5 - tb["alignment_quality"][rows]
            assert np.array_equal(p, (z_sc > 0) * (1.0 / (1.0 + np.exp(-z_al))) * tb["prediction pos ok"][rows])
    # the whole chain on the model's curves
    out = ev.evaluate(models=models, curves=M.loop_curves_model)
    assert [o["name"] for o in out] == [s["name"] for s in st] and all(o["record"]["status"] == L.OK for o in out)
    assert all(0.0 <= o["record"]["auc"] <= 1.0 and o["roc_fpr"].size == o["record"]["n_roc"] for o in out)
    models["status"][2] = L.ERR_SOLVER
    with pytest.raises(ValueError):
        ev.evaluate(models=models, curves=M.loop_curves_model)


def test_csv_round_trip_and_rounding(tmp_path):
    off, gt, has, cands, _ = M.stats_cases()
    rows = M.loop_stats_model(off, gt, has, cands)
    graphs = [(gt[off[g]:off[g + 1]], has[off[g]:off[g + 1]]) for g in range(len(off) - 1)]
    n = len(cands)
    q = {"sc-sim": np.linspace(0.0, 1.0, n) / 3.0, "odom-bounds": np.full(n, 1.0), "alignment_quality": np.linspace(-20.0, 5.0, n)}
    t = api.loop_table(graphs, cands, rows, q, dataset="oxford", sequence="s1")
    assert list(t)[:18] == api.LOOP_CSV_HEADER and list(t)[18:] == ["alignment_quality", "odom-bounds", "sc-sim", "dataset", "sequence"]
    path = str(tmp_path / "loop.csv")
    api.write_loop_csv(path, t, quality_names=tuple(q))
    lines = open(path).read().splitlines()
    assert lines[0] == ",".join(api.LOOP_CSV_HEADER + ["alignment_quality", "odom-bounds", "sc-sim", "dataset", "sequence"]) and len(lines) == n + 1
    cells = lines[4].split(",")
    assert cells[9] == "%.6g" % rows["diff"][3, 0] and cells[12] == "%.6g" % rows["closest_loop_distance"][3] and cells[14] == str(cands["from"][3])
    assert cells[18] == "%.6f" % q["alignment_quality"][3] and cells[19] == "1.000000" and cells[-2:] == ["oxford", "s1"]
    assert lines[1].split(",")[12] == "100000"                       # the no-loop distance as setprecision(6) writes it
    back = api.read_loop_csv(path)
    assert list(back) == list(t) and back["id_from"].dtype == np.int64 and back["dataset"].tolist() == ["oxford"] * n
    for k in api.LOOP_CSV_HEADER[:14]:
        assert back[k].dtype.kind in "fi" and np.allclose(back[k], t[k], rtol=5e-6, atol=0)
    assert (back["guess_nr"] == cands["guess_nr"]).all() and (back["id_close"] == rows["id_close"]).all()
    assert any((back[k] != t[k]).any() for k in ("diff.x", "diff.y", "diff.z"))                # the file holds rounded rows


def test_write_loop_result(tmp_path):
    train = dict(accuracy=0.91234, precision=0.5, recall=1.0)
    test = np.zeros(1, L.LOOP_CURVES_RESULT_DTYPE)[0]
    test["accuracy"], test["precision"], test["recall"] = 0.75, 0.25, 0.125
    path = str(tmp_path / "result.txt")
    lines = api.write_loop_result(path, train, test, [0.5, -1.0, 2.0], 0.25, 0.9, 30, 40)
    assert open(path).read() == "".join(lines)
    assert lines[:9] == ["Training accuracy[%], 91.234\n", "Training precision [%], 50.000\n", "Training recall [%], 100.000\n",
                         "Testing accurac [%], 75.000\n", "Testing precision [%], 25.000\n", "Testing recall [%], 12.500\n",
                         "nr correct candidates, 30\n", "nr loops, 40\n", "correct_loop_ratio [%], 75.000\n"]
    assert lines[9] == "Coef, [[ 0.5 -1.   2. ]]\n" and lines[10] == "Intercept [0.25]\n" and lines[11] == "Threshold, 0.9\n"


def test_cpp_signature_compiles_and_refuses(tmp_path):
    exe = str(tmp_path / "loopeval_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loopeval_signature.cpp"), "-o", exe, "-L", so_dir, "-lcfear_hip",
                           "-Wl,-rpath," + so_dir])
    out = subprocess.check_output([exe]).decode().split()
    inv = str(L.ERR_INVALID_ARGUMENT)
    assert out == [inv, "1", inv, "-1", inv, "1", "6", "4", "2.5", "100000", "10", "0.9", "1", "1"]
