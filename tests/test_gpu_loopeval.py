"""GPU: cfear_loop_stats_batch and cfear_loop_curves_batch (csrc/loopeval.hip) against their NumPy models
(tests/loopeval_cpu.py, which the CPU tests pin to a transcription of the reference and to sklearn), and LoopClosureEval end to
end.  Only batch invariance and host-against-device compare the device with itself.

Loop rows: closest_loop_distance, candidate_loop_distance, close_xy and id_close must be bitwise equal (+ * sqrt are correctly
rounded on both sides, the kernels are built without contraction) and the flags equal (the CPU test asserts that no case lies
within 1e-9 of a limit).  diff, transl_error and rot_error go through the device's cos / sin / atan2: the largest deviation
from the model measured over the cases of this file on an MI355X is 1.110e-16 (STATS_MEASURED; EXPERIMENTS.md, "Scoring the loop detector");
the bound is ten times that, the margin the closure tests took for the same functions, and must stay under 1e-12.

Curves: every array and every count bitwise equal; |auc - model| <= n_roc 2^-52, since the trapezoid's terms are not negative
and sum to at most 1, so two summation orders differ by no more than that."""
import functools

import numpy as np
import pytest

import loopeval_cpu as M
from tbv_slam_public_amd import _lib as L
from tbv_slam_public_amd import api

pytestmark = pytest.mark.gpu

STATS_MEASURED = 1.110e-16
STATS_BOUND = 10.0 * STATS_MEASURED
EXACT = ("closest_loop_distance", "candidate_loop_distance", "close_xy", "id_close", "is_loop", "candidate_close", "prediction_pos_ok")
CLOSE = ("diff", "transl_error", "rot_error")


@functools.lru_cache(maxsize=None)
def _stats():
    off, gt, has, cands, ties = M.stats_cases()
    return off, gt, has, cands, ties, M.loop_stats_model(off, gt, has, cands)


def _same_rows(dev, want, where):
    for f in EXACT:
        assert dev[f].tobytes() == want[f].tobytes(), (where, f)
    d = max(float(np.abs(dev[f] - want[f]).max()) for f in CLOSE) if len(want) else 0.0
    print("%s: %d candidates, max |diff, transl_error, rot_error - model| = %.3e" % (where, len(want), d))
    assert STATS_BOUND < 1e-12 and d <= STATS_BOUND, (where, d)


def test_stats_parity_with_the_model():
    off, gt, has, cands, ties, want = _stats()
    dev = api.loop_stats_flat(off, gt, has, cands)
    _same_rows(dev, want, "all cases")
    for i, node in ties.items():
        assert dev["id_close"][i] == node
    for par in (dict(min_index_gap=0), dict(min_index_gap=70, max_distance=30.0), dict(no_loop_distance=4.0, max_registration_translation=0.3)):
        _same_rows(api.loop_stats_flat(off, gt, has, cands, **par), M.loop_stats_model(off, gt, has, cands, **par), str(par))
    assert len(api.loop_stats_flat(off, gt, has, cands[:0])) == 0


def test_stats_batch_invariance():
    off, gt, has, cands, _, _ = _stats()
    whole = api.loop_stats_flat(off, gt, has, cands)
    n_g = len(off) - 1
    graphs = [(gt[off[g]:off[g + 1]], has[off[g]:off[g + 1]]) for g in range(n_g)]
    # every graph alone, and the batch with graphs and candidates reversed
    for g in range(n_g):
        mine = np.flatnonzero(cands["graph"] == g)
        c = cands[mine].copy()
        c["graph"] = 0
        assert api.loop_stats([graphs[g]], c).tobytes() == whole[mine].tobytes(), g
    c = cands[::-1].copy()
    c["graph"] = n_g - 1 - c["graph"]
    assert api.loop_stats(graphs[::-1], c).tobytes() == whole[::-1].tobytes()


def test_stats_host_against_device_buffers():
    import torch
    off, gt, has, cands, _, _ = _stats()
    whole = api.loop_stats_flat(off, gt, has, cands)
    d_c = torch.from_numpy(cands.view(np.uint8).copy()).cuda()
    d_gt, d_has = torch.from_numpy(gt.copy()).cuda(), torch.from_numpy(has.copy()).cuda()
    dev = api.loop_stats_flat(off, d_gt, d_has, d_c)
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == whole.tobytes()
    # device buffers are checked on the device, before the rows are computed: the lowest faulty candidate is named
    bad = cands.copy()
    bad["to"][9] = 100000
    bad["guess_nr"][4] = -1
    with pytest.raises(L.CfearError) as e:
        api.loop_stats_flat(off, d_gt, d_has, torch.from_numpy(bad.view(np.uint8).copy()).cuda())
    assert e.value.status == L.ERR_INVALID_ARGUMENT and e.value.candidate == 4
    with pytest.raises(L.CfearError) as e:                       # host and device buffers mixed
        api.loop_stats_flat(off, gt, d_has, d_c)
    assert e.value.status == L.ERR_INVALID_ARGUMENT and e.value.candidate == -1


# ---- curves --------------------------------------------------------------------------------------------------------------------
PARAMS = [dict(drop_intermediate=d, reference_endpoints=r) for d in (1, 0) for r in (1, 0)]


def _same_curves(arrays, rec, want_arrays, want_rec, where):
    for k in M.CURVE_ARRAYS:
        a = arrays[k].cpu().numpy() if hasattr(arrays[k], "cpu") else arrays[k]
        assert a.view(np.uint64).tolist() == want_arrays[k].view(np.uint64).tolist(), (where, k)
    for f in rec.dtype.names:
        if f != "auc":
            assert rec[f].tolist() == want_rec[f].tolist(), (where, f)
    d = np.abs(rec["auc"] - want_rec["auc"])
    print("%s: n_roc %s, |auc - model| %s" % (where, rec["n_roc"].tolist(), d.tolist()))
    assert (d <= rec["n_roc"] * 2.0 ** -52).all(), (where, d)


def _routes(fn):
    ctx = api.default_context()
    ctx.profile_enable(True)
    ctx.profile_read()
    try:
        out = fn()
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    return out, {k: v[1] for k, v in prof.items() if k.startswith("loop_curves") and v[1]}


@pytest.mark.parametrize("n,mode", M.CURVE_CASES)
def test_curves_parity_with_the_model(n, mode):
    y, s, ok = M.curve_case(n, mode)
    off = np.array([0, n], np.int64)
    for par in PARAMS if n <= 4 * M.LDS_ROWS else PARAMS[:1] + PARAMS[3:]:
        (arrays, rec), routes = _routes(lambda: api.loop_curves_flat(off, y, s, ok, **par))
        assert routes == ({"loop_curves_lds": 1} if n <= M.LDS_ROWS else {"loop_curves_global": 1}), (n, routes)
        want = M.loop_curves_model(off, y, s, ok, **par)
        assert rec["status"][0] == L.OK and rec["n_pos"][0] + rec["n_neg"][0] == n
        _same_curves(arrays, rec, *want, "n=%d %s %s" % (n, mode, par))
    if mode == "masked":                                          # a score equal to p_threshold counts as a prediction
        assert (s == 0.9).sum() == (1 if n > 2 else 0)
        lo = api.loop_curves_flat(off, y, s, None, p_threshold=np.nextafter(0.9, 1.0))[1]
        hi = api.loop_curves_flat(off, y, s, None)[1]
        assert (hi["confusion"][0, 1] + hi["confusion"][0, 3]) - (lo["confusion"][0, 1] + lo["confusion"][0, 3]) == (1 if n > 2 else 0)


@functools.lru_cache(maxsize=None)
def _good():
    return [M.curve_case(257, "decimal"), M.curve_case(65, "masked"), M.curve_case(1500, "distinct")]


def test_curves_refused_experiments_leave_the_others_alone():
    good = _good()
    alone = [M.loop_curves_model(*M.curve_batch([g])) for g in good]
    y5, s5, ok5 = M.curve_case(5, "distinct")
    nan = s5.copy()
    nan[3] = np.nan
    two = y5.copy()
    two[1] = 2
    bads = [(np.ones(7, np.uint8), np.linspace(0, 1, 7), np.ones(7, np.uint8)), (np.zeros(4, np.uint8), np.linspace(0, 1, 4), np.ones(4, np.uint8)),
            (y5, nan, ok5), (two, s5, ok5), (np.zeros(0, np.uint8), np.zeros(0), np.zeros(0, np.uint8))]
    for k, bad in enumerate(bads):
        batch = M.curve_batch([good[0], bad, good[1], bad, good[2]])
        arrays, rec = api.loop_curves_flat(*batch)
        _same_curves(arrays, rec, *M.loop_curves_model(*batch), "bad experiment %d" % k)
        assert rec["status"].tolist() == [L.OK, L.ERR_INVALID_ARGUMENT, L.OK, L.ERR_INVALID_ARGUMENT, L.OK]
        for f in ("n_pos", "n_neg", "n_thresholds", "n_roc", "n_pr", "auc"):
            assert rec[f][1] == 0 and rec[f][3] == 0 and not rec["confusion"][1].any()
        sl = api.loop_curve_slices(arrays, rec, batch[0])
        for g, e in enumerate((0, 2, 4)):
            one = api.loop_curve_slices(*alone[g], np.array([0, len(good[g][0])]))[0]
            for name in M.CURVE_ARRAYS:
                assert sl[e][name].tobytes() == one[name].tobytes(), (k, g, name)


def test_curves_batch_invariance_across_both_routes():
    cases = _good() + [M.curve_case(M.LDS_ROWS + 1, "decimal"), M.curve_case(2, "distinct"), M.curve_case(M.LDS_ROWS, "masked")]
    alone = [api.loop_curves([c]) for c in cases]
    (whole, routes) = _routes(lambda: api.loop_curves(cases[::-1]))
    assert routes == {"loop_curves_lds": 1, "loop_curves_global": 1}
    for a, w in zip(alone, whole[::-1]):
        assert a[0]["record"].tobytes() == w["record"].tobytes()
        for name in M.CURVE_ARRAYS:
            assert a[0][name].tobytes() == w[name].tobytes(), name


def test_curves_host_against_device_buffers():
    import torch
    batch = M.curve_batch(_good() + [M.curve_case(M.LDS_ROWS + 1, "masked")])
    off, y, s, ok = batch
    arrays, rec = api.loop_curves_flat(off, y, s, ok)
    d_arrays, d_rec = api.loop_curves_flat(off, torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(ok).cuda())
    assert d_rec.tobytes() == rec.tobytes()
    for k in M.CURVE_ARRAYS:
        assert d_arrays[k].is_cuda and d_arrays[k].cpu().numpy().tobytes() == arrays[k].tobytes(), k
    d_arrays, d_rec = api.loop_curves_flat(off, torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), None, p_threshold=0.5)
    assert d_rec.tobytes() == api.loop_curves_flat(off, y, s, None, p_threshold=0.5)[1].tobytes()
    with pytest.raises(L.CfearError) as e:
        api.loop_curves_flat(off, y, torch.from_numpy(s).cuda(), ok)
    assert e.value.status == L.ERR_INVALID_ARGUMENT


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_loop_closure_eval_end_to_end():
    """LoopClosureEval on the device (classifiers by cfear_logreg_fit_batch, which test_gpu_logreg.py pins; curves by
    cfear_loop_curves_batch) against the same chain on the curve model, with the device's own fitted coefficients."""
    ev = api.LoopClosureEval(M.synthetic_table())
    dev = ev.evaluate()
    assert [d["name"] for d in dev] and sorted(d["name"] for d in dev) == api.LoopClosureEval.settings_name()
    want = ev.evaluate(models=ev.models_, curves=M.loop_curves_model)
    for d, w in zip(dev, want):
        assert d["name"] == w["name"] and d["y_prob"].tobytes() == w["y_prob"].tobytes() and (d["rows"] == w["rows"]).all()
        for name in M.CURVE_ARRAYS:
            assert d[name].tobytes() == w[name].tobytes(), (d["name"], name)
        for f in d["record"].dtype.names:
            if f != "auc":
                assert d["record"][f].tolist() == w["record"][f].tolist(), (d["name"], f)
        assert abs(d["record"]["auc"] - w["record"]["auc"]) <= d["record"]["n_roc"] * 2.0 ** -52
        assert d["record"]["status"] == L.OK and 0.5 < d["record"]["auc"] <= 1.0, (d["name"], d["record"]["auc"])
        print(d["name"], "auc %.4f" % d["record"]["auc"], "thresholds", d["record"]["n_thresholds"])
