"""GPU: the scan matcher on every cost metric, loss, weight option and limit cfear_check_reg_params accepts.

Scans are uploaded from the oracle's cells (MapPointNormal(cells=...)), so that a 1e-9 difference in a mean cannot decide a
tie.  The references are the CPU oracle (oracle/cfear_oracle.cpp) and, for everything point-wise, DenseProblem of
tests/test_oracle_pinning.py evaluated in np.longdouble with the losses restated from their definitions (`_loss`).

Bounds (the project's existing ones): association pairs identical, weights rtol 1e-12; H rtol 1e-10, g 1e-9, cost 1e-11
(test_association_pairs_and_normal_equations); GetCost residuals rtol 1e-9, cost and score 1e-11
(test_get_cost_matches_oracle...); registrations as _compare_register: status, outer_iters, lm_iters, num_residuals equal, pose
within 1e-4 m / 1e-5 rad, cost rtol 1e-9.  Raw residuals and Jacobians (no loss involved) against DenseProblem.raw: absolute,
(64 + 2 kappa) eps x the largest Jacobian entry of the problem.  The entries are sums of two or three products of a coordinate
(up to ~150 m) with a unit vector or a factor of the information matrix's Cholesky root, each product an ulp or two off (the
kernels' sincos is a polynomial): a few ulps of the largest entry, 64 as a loose ceiling over that.  P2D's root comes from a
2 x 2 inverse by cofactors whose determinant cancels, so fp64 leaves a relative error of the order of kappa(tar_cov) eps in
it whoever computes it: NumPy's float64 evaluation of the same formulas is 0.1 - 0.25 kappa eps from the longdouble one on
these problems (kappa = 52 ... 9 700 over the regularizations used); the allowance is 2 kappa eps, kappa the problem's largest.

Evaluation poses of the point-wise test (a).  For every (cost, limit) the reference must show >= 5 % of the blocks on each
side of the branch a loss has (s <= a^2 / s > a^2 for Huber and Tukey, ln(1 + s) <= 1 / > 1 for Combined); _EVAL holds, per cost
and limit, the start offset (a multiple k of (0.4, -0.3, 0.01) from the truth) and the evaluation point (the start pose +
d x (0.05, -0.02, 0.003)) chosen on the CPU oracle for that.  Three cases cannot get there by any pose of scan 1 or 2 against
scan 0 (P2P at 0.1, P2D at 0.1 and 0.3: at the true pose 1 % of the P2D blocks lie within 0.1 sigma): they move to a copy of
scan 0 as the moving scan at (0.01, -0.005, 0.001), where the residual grows from 0 at the sensor outwards.

The 42 instantiations of matcher_kernel (3 costs x {Huber compiled in, runtime loss} x 7 forms) and the test that launches each:
  4 wavefronts, regular      x 6   test_forms[*] (4, 40) and (4, 14); test_register_matrix in any batch the library routes there
  2 wavefronts               x 6   test_forms[*] (2, 20)
  8 wavefronts, 128 VGPRs    x 6   test_forms[*] (8, 80) with 4 x 72 jobs (more than one workgroup per CU)
  8 wavefronts, wide         x 6   test_forms[*] (8, 80) with 72 jobs; test_register_matrix (two jobs: 8 wavefronts, wide)
  16 wavefronts              x 6   test_forms[*] (16, 160)
  cost-only, 4 wavefronts    x 6   test_get_cost_batch[cost-loss], the batch of more than two workgroups per CU
  cost-only, 8 wavefronts    x 6   test_get_cost_batch[cost-loss], the batch of six jobs
where [*] = P2P-Huber, P2P-SoftLOne, P2L-Huber, P2L-Tukey, P2D-Huber, P2D-Combined and [cost-loss] runs over all 18 pairs
(Huber takes the compiled-in build, the other five the runtime-loss build).  eval_kernel's own loss_eval call (cfear_cost) is
run with all six losses by test_pointwise.

Replaced cases (section 3 of the issue: a start offset changed because the oracle's own deciding quantity lay within 1e-9
relative of its threshold): none.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL = 1e-4, 1e-5
COSTS = ("P2P", "P2L", "P2D")
LOSSES = ("None", "Huber", "Cauchy", "SoftLOne", "Combined", "Tukey")
BRANCHED = ("Huber", "Tukey", "Combined")
OFFSET = np.array([0.4, -0.3, 0.01])
DELTA = np.array([0.05, -0.02, 0.003])
SELF = "self"
# cost -> limit (or "Combined") -> (k, d), or SELF: see the module docstring
_EVAL = {"P2P": {0.1: SELF, 0.3: (0, 0), 1.0: (1, 1), 2.0: (0, 10), "Combined": (0.5, 4)},
         "P2L": {0.1: (0, 1), 0.3: (0.5, 1), 1.0: (0.5, 10), 2.0: (1, 20), "Combined": (1, 10)},
         "P2D": {0.1: SELF, 0.3: SELF, 1.0: (0.1, 0), 2.0: (0.1, 0), "Combined": (0.1, 0)}}
_CACHE = {}
_WORST = {}


def _scene_cells(seed=1, n=4):
    """(oracle cells of the first n frames of synth.scene_v1(seed), ground truth); built once."""
    if (seed, n) not in _CACHE:
        from oracle import pyoracle as O
        from tbv_slam_public_amd import synth
        imgs, gt, _ = synth.scene_v1(seed, n)
        cells = []
        for f in range(n):
            sr, si, sc = O.kstrongest(imgs[f], 40, 60)
            cells.append(O.surface_points(O.kstrongest_cloud(sr, si, sc, 0.0438, 2.5), 3.0, 1.0, (0, 0), True))
        _CACHE[(seed, n)] = (cells, gt)
    return _CACHE[(seed, n)]


def _scene(seed=1, n=4):
    """(cells, their uploads, ground truth)."""
    if ("maps", seed, n) not in _CACHE:
        from tbv_slam_public_amd import api
        _CACHE[("maps", seed, n)] = [api.MapPointNormal(cells=c) for c in _scene_cells(seed, n)[0]]
    cells, gt = _scene_cells(seed, n)
    return cells, _CACHE[("maps", seed, n)], gt


def _reg(cost, loss, limit, wopt, **kw):
    from tbv_slam_public_amd import api
    reg = api.n_scan_normal_reg(cost, loss, limit, wopt)
    for k, v in kw.items():
        assert hasattr(reg.par, k), k
        setattr(reg.par, k, v)
    return reg


def _opar(reg):
    """The oracle's parameter record for a device one, field by field."""
    from oracle import pyoracle as O
    p = reg.par
    o = O.reg_params(cost=p.cost, loss=p.loss, loss_limit=p.loss_limit, weight_opt=p.weight_opt, max_outer=p.max_itr_association,
                     max_inner=p.max_itr_solver, min_outer=p.min_itr, radius=p.radius, cov_scale=p.cov_scale,
                     regularization=p.regularization, first_itr=p.itr)
    o.score_tolerance = p.score_tolerance
    return o


def _note(test, loss, **dev):
    """Keeps the worst deviation seen per (test, loss, quantity); written out where CFEAR_MATRIX_REPORT names a file."""
    slot = _WORST.setdefault(test, {}).setdefault(loss, {})
    for k, v in dev.items():
        slot[k] = max(slot.get(k, 0.0), float(v))
    path = os.environ.get("CFEAR_MATRIX_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_WORST, f, indent=1, sort_keys=True)


def _pointwise_problem(cost, key, n_scans, upload=True):
    """(cells, uploads, association poses, evaluation point) of one point-wise problem: 2 or 3 scans, placed by _EVAL."""
    cells, gt = _scene_cells()
    maps = _scene()[1] if upload else [None] * len(cells)
    idx = list(range(n_scans))
    poses = np.array([gt[i] - gt[0] for i in idx], dtype=np.float64)
    sel = _EVAL[cost][key]
    if sel == SELF:
        idx[-1] = 0
        poses[-1] = [0.01, -0.005, 0.001]
        x = poses[-1].copy()
    else:
        poses[-1] += sel[0] * OFFSET
        x = poses[-1] + sel[1] * DELTA
    return [cells[i] for i in idx], [maps[i] for i in idx], poses, x


def _check_pointwise(reg, use, maps, poses, x, itr, cost, loss, limit, d2d=(1.0, 0.01)):
    """One association set on the device against the oracle and the longdouble DenseProblem.  -> share of blocks beyond the branch"""
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    from tests.test_oracle_pinning import DenseProblem
    opar = _opar(reg)
    cc = api.CeresCost(reg, maps, poses, itr=itr)
    try:
        pairs_g, w_g = cc.blocks()
        pairs_o, w_o = O.associate(use, poses, opar, itr)
        np.testing.assert_array_equal(pairs_g, pairs_o)
        np.testing.assert_allclose(w_g, w_o, rtol=1e-12)
        assert len(pairs_o) > 30
        prob = DenseProblem(use, poses, pairs_o, w_o, cost, loss, limit, regularization=d2d[1], cov_scale=d2d[0], dtype=np.longdouble)
        H, g, c = prob.normal_eq(x)
        H, g, c = H.astype(np.float64), g.astype(np.float64), float(c)
        Hg, gg, cg = cc.normal_eq(x)
        Ho, go, co, nres = O.normal_eq(use, poses, opar, itr, x)
        for Hr, gr, cr in ((H, g, c), (Ho, go, co)):                  # the independent reference, then the oracle
            np.testing.assert_allclose(Hg, Hr, rtol=1e-10, atol=1e-10)
            np.testing.assert_allclose(gg, gr, rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(cg, cr, rtol=1e-11)
        r, J = cc.evaluate(x)
        assert r.shape[0] == nres == len(pairs_o) * prob.rpb
        rr, Jr = prob.raw(x)
        Jr = Jr.reshape(-1, 3).astype(np.float64)
        kappa = float(prob.kappa.max()) if cost == "P2D" else 0.0
        atol = (64 + 2 * kappa) * np.finfo(np.float64).eps * max(1.0, float(np.abs(Jr).max()))
        np.testing.assert_allclose(r, rr.reshape(-1).astype(np.float64), rtol=0, atol=atol)
        np.testing.assert_allclose(J, Jr, rtol=0, atol=atol)
        _note("pointwise", loss, H=np.abs(Hg - H).max() / np.abs(H).max(), g=np.abs(gg - g).max() / max(np.abs(g).max(), 1e-300),
              cost=abs(cg - c) / max(abs(c), 1e-300), raw=max(np.abs(r - rr.reshape(-1).astype(np.float64)).max(), np.abs(J - Jr).max()) / atol)
        if loss == "Combined":
            return float((np.log1p(prob.sq) > 1.0).mean())
        return float((prob.sq > np.longdouble(limit) ** 2).mean())
    finally:
        cc.close()


# =====================================================================================================
# a. point-wise: 90 triples x 4 limits x {2, 3 scans} x itr {1, 2}
# =====================================================================================================
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("cost", COSTS)
def test_pointwise(cost, loss):
    n = 0
    for limit in (0.1, 0.3, 1.0, 2.0):
        key = "Combined" if loss == "Combined" else limit
        for n_scans in (2, 3):
            use, maps, poses, x = _pointwise_problem(cost, key, n_scans)
            for itr in (1, 2):
                for wopt in range(5):
                    share = _check_pointwise(_reg(cost, loss, limit, wopt), use, maps, poses, x, itr, cost, loss, limit)
                    if loss in BRANCHED:
                        assert 0.05 <= share <= 0.95, (cost, loss, limit, n_scans, itr, share)
                    n += 1
    assert n == 80


# =====================================================================================================
# b. GetCost: the cost-only kernels, every (cost, loss), the 4- and the 8-wavefront build
# =====================================================================================================
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("cost", COSTS)
def test_get_cost_batch(cost, loss):
    """Six three-scan jobs: a batch of six (at most two workgroups per CU and not two-scan pairs: first_form gives 8 wavefronts)
    and the same six repeated to more than two workgroups per CU (4 wavefronts).  No job is `large` (reserved == 0 in a
    registration of the same jobs: RegLaunchHint::big_pass / whole_cu stay off, which would force 8 wavefronts), so the batch
    size alone decides, as first_form states it; the profile counters name both builds "get_cost" and can only count launches."""
    import torch
    from oracle import pyoracle as O
    cells, maps, gt = _scene()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    limit = 0.3 if cost == "P2L" else 1.0                            # blocks on both sides of the branch (ISSUE table)
    reg = _reg(cost, loss, limit, 4)
    truth = np.array([gt[i] - gt[0] for i in range(3)], dtype=np.float64)
    jobs, ojobs = [], []
    for q, k in enumerate((0.0, 0.25, 0.5, 1.0, 1.5, 2.0)):
        T = truth.copy()
        T[-1] += k * OFFSET * (1 if q % 2 == 0 else -1)
        jobs.append((maps[:3], T))
        ojobs.append((cells[:3], T))
    assert (reg.RegisterBatch(jobs)["reserved"] == 0.0).all()
    reps = (2 * n_cu) // len(jobs) + 1
    for itr in (0, 1, 5):                                            # GetCost's radius follows the leftover itr_
        reg.par.itr = itr
        ref = [O.get_cost(c, T, _opar(reg)) for c, T in ojobs]
        for batch, launches in ((jobs, 1), (jobs * reps, 1)):
            assert (len(batch) <= 2 * n_cu) == (batch is jobs)
            reg.ctx.profile_enable(True); reg.ctx.profile_read(reset=True)
            out = reg.GetCostBatch(batch)
            prof = reg.ctx.profile_read(reset=True); reg.ctx.profile_enable(False)
            assert prof["get_cost"][1] == launches and not any(v[1] for k, v in prof.items() if k.startswith("register")), prof
            for i, r in enumerate(out):
                ok_o, cost_o, res_o, score_o = ref[i % len(jobs)]
                assert ok_o and r["status"] == 0 and r["num_residuals"] == res_o.shape[0]
                np.testing.assert_allclose(r["final_cost"], cost_o, rtol=1e-11)
                np.testing.assert_allclose(r["score"], score_o, rtol=1e-11)
        # the robustified residual vector comes from the single-job entry (cfear_get_cost: eval_kernel)
        for (m, T), (ok_o, cost_o, res_o, score_o) in zip(jobs, ref):
            ok, cst, res = reg.GetCost(m, T)
            assert ok and res.shape == res_o.shape
            np.testing.assert_allclose(cst, cost_o, rtol=1e-11)
            np.testing.assert_allclose(res, res_o, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(reg.getScore(), score_o, rtol=1e-11)


# =====================================================================================================
# c. Register: 90 triples x limits {0.1, 0.3, 1.0}, a pair and a 4-scan window per parameter set
# =====================================================================================================
def _register_jobs():
    cells, maps, gt = _scene()
    jobs, ojobs = [], []
    for idx in ([0, 2], [0, 1, 2, 3]):
        T = np.array([gt[i] - gt[0] for i in idx], dtype=np.float64)
        T[-1] += OFFSET
        jobs.append(([maps[i] for i in idx], T))
        ojobs.append(([cells[i] for i in idx], T))
    return jobs, ojobs


def _judge_register(reg, r, c, T, what, note=None):
    """The statements of test_gpu_register._compare_register on one record of a batch."""
    from oracle import pyoracle as O
    ok_o, po, ro = O.register(c, T, _opar(reg))
    assert (r["status"] == 0) == ok_o, (what, int(r["status"]), ok_o)
    got = (int(r["outer_iters"]), int(r["lm_iters"]), int(r["num_residuals"]))
    assert got == (ro.outer_iters, ro.lm_iters, ro.num_residuals), (what, got, (ro.outer_iters, ro.lm_iters, ro.num_residuals))
    assert np.abs(r["pose"][:2] - po[-1, :2]).max() <= POS_TOL, (what, r["pose"], po[-1])
    assert abs(r["pose"][2] - po[-1, 2]) <= ROT_TOL, (what, r["pose"], po[-1])
    np.testing.assert_allclose(r["final_cost"], ro.final_cost, rtol=1e-9, atol=1e-12, err_msg=str(what))
    np.testing.assert_allclose(r["score"], ro.score, rtol=1e-9, atol=1e-12, err_msg=str(what))
    if note:
        _note("register", note, pose=np.abs(r["pose"][:2] - po[-1, :2]).max(), angle=abs(r["pose"][2] - po[-1, 2]),
              cost=abs(r["final_cost"] - ro.final_cost) / max(abs(ro.final_cost), 1e-300))
    return ok_o, ro


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("cost", COSTS)
def test_register_matrix(cost, loss):
    jobs, ojobs = _register_jobs()
    n_ok = 0
    for limit in (0.1, 0.3, 1.0):
        for wopt in range(5):
            reg = _reg(cost, loss, limit, wopt)
            out = reg.RegisterBatch(jobs)
            for r, (c, T) in zip(out, ojobs):
                ok_o, _ = _judge_register(reg, r, c, T, (cost, loss, limit, wopt, len(c)), note=loss)
                n_ok += ok_o
    assert n_ok == 30                                                 # the oracle registers every case of this grid


# =====================================================================================================
# d. forms: every build of the full registration, for each cost with Huber and with one runtime loss
# =====================================================================================================
@pytest.mark.parametrize("cost,loss,opt", [("P2P", "Huber", 4), ("P2P", "SoftLOne", 3), ("P2L", "Huber", 0), ("P2L", "Tukey", 2),
                                           ("P2D", "Huber", 0), ("P2D", "Combined", 1)])
def test_forms(cost, loss, opt):
    """test_gpu_register.test_every_form_of_the_matcher_agrees, row by row, for the builds that test leaves out."""
    from tbv_slam_public_amd import api
    from tbv_slam_public_amd import _lib as L
    from tests.test_gpu_register import _cells
    rng = np.random.default_rng(5)
    reg = _reg(cost, loss, 0.1, opt)
    reg.SetParameters(8, 100)
    jobs, ojobs = [], []
    for seed in (31, 32):
        cells, gt = _cells(seed, [0, 1, 2, 3, 4], k=20)
        scans = [api.MapPointNormal(cells=c) for c in cells]
        for rep in range(36):
            n = int(rng.integers(2, 6))
            idx = sorted(rng.choice(5, size=n, replace=False).tolist())
            T = np.array([gt[i] for i in idx], dtype=np.float64)
            T[-1] += np.concatenate([rng.normal(0, 0.4, 2), rng.normal(0, 0.015, 1)])
            jobs.append(([scans[i] for i in idx], T))
            ojobs.append(([cells[i] for i in idx], T))
    base = reg.RegisterBatch(jobs)
    runs = {}
    try:
        for waves, kb in ((4, 40), (4, 14), (8, 80), (16, 160), (2, 20)):
            reg.ctx.set_option(L.OPT_MATCHER_WAVES, waves); reg.ctx.set_option(L.OPT_MATCHER_LDS_KB, kb)
            runs["%d x %d KB" % (waves, kb)] = reg.RegisterBatch(jobs)
        # 72 workgroups (at most one per CU) took the wide 8-wavefront build above; 288 take the 128-VGPR build
        reg.ctx.set_option(L.OPT_MATCHER_WAVES, 8); reg.ctx.set_option(L.OPT_MATCHER_LDS_KB, 80)
        many = reg.RegisterBatch(jobs * 4)
        for a, b in zip(runs["8 x 80 KB"], many[:len(jobs)]):
            for f in ("status", "outer_iters", "lm_iters", "num_residuals", "final_cost", "score"):
                assert a[f] == b[f], (cost, f, a[f], b[f])
            assert np.array_equal(a["pose"], b["pose"]), (cost, a["pose"], b["pose"])
    finally:
        reg.ctx.set_option(L.OPT_MATCHER_WAVES, 0); reg.ctx.set_option(L.OPT_MATCHER_LDS_KB, 0)
    for name, out in runs.items():
        for a, b in zip(base, out):
            key = lambda r: (int(r["status"]), int(r["outer_iters"]), int(r["lm_iters"]), int(r["num_residuals"]))
            assert key(a) == key(b), (cost, name, key(a), key(b))
            np.testing.assert_allclose(b["pose"], a["pose"], rtol=0, atol=1e-11, err_msg=name)
            np.testing.assert_allclose(b["final_cost"], a["final_cost"], rtol=1e-10, err_msg=name)
    for r, (c, T) in list(zip(runs["4 x 14 KB"], ojobs))[::6]:            # a sample against the oracle itself
        _judge_register(reg, r, c, T, (cost, loss, "4 x 14 KB"))


# =====================================================================================================
# e. the remaining parameters, against the oracle
# =====================================================================================================
@pytest.mark.parametrize("field,value", [("radius", 1.0), ("radius", 3.0), ("min_itr", 0), ("min_itr", 6), ("score_tolerance", 0.0),
                                         ("score_tolerance", 1e-2), ("max_itr_solver", 0), ("max_itr_solver", 1),
                                         ("max_itr_association", 1)])
def test_register_with_other_parameters(field, value):
    """With max_itr_solver = 0 Ceres 2.1 records iteration 0 and stops with NO_CONVERGENCE (MaxSolverIterationsReached is
    checked after the record is pushed, trust_region_minimizer.cc), which IsSolutionUsable() accepts: the oracle does exactly
    that, each solve leaves the pose where it was, and Register ends with status ok -- the device must do the same."""
    jobs, ojobs = _register_jobs()
    for cost, loss, limit, wopt in (("P2P", "Huber", 0.3, 4), ("P2L", "Cauchy", 0.3, 0), ("P2D", "Tukey", 1.0, 2), ("P2L", "Huber", 0.1, 0)):
        reg = _reg(cost, loss, limit, wopt, **{field: value})
        out = reg.RegisterBatch(jobs)
        for r, (c, T) in zip(out, ojobs):
            ok_o, ro = _judge_register(reg, r, c, T, (field, value, cost, loss, len(c)))
            assert ok_o
            if field == "max_itr_solver" and value == 0:
                assert ro.lm_iters == 0 and np.array_equal(r["pose"], T[-1])
            if field == "max_itr_association":
                assert ro.outer_iters == 2                             # the loop counter after its only pass
        if field == "radius":                                          # the association itself, at both radii of the schedule
            use, maps, poses, x = _pointwise_problem(cost, 1.0, 3)
            for itr in (1, 2):
                _check_pointwise(reg, use, maps, poses, x, itr, cost, loss, limit)


@pytest.mark.parametrize("cov_scale,regularization", [(1.0, 0.0), (1.0, 0.1), (0.25, 0.01), (4.0, 0.01)])
def test_p2d_cov_scale_and_regularization(cov_scale, regularization):
    """tar_cov = (regularization I + R Sigma R^T) cov_scale, inverted, then its Cholesky root (n_scan_normal.cpp:288-297):
    point-wise against DenseProblem, which takes both, and a registration against the oracle."""
    jobs, ojobs = _register_jobs()
    for loss, limit in (("Huber", 1.0), ("Cauchy", 0.3), ("Tukey", 2.0)):
        reg = _reg("P2D", loss, limit, 4, cov_scale=cov_scale, regularization=regularization)
        for n_scans in (2, 3):
            use, maps, poses, x = _pointwise_problem("P2D", 1.0, n_scans)
            for itr in (1, 2):
                _check_pointwise(reg, use, maps, poses, x, itr, "P2D", loss, limit, d2d=(cov_scale, regularization))
        out = reg.RegisterBatch(jobs)
        for r, (c, T) in zip(out, ojobs):
            _judge_register(reg, r, c, T, (cov_scale, regularization, loss, len(c)))


# =====================================================================================================
# f. refusals
# =====================================================================================================
def _bad_params():
    from tbv_slam_public_amd import api
    out = []
    for field, value in (("cost", -1), ("cost", 3), ("loss", -1), ("loss", 6), ("weight_opt", -1), ("weight_opt", 5), ("radius", 0.0),
                         ("radius", -2.0), ("radius", float("nan")), ("max_itr_association", 0), ("max_itr_solver", -1)):
        reg = api.n_scan_normal_reg("P2L")
        setattr(reg.par, field, value)
        out.append(("%s=%r" % (field, value), C.byref(reg.par), reg))
    out.append(("null", None, api.n_scan_normal_reg("P2L")))
    return out


def test_refusals():
    """Every parameter record cfear_check_reg_params must refuse, through the four entries that take one: CFEAR_ERR_INVALID_ARGUMENT, the
    input poses untouched, the outputs as they were, and not one kernel launched (the profile counters stay 0)."""
    from tbv_slam_public_amd import api, _lib as L
    cells, maps, gt = _scene()
    ctx = api.default_context()
    lib = ctx._lib
    poses0 = np.array([[0.0, 0.0, 0.0], gt[1] - gt[0] + OFFSET])
    d3 = C.POINTER(C.c_double)
    n_bad = 0
    for name, par, reg in _bad_params():
        poses = poses0.copy()
        hs = reg._handles(maps[:2])
        job = (L.RegJob * 1)()
        job[0].scans = C.cast(hs, C.POINTER(C.c_void_p)); job[0].n_scans = 2; job[0].poses_xyt = poses.ctypes.data_as(d3)
        ctx.profile_enable(True); ctx.profile_read(reset=True)
        res = L.RegResult()
        res.status = 77
        rcs = [lib.cfear_register(ctx.h, hs, 2, poses.ctypes.data_as(d3), par, C.byref(res))]
        out = np.zeros(1, L.RESULT_DTYPE)
        out["status"] = 77
        rcs.append(lib.cfear_register_batch(ctx.h, job, 1, par, out.ctypes.data))
        assert out["status"][0] == 77
        rcs.append(lib.cfear_get_cost_batch(ctx.h, job, 1, par, out.ctypes.data))
        assert out["status"][0] == 77 and res.status == 77
        h = C.c_void_p(123)
        rcs.append(lib.cfear_cost_prepare(ctx.h, hs, 2, poses.ctypes.data_as(d3), par, 1, C.byref(h)))
        assert not h.value                                            # no object comes back
        prof = ctx.profile_read(reset=True); ctx.profile_enable(False)
        assert rcs == [L.ERR_INVALID_ARGUMENT] * 4, (name, rcs)
        assert not any(v[1] for v in prof.values()), (name, prof)
        np.testing.assert_array_equal(poses, poses0)
        n_bad += 1
    assert n_bad == 12
    good = api.n_scan_normal_reg("P2L")                               # and the same calls with a valid record do launch
    ctx.profile_enable(True); ctx.profile_read(reset=True)
    assert good.Register(maps[:2], poses0)[0]
    prof = ctx.profile_read(reset=True); ctx.profile_enable(False)
    assert prof["register"][1] >= 1, prof


# =====================================================================================================
# g. Tukey where every block is an outlier
# =====================================================================================================
def test_tukey_with_every_block_beyond_the_limit():
    """P2D, Tukey 0.1 from the usual start offset: rho' = 0 on every block, so H = 0 and g = 0.  A legal input, run once; status
    and counts are the oracle's (it stops at iteration 0 on the gradient tolerance, and so must the device)."""
    from oracle import pyoracle as O
    from tests.test_oracle_pinning import DenseProblem
    jobs, ojobs = _register_jobs()
    reg = _reg("P2D", "Tukey", 0.1, 0)
    c, T = ojobs[0]
    pairs, w = O.associate(c, T, _opar(reg), 1)
    prob = DenseProblem(c, T, pairs, w, "P2D", "Tukey", 0.1, dtype=np.longdouble)
    H, g, _ = prob.normal_eq(T[-1])
    assert len(pairs) > 30 and not H.any() and not g.any() and (prob.sq > np.longdouble(0.1) ** 2).all()
    out = reg.RegisterBatch(jobs[:1])
    ok_o, po, ro = O.register(c, T, _opar(reg))
    r = out[0]
    assert (r["status"] == 0) == ok_o
    assert (int(r["outer_iters"]), int(r["lm_iters"]), int(r["num_residuals"])) == (ro.outer_iters, ro.lm_iters, ro.num_residuals)
    np.testing.assert_allclose(r["final_cost"], ro.final_cost, rtol=1e-9, atol=1e-12)
    assert np.abs(r["pose"][:2] - po[-1, :2]).max() <= POS_TOL and abs(r["pose"][2] - po[-1, 2]) <= ROT_TOL
