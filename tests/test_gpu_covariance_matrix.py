"""GPU: covariance by cost sampling (approximateCovarianceBySampling, odometrykeyframefuser.cpp:261-380 and
loopclosure.cpp:99-208) on every branch, sample count and launch form: the sampling mode of the cost-only matcher_kernel
(n_samples > 0), the host loop that carries sample costs, and the host fit (csrc/covfit.hpp).

Cases: tests/covariance_cases.py, judged on the CPU oracle by tests/test_covariance_cases_cpu.py.  Scans are uploaded from the
oracle's cells; poses, leftover itr_ and the registration summary are the oracle's, so only the sampling and the fit differ.

Bounds.  Sample grid: bit-equal to the oracle's.  Sample cost against the oracle: rtol 1e-11 (the matcher matrix's GetCost
bound; no pair needs the older 1e-10).  Sampling launch against a GetCostBatch of the n^3 explicit poses, and a job in a
batch against the same job alone: rtol 1e-12 (the project's single-versus-batch bound).  Carried values: exactly the
previous record's.  The fit: the library's covariance against the mpmath fit of the library's OWN returned samples at
covfit_ref.FIT_TOL (16 x NumPy's worst deviation from mpmath, measured in tests/test_covfit_cpu.py), in units of the
covariance's standard deviations -- the 1e-4 against the oracle's covariance (which also carries the fit's amplification of
the 1e-11 sample differences) stays beside it.  A rejected fit returns exactly diag(0.01, 0.01, 0, 0, 0, 1e-4).

Which test launches which cost-only build in sampling mode (NW = wavefronts; the Huber build is compiled in, the other
five losses take the runtime-loss build; "rounds" = samples one workgroup walks = ceil(n^3 / blocks_per_job)):
  8 NW, half a CU's LDS, 1 round      x 18  test_every_sample[cost-loss]: one three-scan job, 27 workgroups
  4 NW, half a CU's LDS, 1 round      x 1   test_carry_and_rejections, test_sample_counts (n <= 5): a two-scan job alone
  4 NW, regular, rounds 1 and 2       x 6   test_rounds_per_workgroup[*]: 40 jobs x 26 workgroups (workgroup 0: samples 0, 26)
  4 NW, regular, rounds 3 and 4       x 6   test_rounds_per_workgroup[*]: 128 jobs x 8
  4 NW, regular, 27 rounds            x 6   test_rounds_per_workgroup[*]: 1100 jobs x 1 (more than 1024 jobs)
  4 NW x 14 KB, 4 NW x 40 KB, 27 rounds x 6 test_rounds_per_workgroup[*]: the 1100 jobs with the form forced
  8 NW x 80 KB, 27 rounds             x 6   test_rounds_per_workgroup[*]: the 1100 jobs with the form forced
  4 NW, 3 and 4 rounds of 3375        x 1   test_sample_counts: n = 15, one two-scan job, 1024 workgroups (P2L, Huber)
  8 NW, the CU's whole LDS, 1 round   x 2   test_large_forms[dense], [huge] alone: first_form() gives a lone large job all of it
  8 NW, half a CU (big_pass), 1 round x 1   test_large_forms[dense] x 70: three dense scans (reserved == 1 in a registration)
  8 NW, the CU's whole LDS (whole_cu) x 1   test_large_forms[huge] x 70: a pair of scans of ~4 000 cells
where [*] = P2P-Huber, P2P-SoftLOne, P2L-Huber, P2L-Tukey, P2D-Huber, P2D-Combined.
The fuser's `prior` mode (blocks_per_job = 1 behind a Register launch) stays with
test_gpu_covariance.test_odometry_with_cov_sampling_matches_oracle_fuser: the fuser exposes neither the submap's poses nor
final_cost / num_residuals of its registration, so the same job cannot be rebuilt through the public entry without new ABI.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import covariance_cases as CC      # noqa: E402
from tests import covfit_ref as R             # noqa: E402

REJECTED = np.diag([0.01, 0.01, 0, 0, 0, 1e-4])
_CACHE = {}
_WORST = {}


def _note(test, **dev):
    """Keeps the worst deviation seen per (test, quantity); written out where CFEAR_MATRIX_REPORT names a file."""
    slot = _WORST.setdefault(test, {})
    for k, v in dev.items():
        slot[k] = max(slot.get(k, 0.0), float(v))
    path = os.environ.get("CFEAR_MATRIX_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_WORST, f, indent=1, sort_keys=True)


def _maps(scene_key):
    if scene_key not in _CACHE:
        from tbv_slam_public_amd import api
        _CACHE[scene_key] = [api.MapPointNormal(cells=c) for c in CC.scene(scene_key)[0]]
    return _CACHE[scene_key]


def _reg(case):
    """The device registration object of a case, held field by field to the oracle's parameter record."""
    from tbv_slam_public_amd import api
    from tests.test_gpu_matcher_matrix import _opar
    reg = api.n_scan_normal_reg(case["cost"], case["loss"], case["limit"], case["wopt"])
    reg.SetParameters(case["outer"], case["inner"])
    reg.par.itr = case["first_itr"]
    a, b = _opar(reg), CC.oracle_par(case)
    for name, _ in a._fields_:
        assert getattr(a, name) == getattr(b, name), (case["name"], name)
    return reg


def _job(case):
    maps = _maps(case["scene"])
    return [maps[i] for i in case["window"]], np.array(case["poses"], dtype=np.float64)


def _record(case):
    from tbv_slam_public_amd import _lib as L
    r = np.zeros(1, L.RESULT_DTYPE)
    r["final_cost"], r["num_residuals"], r["outer_iters"] = case["summary"][0], case["summary"][1], case["first_itr"]
    r["pose"] = case["poses"][-1]
    return r


def _sp(reg, case):
    return reg.sampling_params(case["xy_range"], case["yaw_range"], case["n"], case["scaler"])


def _sample_batch(reg, jobs, regs, sp):
    """cfear_covariance_by_sampling_batch with a samples buffer -> (ok [n] bool, cov [n, 6, 6], samples [n, m, 4])"""
    from tbv_slam_public_amd import _lib as L
    arr, n, _keep = reg.PrepareBatch(jobs)
    regs = np.ascontiguousarray(regs, dtype=L.RESULT_DTYPE)
    assert regs.shape == (n,)
    m = sp.samples_per_axis ** 3
    cov = np.full((n, 6, 6), np.nan)
    smp = np.full((n, m, 4), np.nan)
    ok = np.full(n, -1, np.int32)
    reg.ctx.check(reg.ctx._lib.cfear_covariance_by_sampling_batch(reg.ctx.h, arr, n, C.byref(reg.par), regs.ctypes.data, C.byref(sp),
                                                                  cov.ctypes.data, smp.ctypes.data, ok.ctypes.data))
    assert set(ok.tolist()) <= {0, 1}
    return ok.astype(bool), cov, smp


def _profiled(reg, fn):
    reg.ctx.profile_enable(True); reg.ctx.profile_read(reset=True)
    try:
        out = fn()
        prof = reg.ctx.profile_read(reset=True)
    finally:
        reg.ctx.profile_enable(False)
    return out, prof


def _only_get_cost(prof, launches):
    assert prof["get_cost"][1] == launches and not any(v[1] for k, v in prof.items() if k.startswith("register")), prof


def _check_fit(name, ok, cov, smp, case):
    """The library's verdict and covariance against the mpmath fit of the library's own samples."""
    fc, nres = case["summary"]
    if nres - 3 == 0:
        assert not ok
    else:
        exp_ok, ref3, _ = R.mp_fit(smp[:, :3], smp[:, 3], fc / (nres - 3), case["scaler"])
        assert ok == exp_ok, name
        if ok and fc != 0.0:
            sign = 1.0 if nres > 3 else -1.0                      # (10, 2): the reference's negative scale
            dev = R.deviation(sign * R.block3(cov), sign * ref3)
            _note("fit", deviation=dev)
            assert dev <= R.FIT_TOL, (name, dev)
    rest = cov.copy()
    if ok:
        rest[np.ix_(R.IDX3, R.IDX3)] = 0
        assert np.array_equal(rest, np.diag([0, 0, 1.0, 1.0, 1.0, 0])), name       # Identity elsewhere (:368)
    else:
        assert np.array_equal(cov, REJECTED), name


def _check_against_oracle(case, ok, cov, smp, explicit=True):
    """One sampled job against the oracle (grid, costs, verdict, covariance) and against explicit GetCost jobs."""
    name = case["name"]
    s = CC.oracle_samples(case)
    exp_ok, exp_cov, exp_smp = CC.oracle_cov(case)
    assert np.array_equal(smp[:, :3], exp_smp[:, :3]), name                        # the sample grid itself is exact
    np.testing.assert_allclose(smp[:, 3], exp_smp[:, 3], rtol=1e-11, atol=0, err_msg=name)
    good = exp_smp[:, 3] != 0
    _note("samples", vs_oracle=(np.abs(smp[good, 3] - exp_smp[good, 3]) / np.abs(exp_smp[good, 3])).max() if good.any() else 0.0)
    for i in np.flatnonzero(~s["ok"]):                                             # carried exactly, where the oracle carries
        assert smp[i, 3] == (smp[i - 1, 3] if i else 0.0), (name, i)
    assert ok == exp_ok, name
    if exp_ok:
        np.testing.assert_allclose(R.block3(cov), R.block3(exp_cov), rtol=1e-4, atol=1e-14, err_msg=name)
    if exp_ok and case["summary"][0] != 0.0:
        _note("cov", vs_oracle=(np.abs(R.block3(cov) - R.block3(exp_cov)) / np.abs(R.block3(exp_cov))).max())
    _check_fit(name, ok, cov, smp, case)
    if explicit:
        reg = _reg(case)
        maps, poses = _job(case)
        jobs = []
        for o in s["offsets"]:
            p = poses.copy()
            p[-1] = [o[0] + poses[-1][0], o[1] + poses[-1][1], o[2] + poses[-1][2]]
            jobs.append((maps, p))
        out = reg.GetCostBatch(jobs)
        assert np.array_equal(out["status"] == 0, s["ok"]), name
        assert np.array_equal(out["num_residuals"][s["ok"]], s["blocks"][s["ok"]] * (1 if case["cost"] == "P2L" else 2)), name
        assert np.array_equal(out["pose"], smp[:, :3] + poses[-1]), name
        np.testing.assert_allclose(smp[s["ok"], 3], out["final_cost"][s["ok"]], rtol=1e-12, atol=0, err_msg=name)
        if s["ok"].any():
            _note("samples", vs_explicit=(np.abs(smp[s["ok"], 3] - out["final_cost"][s["ok"]]) / out["final_cost"][s["ok"]]).max())


def _run_case(case):
    """Batch entry (a batch of one) and single entry of one case; they must agree bit for bit."""
    reg = _reg(case)
    maps, poses = _job(case)
    sp, rec = _sp(reg, case), _record(case)
    (ok, cov, smp), prof = _profiled(reg, lambda: _sample_batch(reg, [(maps, poses)], rec, sp))
    _only_get_cost(prof, 1)
    ok1, cov1, smp1 = reg.approximateCovarianceBySampling(maps, poses, reg_result=rec[0], sampling=sp, want_samples=True)
    assert ok1 == bool(ok[0]) and np.array_equal(cov1, cov[0]) and np.array_equal(smp1, smp[0]), case["name"]
    return bool(ok[0]), cov[0], smp[0]


# =====================================================================================================
# 1. every sample of every (cost, loss) against the oracle and the one-pose launch; 5. the fit alone
# =====================================================================================================
@pytest.mark.parametrize("loss", CC.LOSSES)
@pytest.mark.parametrize("cost", CC.COSTS)
def test_every_sample(cost, loss):
    case = CC.by_name("matrix-%s-%s" % (cost, loss))
    ok, cov, smp = _run_case(case)
    _check_against_oracle(case, ok, cov, smp)
    if (cost, loss) in CC.ACCEPTED:
        assert ok


# =====================================================================================================
# 2. rounds per workgroup: the same jobs alone and in batches of 40, 128 and 1100, on every form
# =====================================================================================================
def _round_jobs(reg):
    """Five distinct jobs on the sampling matrix's scans (two- and three-scan windows), registered by the library itself; the
    leftover itr_ (GetCost's radius follows it) is set per job, since these registrations all stop after the same pass."""
    maps = _maps(CC.MATRIX_SCENE)
    _, truth = CC.scene(CC.MATRIX_SCENE)
    jobs = []
    for window, k in (((0, 1, 2), 1.0), ((0, 2), -1.5), ((1, 2), 0.5), ((0, 1), 2.5), ((0, 1, 2), -3.0)):
        T = np.array([CC.rel(truth[window[0]], truth[i]) for i in window], dtype=np.float64)
        T[-1] += k * np.array([0.4, -0.3, 0.01])
        jobs.append(([maps[i] for i in window], T))
    regs = reg.RegisterBatch(jobs)
    assert (regs["status"] == 0).all(), regs["status"]
    regs["outer_iters"] = [1, 2, 3, 4, 6]
    return [(sc, np.vstack([T[:-1], r["pose"]])) for (sc, T), r in zip(jobs, regs)], regs


@pytest.mark.parametrize("cost,loss,opt", [("P2P", "Huber", 4), ("P2P", "SoftLOne", 3), ("P2L", "Huber", 0), ("P2L", "Tukey", 2),
                                           ("P2D", "Huber", 0), ("P2D", "Combined", 1)])
def test_rounds_per_workgroup(cost, loss, opt):
    from tbv_slam_public_amd import api
    from tbv_slam_public_amd import _lib as L
    reg = api.n_scan_normal_reg(cost, loss, CC.matrix_limit(cost), opt)
    jobs, regs = _round_jobs(reg)
    sp = reg.sampling_params()
    alone = [_sample_batch(reg, [j], regs[i:i + 1], sp) for i, j in enumerate(jobs)]
    for (ok, cov, smp), j in zip(alone, jobs):
        assert np.isfinite(smp).all() and (smp[0, :, 3] > 0).all()
    rng = np.random.default_rng(11)

    def run(n_jobs, what):
        order = np.concatenate([rng.permutation(len(jobs)) for _ in range(n_jobs // len(jobs) + 1)])[:n_jobs]
        (ok, cov, smp), prof = _profiled(reg, lambda: _sample_batch(reg, [jobs[i] for i in order], regs[order], sp))
        _only_get_cost(prof, 1)
        for i in range(len(jobs)):
            mine = np.flatnonzero(order == i)
            assert len(mine) >= 2
            a_ok, a_cov, a_smp = alone[i]
            assert np.array_equal(smp[mine, :, :3], np.broadcast_to(a_smp[0, :, :3], (len(mine), 27, 3))), (what, i)
            np.testing.assert_allclose(smp[mine, :, 3], np.broadcast_to(a_smp[0, :, 3], (len(mine), 27)), rtol=1e-12, atol=0,
                                       err_msg="%s job %d" % (what, i))
            _note("rounds", vs_alone=(np.abs(smp[mine, :, 3] - a_smp[0, :, 3]) / a_smp[0, :, 3]).max())
            assert (ok[mine] == a_ok[0]).all(), (what, i)
            # the same job at another position of the same launch: the same bits
            assert (smp[mine] == smp[mine[0]]).all() and (cov[mine] == cov[mine[0]]).all(), (what, i)

    run(40, "40 x 26")
    run(128, "128 x 8")
    run(1100, "1100 x 1")
    try:
        for waves, kb in ((4, 14), (4, 40), (8, 80)):
            reg.ctx.set_option(L.OPT_MATCHER_WAVES, waves); reg.ctx.set_option(L.OPT_MATCHER_LDS_KB, kb)
            run(1100, "1100 x 1, %d x %d KB" % (waves, kb))
    finally:
        reg.ctx.set_option(L.OPT_MATCHER_WAVES, 0); reg.ctx.set_option(L.OPT_MATCHER_LDS_KB, 0)


# =====================================================================================================
# 3. the large forms: big_pass (a dense window) and whole_cu (a window beyond half a CU's LDS), n = 2
# =====================================================================================================
def _large_window(kind):
    """(cells, poses): "dense" = three scans of test_gpu_register's dense scene (7), ~1 600 cells each; "huge" = a pair of
    scans of ~3 600 cells, three dense scenes side by side 600 m apart (as test_large_registrations_on_every_form builds
    its windows).  Half a CU's LDS holds a job while 1792 + 160 last + 16 n_src + 2064 + 10 max_pad <= 76 544 bytes (mt_fit with
    the match table in global scratch): a pair beyond 2 790 cells per scan does not fit."""
    from oracle import pyoracle as O
    from tbv_slam_public_amd import synth
    from tests.test_gpu_register import _dense_cells, _rel
    if kind == "dense":
        frames = [0, 1, 2]
        cells, gt = _dense_cells(7, frames)
    else:
        frames = [0, 1]
        worlds = [synth.scene_dense(seed, 2) for seed in (9, 10, 11)]
        gt = worlds[0][1]
        cells = []
        for f in frames:
            parts = []
            for w, (imgs, _, _) in enumerate(worlds):
                sr, si, sc = O.kstrongest(imgs[f], 40, 60)
                c = O.surface_points(O.kstrongest_cloud(sr, si, sc, 0.0438, 2.5), 3.0, 1.0, (0, 0), True).copy()
                c["mean"][:, 0] += 600.0 * w
                parts.append(c)
            cells.append(np.concatenate(parts))
        assert all(3000 < len(c) < 5000 for c in cells), [len(c) for c in cells]
    poses = np.array([_rel(gt[0], gt[f]) for f in frames])
    poses[-1] += [0.25, -0.15, 0.006]
    return cells, poses


@pytest.mark.parametrize("kind", ["dense", "huge"])
def test_large_forms(kind):
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    from tbv_slam_public_amd import _lib as L
    from tests.test_gpu_register import _oracle_par
    cells, poses = _large_window(kind)
    maps = [api.MapPointNormal(cells=c) for c in cells]
    reg = api.n_scan_normal_reg("P2P", "Huber", 0.1, 4)
    r = reg.RegisterBatch([(maps, poses)])
    assert r["status"][0] == 0 and r["reserved"][0] == 1.0               # a large registration: RegLaunchHint::big_pass
    if kind == "huge":
        # beyond half a CU: with the regular form forced, neither it nor the half-CU form holds the job and the whole-CU form
        # (16 wavefronts) is the launch that does the work -- the capacity RegLaunchHint::whole_cu gives the cost-only launch
        try:
            reg.ctx.set_option(L.OPT_MATCHER_WAVES, 4); reg.ctx.set_option(L.OPT_MATCHER_LDS_KB, 40)
            _, prof = _profiled(reg, lambda: reg.RegisterBatch([(maps, poses)]))
        finally:
            reg.ctx.set_option(L.OPT_MATCHER_WAVES, 0); reg.ctx.set_option(L.OPT_MATCHER_LDS_KB, 0)
        assert prof["register_large16"][0] > 5 * max(prof["register"][0], prof["register_large"][0]), prof
    pg = np.vstack([poses[:-1], r["pose"][0]])
    sp = reg.sampling_params(samples_per_axis=2)
    (ok, cov, smp), prof = _profiled(reg, lambda: _sample_batch(reg, [(maps, pg)], r, sp))
    _only_get_cost(prof, 1)
    opar = _oracle_par(reg)
    opar.first_itr = int(r["outer_iters"][0])
    exp_ok, exp_cov, exp_smp = O.cov_by_sampling(cells, pg, opar, float(r["final_cost"][0]), int(r["num_residuals"][0]),
                                                 sp.xy_range, sp.yaw_range, 2, sp.covariance_scaler)
    off = R.offsets(2, sp.xy_range * 0.5, sp.yaw_range * 0.5)
    for o, c in zip(off, exp_smp[:, 3]):                                 # every sample succeeds on the oracle: no carried value
        p = pg.copy()
        p[-1] = [o[0] + pg[-1][0], o[1] + pg[-1][1], o[2] + pg[-1][2]]
        good, cost_o, _, _ = O.get_cost(cells, p, opar)
        assert good and cost_o == c
    assert np.array_equal(smp[0, :, :3], exp_smp[:, :3])
    np.testing.assert_allclose(smp[0, :, 3], exp_smp[:, 3], rtol=1e-11, atol=0)      # (an ERR_CAPACITY sample would carry)
    _note("large", vs_oracle=(np.abs(smp[0, :, 3] - exp_smp[:, 3]) / exp_smp[:, 3]).max())
    assert bool(ok[0]) == exp_ok
    case = dict(summary=(float(r["final_cost"][0]), int(r["num_residuals"][0])), scaler=sp.covariance_scaler)
    _check_fit(kind, bool(ok[0]), cov[0], smp[0], case)
    # The same job 70 times: 560 workgroups, more than two per CU, for which first_form() alone picks 4 wavefronts and a
    # quarter of the LDS: the batch's hint must override it (big_pass: 8 wavefronts on half a CU; whole_cu: the CU's whole LDS).
    import torch
    many = 70
    assert many * 8 > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    (okm, covm, smpm), prof = _profiled(reg, lambda: _sample_batch(reg, [(maps, pg)] * many, np.repeat(r, many), sp))
    _only_get_cost(prof, 1)
    np.testing.assert_allclose(smpm[:, :, 3], np.broadcast_to(smp[0, :, 3], (many, 8)), rtol=1e-12, atol=0)
    _note("large", vs_alone=(np.abs(smpm[:, :, 3] - smp[0, :, 3]) / smp[0, :, 3]).max())
    assert (smpm == smpm[0]).all() and (covm == covm[0]).all() and (okm == ok[0]).all()


# =====================================================================================================
# 4. carry and rejections
# =====================================================================================================
@pytest.mark.parametrize("name", ["failing-samples", "all-fail", "far-from-optimum", "summary-10-200", "summary-0-200", "summary-10-3",
                                  "summary-10-2"])
def test_carry_and_rejections(name):
    case = CC.by_name(name)
    ok, cov, smp = _run_case(case)
    _check_against_oracle(case, ok, cov, smp)
    if name == "failing-samples":
        assert smp[0, 3] == 0.0 and smp[3, 3] == 0.0 and smp[4, 3] > 0 and smp[5, 3] == smp[4, 3] and smp[26, 3] == smp[22, 3] != smp[13, 3]
    if name == "all-fail":
        assert (smp[:, 3] == 0.0).all() and not ok
    if name in ("far-from-optimum", "summary-10-3"):
        assert not ok and np.array_equal(cov, REJECTED)
    if name == "summary-0-200":
        assert ok and np.array_equal(R.block3(cov), np.zeros((3, 3)))
    if name == "summary-10-2":
        assert ok and cov[0, 0] < 0 and cov[5, 5] < 0


# =====================================================================================================
# 6. sample counts
# =====================================================================================================
@pytest.mark.parametrize("n", [1, 2, 4, 5, 15])
def test_sample_counts(n):
    case = CC.by_name("count-%d" % n)
    ok, cov, smp = _run_case(case)                                       # n = 15: 1024 workgroups walk 3 or 4 of the 3375 samples
    assert smp.shape == (n ** 3, 4)
    _check_against_oracle(case, ok, cov, smp, explicit=n <= 5)
