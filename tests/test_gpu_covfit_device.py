"""GPU: the covariance fit of cost sampling as a kernel (cfear_cov_fit_records, csrc/covfit.hip) against the host fit it
restates, for BYTE equality.

The yardstick is tests/cpp/covfit_check.cpp `fit`, the stand-alone g++ build of csrc/covfit.hpp that tests/test_covfit_cpu.py
holds to mpmath: its hex-float cov36 and verdict.  The driver takes costs, so the test forward-fills failed samples in NumPy
(a failed sample keeps the previous cost, 0.0 before the first good one) before feeding it; where the driver's verdict is 0,
or where num_residuals - 3 == 0 (GetCovarianceScaler refuses, the driver is not asked), the expected record is Register's
constant diag(0.01, 0.01, 0, 0, 0, 1e-4) with success = 0.

Jobs: the oracle's sample costs of every case of tests/covariance_cases.py (samples_per_axis 1, 2, 3, 4, 5 and 15; samples
that fail, a job whose samples all fail, num_residuals 3 and 2, a zero final cost, an indefinite fit) and, on the costs of
six of them, a first and a middle sample marked failed, every sample failed, num_residuals = 3, negated costs, a NaN and
an infinite cost.  One call takes one sampling grid, so the jobs are grouped by (samples_per_axis, ranges, scaler); a batch
of any length cycles over its group's jobs.  cov_fit_kernel runs one lane per job in workgroups of 256: the job counts are
1, one below / at / one above a wavefront (64) and a workgroup (256), and 4097.  Host pointers and device pointers must give
the same bytes."""
import numpy as np
import pytest

from tests import covariance_cases as K
from tests import covfit_ref as R

pytestmark = pytest.mark.gpu

CONST = np.zeros(36)
CONST[0] = CONST[7] = 0.01
CONST[35] = 1e-4
FAILED = -4                                                              # CFEAR_ERR_TOO_FEW_RESIDUALS: what a failed GetCost reports
COUNTS = (1, 63, 64, 65, 255, 256, 257)
MAIN = (3, 0.4, 0.0043625, 4.0)
_STATE = {}


def _job(name, case, raw, ok, summary=None):
    fc, nres = summary or case["summary"]
    return dict(name=name, key=(case["n"], case["xy_range"], case["yaw_range"], case["scaler"]), raw=np.asarray(raw, np.float64),
                ok=np.asarray(ok, bool), final_cost=float(fc), num_residuals=int(nres))


def _jobs():
    """Every distinct job, grouped by sampling grid -> {key: [job]}."""
    if "jobs" not in _STATE:
        out = []
        for c in K.cases():
            s = K.oracle_samples(c)
            out.append(_job(c["name"], c, s["raw"], s["ok"]))
        assert len(out) == K.EXPECTED_CASES
        for base in ("matrix-P2P-Huber", "matrix-P2L-Cauchy", "count-4", "count-15", "count-1", "count-2"):
            c = K.by_name(base)
            s = K.oracle_samples(c)
            m = c["n"] ** 3
            assert s["ok"].all() and len(s["raw"]) == m
            some = np.ones(m, bool)
            some[0] = False
            out.append(_job(base + " first failed", c, s["raw"], some))
            mid = np.ones(m, bool)
            mid[m // 2] = False
            out.append(_job(base + " middle failed", c, s["raw"], mid))
            out.append(_job(base + " every sample failed", c, s["raw"], np.zeros(m, bool)))
            out.append(_job(base + " num_residuals 3", c, s["raw"], s["ok"], (c["summary"][0], 3)))
            out.append(_job(base + " negated", c, -s["raw"], s["ok"]))
            for word, val in (("NaN", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
                bad = s["raw"].copy()
                bad[m // 3] = val
                out.append(_job(base + " " + word + " cost", c, bad, s["ok"]))
        groups = {}
        for j in out:
            groups.setdefault(j["key"], []).append(j)
        assert {k[0] for k in groups} >= {1, 2, 3, 4, 15} and MAIN in groups
        _STATE["jobs"] = groups
    return _STATE["jobs"]


def _filled(job):
    """The carry-over of failed samples, in NumPy."""
    costs, last = [], 0.0
    for good, c in zip(job["ok"], job["raw"]):
        if good:
            last = c
        costs.append(last)
    return np.array(costs)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_check(tmp_path_factory.mktemp("covfit_device"))


def _expected(exe, key):
    """(success [k] int32, cov [k, 36]) of the group's distinct jobs from the stand-alone host fit; computed once per group."""
    if ("exp", key) not in _STATE:
        n, xy, yaw, scaler = key
        ok, cov = [], []
        for j in _jobs()[key]:
            if j["num_residuals"] - 3 == 0:
                ok.append(0); cov.append(CONST)
                continue
            r = R.run_fit(exe, n, xy * 0.5, yaw * 0.5, j["final_cost"] / (j["num_residuals"] - 3), scaler, _filled(j))
            ok.append(int(r["verdict"])); cov.append(r["cov36"] if r["verdict"] else CONST)
        _STATE[("exp", key)] = (np.array(ok, np.int32), np.array(cov))
    return _STATE[("exp", key)]


def _records(key, count):
    from tbv_slam_public_amd import _lib as L
    jobs = _jobs()[key]
    m = key[0] ** 3
    idx = np.arange(count) % len(jobs)
    regs1, smp1 = np.zeros(len(jobs), L.RESULT_DTYPE), np.zeros((len(jobs), m), L.RESULT_DTYPE)
    for i, j in enumerate(jobs):
        regs1["final_cost"][i], regs1["num_residuals"][i] = j["final_cost"], j["num_residuals"]
        smp1["final_cost"][i] = j["raw"]
        smp1["status"][i] = np.where(j["ok"], 0, FAILED)
    return regs1[idx].copy(), smp1[idx].copy(), idx


def _run_both(key, count):
    """cfear_cov_fit_records with host pointers and with device pointers -> (success, cov [count, 36]) of the host call, after
    asserting that the device call left the same bytes."""
    import torch
    from tbv_slam_public_amd import api
    regs, smp, idx = _records(key, count)
    sp = api.n_scan_normal_reg.sampling_params(key[1], key[2], key[0], key[3])
    ok, cov = api.cov_fit_records(regs, smp, sp)
    d_ok, d_cov = api.cov_fit_records(torch.from_numpy(regs.view(np.uint8)).cuda(), torch.from_numpy(smp.view(np.uint8).reshape(-1)).cuda(), sp)
    assert d_ok.cpu().numpy().tobytes() == ok.tobytes() and d_cov.cpu().numpy().tobytes() == cov.tobytes()
    return ok, cov.reshape(count, 36), idx


def _assert_equal(exe, key, ok, cov, idx):
    exp_ok, exp_cov = _expected(exe, key)
    jobs = _jobs()[key]
    for row, i in enumerate(idx):
        assert ok[row] == exp_ok[i] and cov[row].tobytes() == exp_cov[i].tobytes(), (
            "job %d = %r: success %d (host fit %d)\n%r\n%r" % (row, jobs[i]["name"], ok[row], exp_ok[i], cov[row], exp_cov[i]))


def test_the_jobs_hold_what_they_are_meant_to(exe):
    """From the host fit alone: accepted and refused fits in the main group, every refusal reason present."""
    groups = _jobs()
    ok, cov = _expected(exe, MAIN)
    names = [j["name"] for j in groups[MAIN]]
    assert ok.sum() >= 15 and (ok == 0).sum() >= 8
    big = (15, 0.4, 0.0044, 4.0)                                            # among 3375 samples one carried cost leaves the fit convex
    assert any("failed" in j["name"] and o == 1 for j, o in zip(groups[big], _expected(exe, big)[0]))
    for word in ("negated", "NaN cost", "inf cost", "-inf cost", "every sample failed", "num_residuals 3", "far-from-optimum", "summary-10-3"):
        hit = [i for i, nm in enumerate(names) if word in nm]
        assert hit and all(ok[i] == 0 for i in hit), word
    for word in ("first failed", "middle failed"):                          # a carried cost bends the fit, it does not refuse it by itself
        assert any(word in nm for nm in names)
    assert any(not j["ok"][0] and j["ok"].any() for j in groups[(3, 800.0, 0.0043625, 4.0)])       # the oracle's own failed first sample
    assert any(not j["ok"].any() for j in groups[(3, 800.0, 0.0043625, 4.0)])                      # ... and its job without a good one
    acc = cov[ok == 1].reshape(-1, 6, 6)
    assert (acc[:, 2, 2] == 1.0).all() and (cov[ok == 0] == CONST).all()
    assert (acc[:, 0, 0] > 0).sum() >= 13 and (acc[:, 0, 0] == 0).any() and (acc[:, 0, 0] < 0).any()   # final_cost 0; num_residuals 2


@pytest.mark.parametrize("key", sorted(k for k in [(1, 0.4, 0.0043625, 4.0), (2, 0.4, 0.0043625, 4.0), (3, 0.4, 0.0043625, 4.0),
                                                   (3, 800.0, 0.0043625, 4.0), (4, 0.4, 0.0043625, 4.0), (5, 0.4, 0.0043625, 4.0),
                                                   (15, 0.4, 0.0044, 4.0)]))
def test_every_job_of_every_sampling_grid(exe, key):
    """Each group's distinct jobs once, in one call (and the grouping above names every group there is)."""
    assert set(_jobs()) == {(1, 0.4, 0.0043625, 4.0), (2, 0.4, 0.0043625, 4.0), (3, 0.4, 0.0043625, 4.0), (3, 800.0, 0.0043625, 4.0),
                            (4, 0.4, 0.0043625, 4.0), (5, 0.4, 0.0043625, 4.0), (15, 0.4, 0.0044, 4.0)}
    ok, cov, idx = _run_both(key, len(_jobs()[key]))
    _assert_equal(exe, key, ok, cov, idx)


@pytest.mark.parametrize("count", COUNTS + (4097,))
def test_job_counts_on_lane_and_workgroup_boundaries(exe, count):
    ok, cov, idx = _run_both(MAIN, count)
    _assert_equal(exe, MAIN, ok, cov, idx)


@pytest.mark.parametrize("key,count", [((1, 0.4, 0.0043625, 4.0), 65), ((1, 0.4, 0.0043625, 4.0), 257), ((15, 0.4, 0.0044, 4.0), 65)])
def test_job_counts_with_other_grids(exe, key, count):
    """The smallest and the largest grid past a wavefront (and the smallest past a workgroup): m = 1, where the sample loop
    runs once, and m = 3375, 243 KB of sample records per job."""
    ok, cov, idx = _run_both(key, count)
    _assert_equal(exe, key, ok, cov, idx)


def test_mixed_memories_are_refused_and_nothing_is_written():
    import ctypes as C
    import torch
    from tbv_slam_public_amd import api, _lib as L
    ctx = api.default_context()
    regs, smp, _ = _records(MAIN, 4)
    sp = api.n_scan_normal_reg.sampling_params()
    d_regs = torch.from_numpy(regs.view(np.uint8)).cuda()
    d_smp = torch.from_numpy(smp.view(np.uint8).reshape(-1)).cuda()
    cov, ok = np.full((4, 36), 7.0), np.full(4, 7, np.int32)
    d_cov = torch.full((4, 36), 7.0, dtype=torch.float64, device="cuda")
    d_ok = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    host = (regs.ctypes.data, smp.ctypes.data, cov.ctypes.data, ok.ctypes.data)
    dev = (d_regs.data_ptr(), d_smp.data_ptr(), d_cov.data_ptr(), d_ok.data_ptr())
    for swap in range(4):
        for a, b in ((host, dev), (dev, host)):
            p = [b[k] if k == swap else a[k] for k in range(4)]
            rc = ctx._lib.cfear_cov_fit_records(ctx.h, p[0], p[1], 4, C.byref(sp), p[2], p[3])
            assert rc == L.ERR_INVALID_ARGUMENT and "all host or all device" in ctx._lib.cfear_last_error(ctx.h).decode()
    assert (cov == 7.0).all() and (ok == 7).all() and (d_cov.cpu().numpy() == 7.0).all() and (d_ok.cpu().numpy() == 7).all()
    assert ctx._lib.cfear_cov_fit_records(ctx.h, host[0], host[1], 0, C.byref(sp), host[2], host[3]) == L.OK
    assert (cov == 7.0).all() and (ok == 7).all()
