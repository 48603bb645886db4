"""GPU: covariance by cost sampling for candidate pairs of a scan table (cfear_covariance_by_sampling_candidates: expand ->
matcher around device-resident centres -> cov_fit_kernel, nothing read back in between) against
cfear_covariance_by_sampling_batch, the route with the host between the samples and the fit, on the same problems:
  - the two-scan cases of tests/covariance_cases.py, each with its own sampling grid (1, 2, 3, 4, 5 and 15 samples per axis,
    failing samples, a job whose samples all fail, an indefinite fit), poses and summaries the oracle's;
  - the pool of tests/verify_cases.py: about two dozen loop candidates, registered here with RegisterLoopCandidate's
    parameters, two of which fail -- those are sampled around the candidate's own source pose -- tiled to 1, 255, 256 and 257.

Bounds.  `success` equal.  The (x, y, yaw) block within rtol 1e-4, atol 1e-12, the tolerance the project holds sampled
covariances to (tests/test_gpu_verify_matrix.py::test_host_chain_against_device_chain): the two routes may choose different
matcher forms, whose fp64 sums differ in order, and the fit amplifies the ~1e-12 sample differences.
The rest of the 6 x 6 equal.  The worst relative difference seen is printed (EXPERIMENTS.md, "Covariance sampling on the
device").  Outputs left on the device are byte-equal to the host outputs of the same call."""
import ctypes as C

import numpy as np
import pytest

from tests import covariance_cases as CC
from tests import verify_cases as V

pytestmark = pytest.mark.gpu

BLOCK = np.ix_([0, 1, 5], [0, 1, 5])
REJECTED = np.diag([0.01, 0.01, 0, 0, 0, 1e-4])
_WORST = {"rel": 0.0}


def _compare(ok_c, cov_c, ok_b, cov_b, names):
    """The candidate route against the batch route."""
    np.testing.assert_array_equal(ok_c.astype(bool), ok_b.astype(bool))
    worst = 0.0
    for a, b, good, name in zip(cov_c, cov_b, ok_b, names):
        if not good:
            assert np.array_equal(a, REJECTED) and np.array_equal(b, REJECTED), name
            continue
        rel = float((np.abs(a[BLOCK] - b[BLOCK]) / np.abs(b[BLOCK])).max())
        worst = max(worst, rel)
        np.testing.assert_allclose(a[BLOCK], b[BLOCK], rtol=1e-4, atol=1e-12, err_msg=name)
        ra, rb = a.copy(), b.copy()
        ra[BLOCK] = rb[BLOCK] = 0.0
        assert np.array_equal(ra, rb) and np.array_equal(ra, np.diag([0, 0, 1.0, 1.0, 1.0, 0])), name
    _WORST["rel"] = max(_WORST["rel"], worst)
    print("candidate route against batch route: worst relative difference of a covariance entry %.3e over %d jobs (so far %.3e)"
          % (worst, len(names), _WORST["rel"]))
    return worst


def _device_form(table, cands, regs, reg, sp):
    """The same call with the candidates, the records and the outputs on the device -> (success, cov) copied back."""
    import torch
    from tbv_slam_public_amd import api
    d_c = torch.from_numpy(cands.view(np.uint8)).cuda()
    d_r = torch.from_numpy(regs.view(np.uint8)).cuda()
    ok, cov = api.covariance_by_sampling_candidates(table, d_c, d_r, reg, sp)
    return ok.cpu().numpy(), cov.cpu().numpy()


# ---- the two-scan cases of the covariance matrix -----------------------------------------------------------------------------
TWO_SCAN = ("failing-samples", "all-fail", "far-from-optimum", "count-1", "count-2", "count-4", "count-5", "count-15")


def test_two_scan_cases_are_all_here():
    assert sorted(TWO_SCAN) == sorted(c["name"] for c in CC.cases() if len(c["window"]) == 2)


@pytest.mark.parametrize("name", TWO_SCAN)
def test_covariance_cases_against_the_batch_route(name):
    from tbv_slam_public_amd import api
    from tests.test_gpu_covariance_matrix import _job, _record, _reg, _sp
    case = CC.by_name(name)
    reg, (maps, poses), rec = _reg(case), _job(case), _record(case)
    sp = _sp(reg, case)
    ok_b, cov_b = reg.approximateCovarianceBySamplingBatch([(maps, poses)], rec, sp)
    table = api.ScanTable(maps)
    cands = table.candidates([0], [1], poses[1:2], poses[0:1])
    ok_c, cov_c = api.covariance_by_sampling_candidates(table, cands, rec, reg, sp)
    _compare(ok_c, cov_c, ok_b, cov_b, [name])
    exp_ok = CC.oracle_cov(case)[0]
    assert bool(ok_c[0]) == bool(exp_ok)                                     # (the verdicts are robust: covariance_cases.robust)
    d_ok, d_cov = _device_form(table, cands, rec, reg, sp)
    assert d_ok.tobytes() == ok_c.tobytes() and d_cov.tobytes() == cov_c.tobytes()


# ---- the verification pool ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """nodes with scans, the table over them, RegisterLoopCandidate's registration object, the candidates as table records
    (scans {to, from}, poses {Tfrom * guess, Tfrom}) and their registration records."""
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    nodes = V.attach_scans(V.base_nodes())
    cands = V.base_cands(nodes)
    table = api.ScanTable([nd["scan"] for nd in nodes])
    reg = api.n_scan_normal_reg("P2L", "Huber", 0.1, 0)
    reg.SetParameters(4, 10)                                                 # loopclosure.cpp:56-57
    rec = table.candidates([c["t"] for c in cands], [c["f"] for c in cands], [c["from_pose"] for c in cands],
                           [O.xyt_compose(c["from_pose"], c["t_be_guess"]) for c in cands])
    regs = reg.RegisterCandidates(table, rec)
    assert (regs["status"] != 0).sum() >= 2 and (regs["status"] == 0).sum() >= 18
    return dict(nodes=nodes, cands=cands, table=table, reg=reg, rec=rec, regs=regs,
                sp=reg.sampling_params(0.4, 0.0044, 3, 4.0))                 # loopclosure.cpp:108-112


def _batch_jobs(p, idx):
    """What verify_host_chain hands to cfear_covariance_by_sampling_batch: the poses after Register, the guess where it failed."""
    jobs = []
    for i in idx:
        c, r = p["rec"][i], p["regs"][i]
        src = r["pose"] if r["status"] == 0 else c["source_xyt"]
        jobs.append(([p["nodes"][c["target"]]["scan"], p["nodes"][c["source"]]["scan"]], np.array([c["target_xyt"], src])))
    return jobs


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_pool_against_the_batch_route(pool, n):
    from tbv_slam_public_amd import api
    p = pool
    idx = np.arange(n) % len(p["cands"])
    rec, regs = p["rec"][idx].copy(), p["regs"][idx].copy()
    ok_b, cov_b = p["reg"].approximateCovarianceBySamplingBatch(_batch_jobs(p, idx), regs, p["sp"])
    ok_c, cov_c = api.covariance_by_sampling_candidates(p["table"], rec, regs, p["reg"], p["sp"])
    _compare(ok_c, cov_c, ok_b, cov_b, [p["cands"][i]["name"] for i in idx])
    if n >= len(p["cands"]):
        assert ok_c.sum() >= n // 2 and (regs["status"] != 0).any()
        for q in np.unique(idx):                                             # copies of a candidate inside one call: the same bytes
            rows = np.nonzero(idx == q)[0]
            assert all(cov_c[r].tobytes() == cov_c[rows[0]].tobytes() and ok_c[r] == ok_c[rows[0]] for r in rows), p["cands"][q]["name"]
    d_ok, d_cov = _device_form(p["table"], rec, regs, p["reg"], p["sp"])
    assert d_ok.tobytes() == ok_c.tobytes() and d_cov.tobytes() == cov_c.tobytes()
    # host candidates with device records, and device candidates with host records: the same bytes again
    import torch
    m_ok, m_cov = api.covariance_by_sampling_candidates(p["table"], rec, torch.from_numpy(regs.view(np.uint8)).cuda(), p["reg"], p["sp"])
    assert m_ok.cpu().numpy().tobytes() == ok_c.tobytes() and m_cov.cpu().numpy().tobytes() == cov_c.tobytes()
    h_ok, h_cov = api.covariance_by_sampling_candidates(p["table"], torch.from_numpy(rec.view(np.uint8)).cuda(), regs, p["reg"], p["sp"])
    assert h_ok.tobytes() == ok_c.tobytes() and h_cov.tobytes() == cov_c.tobytes()


def test_a_failed_record_is_sampled_around_the_candidates_own_source_pose(pool):
    """Registered candidates whose records are marked failed and carry a pose far away: the samples must be centred on
    source_xyt, so the result is that of records whose pose IS source_xyt, byte for byte (same batch, same forms)."""
    from tbv_slam_public_amd import api
    p = pool
    good = np.nonzero(p["regs"]["status"] == 0)[0][:6]
    rec, regs = p["rec"][good].copy(), p["regs"][good].copy()
    rec["source_xyt"] = regs["pose"]                                         # the candidate's own pose = where the registration ended
    ref_ok, ref_cov = api.covariance_by_sampling_candidates(p["table"], rec, regs, p["reg"], p["sp"])
    assert ref_ok.sum() >= 3
    failed = regs.copy()
    failed["status"] = -4
    failed["pose"] = (1e6, -1e6, 2.0)
    ok, cov = api.covariance_by_sampling_candidates(p["table"], rec, failed, p["reg"], p["sp"])
    assert ok.tobytes() == ref_ok.tobytes() and cov.tobytes() == ref_cov.tobytes()
    # ... and a record that succeeded is sampled around ITS pose, whatever the candidate says
    moved = rec.copy()
    moved["source_xyt"] = (1e6, -1e6, 2.0)
    ok, cov = api.covariance_by_sampling_candidates(p["table"], moved, regs, p["reg"], p["sp"])
    assert ok.tobytes() == ref_ok.tobytes() and cov.tobytes() == ref_cov.tobytes()
    # the pool's own failures: registered nowhere, sampled at the guess -- what the batch route is given by _batch_jobs
    bad = np.nonzero(p["regs"]["status"] != 0)[0]
    ok_c, cov_c = api.covariance_by_sampling_candidates(p["table"], p["rec"][bad].copy(), p["regs"][bad].copy(), p["reg"], p["sp"])
    ok_b, cov_b = p["reg"].approximateCovarianceBySamplingBatch(_batch_jobs(p, bad), p["regs"][bad].copy(), p["sp"])
    _compare(ok_c, cov_c, ok_b, cov_b, [p["cands"][i]["name"] for i in bad])


def test_refusals_that_need_a_device(pool):
    import torch
    from tbv_slam_public_amd import api, _lib as L
    p = pool
    ctx = api.default_context()
    rec, regs = p["rec"][:5].copy(), p["regs"][:5].copy()
    cov, ok = np.full((5, 36), 7.0), np.full(5, 7, np.int32)
    d_cov = torch.full((5, 36), 7.0, dtype=torch.float64, device="cuda")
    d_ok = torch.full((5,), 7, dtype=torch.int32, device="cuda")
    d_regs = torch.from_numpy(regs.view(np.uint8)).cuda()
    torch.cuda.synchronize()

    def call(c, r, cv, k):
        rc = ctx._lib.cfear_covariance_by_sampling_candidates(ctx.h, p["table"]._h, c, 5, C.byref(p["reg"].par), r, C.byref(p["sp"]), cv, k)
        return rc, ctx._lib.cfear_last_error(ctx.h).decode()

    for r, cv, k in ((d_regs.data_ptr(), cov.ctypes.data, ok.ctypes.data), (regs.ctypes.data, d_cov.data_ptr(), ok.ctypes.data),
                     (regs.ctypes.data, cov.ctypes.data, d_ok.data_ptr()), (d_regs.data_ptr(), d_cov.data_ptr(), ok.ctypes.data)):
        rc, msg = call(rec.ctypes.data, r, cv, k)
        assert rc == L.ERR_INVALID_ARGUMENT and "all host or all device" in msg, msg
    bad = rec.copy()
    bad["source"][3] = len(p["nodes"])
    bad["target"][4] = -1
    rc, msg = call(bad.ctypes.data, regs.ctypes.data, cov.ctypes.data, ok.ctypes.data)
    assert rc == L.ERR_INVALID_ARGUMENT and "candidate 3 " in msg, msg
    d_bad = torch.from_numpy(bad.view(np.uint8)).cuda()                      # a device list is checked by the kernel that reads it
    torch.cuda.synchronize()
    for r, cv, k in ((regs.ctypes.data, cov.ctypes.data, ok.ctypes.data), (d_regs.data_ptr(), d_cov.data_ptr(), d_ok.data_ptr())):
        rc, msg = call(d_bad.data_ptr(), r, cv, k)
        assert rc == L.ERR_INVALID_ARGUMENT and "candidate 3 " in msg, msg
    assert (cov == 7.0).all() and (ok == 7).all() and (d_cov.cpu().numpy() == 7.0).all() and (d_ok.cpu().numpy() == 7).all()
    after_ok, after_cov = api.covariance_by_sampling_candidates(p["table"], rec, regs, p["reg"], p["sp"])      # the context goes on
    assert after_ok.shape == (5,) and set(after_ok.tolist()) <= {0, 1}
