"""GPU: the tie audit (cfear_association_ties_batch, cfear_scan_closest_ties, api.flip_ties, api.tie_sensitivity) against
the NumPy restatement of tests/tieaudit_cpu.py -- exactly -- and, where a registration is involved, against the oracle at
the project's bar (POS_TOL / ROT_TOL of tests/test_gpu_register.py).  The cases are the ones tests/test_tieaudit_cpu.py pins
to the oracle on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests import tieaudit_cpu as R
from tests.test_gpu_register import POS_TOL, ROT_TOL
from tests.test_tieaudit_cpu import NATURAL_SEEDS, RADIUS, natural_inputs

pytestmark = pytest.mark.gpu


def _records(rec):
    return [tuple(int(v) for v in r) for r in rec]


def _device_jobs(jobs):
    from tbv_slam_public_amd import api
    return [([api.MapPointNormal(cells=c) for c in scans], poses) for scans, poses in jobs]


@pytest.fixture(scope="module")
def constructed():
    jobs = R.constructed_jobs()
    return jobs, _device_jobs(jobs)


@pytest.fixture(scope="module")
def natural():
    """The natural seeds through the library's own filter and surface-point stages (k = 40, z_min = 60, radius 3,
    weight_intensity): {seed: ((target, source) scans, their cells, poses)}."""
    from tbv_slam_public_amd import api
    out = {}
    for seed in NATURAL_SEEDS:
        imgs, poses = natural_inputs(seed)
        scans = []
        for f in range(2):
            r = api.filter_kstrongest(imgs[f], 40, 60, 0.0438, 2.5)
            scans.append(api.MapPointNormal(r["xyzi"][0, :int(r["n_points"][0])].copy(), 3.0, (0.0, 0.0), True))
        out[seed] = (scans, [s.GetCells() for s in scans], poses)
    return out


def test_closest_ties_on_the_constructed_target():
    import torch
    from tbv_slam_public_amd import api
    cells, q = R.closest_case()
    m = api.MapPointNormal(cells=cells)
    exp = R.closest_ties(cells, q, R.CLOSEST_D)
    got = m.GetClosestTies(q, R.CLOSEST_D)
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    np.testing.assert_array_equal(got[0], m.GetClosestIdx(q, R.CLOSEST_D))
    assert (int(got[0][0]), int(got[1][0]), int(got[2][0])) == (5, 8, 4)
    dev = m.GetClosestTies(torch.from_numpy(q).cuda(), R.CLOSEST_D)
    for g, e in zip(dev, exp):
        np.testing.assert_array_equal(g.cpu().numpy(), e)
    assert m.GetClosestTies(q[1], R.CLOSEST_D) == (0, 2, 3) and m.GetClosestTies(q[5], R.CLOSEST_D) == (-1, -1, 0)
    # more cells than one LDS tile: a copy of cell 3 behind the tile boundary joins its group
    big = np.concatenate([cells, R.make_cells(np.column_stack([np.linspace(200, 900, R.TILE), np.full(R.TILE, 77.0)])), cells[3:4]])
    mb = api.MapPointNormal(cells=big)
    exp = R.closest_ties(big, q, R.CLOSEST_D)
    assert tuple(int(v[2]) for v in exp) == (3, big.shape[0] - 1, 3)
    for g, e in zip(mb.GetClosestTies(q, R.CLOSEST_D), exp):
        np.testing.assert_array_equal(g, e)


@pytest.mark.parametrize("itr", [1, 2])
def test_association_ties_on_constructed_jobs(constructed, itr):
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    jobs, dev = constructed
    rec, pq, offs = api.association_ties(dev, None, itr, want_queries=True)
    e_rec, e_pq, e_offs = R.audit_batch(jobs, RADIUS, itr)
    print(_records(rec))
    assert _records(rec) == [R.record_tuple(r) for r in e_rec]
    np.testing.assert_array_equal(offs, e_offs)
    np.testing.assert_array_equal(pq, e_pq)
    np.testing.assert_array_equal(api.association_ties(dev, None, itr), rec)            # without the per-query output
    par = O.reg_params(radius=RADIUS)
    reg = api.n_scan_normal_reg()
    for j, (scans, poses) in enumerate(jobs):
        pairs, _ = O.associate(scans, poses, par, itr)
        n = len(scans[-1])
        assert rec["n_associated"][j] == len(pairs)
        assert (pq[offs[j] + pairs[:, 0] * n + pairs[:, 2], 0] == pairs[:, 1]).all()
        blocks, _ = api.CeresCost(reg, dev[j][0], poses, itr).blocks()                   # what cfear_cost_prepare builds
        assert {tuple(int(v) for v in b) for b in blocks} == {tuple(int(v) for v in p) for p in pairs}
    if itr == 1:                                                                          # the cases the jobs were built for
        assert tuple(pq[offs[6]]) == (5, R.TILE, 2)
        assert tuple(pq[offs[3] + 3]) == (0, pq[offs[3] + 3, 1], 2) and pq[offs[3] + 4, 2] == 1
    else:
        assert pq[offs[3] + 4, 2] == 0


def test_batch_position_and_memory_side_do_not_matter(constructed):
    import torch
    from tbv_slam_public_amd import api, _lib as L
    _, dev = constructed
    assert len(dev) == 7
    rec, pq, offs = api.association_ties(dev, None, 1, want_queries=True)
    one, pq1, offs1 = api.association_ties([dev[3]], None, 1, want_queries=True)
    assert one[0].tobytes() == rec[3].tobytes() and offs1[1] == offs[4] - offs[3]
    np.testing.assert_array_equal(pq1, pq[offs[3]:offs[4]])
    drec, dpq, _ = api.association_ties(dev, None, 1, want_queries=True, device_out=True)
    torch.cuda.synchronize()
    api.default_context().synchronize()
    assert drec.cpu().numpy().view(L.TIE_RECORD_DTYPE).reshape(-1).tobytes() == rec.tobytes()
    np.testing.assert_array_equal(dpq.cpu().numpy(), pq)


def test_status_is_what_get_cost_batch_reports(constructed):
    """status: CFEAR_OK, too few residuals (the one-cell source), or CFEAR_ERR_CAPACITY for a source the matcher's LDS cannot
    hold -- 12 000 cells -- which the audit itself still counts."""
    from tbv_slam_public_amd import api, _lib as L
    jobs, dev = constructed
    rng = np.random.default_rng(5)
    big = R.make_cells(rng.uniform(-60, 60, (12000, 2)))
    huge = ([dev[3][0][0], api.MapPointNormal(cells=big)], dev[3][1])
    for cost in ("P2L", "P2P"):
        reg = api.n_scan_normal_reg(cost)
        reg.par.itr = 1
        rec = api.association_ties(dev + [huge], reg, 1)
        res = reg.GetCostBatch(dev + [huge])
        np.testing.assert_array_equal(rec["status"], res["status"])
        held = res["status"] != L.ERR_CAPACITY
        np.testing.assert_array_equal(rec["n_associated"][held] * (1 if cost == "P2L" else 2), res["num_residuals"][held])
        assert rec["status"][0] == (L.ERR_TOO_FEW_RESIDUALS if cost == "P2L" else L.OK) and rec["status"][-1] == L.ERR_CAPACITY
        e = R.audit([jobs[3][0][0], big], jobs[3][1], RADIUS, 1, 1 if cost == "P2L" else 2)[0]
        assert tuple(int(v) for v in rec[-1])[:6] == R.record_tuple(e)[:6] and rec["n_queries"][-1] == 12000


def test_natural_ties(natural):
    from tbv_slam_public_amd import api
    jobs = [(scans, poses) for scans, _, poses in natural.values()]
    for itr in (1, 2):
        rec, pq, _ = api.association_ties(jobs, None, itr, want_queries=True)
        e_rec, e_pq, _ = R.audit_batch([(cells, poses) for _, cells, poses in natural.values()], RADIUS, itr)
        print(itr, _records(rec))
        assert _records(rec) == [R.record_tuple(r) for r in e_rec]
        np.testing.assert_array_equal(pq, e_pq)
        if itr == 1:
            assert (rec["n_tied"] >= 1).all()


def test_flip_ties_reverses_the_cells(natural):
    from tbv_slam_public_amd import api
    scans, cells, _ = natural[NATURAL_SEEDS[0]]
    f = api.flip_ties(scans[0])
    assert f.GetCells().tobytes() == cells[0][::-1].tobytes() and f.GetSize() == len(cells[0])


@pytest.mark.parametrize("preset", ["cfear3", "uniform"])
def test_tie_sensitivity(natural, preset):
    """CFEAR-3's weights (P2P, Huber 0.1, weight option 4), and weight option 0 -- the loop-closure preset's, with which a
    tie can only matter through a differing mean, normal or covariance.  No bound on the spread itself: that is the
    reference's to set."""
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    cost, opt = ("P2P", 4) if preset == "cfear3" else ("P2L", 0)
    reg = api.n_scan_normal_reg(cost, "Huber", 0.1, opt)
    par = O.reg_params(cost=cost, loss="Huber", loss_limit=0.1, weight_opt=opt)
    rpb = 1 if cost == "P2L" else 2
    jobs = [(scans, poses) for scans, _, poses in natural.values()]
    out = api.tie_sensitivity(jobs, reg)
    print(preset, out["delta"].tolist(), _records(out["ties_start"]), _records(out["ties_end"]))
    np.testing.assert_array_equal(out["delta"], np.abs(out["result"]["pose"] - out["result_flipped"]["pose"]))
    for j, (_, cells, poses) in enumerate(natural.values()):
        for key, scans in (("result", cells), ("result_flipped", [cells[0][::-1].copy(), cells[1]])):
            ok, po, _ = O.register(scans, poses, par)
            r = out[key][j]
            assert ok and r["status"] == 0
            assert np.abs(r["pose"][:2] - po[-1, :2]).max() <= POS_TOL and abs(r["pose"][2] - po[-1, 2]) <= ROT_TOL, (key, j)
        end = poses.copy()
        end[-1] = out["result"]["pose"][j]
        assert tuple(int(v) for v in out["ties_start"][j]) == R.record_tuple(R.audit(cells, poses, RADIUS, 1, rpb)[0])
        assert tuple(int(v) for v in out["ties_end"][j]) == R.record_tuple(R.audit(cells, end, RADIUS, 2, rpb)[0])


def test_refusals_leave_the_outputs_alone(constructed):
    from tbv_slam_public_amd import api, _lib as L
    _, dev = constructed
    ctx = api.default_context()
    lib = ctx._lib
    reg = api.n_scan_normal_reg()
    arr, n, keep = reg.PrepareBatch(dev[:3])
    total = sum(len(s[-1].GetCells()) * (len(s) - 1) for s, _ in dev[:3])
    rec = np.full(n, 0x5A5A5A5A, np.int32).repeat(8).view(L.TIE_RECORD_DTYPE)
    pq = np.full((total, 3), 0x5A5A5A5A, np.int32)
    par = C.byref(reg.par)

    def refused(rc, status, needle=""):
        assert rc == status
        msg = lib.cfear_last_error(ctx.h).decode()
        assert msg and needle in msg, msg
        assert (rec.view(np.int32) == 0x5A5A5A5A).all() and (pq == 0x5A5A5A5A).all()

    call = lib.cfear_association_ties_batch
    refused(call(ctx.h, None, n, par, 1, rec.ctypes.data, pq.ctypes.data, total), L.ERR_INVALID_ARGUMENT)
    refused(call(ctx.h, arr, n, par, 1, None, pq.ctypes.data, total), L.ERR_INVALID_ARGUMENT)
    refused(call(ctx.h, arr, n, None, 1, rec.ctypes.data, pq.ctypes.data, total), L.ERR_INVALID_ARGUMENT)
    refused(call(ctx.h, arr, -1, par, 1, rec.ctypes.data, pq.ctypes.data, total), L.ERR_INVALID_ARGUMENT)
    refused(call(ctx.h, arr, n, par, -1, rec.ctypes.data, pq.ctypes.data, total), L.ERR_INVALID_ARGUMENT)
    refused(call(ctx.h, arr, n, par, 1, rec.ctypes.data, pq.ctypes.data, total - 1), L.ERR_CAPACITY)
    arr[1].n_scans = 1
    refused(call(ctx.h, arr, n, par, 1, rec.ctypes.data, pq.ctypes.data, total), L.ERR_INVALID_ARGUMENT, "job 1")
    arr[1].n_scans = 3
    for bad in (float("nan"), float("inf")):
        poses = dev[2][1].copy()
        poses[1, 2] = bad
        arr2, _, keep2 = reg.PrepareBatch([dev[0], dev[1], (dev[2][0], poses)])
        refused(call(ctx.h, arr2, n, par, 1, rec.ctypes.data, pq.ctypes.data, total), L.ERR_INVALID_ARGUMENT, "job 2")
    assert call(ctx.h, arr, 0, par, 1, rec.ctypes.data, pq.ctypes.data, total) == L.OK
    assert call(ctx.h, arr, n, par, 1, rec.ctypes.data, pq.ctypes.data, total) == L.OK and (pq != 0x5A5A5A5A).all()
    # the tie-aware GetClosestIdx
    rec[:] = np.full(n, 0x5A5A5A5A, np.int32).repeat(8).view(L.TIE_RECORD_DTYPE)
    pq[:] = 0x5A5A5A5A
    scan = dev[0][0][0]
    q = np.zeros((4, 2))
    lo, hi, cnt = pq[:4, 0].copy(), pq[:4, 1].copy(), pq[:4, 2].copy()
    ties = lib.cfear_scan_closest_ties
    for args in ((scan._h, None, 4, 2.0, lo.ctypes.data, hi.ctypes.data, cnt.ctypes.data), (scan._h, q.ctypes.data, 4, 2.0, None, None, None),
                 (scan._h, q.ctypes.data, -1, 2.0, lo.ctypes.data, None, None), (scan._h, q.ctypes.data, 4, 0.0, lo.ctypes.data, hi.ctypes.data, cnt.ctypes.data),
                 (scan._h, q.ctypes.data, 4, -1.0, lo.ctypes.data, None, None), (scan._h, q.ctypes.data, 4, float("nan"), lo.ctypes.data, None, None)):
        refused(ties(*args), L.ERR_INVALID_ARGUMENT)
        assert (lo == 0x5A5A5A5A).all() and (hi == 0x5A5A5A5A).all() and (cnt == 0x5A5A5A5A).all()
    assert ties(scan._h, q.ctypes.data, 0, 2.0, lo.ctypes.data, None, None) == L.OK
    assert ties(scan._h, q.ctypes.data, 4, 2.0, lo.ctypes.data, None, None) == L.OK and (lo != 0x5A5A5A5A).all()      # hi, count optional
