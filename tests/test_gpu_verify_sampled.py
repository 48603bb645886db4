"""GPU: sampled covariances for loop candidates that were verified on the device (cfear_verify_sample_covariances), as a pass
over the records cfear_verify_graph_candidates / cfear_verify_sc_rows wrote.

The candidates are the pool of tests/verify_cases.py.  The graph route looks a candidate's scans, peaks and query pose up by
node, so every pool candidate gets two nodes of its own -- `to` with the candidate's target scan, `from` with its query scan
at the candidate's from_pose -- in a batch of three graphs (the middle one empty); the one odometry step between the two is
chosen so that VerifyByOdometry returns the candidate's odom_bounds (to rounding: no candidate of the pool sits within 1e-3
of the acceptance threshold, verify_cases.Pool.check).

Against the oracle's chain with sampling (pool.expected(True)) and against verify_host_chain (cfear_verify_loop_candidates
with use_covariance_sampling) on the same candidates: cov_sampled equal, the (x, y, yaw) block within rtol 1e-4, atol 1e-12
(tests/test_gpu_verify_matrix.py::test_host_chain_against_device_chain), the sampled block positive definite,
cov[2:5, 2:5] the identity to 1e-15.  Every byte outside `cov` and `cov_sampled` is what it was before the pass; skipped and
failed candidates are unchanged altogether; list and results on the device give the bytes of the host form."""
import ctypes as C

import numpy as np
import pytest

from tests import verify_cases as V

pytestmark = pytest.mark.gpu

BLOCK = np.ix_([0, 1, 5], [0, 1, 5])
SPLIT = 10                                                                   # pool candidates [0, 10) in graph 0, the rest in graph 2
SIGMA = 0.03
_WORST = {"oracle": 0.0, "host": 0.0}


def _step_for(odom_bounds):
    """Length of ONE odometry step whose VerifyByOdometry similarity is odom_bounds: 1 - exp(-((d - 5) / d)^2 / 2 sigma^2)."""
    if odom_bounds <= 0.0:
        return 1.0                                                           # within 5 m: exactly 0
    if odom_bounds >= 1.0:
        return 50.0                                                          # exp(-450) vanishes beside 1
    r = SIGMA * np.sqrt(-2.0 * np.log1p(-odom_bounds))
    return 5.0 / (1.0 - r)


@pytest.fixture(scope="module")
def pool():
    p = V.Pool(V.attach_scans(V.base_nodes()), None)
    p.cands = V.base_cands(p.nodes)
    p.check()
    return p


@pytest.fixture(scope="module")
def graphs(pool):
    """dict for api.verify_graph_candidates: pool candidate i owns flat nodes 2 i (to) and 2 i + 1 (from)."""
    from tbv_slam_public_amd import api
    scans, peaks, poses, rel = [], [], [], []
    for c in pool.cands:
        for k, pose, step in ((c["t"], (0.0, 0.0, 0.0), _step_for(c["odom_bounds"])), (c["f"], c["from_pose"], 1.0)):
            scans.append(pool.nodes[k]["scan"]); peaks.append(pool.nodes[k]["peaks"]); poses.append(pose); rel.append((step, 0.0, 0.0))
    n0 = 2 * SPLIT
    return dict(node_off=np.array([0, n0, n0, len(scans)], np.int32), table=api.ScanTable(scans), xyzi=np.concatenate(peaks),
                point_off=np.concatenate([[0], np.cumsum([len(x) for x in peaks])]).astype(np.int64), poses=np.array(poses, np.float64),
                rel=np.array(rel, np.float64))


def _list(pool, n, skip_every=0):
    """n candidates cycling over the pool, one query per cycle -> (records, pool index of each)."""
    from tbv_slam_public_amd import api
    idx = np.arange(n) % len(pool)
    out = []
    for j, i in enumerate(idx):
        c = pool.cands[i]
        g, local = (0, i) if i < SPLIT else (2, i - SPLIT)
        out.append({"graph": g, "from": 2 * local + 1, "to": 2 * local, "guess_nr": 0, "query": int(j // len(pool)),
                    "guess_xyt": c["t_be_guess"], "sc_sim": c["sc_sim"], "skip": int(bool(skip_every) and j % skip_every == 2),
                    "odom_term": 0.875})
    return api.loop_verify_candidates(out), idx


def _masked(res):
    """The records' bytes with `cov` and `cov_sampled` blanked."""
    r = res.copy()
    r["cov"] = 0.0
    r["cov_sampled"] = 0
    return r.tobytes()


def _verified(graphs, lst):
    from tbv_slam_public_amd import api
    out = api.verify_graph_candidates(graphs, lst)
    assert (out["results"]["cov_sampled"] == 0).all()
    return out


def _check_pass(pool, before, after, lst, idx, exp):
    """What the pass may and must change, and the sampled covariances against the oracle's."""
    assert _masked(after) == _masked(before)
    takes_part = (lst["skip"] == 0) & (before["reg_ok"] == 1)
    rest = np.nonzero(~takes_part)[0]
    assert after[rest].tobytes() == before[rest].tobytes()                   # skipped and failed candidates: unchanged altogether
    worst = 0.0
    for j in np.nonzero(takes_part)[0]:
        e, g, name = exp[idx[j]], after[j], pool.cands[idx[j]]["name"]
        assert bool(g["cov_sampled"]) == bool(e["cov_sampled"]), name
        if not g["cov_sampled"]:
            assert g["cov"].tobytes() == before["cov"][j].tobytes(), name    # a refused fit leaves Register's constant, rotated
            continue
        worst = max(worst, float((np.abs(g["cov"][BLOCK] - e["cov"][BLOCK]) / np.abs(e["cov"][BLOCK])).max()))
        np.testing.assert_allclose(g["cov"][BLOCK], e["cov"][BLOCK], rtol=1e-4, atol=1e-12, err_msg=name)
        assert np.linalg.eigvalsh(g["cov"][BLOCK]).min() > 0, name
        np.testing.assert_allclose(g["cov"][2:5, 2:5], np.eye(3), atol=1e-15, err_msg=name)
    _WORST["oracle"] = max(_WORST["oracle"], worst)
    print("sampled covariances against the oracle: worst relative difference of a block entry %.3e over %d candidates (so far %.3e)"
          % (worst, int(takes_part.sum()), _WORST["oracle"]))


@pytest.mark.parametrize("n", [1, 256, 257])
def test_pass_over_verified_candidates(pool, graphs, n):
    import torch
    from tbv_slam_public_amd import api
    hits = pool.check_sampling()
    exp = pool.expected(True)
    lst, idx = _list(pool, n, skip_every=0 if n == 1 else 9)
    out = _verified(graphs, lst)
    before = out["results"].copy()
    # the same records on the device, before the host pass touches them
    d_out = dict(n=n, results=torch.from_numpy(before.view(np.uint8).copy()).cuda(), list=torch.from_numpy(out["list"].view(np.uint8).copy()).cuda())
    api.verify_sample_covariances(graphs, out)
    after = out["results"]
    _check_pass(pool, before, after, lst, idx, exp)
    api.verify_sample_covariances(graphs, d_out)
    assert d_out["results"].cpu().numpy().tobytes() == after.tobytes()       # list and results on the device: the host form's bytes
    assert d_out["list"].cpu().numpy().tobytes() == lst.tobytes()
    if n == 1:
        assert after["cov_sampled"][0] == 1
        return
    assert (lst["skip"] == 1).sum() >= 20 and (before["reg_ok"] == 0).sum() >= 10 and after["cov_sampled"].sum() >= n // 2
    assert (after["cov_sampled"][lst["skip"] == 1] == 0).all()
    # the candidates that put R C R^T under test: accepted, sampled, a yaw beyond 0.5 rad and unequal variances
    rotated = sum(bool(g["accepted"]) and bool(g["cov_sampled"]) and pool.cands[i]["name"] in hits for g, i in zip(after, idx))
    assert rotated >= len(hits)
    for q in np.unique(idx):                                                 # copies of a candidate inside one call: the same covariance
        rows = [r for r in np.nonzero(idx == q)[0] if lst["skip"][r] == 0]
        assert all(after["cov"][r].tobytes() == after["cov"][rows[0]].tobytes() for r in rows), pool.cands[q]["name"]
    # ---- verify_host_chain on the same candidates ------------------------------------------------------------------------------
    keep = np.nonzero(lst["skip"] == 0)[0]
    cands = [dict(pool.cands[idx[j]], group=int(lst["query"][j]), odom_bounds=float(before["odom_bounds"][j])) for j in keep]
    host = api.verify_loop_candidates(V.make_jobs(pool.nodes, cands), api.verify_params(use_covariance_sampling=1))
    np.testing.assert_array_equal(host["reg_ok"], after["reg_ok"][keep])
    np.testing.assert_array_equal(host["cov_sampled"], after["cov_sampled"][keep])
    np.testing.assert_array_equal(host["accepted"], after["accepted"][keep])
    worst = 0.0
    for h, g, c in zip(host, after[keep], cands):
        if h["cov_sampled"]:
            worst = max(worst, float((np.abs(g["cov"][BLOCK] - h["cov"][BLOCK]) / np.abs(h["cov"][BLOCK])).max()))
            np.testing.assert_allclose(g["cov"][BLOCK], h["cov"][BLOCK], rtol=1e-4, atol=1e-12, err_msg=c["name"])
            assert np.linalg.eigvalsh(h["cov"][BLOCK]).min() > 0
            np.testing.assert_allclose(g["cov"][2:5, 2:5], np.eye(3), atol=1e-15)
            rest_g, rest_h = g["cov"].copy(), h["cov"].copy()
            rest_g[BLOCK] = rest_h[BLOCK] = 0.0
            assert np.array_equal(rest_g, rest_h), c["name"]
    _WORST["host"] = max(_WORST["host"], worst)
    print("sampled covariances against verify_host_chain: worst relative difference of a block entry %.3e (so far %.3e)" % (worst, _WORST["host"]))


def test_device_out_of_the_graph_route_is_accepted_as_it_is(pool, graphs):
    """verify_graph_candidates(device_out) -> the pass -> the records of the host form, selection aside (accepted = rank = 0 on
    the device: verify_apply_constraints is the caller's)."""
    from tbv_slam_public_amd import api, _lib as L
    lst, idx = _list(pool, 65, skip_every=9)
    host = api.verify_sample_covariances(graphs, _verified(graphs, lst))["results"].copy()
    dev = api.verify_graph_candidates(graphs, lst, device_out=True)
    api.verify_sample_covariances(graphs, dev)
    got = dev["results"].cpu().numpy().view(L.VERIFY_RESULT_DTYPE).copy()
    assert got["cov_sampled"].sum() >= 20
    host["accepted"] = 0
    host["rank"] = 0
    assert got.tobytes() == host.tobytes()


def test_rows_left_on_the_device_are_accepted_as_they_are():
    """cfear_verify_sc_rows with the detector's rows, the list and the results on the device, then the pass on what it returned;
    against the same two calls in host memory."""
    import torch
    from tbv_slam_public_amd import api, _lib as L
    from tests.test_gpu_loop_verify import _sc_batch
    g, rows, n_out, n_detect = _sc_batch()
    par = api.loop_verify_params(speedup=1)
    host = api.verify_sc_rows(g, rows, n_out, n_detect, par)
    before = host["results"].copy()
    api.verify_sample_covariances(g, host, par)
    after, lst = host["results"], host["list"]
    assert _masked(after) == _masked(before)
    takes_part = (lst["skip"] == 0) & (before["reg_ok"] == 1)
    assert after[~takes_part].tobytes() == before[~takes_part].tobytes()
    # (no definiteness here: the reference rotates the x-y-z block and leaves the x-yaw and y-yaw terms where they were,
    # loopclosure.cpp:93, so with the arbitrary pairs of this batch the rotated block need not stay positive definite)
    for j in np.nonzero(after["cov_sampled"] == 1)[0]:
        c = after["cov"][j]
        assert takes_part[j] and c[0, 0] > 0 and c[1, 1] > 0 and c[5, 5] > 0 and c[0, 0] * c[1, 1] > c[0, 1] * c[1, 0]
        np.testing.assert_allclose(c[2:5, 2:5], np.eye(3), atol=1e-15)
    print("rows form: %d candidates, %d skipped, %d registered, %d sampled" % (host["n"], int((lst["skip"] == 1).sum()),
                                                                             int(takes_part.sum()), int(after["cov_sampled"].sum())))
    assert (lst["skip"] == 1).any() and takes_part.any()
    d_rows = torch.from_numpy(rows.view(np.uint8).reshape(rows.shape[0], rows.shape[1], 64)).cuda()
    dev = api.verify_sc_rows(g, d_rows, torch.from_numpy(n_out).cuda(), n_detect, par, device_out=True)
    assert dev["n"] == host["n"]
    api.verify_sample_covariances(g, dev, par)
    got = dev["results"].cpu().numpy().view(L.VERIFY_RESULT_DTYPE).copy()
    ref = after.copy()
    ref["accepted"] = 0
    ref["rank"] = 0                                                          # (device records: no selection was made, skipped ones included)
    assert got.tobytes() == ref.tobytes()
    assert dev["list"].cpu().numpy().tobytes() == lst.tobytes()


def test_a_bad_device_list_is_refused_naming_the_candidate(pool, graphs):
    import torch
    from tbv_slam_public_amd import api, _lib as L
    ctx = api.default_context()
    lst, idx = _list(pool, 9)
    out = _verified(graphs, lst)
    bad = out["list"].copy()
    bad["to"][7] = bad["from"][7]
    bad["graph"][8] = 9
    d_res = torch.from_numpy(out["results"].view(np.uint8).copy()).cuda()
    d_bad = torch.from_numpy(bad.view(np.uint8)).cuda()
    g, keep = api._loop_graphs(graphs)
    par = api.loop_verify_params()
    torch.cuda.synchronize()
    rc = ctx._lib.cfear_verify_sample_covariances(ctx.h, C.byref(g), d_bad.data_ptr(), 9, C.byref(par), d_res.data_ptr())
    assert rc == L.ERR_INVALID_ARGUMENT and "candidate 7" in ctx._lib.cfear_last_error(ctx.h).decode()
    assert d_res.cpu().numpy().tobytes() == out["results"].tobytes()         # the records untouched
    # a registered pose that is not finite, in a record on the device
    nan = out["results"].copy()
    nan["reg"]["pose"][int(np.nonzero(nan["reg_ok"] == 1)[0][1]), 0] = np.nan
    d_nan = torch.from_numpy(nan.view(np.uint8).copy()).cuda()
    d_lst = torch.from_numpy(out["list"].view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    rc = ctx._lib.cfear_verify_sample_covariances(ctx.h, C.byref(g), d_lst.data_ptr(), 9, C.byref(par), d_nan.data_ptr())
    assert rc == L.ERR_INVALID_ARGUMENT and "candidate %d" % int(np.nonzero(nan["reg_ok"] == 1)[0][1]) in ctx._lib.cfear_last_error(ctx.h).decode()
    assert d_nan.cpu().numpy().tobytes() == nan.tobytes()
    # list and results in different memories
    rc = ctx._lib.cfear_verify_sample_covariances(ctx.h, C.byref(g), out["list"].ctypes.data, 9, C.byref(par), d_res.data_ptr())
    assert rc == L.ERR_INVALID_ARGUMENT and "both host or both device" in ctx._lib.cfear_last_error(ctx.h).decode()
    del keep
    # the context goes on, and the good list passes
    api.verify_sample_covariances(graphs, out)
    assert out["results"]["cov_sampled"].sum() >= 3
