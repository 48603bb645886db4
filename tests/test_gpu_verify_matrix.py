"""GPU: loop-candidate verification (cfear_verify_loop_candidates, csrc/verify.hip) beyond six candidates, on every route the
chain can take: glue kernels past one workgroup, every matcher form inside the chain, deferred large registrations, CorAl in
two launches, the refusal that comes back from the device, the host chain against the device chain, and records left on the
device -- each against the CPU oracle's chain of the same reference functions (tests/verify_cases.py computes it once per
distinct candidate).  Tolerances against the oracle are tests/test_gpu_verify.py::_compare's: poses 1e-4 m / 1e-5 rad, integer
outcomes identical, CorAl rtol 1e-6, probabilities 1e-6.  Inside one call the copies of a candidate are byte-identical in every
field but `accepted` and `rank`; across matcher forms and between the two chains one candidate agrees in every integer outcome
and to 1e-11 in pose."""
import time

import numpy as np
import pytest

from tests import verify_cases as V

pytestmark = pytest.mark.gpu

FORMS = ((2, 20), (4, 40), (8, 80), (16, 160))
REG_INTS = ("num_residuals", "outer_iters", "lm_iters", "status")


@pytest.fixture(scope="module")
def pool():
    t0 = time.time()
    p = V.Pool(V.attach_scans(V.base_nodes()), None)
    p.cands = V.base_cands(p.nodes)
    p.check()
    print("verify pool: %d candidates, oracle %.2f s" % (len(p), time.time() - t0))
    return p


@pytest.fixture(scope="module")
def dense(pool):
    """The base pool's nodes followed by the dense ones; (pool of ordinary + big_pass candidates, pool of ordinary + whole_cu)."""
    t0 = time.time()
    dn = V.attach_scans(V.dense_nodes())
    hints = [V.predict_hint(len(nd["cells"])) for nd in dn]
    assert all(h["big_pass"] and not h["small_pairs"] for h in hints)
    assert [h["whole_cu"] for h in hints] == [False, False, False, True, True], [len(nd["cells"]) for nd in dn]
    nodes = pool.nodes + dn
    off = len(pool.nodes)
    big, huge = V.dense_cands(nodes, off)
    ordinary = pool.cands[:12]
    pb, ph = V.Pool(nodes, ordinary + big), V.Pool(nodes, ordinary + huge)
    pb._exp[False] = pool.expected()[:12] + [V.oracle_answer(nodes, c) for c in big]
    ph._exp[False] = pool.expected()[:12] + [V.oracle_answer(nodes, c) for c in huge]
    assert all(e["reg_ok"] for e in pb._exp[False][12:] + ph._exp[False][12:])
    print("dense nodes and oracle %.2f s" % (time.time() - t0))
    return pb, ph


def _run(pool, cands, peaks_on="host", overrides=None, ctx=None, nodes=None, device_ptr=None, **pk):
    from tbv_slam_public_amd import api
    par = api.verify_params(**pk)
    jobs = V.make_jobs(nodes or pool.nodes, cands, peaks_on, overrides)
    return api.verify_loop_candidates(jobs, par, ctx=ctx, device_ptr=device_ptr)


def _bytes_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def _copy_fields():
    from tbv_slam_public_amd import _lib as L
    return [f for f in L.VERIFY_RESULT_DTYPE.names if f not in ("accepted", "rank")]


def _assert_copies_identical(pool, got, idx):
    for p in np.unique(idx):
        rows = np.nonzero(idx == p)[0]
        for f in _copy_fields():
            b = _bytes_of(got[f][rows])
            diff = np.nonzero((b != b[0]).any(axis=1))[0]
            assert diff.size == 0, "candidate %r, field %s: job %d differs from job %d: %r vs %r" % (
                pool.cands[p]["name"], f, rows[diff[0]], rows[0], got[f][rows[diff[0]]], got[f][rows[0]])


def _assert_rank(got, cands):
    """rank = position in the stable descending probability order of the candidate's query."""
    groups = np.array([c["group"] for c in cands])
    for g in np.unique(groups):
        members = np.nonzero(groups == g)[0]
        order = members[np.argsort(-got["probability"][members], kind="stable")]
        np.testing.assert_array_equal(got["rank"][order], np.arange(len(members)), err_msg="query %d" % g)


def _check(pool, got, cands, idx, sampling=False, thr=0.8, all_candidates=True):
    from tests.test_gpu_verify import _compare
    exp = pool.expected(sampling)
    _compare(got, [exp[i] for i in idx], cands, thr, all_candidates)
    _assert_copies_identical(pool, got, idx)
    _assert_rank(got, cands)
    np.testing.assert_array_equal(got["sc_sim"], [c["sc_sim"] for c in cands])
    np.testing.assert_array_equal(got["odom_bounds"], [c["odom_bounds"] for c in cands])
    np.testing.assert_array_equal(got["reg"]["status"] == 0, got["reg_ok"] == 1)


def _reg_part(got):
    return b"".join(_bytes_of(got[f]).tobytes() for f in ("reg", "reg_ok", "t_be", "cov", "cov_sampled"))


def _assert_same_job_across_forms(a, b, what, t_be_atol=1e-11):
    """one job across matcher forms -- every integer outcome equal, the pose within 1e-11."""
    for f in REG_INTS:
        np.testing.assert_array_equal(a["reg"][f], b["reg"][f], err_msg="%s: reg.%s" % (what, f))
    for f in ("reg_ok", "cov_sampled"):
        np.testing.assert_array_equal(a[f], b[f], err_msg="%s: %s" % (what, f))
    np.testing.assert_array_equal(a["cfear"][:, 1:], b["cfear"][:, 1:], err_msg=what)
    d = np.abs(a["t_be"] - b["t_be"]).max()
    print("%s: max |t_be difference| %.3e, max |probability difference| %.3e" % (what, d, np.abs(a["probability"] - b["probability"]).max()))
    assert d <= t_be_atol, (what, d)
    return d


# ---- 1. the glue kernels past one workgroup ------------------------------------------------------------------------------------
@pytest.mark.parametrize("peaks_on", ["host", "device", "mixed"])
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_workgroup_boundaries(pool, n, peaks_on):
    """verify_expand / verify_prepare / verify_finish index with blockIdx.x * 256 + threadIdx.x: a last block that is full, one
    short of full, one job long; three blocks.  Query ids grouped (host clouds) or shuffled and negative; every candidate or
    only the best of each query (mixed clouds)."""
    allc = 0 if peaks_on == "mixed" else 1
    cands, idx = V.tile(pool, n, "cycle" if peaks_on == "host" else "shuffled", seed=n)
    got = _run(pool, cands, peaks_on, all_candidates=allc)
    assert got.shape == (n,)
    _check(pool, got, cands, idx, all_candidates=bool(allc))
    assert got["accepted"].sum() >= (n // len(pool) if not allc else n // 4)
    if not allc:
        groups = np.array([c["group"] for c in cands])
        assert all(got["accepted"][groups == g].sum() <= 1 for g in np.unique(groups))


# ---- 2. the matcher's forms, launched from the chain ---------------------------------------------------------------------------
def test_forms_inside_the_chain(pool):
    """Every form forced through the context options at n = 257, each against the oracle and against the default run; then
    n = 8 x CUs + 1 with nothing forced, where first_form picks the 2-wavefront pairs form for the registration: its records
    carry the registration bytes of the forced (2, 20) run."""
    import torch
    from tbv_slam_public_amd import api, _lib as L
    ctx = api.default_context()
    cands, idx = V.tile(pool, 257)
    base = _run(pool, cands)
    _check(pool, base, cands, idx)
    runs, worst = {}, 0.0
    try:
        for waves, kb in FORMS:
            ctx.set_option(L.OPT_MATCHER_WAVES, waves); ctx.set_option(L.OPT_MATCHER_LDS_KB, kb)
            runs[(waves, kb)] = _run(pool, cands)
    finally:
        ctx.set_option(L.OPT_MATCHER_WAVES, 0); ctx.set_option(L.OPT_MATCHER_LDS_KB, 0)
    for form, got in runs.items():
        _check(pool, got, cands, idx)
        worst = max(worst, _assert_same_job_across_forms(got, base, "form %d x %d KB against the default" % form))
    print("forms inside the chain: max |t_be difference| to the default run %.3e" % worst)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 8 * n_cu + 1
    cands_n, idx_n = V.tile(pool, n)
    ctx.profile_enable(True); ctx.profile_read(reset=True)
    try:
        chosen = _run(pool, cands_n)
        prof = ctx.profile_read(reset=True)
    finally:
        ctx.profile_enable(False)
    _check(pool, chosen, cands_n, idx_n)
    m = len(pool)
    assert _reg_part(chosen[:m]) == _reg_part(runs[(2, 20)][:m]), (
        "the chosen form at n = %d is not the 2-wavefront pairs form: profile %r, reg.reserved %r" % (n, prof, chosen["reg"]["reserved"][:m]))


# ---- 3. dense scans in the chain -------------------------------------------------------------------------------------------------
def test_dense_scans_in_the_chain(dense, pool):
    """A batch's launch hint comes from its LARGEST scan.  With ~1 600-cell scans among ordinary candidates (big_pass) the
    regular form defers them to register_large / register_large16, and verify_prepare reads the records those launches wrote;
    with a ~3 000-cell pair (whole_cu) the cost launch takes the CU's whole LDS.  n = 2 x CUs + 5 puts three workgroups on a
    CU, where first_form gives the same form (4 wavefronts, a third of the LDS) with and without small_pairs -- so the
    ordinary candidates' registration bytes must equal those of a batch without the dense ones."""
    import torch
    from tbv_slam_public_amd import api
    ctx = api.default_context()
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    for p, large_names in zip(dense, (("register_large", "register_large16"), ("register_large16", "register_large"))):
        cands, idx = V.tile(p, n)
        ctx.profile_enable(True); ctx.profile_read(reset=True)
        try:
            got = _run(p, cands)
            prof = ctx.profile_read(reset=True)
        finally:
            ctx.profile_enable(False)
        _check(p, got, cands, idx)
        assert sum(prof.get(k, (0.0, 0))[1] for k in large_names) >= 1, prof
        is_dense = idx >= 12
        assert (got["reg"]["reserved"][is_dense] == 1.0).all() and (got["reg"]["reserved"][~is_dense] == 0.0).all()
        large_ms = sum(prof.get(k, (0.0, 0))[0] for k in large_names)
        print("dense chain %s: profile %r" % (p.cands[-1]["name"], {k: v for k, v in prof.items() if k.startswith(("register", "get_cost"))}))
        assert large_ms > 0.0
        # the same batch positions without the dense candidates: same first form, so the same registration bytes
        plain_cands = [dict(pool.cands[i % 12], group=c["group"]) for i, c in zip(idx, cands)]
        plain = _run(pool, plain_cands)
        keep = np.nonzero(~is_dense)[0]
        assert _reg_part(got[keep]) == _reg_part(plain[keep])


# ---- 4. CorAl launched from the chain in two launches ----------------------------------------------------------------------------
def test_coral_in_two_launches(pool):
    """One candidate's merged peak cloud just under cfear_coral_max_points() (coral_geometry.MAX_POINTS) sets the batch's scratch stride; enough ordinary
    candidates around it that n x stride exceeds the 1 GiB a CorAl launch may use.  The profile counts one scope for all
    launches, so the split is asserted by its arithmetic (verify_cases.coral_chunk restates coral_launch's)."""
    from oracle import pyoracle as O
    from tests import coral_geometry as G
    from tests.test_oracle_coral import _tf
    nodes = [dict(nd) for nd in pool.nodes]
    max_pts = G.MAX_POINTS
    room = max_pts - 4 - len(nodes[4]["peaks"]) - len(nodes[0]["peaks"])
    extra = G.cluster_pair(60, room // 2, room - room // 2, (150, 200, 150, 200))
    for i, e in ((4, extra[0]), (0, extra[1])):
        w = e.copy()
        w[:, :2] = _tf(e, O.xyt_inverse(nodes[i]["T"]))
        nodes[i] = dict(nodes[i], peaks=np.ascontiguousarray(np.concatenate([nodes[i]["peaks"], w]), dtype=np.float32))
    nodes += [nodes[4], nodes[0]]                                        # the padded clouds as nodes of their own ...
    nodes[4], nodes[0] = pool.nodes[4], pool.nodes[0]                    # ... the pool's stay what they were
    a, b = len(nodes) - 2, len(nodes) - 1
    padded = V.cand(nodes, a, b, (0.5, -0.4, 0.03), 0.15, 0.0, name="padded")
    cap = len(nodes[a]["peaks"]) + len(nodes[b]["peaks"])
    assert max_pts - 8 <= cap < max_pts
    chunk = V.coral_chunk(cap)
    n = chunk + 35
    assert n * V.coral_scratch_bytes(cap) > 1 << 30 and chunk < n <= 2 * chunk and 1300 < chunk < 1400      # two launches
    p = V.Pool(nodes, pool.cands + [padded])
    p._exp[False] = pool.expected() + [V.oracle_answer(nodes, padded)]
    cands, idx = V.tile(pool, n)
    where = chunk + 7                                                    # the padded candidate rides in the second launch
    cands[where] = dict(padded, group=cands[where]["group"])
    idx[where] = len(pool)
    got = _run(p, cands, nodes=nodes)
    _check(p, got, cands, idx)
    assert got["reg_ok"][where] == 1 and got["coral"][where][2] > 0.1
    assert set(idx[:chunk]) == set(idx[chunk:]) - {len(pool)} == set(range(len(pool)))     # every candidate on both sides of the split


# ---- 5. the refusal that comes back from the device ------------------------------------------------------------------------------
def _beyond_the_grid(nodes, c):
    """The query node's peak cloud with two small clusters 4 500 m apart along the WORLD's y at the candidate's from_pose: more
    than 4096 grid rows, which coral_kernel refuses with CFEAR_ERR_CAPACITY as the job's status
    (tests/test_gpu_coral_geometry.py::test_refusals_by_size_radius_and_grid)."""
    from oracle import pyoracle as O
    from tests import coral_geometry as G
    from tests.test_oracle_coral import _tf
    x, y = c["from_pose"][:2]
    extra = np.concatenate([G.clutter(70, 40, x, x + 8.0, y, y + 8.0), G.clutter(80, 40, x, x + 8.0, y + 4500.0, y + 4508.0)])
    extra[:, :2] = _tf(extra, O.xyt_inverse(c["from_pose"]))
    return np.ascontiguousarray(np.concatenate([nodes[c["f"]]["peaks"], extra]), dtype=np.float32)


def _with_nan(cloud):
    c = cloud.copy()
    c[7, 1] = np.nan
    return c


def test_refusal_from_the_device_names_the_first_job(pool):
    """Jobs 300 and 40 (two different workgroups of verify_finish) are refused by coral_kernel: the call fails with their status
    and names the SMALLEST index; the same holds with a device results pointer; afterwards the context verifies the clean
    batch and its records equal a fresh context's byte for byte (first_bad is reset by every call).
    What coral_kernel refuses per job is a grid of more than 4096 rows.  A single NaN coordinate is NOT refused (measured:
    fminf / fmaxf drop it from the bounding box and the point is nobody's neighbour; tests/test_gpu_robustness.py pins the
    finite outcome), so the same two jobs with a NaN coordinate leave the call successful and every other record untouched."""
    import torch
    from tbv_slam_public_amd import api, _lib as L
    n = 513
    cands, idx = V.tile(pool, n)
    bad = {}
    for j in (300, 40):
        assert len(pool.nodes[cands[j]["t"]]["peaks"]), "job %d must reach the kernel's grid, not its empty-cloud exit" % j
        bad[j] = dict(from_peaks=_beyond_the_grid(pool.nodes, cands[j]))
    buf = torch.zeros(n * L.VERIFY_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    for device_ptr in (None, buf.data_ptr()):
        with pytest.raises(L.CfearError) as e:
            _run(pool, cands, overrides=bad, device_ptr=device_ptr)
        assert e.value.status == L.ERR_CAPACITY
        assert "job 40:" in str(e.value), str(e.value)
    with pytest.raises(L.CfearError) as e:                               # one bad job only, in the last workgroup
        _run(pool, cands, overrides={512: dict(from_peaks=_beyond_the_grid(pool.nodes, cands[512]))})
    assert e.value.status == L.ERR_CAPACITY and "job 512:" in str(e.value), str(e.value)
    after = _run(pool, cands)
    _check(pool, after, cands, idx)
    nan = _run(pool, cands, overrides={j: dict(to_peaks=_with_nan(pool.nodes[cands[j]["t"]]["peaks"])) for j in (300, 40)})
    others = np.setdiff1d(np.arange(n), (300, 40))
    assert nan[others].tobytes() == after[others].tobytes()
    for j in (300, 40):
        assert nan["reg"][j].tobytes() == after["reg"][j].tobytes() and np.isfinite(nan["coral"][j]).all() and np.isfinite(nan["probability"][j])
    fresh_ctx = api.Context(0, torch.cuda.current_stream(0).cuda_stream or 1)
    try:
        fresh_nodes = V.attach_scans(pool.nodes, ctx=fresh_ctx)
        fresh = _run(pool, cands, nodes=fresh_nodes, ctx=fresh_ctx)
        del fresh_nodes
    finally:
        fresh_ctx.synchronize()
    assert after.tobytes() == fresh.tobytes()


# ---- 6. the host chain against the device chain -----------------------------------------------------------------------------------
def test_host_chain_against_device_chain(pool):
    """verify_host_chain (use_covariance_sampling) restates the chain on the host: the same 257 candidates through both, each
    against the oracle with the same setting, and against each other -- registration integers and cfear[1:] equal, t_be within
    1e-11, probability within 1e-9 (the same kernels on poses that differ by libm's last bit)."""
    hits = pool.check_sampling()
    cands, idx = V.tile(pool, 257)
    dev = _run(pool, cands, use_covariance_sampling=0)
    host = _run(pool, cands, use_covariance_sampling=1)
    _check(pool, dev, cands, idx)
    from tests.test_gpu_verify import _compare
    exp = pool.expected(True)
    _compare(host, [exp[i] for i in idx], cands)
    _assert_rank(host, cands)
    for f in REG_INTS:
        np.testing.assert_array_equal(host["reg"][f], dev["reg"][f], err_msg=f)
    np.testing.assert_array_equal(host["reg_ok"], dev["reg_ok"])
    np.testing.assert_array_equal(host["cfear"][:, 1:], dev["cfear"][:, 1:])
    dt, dp = np.abs(host["t_be"] - dev["t_be"]).max(), np.abs(host["probability"] - dev["probability"]).max()
    print("host chain against device chain: max |t_be difference| %.3e, max |probability difference| %.3e" % (dt, dp))
    assert dt <= 1e-11 and dp <= 1e-9, (dt, dp)
    np.testing.assert_array_equal(host["accepted"], dev["accepted"])
    # the sampled covariances, and the candidates that put R C R^T under test
    block = np.ix_([0, 1, 5], [0, 1, 5])
    rotated = 0
    for g, i, c in zip(host, idx, cands):
        e = exp[i]
        assert bool(g["cov_sampled"]) == e["cov_sampled"]
        if e["cov_sampled"]:
            np.testing.assert_allclose(g["cov"][block], e["cov"][block], rtol=1e-4, atol=1e-12, err_msg=c["name"])
            assert np.linalg.eigvalsh(g["cov"][block]).min() > 0
            np.testing.assert_allclose(g["cov"][2:5, 2:5], np.eye(3), atol=1e-15)
            rotated += bool(g["accepted"]) and c["name"] in hits
    assert rotated >= len(hits)
    for p in np.unique(idx):                                             # copies inside the host chain's call
        rows = np.nonzero(idx == p)[0]
        for f in _copy_fields():
            b = _bytes_of(host[f][rows])
            assert (b == b[0]).all(), (pool.cands[p]["name"], f)


# ---- 7. records left on the device, at scale ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("allc", [0, 1])
def test_records_left_on_the_device_at_scale(pool, allc):
    """tests/test_gpu_verify.py::test_verify_records_left_on_the_device_equal_the_host_records at n = 513 with shuffled query
    ids: the device-pointer route plus cfear_verify_apply_constraints equals the host-pointer route byte for byte."""
    import torch
    from tbv_slam_public_amd import api, _lib as L
    n = 513
    cands, idx = V.tile(pool, n, "shuffled", seed=7)
    host = _run(pool, cands, all_candidates=allc)
    _check(pool, host, cands, idx, all_candidates=bool(allc))
    buf = torch.full((n * L.VERIFY_RESULT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    assert _run(pool, cands, device_ptr=buf.data_ptr(), all_candidates=allc) == n
    dev = buf.cpu().numpy().view(L.VERIFY_RESULT_DTYPE).copy()
    assert (dev["accepted"] == 0).all() and (dev["rank"] == 0).all()
    api.verify_apply_constraints(dev, [c["group"] for c in cands], api.verify_params(all_candidates=allc))
    assert dev.tobytes() == host.tobytes()
    assert host["accepted"].sum() >= 20
