"""GPU: trajectory synchronisation (cfear_sync_trajectories, csrc/trajsync.hip) against the serial restatement
tests/trajsync_cpu.py (pinned by properties in tests/test_trajsync_cpu.py), on host and on device buffers, in both modes.

Exact, bit for bit, on every case: counts, every est_index, gt_index and alpha, stamps_out, the kept estimate poses, and the
ground truth's translation column including the z of 0; what lies behind a pair's kept rows and between the pairs is not
written.  A pair's outputs are identical whatever batch it sits in, wherever it sits, and whether the buffers are host or
device memory.

Rotation entries: TOL below.  The interpolation calls acos once and sin three times; the device's may differ from libm's in
the last place, and the difference passes through a division and the products of toRotationMatrix.  TOL is 10 x the largest
deviation of a rotation entry measured on the MI355X against the restatement over all cases of this file, the batch of
300 included (EXPERIMENTS.md, "Trajectory synchronisation"): the largest deviation seen was 1.332e-15 (six units in the last
place of an entry near 1, in the case rotations_all_branches), so TOL = 1.332e-14."""
import os
import subprocess

import numpy as np
import pytest

import trajsync_cpu as M
from tbv_slam_public_amd import _lib as L

pytestmark = pytest.mark.gpu

MEASURED_DEVIATION = 1.3322676295501878e-15       # on the MI355X, over every case of this file
TOL = 10 * MEASURED_DEVIATION
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = M.cases()
MODES = ("chained", "independent")
WORST = [0.0]                   # the largest rotation deviation seen so far (printed by every test that compares rotations)
ROT = [0, 1, 2, 4, 5, 6, 8, 9, 10]
_REF = {}


def _api():
    from tbv_slam_public_amd import api
    return api


def ref(c, mode, with_est=True):
    """The restatement's result of a case, computed once and shared."""
    key = (c["name"], mode, with_est)
    if key not in _REF:
        _REF[key] = M.sync_pair(c["est"] if with_est else None, c["est_stamps"], c["gt"], c["gt_stamps"], mode)
    return _REF[key]


def lib_sync(pairs, mode, eo=None, go=None, device=False, with_est=True):
    """cfear_sync_trajectories on `pairs`, laid out at eo / go (None: one after the other, offsets NULL) in arrays whose gaps
    hold NaN / -1; the outputs are pre-filled with 7.  -> dict of host arrays est, gt, stamps, rows, counts, offsets."""
    import torch
    api = _api()
    le = np.array([len(p["est_stamps"]) for p in pairs], np.int32)
    lg = np.array([len(p["gt_stamps"]) for p in pairs], np.int32)
    e_at = np.concatenate([[0], np.cumsum(le)]).astype(np.int64) if eo is None else np.asarray(eo, np.int64)
    g_at = np.concatenate([[0], np.cumsum(lg)]).astype(np.int64) if go is None else np.asarray(go, np.int64)
    ne, ng = int(e_at[-1]), int(g_at[-1])
    est, gt = np.full((ne, 12), np.nan), np.full((ng, 12), np.nan)
    es, gs = np.full(ne, -1, np.int64), np.full(ng, -1, np.int64)
    for t, p in enumerate(pairs):
        est[e_at[t]:e_at[t] + le[t]], es[e_at[t]:e_at[t] + le[t]] = p["est"], p["est_stamps"]
        gt[g_at[t]:g_at[t] + lg[t]], gs[g_at[t]:g_at[t] + lg[t]] = p["gt"], p["gt_stamps"]
    outs = [np.full((ne, 12), 7.0), np.full((ne, 12), 7.0), np.full(ne, 7, np.int64), np.full(ne, 7, L.SYNC_ROW_DTYPE)]
    counts = np.full(len(pairs), 7, np.int32)
    ins = [est if with_est else None, es, gt, gs]
    if device:
        up = lambda a: None if a is None else torch.from_numpy(a.view(np.uint8) if a.dtype == L.SYNC_ROW_DTYPE else a).cuda()
        ins, d_outs = [up(a) for a in ins], [up(a) for a in outs]
        torch.cuda.synchronize()
    else:
        d_outs = outs
    ptr = lambda a: None if a is None else (a.data_ptr() if device else a.ctypes.data)
    ctx = api.default_context()
    ctx.check(ctx._lib.cfear_sync_trajectories(ctx.h, L.SYNC_MODE[mode], ptr(ins[0]), ptr(ins[1]), None if eo is None else e_at.ctypes.data, le.ctypes.data,
                                               ptr(ins[2]), ptr(ins[3]), None if go is None else g_at.ctypes.data, lg.ctypes.data, len(pairs),
                                               ptr(d_outs[0]) if with_est else None, ptr(d_outs[1]), ptr(d_outs[2]), ptr(d_outs[3]), counts.ctypes.data))
    if device:
        ctx.synchronize()
        outs = [o.cpu().numpy() for o in d_outs]
        outs[3] = outs[3].view(L.SYNC_ROW_DTYPE).reshape(-1)
    return dict(est=outs[0], gt=outs[1], stamps=outs[2], rows=outs[3], counts=counts, offsets=e_at, lengths=le, device=d_outs)


def pair_bytes(out, t):
    o, n = int(out["offsets"][t]), int(out["counts"][t])
    return b"".join(out[k][o:o + n].tobytes() for k in ("est", "gt", "stamps", "rows"))


def check_pair(out, t, want, with_est=True):
    """Pair t of a library result against the restatement: everything exact but the rotation entries."""
    o, n = int(out["offsets"][t]), int(out["counts"][t])
    assert n == want["count"]
    assert out["rows"][o:o + n].tobytes() == want["rows"].tobytes()                       # est_index, gt_index, alpha
    assert out["stamps"][o:o + n].tobytes() == want["stamps"].tobytes()
    if with_est:
        assert out["est"][o:o + n].tobytes() == want["est"].tobytes()                     # copied bit for bit
    g = out["gt"][o:o + n]
    assert g[:, [3, 7, 11]].tobytes() == want["gt"][:, [3, 7, 11]].tobytes() and (g[:, 11] == 0.0).all() and not np.signbit(g[:, 11]).any()
    dev = float(np.abs(g[:, ROT] - want["gt"][:, ROT]).max()) if n else 0.0
    WORST[0] = max(WORST[0], dev)
    assert dev <= TOL, (dev, TOL)
    # behind the kept rows of the pair nothing is written
    tail = slice(o + n, o + int(out["lengths"][t]))
    assert (out["gt"][tail] == 7.0).all() and (out["stamps"][tail] == 7).all() and (out["rows"][tail]["est_index"] == 7).all()
    assert (out["est"][tail] == 7.0).all()
    return dev


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_on_host_and_device_buffers(case):
    for mode in MODES:
        want = ref(case, mode)
        host = lib_sync([case], mode)
        dev = lib_sync([case], mode, device=True)
        check_pair(host, 0, want)
        check_pair(dev, 0, want)
        assert pair_bytes(host, 0) == pair_bytes(dev, 0)
    print("largest rotation deviation so far: %.3e" % WORST[0])


def test_modes_differ_where_a_stamp_lies_in_two_intervals():
    c = [k for k in CASES if k["name"] == "est_equals_gt_stamp"][0]
    for device in (False, True):
        a, b = lib_sync([c], "chained", device=device), lib_sync([c], "independent", device=device)
        assert a["counts"][0] == ref(c, "chained")["count"] != ref(c, "independent")["count"] == b["counts"][0]
        rows = lambda out: dict(rows=out["rows"][:out["counts"][0]])
        # estimates both modes keep, on different intervals: the chained walk stays on the later one (max(position, a), alpha 0)
        # where the search from the first pose takes the earlier (a, alpha 1)
        assert M.both_kept_differ(rows(a), rows(b)) == [(1, 5, 0.0, 4, 1.0), (2, 5, 0.0, 4, 1.0), (7, 12, 0.0, 11, 1.0)]
    d = [k for k in CASES if k["name"] == "duplicate_gt_stamps"][0]
    a, b = lib_sync([d], "chained", device=True), lib_sync([d], "independent", device=True)
    assert M.both_kept_differ(dict(rows=a["rows"][:a["counts"][0]]), dict(rows=b["rows"][:b["counts"][0]])) == [(8, 9, 0.0, 6, 1.0)]


def test_batch_of_300_with_explicit_offsets():
    pairs, eo, go = M.batch_300()
    singles = {}
    for device in (False, True):
        for mode in MODES:
            out = lib_sync(pairs, mode, eo, go, device=device)
            for t, p in enumerate(pairs):
                check_pair(out, t, ref(p, mode))
                singles.setdefault((t, mode), pair_bytes(out, t))
                assert pair_bytes(out, t) == singles[(t, mode)]                              # host == device
            # between the pairs nothing is written either
            used = np.zeros(int(eo[-1]), bool)
            for t in range(len(pairs)):
                used[eo[t]:eo[t] + out["lengths"][t]] = True
            assert (~used).any() and (out["gt"][~used] == 7.0).all() and (out["stamps"][~used] == 7).all() and (out["est"][~used] == 7.0).all()
    # a pair's outputs do not depend on the batch or on its place in it: alone, and in a reversed batch without offsets
    for t in (0, 7, 139, 141, 150, 299):
        for mode in MODES:
            assert pair_bytes(lib_sync([pairs[t]], mode, device=True), 0) == singles[(t, mode)]
    rev = lib_sync(pairs[::-1], "chained", device=True)
    assert all(pair_bytes(rev, 299 - t) == singles[(t, "chained")] for t in range(300))
    print("largest rotation deviation so far: %.3e" % WORST[0])


def test_est_null_labels_stamps_in_independent_mode():
    cs = [c for c in CASES if c["name"] in ("est_before_and_after", "backward_mid_chunk", "duplicate_gt_stamps", "gt_len_2", "est_len_65")]
    for device in (False, True):
        out = lib_sync(cs, "independent", device=device, with_est=False)
        for t, c in enumerate(cs):
            o, n = int(out["offsets"][t]), int(out["counts"][t])
            want = ref(c, "independent", with_est=False)
            assert n == want["count"] and out["rows"][o:o + n].tobytes() == want["rows"].tobytes()
            assert out["stamps"][o:o + n].tobytes() == want["stamps"].tobytes() and np.abs(out["gt"][o:o + n] - want["gt"]).max(initial=0.0) <= TOL
        assert (out["est"] == 7.0).all()                                                     # est_out is unused
    api = _api()
    r = api.sync_trajectories(None, [c["est_stamps"] for c in cs], [c["gt"] for c in cs], [c["gt_stamps"] for c in cs], mode="independent")
    assert r.est is None and r.counts.tolist() == [ref(c, "independent", False)["count"] for c in cs]
    assert r.pair(1)["rows"].tobytes() == ref(cs[1], "independent", False)["rows"].tobytes()


def _e2e_pairs():
    """Six pairs of a 4 Hz estimate against a 50 Hz ground truth that starts after the first sweep and ends before the last:
    three with a ground truth of pure translations (the interpolation then has no acos or sin in it: bit-exact), three planar."""
    pairs = []
    for t in range(6):
        n_est = 60 + 7 * t
        es = M.T0 + np.arange(n_est, dtype=np.int64) * 250_000_000
        n_gt = (n_est - 2) * 12
        gs = M.gt_grid(n_gt, start=M.T0 + 300_000_000, jitter=1_000_000, seed=t)
        path = M.planar_path(n_gt, 70 + t)
        path[:, [3, 7]] *= 0.08                                  # 50 Hz steps
        if t < 3:
            path[:, ROT] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        est = M.planar_path(n_est, 80 + t)
        pairs.append(M.case("e2e_%d" % t, es, gs, gt=path, est=est))
    return pairs


def test_device_outputs_go_straight_into_the_evaluator():
    """est_out, gt_out, est_offsets and counts of the device call are cfear_eval_trajectories' arguments as they are.  The result
    equals the evaluator run on the restatement's arrays: byte for byte where the ground truth only translates (nothing in the
    interpolation is then left to acos or sin), and otherwise row for row in every integer, length and speed.  The other
    figures of a rotating pair see the ground truth's rotation entries, which may deviate by d <= TOL:
      * a translation figure (t_err, ATE, RPE in metres) is a rotation block times a position difference of at most X, the
        trajectory's extent, through at most four pose products and inverses: 3 entries x 4 x d x X = 12 TOL X metres, and
        t_err is that divided by its segment's length, at least the shortest evaluated length;
      * a rotation figure is acos(1 - e) ~ sqrt(2 e) near a zero angle, with e = half the error of a trace that went through
        the same products, 0.5 x 3 x 12 d = 2.4e-13: below 1e-6 rad, divided by the length for r_err."""
    api = _api()
    pairs = _e2e_pairs()
    eo = np.concatenate([[2], 2 + np.cumsum([len(p["est_stamps"]) + 3 for p in pairs])]).astype(np.int64)
    out = lib_sync(pairs, "chained", eo=eo, device=True)
    want = [ref(p, "chained") for p in pairs]
    assert out["counts"].tolist() == [w["count"] for w in want] and all(2 <= w["count"] < len(p["est_stamps"]) for w, p in zip(want, pairs))
    par = api.eval_params(step_size=3, lengths=[5, 10, 15, 20, 25, 30, 35, 40])
    d_est, d_gt = out["device"][0], out["device"][1]
    s_dev, r_dev = api.eval_trajectories(d_est, d_gt, lengths=out["counts"], offsets=eo[:-1].copy(), par=par)
    s_ref, r_ref = api.eval_trajectories([w["est"] for w in want], [w["gt"] for w in want], par=par)
    assert len(r_dev) == len(r_ref) > 50 and (s_dev["status"] == L.OK).all()
    for k in ("trajectory", "first_frame", "last_frame", "length"):
        assert (r_dev[k] == r_ref[k]).all(), k
    exact = r_ref["trajectory"] < 3
    assert exact.any() and (~exact).any()
    assert r_dev[exact].tobytes() == r_ref[exact].tobytes() and s_dev[:3].tobytes() == s_ref[:3].tobytes()
    extent = max(np.abs(w[k][:, [3, 7]] - w[k][0, [3, 7]]).max() for w in want for k in ("est", "gt"))
    metres, shortest = 12 * TOL * extent, 5.0
    assert 50 < extent < 500 and metres < 1e-10
    assert r_dev["speed"].tobytes() == r_ref["speed"].tobytes()
    bounds = dict(t_err=metres / shortest, r_err=1e-6 / shortest)
    for k, bound in bounds.items():
        dev = np.abs(r_dev[k] - r_ref[k]).max()
        print("row figure %s: largest deviation %.3e, bound %.3e" % (k, dev, bound))
        assert dev <= bound, k
    for k, bound in dict(ate=metres, rpe_trans=metres, ave_t_err=metres / shortest, rpe_rot=1e-6, ave_r_err=1e-6 / shortest).items():
        dev = np.abs(s_dev[k] - s_ref[k]).max()
        print("summary figure %s: largest deviation %.3e, bound %.3e" % (k, dev, bound))
        assert dev <= bound, k
    # the mirror's own path: sync_trajectories on device tensors, its result handed to eval_trajectories unchanged
    import torch
    cu = lambda xs: [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]
    r = api.sync_trajectories(cu([p["est"] for p in pairs]), cu([p["est_stamps"] for p in pairs]), cu([p["gt"] for p in pairs]),
                              cu([p["gt_stamps"] for p in pairs]))
    s_api, r_api = api.eval_trajectories(r.est, r.gt, lengths=r.counts, offsets=r.offsets, par=par)
    assert s_api.tobytes() == s_dev.tobytes() and r_api.tobytes() == r_dev.tobytes()
    assert all(r.pair(t)["rows"].tobytes() == want[t]["rows"].tobytes() for t in range(6))


def test_device_buffers_are_refused_by_the_check_kernel():
    c = [k for k in CASES if k["name"] == "est_len_65"][0]
    other = [k for k in CASES if k["name"] == "gt_len_4"][0]
    api = _api()
    ctx = api.default_context()

    def refused(pairs):
        with pytest.raises(L.CfearError) as e:
            lib_sync(pairs, "chained", device=True)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        return ctx._lib.cfear_last_error(ctx.h).decode()

    edit = lambda p, key, i, v: dict(p, **{key: np.concatenate([p[key][:i], [v], p[key][i + 1:]]).astype(np.int64)})
    assert refused([other, edit(c, "gt_stamps", 17, c["gt_stamps"][16] - 1)]) == "pair 1: ground-truth stamp 17 is earlier than the one before it"
    assert refused([other, edit(c, "est_stamps", 64, -3)]) == "pair 1: estimate stamp 64 is negative or past 2^32 - 1 seconds"
    assert refused([edit(other, "gt_stamps", 3, 2 ** 32 * 10 ** 9), c]) == "pair 0: ground-truth stamp 3 is negative or past 2^32 - 1 seconds"
    # a batch without a single estimate is still checked: what host buffers are refused for, device buffers are refused for
    import torch
    none = dict(c, est=c["est"][:0], est_stamps=c["est_stamps"][:0])
    assert lib_sync([none], "chained", device=True)["counts"].tolist() == [0]
    assert refused([edit(none, "gt_stamps", 17, c["gt_stamps"][16] - 1)]) == "pair 0: ground-truth stamp 17 is earlier than the one before it"
    # host and device buffers mixed
    d = torch.zeros(65, dtype=torch.int64, device="cuda")
    with pytest.raises(L.CfearError):
        api.sync_trajectories([c["est"]], [d], [c["gt"]], [c["gt_stamps"]])
    h = lib_sync([c], "chained")
    le, lg, counts = np.array([65], np.int32), np.array([len(c["gt_stamps"])], np.int32), np.zeros(1, np.int32)
    rc = ctx._lib.cfear_sync_trajectories(ctx.h, 0, c["est"].ctypes.data, d.data_ptr(), None, le.ctypes.data, c["gt"].ctypes.data,
                                          c["gt_stamps"].ctypes.data, None, lg.ctypes.data, 1, h["est"].ctypes.data, h["gt"].ctypes.data,
                                          h["stamps"].ctypes.data, h["rows"].ctypes.data, counts.ctypes.data)
    assert rc == L.ERR_INVALID_ARGUMENT and "all host or all device" in ctx._lib.cfear_last_error(ctx.h).decode()


def test_collector_saves_the_five_files(tmp_path):
    api = _api()
    p = _e2e_pairs()[4]
    want = ref(p, "chained")
    cov = np.arange(36.0)[None, :] * (1.0 + np.arange(len(p["est_stamps"])))[:, None] * 1e-4
    ev = api.EvalTrajectory()
    for i in range(len(p["est_stamps"])):
        ev.CallbackESTEigen((p["est"][i], cov[i], p["est_stamps"][i]))
    for i in range(len(p["gt_stamps"])):
        ev.CallbackGTEigen((p["gt"][i], None, p["gt_stamps"][i]))
    found, at = ev.Interpolate(int(p["est_stamps"][5]))
    one = M.sync_pair(None, p["est_stamps"][5:6], p["gt"], p["gt_stamps"], "independent")
    assert found and np.abs(at[0] - one["gt"][0]).max() <= TOL and at[2] == p["est_stamps"][5] and not ev.Interpolate(int(M.T0))[0]
    paths = ev.Save(str(tmp_path / "est"), str(tmp_path / "gt"), "03.txt")
    assert [os.path.relpath(q, tmp_path) for q in paths] == ["gt/03.txt", "gt/tum_03.txt", "est/03.txt", "est/tum_03.txt", "est/cov_03.txt"]
    assert ev.GetSize() == want["count"] == len(ev.est_vek) == len(ev.gt_vek)
    assert open(paths[3]).read() == M.tum_text(want["est"], want["stamps"])
    assert open(paths[4]).read() == M.cov_text(cov[want["rows"]["est_index"]], want["stamps"])
    assert open(paths[1]).read() == M.tum_text(want["gt"], want["stamps"])                  # 4 decimals / 4 digits hide the last place
    assert np.allclose(api.kitti_read(paths[0]), want["gt"], atol=1e-6) and np.allclose(api.kitti_read(paths[2]), want["est"], atol=1e-6)
    assert [t for t, _ in ev.GetGtVek()] == want["stamps"].tolist()                            # the estimate's stamps: AddGroundTruth matches them


def test_cpp_collector_runs(tmp_path):
    exe = str(tmp_path / "trajsync_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "trajsync_signature.cpp"), "-o", exe, "-L", so_dir, "-lcfear_hip",
                           "-Wl,-rpath," + so_dir])
    out = subprocess.check_output([exe, "run", str(tmp_path)]).decode().splitlines()
    # estimates at 0, 0.25, ... 2 s; ground truth from 0.3 s to 1.68 s: 0.5 ... 1.5 s are kept
    es = M.T0 + np.arange(9, dtype=np.int64) * 250_000_000
    gs = M.T0 + 300_000_000 + np.arange(70, dtype=np.int64) * 20_000_000
    gt = np.array([M.planar(0.04 * i, 0.02 * i, 0.008 * i) for i in range(70)])
    est = np.array([M.planar(0.5 * i, 0.25 * i, 0.1 * i) for i in range(9)])
    want = M.sync_pair(est, es, gt, gs)
    assert want["count"] == 5 and out[0] == "9 70 1 0"
    first = out[1].split()
    assert first[:3] == ["5", "5", "500000000"] and abs(float(first[3]) - want["gt"][0][3]) == 0.0
    assert open(tmp_path / "est" / "tum_05.txt").read() == M.tum_text(want["est"], want["stamps"])
    assert open(tmp_path / "gt" / "tum_05.txt").read() == M.tum_text(want["gt"], want["stamps"])
    assert len(open(tmp_path / "est" / "cov_05.txt").read().splitlines()) == 5
