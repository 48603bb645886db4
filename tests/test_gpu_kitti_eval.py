"""GPU: the batched KITTI odometry metric (cfear_eval_trajectories, csrc/evaluate.hip).

Against the REFERENCE'S RECORD on the committed jobs (tests/golden/ref_kitti_eval*.npz: inputs and outputs of its own
eval_odom.py --align 6dof), and against the NumPy restatement tests/kitti_eval_cpu.py (itself pinned to that record by
tests/test_kitti_eval_cpu.py) on inputs the reference has no record of.

Exact, no tolerance, on every input: the number of rows and every first_frame, last_frame and length; and a trajectory's
result is bit-identical whatever batch it is evaluated in.

Floating figures: TOL below.  It bounds |r_err / len| and |t_err / len| of a row against the record; it was set to 10 x the
largest deviation measured on the MI355X over all committed jobs (EXPERIMENTS.md, "Trajectory evaluation").  Against the
restatement the same bound is used, scaled by the magnitude of the quantity:
  * a pose product's rounding error grows with the size of the translations it multiplies; the record's trajectories stay
    within ~1.3 km of their origin, so a synthetic trajectory of extent X (largest |translation| after normalisation, in
    either trajectory) gets TOL * max(1, X / 1000 m);
  * a row is an error in metres or radians divided by a length of at least 100 m; the figures that are not divided (ATE,
    RPE, biases, RMSE, in metres or radians) get 100 x that.
With alignment 6dof the restatement is given the [r | t] the library reports (summary field `align`) and applies it in
the same way, so that both sides run one operation sequence behind the SVD, as they do for `none`: rows and figures are
then held to the bound above, with nothing added.  The [r | t] itself is checked against the restatement's own (LAPACK's
SVD of a covariance NumPy summed) in check_alignment, with the bound that is written there.
Each of the 11 summary figures of a committed job, formatted as write_result formats it, must equal the recorded string."""
import os

import numpy as np
import pytest

import kitti_eval_cpu as K
from test_kitti_eval_cpu import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

# measured on the MI355X against the record (both jobs, all 6755 rows): 5.681e-15 (t_err / len), 8.536e-15 (r_err / len);
# the restatement on the CPU sits 7.1e-15 and 6.9e-15 from the same record
TOL = 8.5e-14
FIGS = K.FIGURES
ALIGN_WORST = [0.0, 0.0]        # largest |dr| and |dt| seen by check_alignment, as fractions of their bounds (printed)


def _api():
    from tbv_slam_public_amd import api
    return api


def planar(rng, n, step=2.0, drift=2e-3, decimals=None):
    """A planar random walk and an estimate that drifts away from it; [n, 12] each."""
    th = np.cumsum(rng.normal(0, 0.02, n))
    v = step * (1 + 0.2 * rng.normal(size=n))
    x, y = np.cumsum(v * np.cos(th)), np.cumsum(v * np.sin(th))
    the = th + np.cumsum(rng.normal(0, drift, n)) + 0.3
    xe = np.cumsum(v * (1 + 0.01 * rng.normal(size=n)) * np.cos(the)) + 5.0
    ye = np.cumsum(v * np.sin(the)) - 3.0
    api = _api()
    gt, est = api.kitti_from_xyt(np.stack([x, y, th], 1)), api.kitti_from_xyt(np.stack([xe, ye, the], 1))
    if decimals is not None:
        gt, est = np.round(gt, decimals), np.round(est, decimals)            # a pose file's non-orthonormal blocks
    return est, gt


def _rot(ax, ang):
    c, s, z, o = np.cos(ang), np.sin(ang), np.zeros_like(ang), np.ones_like(ang)
    m = {"x": [o, z, z, z, c, -s, z, s, c], "y": [c, z, s, z, o, z, -s, z, c], "z": [c, -s, z, s, c, z, z, z, o]}[ax]
    return np.stack(m, 1).reshape(-1, 3, 3)


def spatial(rng, n, step=2.0):
    """A truly 3-D pair: yaw, pitch and roll all move, and so does z."""
    def one(yaw, pitch, roll, v):
        R = _rot("z", yaw) @ _rot("y", pitch) @ _rot("x", roll)
        t = np.cumsum(R[:, :, 0] * v[:, None], 0)
        return np.concatenate([R, t[:, :, None]], 2).reshape(-1, 12)
    yaw, pitch, roll = np.cumsum(rng.normal(0, 0.02, n)), 0.3 * np.sin(np.arange(n) / 40.0), np.cumsum(rng.normal(0, 0.005, n))
    v = step * (1 + 0.2 * rng.normal(size=n))
    gt = one(yaw, pitch, roll, v)
    est = one(yaw + np.cumsum(rng.normal(0, 2e-3, n)) + 0.2, pitch + 0.01 * rng.normal(size=n) + 0.1,
              roll + np.cumsum(rng.normal(0, 1e-3, n)), v * 1.01)
    est[:, 3::4] += [4.0, -2.0, 1.0]
    return est, gt


def exact_steps():
    """Ground-truth distances that are exact sums, so that dist[first] + L EQUALS a later dist and only the strict `>`
    (kitti_odometry.py:193) picks the frame after it; with a stationary stretch (equal dist values) across such a tie."""
    seg = [(1.0, 0.0)] * 150 + [(0.0, 0.0)] * 30 + [(1.0, 0.0)] * 120 + [(0.0, 0.5)] * 400 + [(0.0, 0.0)] * 25 + [(0.0, 0.5)] * 900
    xy = np.concatenate([[[0.0, 0.0]], np.cumsum(np.array(seg), 0)])
    th = np.where(np.arange(len(xy)) <= 300, 0.0, np.pi / 2)
    api = _api()
    gt = api.kitti_from_xyt(np.concatenate([xy, th[:, None]], 1))
    est = api.kitti_from_xyt(np.concatenate([xy * 1.01 + [0.5, 0.25], th[:, None] + 0.01], 1))
    return est, gt


def extent(est, gt):
    return max(np.abs(K.normalise(a)[:, 3::4]).max() for a in (est, gt))


def check_alignment(s, est, gt, label=""):
    """The library's [r | t] against K.align_6dof.  Both sides take the singular pairs of a covariance C they summed in
    their own order.  The rotation is the orthogonal polar factor of C with the determinant fixed; a perturbation dC moves
    it by at most 2 |dC| / (s2 + s3) (s1 >= s2 >= s3 the singular values; s3 = 0 for planar data).  |dC| per side: the
    means and C are sums of depth <= ~22 (a strided serial part of n / 256 terms, an 8-level tree; NumPy: pairwise) over
    terms whose magnitudes add up to about 2 s1, i.e. <= 44 * 2^-53 s1, plus an SVD's backward error of ~10 * 2^-53 s1; two
    sides: |dC| <= 128 * 2^-53 s1 with room, so |dr| <= 256 * 2^-53 s1 / (s2 + s3).  t = my - r mx then differs by at most
    |dr| |mx| sqrt(3) + 32 * 2^-53 (|mx| + |my|).  r is also required to be a rotation: r r^T = I within 16 * 2^-53 times
    the same conditioning, and det r = +1 likewise."""
    E, G = K.normalise(est), K.normalise(gt)
    mx, my, cov = K.align_terms(E, G)
    sv = np.linalg.svd(cov, compute_uv=False)
    want = K.align_6dof(E, G).reshape(3, 4)
    got = np.asarray(s["align"]).reshape(3, 4)
    u = 2.0 ** -53
    b_r = 256 * u * sv[0] / (sv[1] + sv[2])
    b_t = b_r * np.linalg.norm(mx) * np.sqrt(3) + 32 * u * (np.linalg.norm(mx) + np.linalg.norm(my))
    d_r, d_t = np.abs(got[:, :3] - want[:, :3]).max(), np.abs(got[:, 3] - want[:, 3]).max()
    assert d_r <= b_r and d_t <= b_t, (label, d_r, b_r, d_t, b_t)
    r = got[:, :3]
    assert np.abs(r @ r.T - np.eye(3)).max() <= max(b_r, 16 * u) and abs(np.linalg.det(r) - 1.0) <= max(b_r, 16 * u), label
    ALIGN_WORST[:] = [max(ALIGN_WORST[0], d_r / b_r), max(ALIGN_WORST[1], d_t / b_t)]
    return d_r / b_r, d_t / b_t


def compare(s, rows, est, gt, step, alignment, label=""):
    """One trajectory's GPU summary record and rows against the restatement (given the library's alignment, see the head
    of the file).  Returns the deviations (rows, means, figures)."""
    if alignment == "6dof":
        check_alignment(s, est, gt, label)
    else:
        assert (s["align"] == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]).all()
    o = K.evaluate(est, gt, step, alignment, align=s["align"] if alignment == "6dof" else None)
    scale = max(1.0, extent(est, gt) / 1000.0)
    assert s["status"] == 0 and s["n_poses"] == len(est)
    assert s["n_rows"] == o["n_rows"] == len(rows), (label, s["n_rows"], o["n_rows"], len(rows))
    assert (rows["first_frame"] == o["first_frame"]).all() and (rows["last_frame"] == o["last_frame"]).all(), label
    assert (rows["length"] == o["length"]).all() and (s["seg_count"] == o["seg_count"]).all(), label
    assert (rows["speed"] == o["speed"]).all(), label
    d_rows = max([np.abs(rows["t_err"] - o["t_err"]).max(), np.abs(rows["r_err"] - o["r_err"]).max()] if len(rows) else [0.0])
    d_seg = max(np.abs(s["seg_t_err"] - o["seg_t_err"]).max(), np.abs(s["seg_r_err"] - o["seg_r_err"]).max(),
                abs(s["ave_t_err"] - o["ave_t_err"]), abs(s["ave_r_err"] - o["ave_r_err"]))
    d_fig = max(abs(s[f] - o[f]) for f in FIGS[2:])
    assert max(d_rows, d_seg) <= TOL * scale, (label, d_rows, d_seg, TOL * scale)
    assert d_fig <= 100 * TOL * scale, (label, d_fig, {f: (s[f], o[f]) for f in FIGS[2:]})
    if o["n_rows"] == 0:
        assert s["ave_t_err"] == 0 and s["ave_r_err"] == 0 and (s["seg_t_err"] == 0).all() and (s["seg_r_err"] == 0).all()
    return d_rows, d_seg, d_fig


def test_committed_jobs_against_the_reference_record():
    api = _api()
    data = [load_golden(name) for name in GOLDEN]
    summaries, rows = api.eval_trajectories([d[0] for d in data], [d[1] for d in data], step_size=10, alignment="6dof")
    worst = 0.0
    for k, (est, gt, rec, result) in enumerate(data):
        r = rows[rows["trajectory"] == k]
        assert len(r) == len(rec) == summaries[k]["n_rows"]
        assert (r["first_frame"] == rec[:, 0]).all() and (r["length"] == rec[:, 3]).all()
        assert (r["speed"] == rec[:, 4]).all()          # the record holds last_frame as speed = len / (0.1 (last - first + 1))
        assert (r["last_frame"] == np.rint(r["length"] / (0.1 * rec[:, 4])) - 1 + r["first_frame"]).all()
        dt, dr = np.abs(r["t_err"] - rec[:, 2]).max(), np.abs(r["r_err"] - rec[:, 1]).max()
        print(GOLDEN[k], "rows", len(r), "max |t_err/len - record| %.3e" % dt, "max |r_err/len - record| %.3e" % dr)
        worst = max(worst, dt, dr)
        got = "".join(api.eval_result_lines(0, summaries[k]))
        print(got)
        assert got == result
        assert summaries[k]["status"] == 0
    print("largest deviation from the record %.3e, bound %.3e" % (worst, TOL))
    assert worst <= TOL


@pytest.mark.parametrize("alignment", ["none", "6dof"])
@pytest.mark.parametrize("step", [1, 10])
def test_synthetic_inputs_against_the_restatement(alignment, step):
    api = _api()
    rng = np.random.default_rng(100 * step + len(alignment))
    pairs = {"planar": planar(rng, 1500), "planar, 6 decimals": planar(rng, 1200, decimals=6), "3-D": spatial(rng, 1400),
             "3-D short": spatial(rng, 300), "shorter than 100 m": planar(rng, 40), "two poses": planar(rng, 2),
             "one pose per thread": planar(rng, 256), "one pose more than threads": spatial(rng, 257),
             "exact steps, stationary stretches": exact_steps()}
    if alignment == "6dof":
        del pairs["two poses"]                          # two positions lie on a line: see test_degenerate_alignment_is_reported
    names = list(pairs)
    summaries, rows = api.eval_trajectories([pairs[k][0] for k in names], [pairs[k][1] for k in names], step_size=step,
                                            alignment=alignment)
    assert summaries["n_rows"].sum() == len(rows)
    for k, name in enumerate(names):
        d = compare(summaries[k], rows[rows["trajectory"] == k], pairs[name][0], pairs[name][1], step, alignment, name)
        print("%-36s %-5s step %2d rows %6d  deviation rows %.2e means %.2e figures %.2e" % ((name, alignment, step, summaries[k]["n_rows"]) + d))
    assert summaries[names.index("shorter than 100 m")]["n_rows"] == 0
    ex = rows[rows["trajectory"] == names.index("exact steps, stationary stretches")]
    # the tie: from frame 0, dist[100] == 100 exactly, so the 100 m segment ends at frame 101, not 100
    r0 = ex[(ex["first_frame"] == 0) & (ex["length"] == 100)]
    assert len(r0) == 1 and r0["last_frame"][0] == 101
    # ... and across the stationary stretch (frames 150 .. 180 share dist = 150): from frame 50 the 100 m segment ends at 181
    r50 = ex[(ex["first_frame"] == 50) & (ex["length"] == 100)]
    assert len(r50) == 1 and r50["last_frame"][0] == 181


def test_degenerate_alignment_is_reported():
    api = _api()
    from tbv_slam_public_amd import _lib as L
    est, gt = planar(np.random.default_rng(1), 2)
    s, _ = api.eval_trajectories([est], [gt], alignment="6dof")
    assert s[0]["status"] == L.ERR_SOLVER and s[0]["n_rows"] == 0
    s, _ = api.eval_trajectories([est], [gt], alignment="none")
    assert s[0]["status"] == L.OK


def test_device_resident_input_and_single_array_form():
    import torch
    api = _api()
    rng = np.random.default_rng(11)
    pairs = [planar(rng, 900), spatial(rng, 700), planar(rng, 333)]
    est, gt = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    lengths = [len(p[0]) for p in pairs]
    host = api.eval_trajectories(est, gt, lengths=lengths)
    dev = api.eval_trajectories(torch.from_numpy(est).cuda(), torch.from_numpy(gt).cuda(), lengths=lengths)
    torch.cuda.synchronize()
    assert host[0].tobytes() == dev[0].tobytes() and host[1].tobytes() == dev[1].tobytes()
    lists = api.eval_trajectories([p[0] for p in pairs], [p[1] for p in pairs])
    assert host[0].tobytes() == lists[0].tobytes() and host[1].tobytes() == lists[1].tobytes()
    no_rows = api.eval_trajectories(est, gt, lengths=lengths, want_rows=False)
    assert no_rows[1] is None and no_rows[0].tobytes() == host[0].tobytes()


def test_ragged_batch_of_thousands_is_bit_identical_to_single_evaluations():
    api = _api()
    rng = np.random.default_rng(2024)
    n_traj = 3000
    lengths = rng.integers(2, 700, n_traj)
    lengths[[5, 1234, 2999]] = [2500, 3, 1800]
    pairs = [spatial(rng, int(n)) if k % 3 == 0 else planar(rng, int(n), decimals=6 if k % 2 else None) for k, n in enumerate(lengths)]
    summaries, rows = api.eval_trajectories([p[0] for p in pairs], [p[1] for p in pairs], step_size=10, alignment="6dof")
    assert summaries["n_rows"].sum() == len(rows) and (np.diff(rows["trajectory"]) >= 0).all()
    base = np.concatenate([[0], np.cumsum(summaries["n_rows"])])
    worst = np.zeros(3)
    for k in range(n_traj):
        r = rows[base[k]:base[k + 1]]
        assert (r["trajectory"] == k).all()
        if summaries[k]["status"] != 0:                 # a short pair whose positions lie on one line within rounding
            assert lengths[k] <= 3
            continue
        worst = np.maximum(worst, compare(summaries[k], r, pairs[k][0], pairs[k][1], 10, "6dof", "pair %d" % k))
    print("ragged batch: %d pairs, %d poses, %d rows; deviation rows %.2e means %.2e figures %.2e"
          % ((n_traj, lengths.sum(), len(rows)) + tuple(worst)))
    print("alignment against the restatement's, largest fraction of the bound so far: rotation %.3f translation %.3f" % tuple(ALIGN_WORST))
    # the same pairs in reversed order: every record and every row is the same bits
    s_rev, r_rev = api.eval_trajectories([p[0] for p in pairs[::-1]], [p[1] for p in pairs[::-1]], step_size=10, alignment="6dof")
    assert s_rev[::-1].tobytes() == summaries.tobytes()
    r_rev = r_rev.copy()
    r_rev["trajectory"] = n_traj - 1 - r_rev["trajectory"]
    assert r_rev[np.argsort(r_rev["trajectory"], kind="stable")].tobytes() == rows.tobytes()
    # ... and alone
    for k in (0, 5, 6, 1234, 1500, 2998, 2999):
        s1, r1 = api.eval_trajectories([pairs[k][0]], [pairs[k][1]], step_size=10, alignment="6dof")
        a, b = summaries[k:k + 1].copy(), rows[base[k]:base[k + 1]].copy()
        b["trajectory"] = 0
        assert s1.tobytes() == a.tobytes(), k
        assert r1.tobytes() == b.tobytes(), k


def test_odometry_streams_through_the_conversion_helper():
    import torch
    from tbv_slam_public_amd import synth
    api = _api()
    n_frames, seeds = 5, (0, 1)
    scenes = [synth.scene_v1(s, n_frames) for s in seeds]
    od = api.OdometryKeyframeFuser(len(seeds), 400, 3360)
    poses = []
    for f in range(n_frames):
        info = od.process(torch.from_numpy(np.stack([sc[0][f] for sc in scenes])).cuda())
        poses.append(info["pose"].copy())
    est = api.kitti_from_xyt(np.stack(poses, 1))                      # [stream, frame, 12]
    gt = api.kitti_from_xyt(np.stack([sc[1] for sc in scenes]))
    summaries, rows = api.eval_trajectories(list(est), list(gt), alignment="6dof")
    assert len(rows) == 0
    for k in range(len(seeds)):
        compare(summaries[k], rows, est[k], gt[k], 10, "6dof", "stream %d" % k)
        print("stream %d: ATE %.4f m, RPE %.4f m / %.5f rad" % (k, summaries[k]["ate"], summaries[k]["rpe_trans"], summaries[k]["rpe_rot"]))
        assert 0 < summaries[k]["ate"] < 0.5 and summaries[k]["bias_theta"] == 0.0


def test_eval_directory_matches_the_devkit_format(tmp_path):
    api = _api()
    est, gt, rec, result = load_golden(GOLDEN[0])
    gt_dir, res_dir = tmp_path / "gt", tmp_path / "est"
    gt_dir.mkdir()
    res_dir.mkdir()
    api.kitti_write(str(gt_dir / "00.txt"), gt)
    api.kitti_write(str(res_dir / "00.txt"), est)
    api.KittiEvalOdom(step_size=10).eval(str(gt_dir), str(res_dir), alignment="6dof")
    assert open(res_dir / "result.txt").read() == result
    lines = open(res_dir / "errors" / "00.txt").read().splitlines()
    assert len(lines) == len(rec)
    got = np.array([[float(t) for t in ln.split(" ")] for ln in lines])
    assert (got[:, [0, 3, 4]] == rec[:, [0, 3, 4]]).all() and np.abs(got[:, 1:3] - rec[:, 1:3]).max() <= TOL
    assert lines[0].split(" ")[0] == "0" and lines[0].split(" ")[3] == "100" and lines[0].split(" ")[4] == "18.51851851851852"


def test_tensor_inputs_are_checked():
    import torch
    from tbv_slam_public_amd import _lib as L
    api = _api()
    est, gt = planar(np.random.default_rng(3), 50)
    de, dg = torch.from_numpy(est).cuda(), torch.from_numpy(gt).cuda()
    for bad_e, bad_g in ((de.float(), dg.float()), (de, gt), (de, dg.float()), (de.reshape(-1), dg.reshape(-1)),
                         (de[:, :6], dg[:, :6]), (torch.from_numpy(est), torch.from_numpy(gt)), (de.t().contiguous().t(), dg)):
        with pytest.raises(L.CfearError) as ei:
            api.eval_trajectories(bad_e, bad_g)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    # lengths in device memory are refused by the library, not read
    import ctypes as C
    ctx = api.default_context()
    dl = torch.tensor([50], dtype=torch.int32).cuda()
    out = np.zeros(1, L.EVAL_SUMMARY_DTYPE)
    p = api.eval_params()
    rc = ctx._lib.cfear_eval_trajectories(ctx.h, de.data_ptr(), dg.data_ptr(), None, dl.data_ptr(), 1, C.byref(p), out.ctypes.data,
                                          None, 0, None)
    assert rc == L.ERR_INVALID_ARGUMENT
    s, _ = api.eval_trajectories(de, dg)
    assert s[0]["status"] == 0


def test_cpp_wrapper_runs(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "eval_signature")
    so_dir = os.path.join(root, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           "-I", os.path.join(root, "tests", "cpp", "standin"), os.path.join(root, "tests", "cpp", "eval_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.split()
    # three planar poses off one line, an estimate 1 % long: one pair, no rows, ATE > 0, status OK, a rotation as alignment
    assert out[:3] == ["1", "0", "0"], out
    assert 0.0 < float(out[3]) < 0.1 and abs(float(out[4]) - 1.0) < 1e-12, out
