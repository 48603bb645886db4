"""CPU: what trajectory synchronisation (cfear_sync_trajectories, cfear_tum_write, cfear_cov_write; csrc/trajsync.hip) needs no
device for -- the serial restatement the GPU results are compared with (tests/trajsync_cpu.py) pinned by properties, the
inputs the GPU tests use, the writers against hand-written lines, the ABI, the refusals (made on host buffers before a
context is needed, their culprit named at cfear_last_error(NULL)) and the signature program."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import trajsync_cpu as M
from tbv_slam_public_amd import _lib as L
from tbv_slam_public_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in M.cases()}


def _rot(p):
    return [list(p[0:3]), list(p[4:7]), list(p[8:11])]


def test_sorted_stamps_chained_equals_a_global_first_interval_search():
    for seed in range(6):
        g = M.gt_grid(50, jitter=15_000_000, seed=seed)
        e = M.est_between(120, g, seed, -0.1, 1.1)
        e[5] = g[7]                                                # stamps that lie in two intervals
        e[6] = g[8]
        e = np.sort(e)
        r = M.sync_pair(None, e, M.planar_path(50, seed), g)
        want = M.global_first_interval(e, g)
        # ascending estimates never find the walk ahead of their first interval, the stamps that lie in two intervals included
        kept = [i for i, j in enumerate(want) if j >= 0]
        assert r["rows"]["est_index"].tolist() == kept and r["rows"]["gt_index"].tolist() == [want[i] for i in kept] and len(kept) > 90
        ind = M.sync_pair(None, e, M.planar_path(50, seed), g, "independent")
        assert ind["rows"].tobytes() == r["rows"].tobytes()


def test_alpha_0_and_1_return_the_end_poses():
    P = M.spatial(12, 3)
    for a, b in zip(P[:-1], P[1:]):
        for t, end in ((10.0, a), (12.0, b)):
            out, alpha = M.pose_interp(t, 10.0, 12.0, a, b)
            assert alpha == (t - 10.0) / 2.0
            assert out[3] == end[3] and out[7] == end[7] and out[11] == 0.0          # translations exact, z set to 0
            assert np.abs(np.array(_rot(out)) - np.array(_rot(end))).max() <= 1e-15
    out, alpha = M.pose_interp(5.0, 5.0, 5.0, P[0], P[1])                              # t2 == t1
    assert alpha == 0.0 and out[3] == P[0][3]


def test_planar_poses_interpolate_the_yaw():
    rng = np.random.default_rng(1)
    wrap = lambda a: math.atan2(math.sin(a), math.cos(a))
    for _ in range(300):
        t1, t2 = rng.uniform(-math.pi, math.pi, 2)
        if abs(abs(wrap(t2 - t1)) - math.pi) < 1e-3:
            continue                                               # the half turn has no shorter side
        alpha = rng.uniform(0.0, 1.0)
        out, a = M.pose_interp(alpha, 0.0, 1.0, M.planar(1.0, 2.0, t1), M.planar(3.0, -1.0, t2))
        want = M.planar(0, 0, t1 + alpha * wrap(t2 - t1))
        assert a == alpha and np.abs(np.array(_rot(out)) - np.array(_rot(want))).max() <= 1e-12
        assert out[3] == (1.0 - alpha) * 1.0 + alpha * 3.0 and out[7] == (1.0 - alpha) * 2.0 + alpha * -1.0


def test_slerp_threshold_and_branches():
    q = M.quat_from_matrix(M.rot_xyz(0.3, -0.2, 1.0))
    assert M.slerp(0.25, q, q)[1] and not M.slerp(0.25, q, M.quat_from_matrix(M.rot_xyz(0.3, -0.2, 1.1)))[1]
    mixed, _ = M.slerp(0.25, q, q)
    assert np.allclose(mixed, q, rtol=0, atol=1e-16)
    # a negative dot negates the second weight: q and -q are one rotation, the result stays next to q
    neg = [-v for v in M.quat_from_matrix(M.rot_xyz(0.3, -0.2, 1.1))]
    a, _ = M.slerp(0.5, q, neg)
    b, _ = M.slerp(0.5, q, [-v for v in neg])
    assert M.quat_dot(q, neg) < 0 and np.allclose(a, b, rtol=0, atol=1e-15)
    # the conversion's four branches, each the inverse of toRotationMatrix
    seen = set()
    for ang in ((0.1, 0.2, 0.3), (3.0, 0.1, 0.1), (0.1, 3.0, 0.1), (0.1, 0.1, 3.0)):
        R = M.rot_xyz(*ang)
        seen.add(M.quat_branch(R))
        assert np.abs(np.array(M.quat_to_matrix(M.quat_from_matrix(R))) - R).max() <= 1e-14
    assert seen == {"trace", 0, 1, 2}


def test_cases_cover_what_they_claim():
    run = lambda c, mode="chained": M.sync_pair(c["est"], c["est_stamps"], c["gt"], c["gt_stamps"], mode)
    for n_gt in (0, 1, 2):
        assert run(CASES["gt_len_%d" % n_gt])["count"] == 0 and len(CASES["gt_len_%d" % n_gt]["est_stamps"]) == 9
    assert run(CASES["gt_len_3"])["count"] == 9 and run(CASES["gt_len_4"])["count"] == 9
    for n in (0, 1, 63, 64, 65, 129):
        assert run(CASES["est_len_%d" % n])["count"] == n
    c = CASES["est_before_and_after"]
    r = run(c)
    assert r["rows"]["est_index"][0] > 0 and r["rows"]["est_index"][-1] < len(c["est_stamps"]) - 1 and r["count"] > 0
    assert run(CASES["est_all_outside"])["count"] == 0
    for name, at in (("backward_mid_chunk", 37), ("backward_at_chunk_boundary", 64)):
        c = CASES[name]
        r = run(c)
        kept = r["rows"]["est_index"].tolist()
        assert at - 1 in kept and at not in kept and at + 1 in kept            # the miss, the reset, the next hit from 0
        assert r["rows"]["gt_index"][kept.index(at + 1)] < r["rows"]["gt_index"][kept.index(at - 1)]
        assert run(c, "independent")["count"] == len(c["est_stamps"])
    # a stamp in two intervals behind a walk that stands on the later one: chained max(position, a), independent a
    a, b = run(CASES["est_equals_gt_stamp"]), run(CASES["est_equals_gt_stamp"], "independent")
    assert M.both_kept_differ(a, b) == [(1, 5, 0.0, 4, 1.0), (2, 5, 0.0, 4, 1.0), (7, 12, 0.0, 11, 1.0)]
    assert a["count"] < b["count"] == 11                                                   # and the steps back to g0 and g20 are dropped
    a, b = run(CASES["duplicate_gt_stamps"]), run(CASES["duplicate_gt_stamps"], "independent")
    assert M.both_kept_differ(a, b) == [(8, 9, 0.0, 6, 1.0)]                                  # the step back into the run of three
    assert tuple(b["rows"][0]) == (0, 0, 0.0) and tuple(b["rows"][5]) == (5, 6, 1.0)           # t2 == t1; the run of three
    e, g, int_keep = M.rounding_case()
    assert len(set(e.tolist()) | set(g.tolist())) == 8
    assert M.to_sec(e[0]) == M.to_sec(g[0]) and M.to_sec(e[2]) == M.to_sec(g[3]) and M.to_sec(e[3]) > M.to_sec(g[3])
    assert run(CASES["tosec_rounding"])["rows"]["est_index"].tolist() == [0, 1, 2] != int_keep == [1]
    gt = CASES["rotations_all_branches"]["gt"]
    assert {M.quat_branch(_rot(p)) for p in gt} == {"trace", 0, 1, 2}
    assert {M.quat_branch(_rot(p)) for p in CASES["rotations_planar"]["gt"]} == {"trace"}
    used = run(CASES["rotations_all_branches"])["rows"]["gt_index"]
    quats = [M.quat_from_matrix(_rot(p)) for p in gt]
    dots = [M.quat_dot(quats[j], quats[j + 1]) for j in sorted(set(used.tolist()))]
    assert min(dots) < 0 < max(dots) and any(abs(d) >= 1.0 - M.DBL_EPSILON for d in dots) and 10 in used
    assert {M.quat_branch(_rot(gt[j])) for j in set(used.tolist())} == {"trace", 0, 1, 2}
    R = np.array(_rot(CASES["non_orthonormal_6_decimals"]["gt"][3]))
    assert 1e-8 < np.abs(R @ R.T - np.eye(3)).max() < 1e-5
    pairs, eo, go = M.batch_300()
    le = np.array([len(p["est_stamps"]) for p in pairs])
    assert len(pairs) == 300 and (le[140:150:1][1::2] == 0).all() and (np.diff(eo) > le).any() and eo[0] > 0
    assert all(len(p["gt_stamps"]) == 0 for p in pairs[140:150:2])
    staying = [t for t, p in enumerate(pairs) if M.both_kept_differ(run(p), run(p, "independent"))]
    assert len(staying) >= 10 and all(t % 5 == 1 for t in staying)


def test_writers_hand_written(tmp_path):
    assert M.stamp_text(5 * 10 ** 9 + 7) == "5.000000007 "
    s = math.sqrt(0.5)
    quarter = [0.0, -1.0, 0.0, 1.23456, 1.0, 0.0, 0.0, -2.00004, 0.0, 0.0, 1.0, 0.0]      # 90 degrees about z: q = (0, 0, s, s)
    q = M.quat_from_matrix(_rot(quarter))
    assert q[:2] == [0.0, 0.0] and abs(q[2] - 0.70710678) < 1e-8 and abs(q[3] - s) < 1e-15
    assert M.tum_line(quarter, 5 * 10 ** 9 + 7) == "5.000000007 1.2346 -2.0000 0.0000 0 0 0.7071 0.7071\n"
    cov = np.zeros(36)
    cov[0], cov[1], cov[35] = 1e-4, 1.23456789, -2.5e-7
    assert M.cov_line(cov, 1547000000 * 10 ** 9 + 120) == "1547000000.000000120 0.0001 1.23457 " + "0 " * 33 + "-2.5e-07\n"
    # the library's writers produce the formatters' bytes
    poses = np.concatenate([M.spatial(20, 1, big=True), M.planar_path(5, 2), np.array([quarter])])
    stamps = M.T0 + np.arange(len(poses), dtype=np.int64) * 250_000_007
    covs = np.random.default_rng(0).normal(size=(len(poses), 36)) * np.logspace(-8, 3, 36)
    api.tum_write(str(tmp_path / "tum"), poses, stamps)
    api.cov_write(str(tmp_path / "cov"), covs, stamps)
    assert open(tmp_path / "tum").read() == M.tum_text(poses, stamps) and open(tmp_path / "cov").read() == M.cov_text(covs, stamps)
    lib = L.lib()
    bad = np.array([-1], np.int64)
    assert lib.cfear_tum_write(os.fsencode(str(tmp_path / "x")), poses.ctypes.data, bad.ctypes.data, 1) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_cov_write(os.fsencode(str(tmp_path / "x")), None, bad.ctypes.data, 1) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_tum_write(os.fsencode(str(tmp_path / "no" / "dir")), poses.ctypes.data, stamps.ctypes.data, 1) == L.ERR_IO
    with pytest.raises(L.CfearError):
        api.tum_write(str(tmp_path / "y"), poses, stamps[:3])


def test_abi_names_the_call_and_its_struct():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_[a-z0-9_]+)\s*\(", hdr))
    names = {"cfear_sync_trajectories", "cfear_tum_write", "cfear_cov_write"}
    assert names <= declared & set(L.EXPORTS) and all(hasattr(lib, n) for n in names) and lib.cfear_abi_version() == 1
    assert int(re.search(r"#define CFEAR_SYNC_CHAINED (\d+)", hdr).group(1)) == L.SYNC_MODE["chained"] == 0
    assert int(re.search(r"#define CFEAR_SYNC_INDEPENDENT (\d+)", hdr).group(1)) == L.SYNC_MODE["independent"] == 1
    dt = L.SYNC_ROW_DTYPE
    assert dt.itemsize == 16 and [(k, dt.fields[k][1]) for k in dt.names] == [("est_index", 0), ("gt_index", 4), ("alpha", 8)]
    assert dt == M.ROW_DTYPE


class _Call:
    """One pair batch on host buffers, every argument replaceable; the outputs are pre-filled so that a write shows."""

    def __init__(self):
        g1, g2 = M.gt_grid(6), M.gt_grid(5, start=M.T0 + 10 ** 9)
        self.est_stamps = np.concatenate([M.est_between(4, g1, 1, 0.1, 0.9), M.est_between(3, g2, 2, 0.1, 0.9)])
        self.gt_stamps = np.concatenate([g1, g2])
        self.est, self.gt = M.spatial(7, 1), M.planar_path(11, 2)
        self.le, self.lg = np.array([4, 3], np.int32), np.array([6, 5], np.int32)
        self.eo, self.go = np.array([0, 4], np.int64), np.array([0, 6], np.int64)
        self.n_traj, self.mode = 2, 0

    def run(self, **kw):
        a = dict(self.__dict__)
        a.update(kw)
        outs = [np.full((7, 12), 7.0), np.full((7, 12), 7.0), np.full(7, 7, np.int64), np.full(7, 7, L.SYNC_ROW_DTYPE), np.full(2, 7, np.int32)]
        before = [o.tobytes() for o in outs]
        ptr = lambda x: None if x is None else x.ctypes.data
        skip = a.get("null_out", -1)
        rc = L.lib().cfear_sync_trajectories(None, a["mode"], ptr(a["est"]), ptr(a["est_stamps"]), ptr(a["eo"]), ptr(a["le"]), ptr(a["gt"]),
                                             ptr(a["gt_stamps"]), ptr(a["go"]), ptr(a["lg"]), a["n_traj"],
                                             *[None if k == skip else ptr(o) for k, o in enumerate(outs)])
        assert [o.tobytes() for o in outs] == before                   # nothing is written
        return rc, L.lib().cfear_last_error(None).decode()


def _edited(x, i, v):
    y = x.copy()
    y[i] = v
    return y


def test_refusals_need_no_device_and_name_the_culprit():
    c = _Call()
    inv = L.ERR_INVALID_ARGUMENT
    assert c.run() == (inv, "null context")                           # valid: only the context is missing
    assert c.run(eo=None, go=None) == (inv, "null context") and c.run(est=None, null_out=0) == (inv, "null context")
    assert c.run(n_traj=0, le=None, lg=None, null_out=4) == (inv, "null context")
    assert c.run(le=np.array([0, 0], np.int32), est_stamps=None, est=None) == (inv, "null context")          # no estimates at all
    assert c.run(mode=2) == (inv, "unknown mode 2") and c.run(mode=-1)[1] == "unknown mode -1"
    assert c.run(n_traj=-1) == (inv, "n_traj is negative")
    for kw in (dict(le=None), dict(lg=None), dict(null_out=4), dict(est_stamps=None), dict(gt=None), dict(gt_stamps=None), dict(null_out=0),
               dict(null_out=1), dict(null_out=2), dict(null_out=3)):
        assert c.run(**kw) == (inv, "null argument"), kw
    assert c.run(le=np.array([4, -3], np.int32)) == (inv, "pair 1: negative length")
    assert c.run(lg=np.array([-1, 5], np.int32)) == (inv, "pair 0: negative length")
    assert c.run(eo=np.array([0, -4], np.int64)) == (inv, "pair 1: negative offset")
    late = (2 ** 32) * 10 ** 9
    assert c.run(est_stamps=_edited(c.est_stamps, 5, -1)) == (inv, "pair 1: estimate stamp 1 is negative or past 2^32 - 1 seconds")
    assert c.run(est_stamps=_edited(c.est_stamps, 2, late)) == (inv, "pair 0: estimate stamp 2 is negative or past 2^32 - 1 seconds")
    assert c.run(est_stamps=_edited(c.est_stamps, 2, late - 1)) == (inv, "null context")                      # the last legal stamp
    assert c.run(gt_stamps=_edited(c.gt_stamps, 10, late)) == (inv, "pair 1: ground-truth stamp 4 is negative or past 2^32 - 1 seconds")
    assert c.run(gt_stamps=_edited(c.gt_stamps, 0, -5)) == (inv, "pair 0: ground-truth stamp 0 is negative or past 2^32 - 1 seconds")
    assert c.run(gt_stamps=_edited(c.gt_stamps, 8, c.gt_stamps[7] - 1)) == (inv, "pair 1: ground-truth stamp 2 is earlier than the one before it")
    assert c.run(gt_stamps=_edited(c.gt_stamps, 3, c.gt_stamps[2])) == (inv, "null context")                  # equal stamps are legal
    # the estimate's stamps may be in any order, and a pair's ground truth may start before the previous pair's ends
    assert c.run(est_stamps=c.est_stamps[::-1].copy()) == (inv, "null context")
    assert c.run(go=np.array([6, 0], np.int64), lg=np.array([5, 6], np.int32)) == (inv, "null context")
    with pytest.raises(L.CfearError):
        api.sync_trajectories([c.est], [c.est_stamps], [c.gt], [c.gt_stamps], mode="nearest")
    with pytest.raises(L.CfearError):
        api.sync_trajectories([c.est], [c.est_stamps[:3]], [c.gt], [c.gt_stamps])
    # eval_trajectories: offsets address one flat array, never a list of trajectories; and they must lie inside it
    with pytest.raises(L.CfearError, match="offsets address one flat array"):
        api.eval_trajectories([c.est], [c.est], offsets=np.array([0], np.int64))
    with pytest.raises(L.CfearError, match="lie inside it"):
        api.eval_trajectories(c.est, c.est, lengths=np.array([4, 3], np.int32), offsets=np.array([0, 5], np.int64))


def test_eval_trajectory_instance_keeps_the_static_methods(tmp_path):
    ev = api.EvalTrajectory()
    assert ev.GetSize() == 0 and api.EvalTrajectory.MatToString((1.0, 2.0, 0.0)).startswith("1.000000 -0.000000 0.000000 1.000000")
    api.EvalTrajectory.Write(str(tmp_path / "t.txt"), np.array([[1.0, 2.0, 0.5]]))
    assert np.allclose(api.EvalTrajectory.Read(str(tmp_path / "t.txt")), [[1.0, 2.0, 0.5]], atol=1e-6)
    P, cov = M.planar_path(3, 1), np.arange(36.0)
    for i in range(3):
        ev.CallbackESTEigen((P[i], cov * i, M.T0 + i))
    ev.CallbackEigen((np.vstack([P[0].reshape(3, 4), [0, 0, 0, 1]]), None, M.T0 + 9), (P[1].reshape(3, 4), None, M.T0 + 9))
    assert ev.GetSize() == 1 and len(ev.est_vek) == 4 and (ev.est_vek[3][0] == P[0]).all()
    assert ev.GetGtVek() == [(M.T0 + 9, (P[1][3], P[1][7], math.atan2(P[1][4], P[1][0])))]
    # without a ground truth Save writes the three estimate-only files and needs no device
    only = api.EvalTrajectory()
    for i in range(3):
        only.CallbackESTEigen((P[i], cov * i, M.T0 + i * 10 ** 8))
    paths = only.Save(str(tmp_path / "est"), str(tmp_path / "gt"), "01.txt")
    assert [os.path.relpath(p, tmp_path) for p in paths] == ["est/01.txt", "est/tum_01.txt", "est/cov_01.txt"] and not os.path.exists(tmp_path / "gt")
    stamps = M.T0 + np.arange(3) * 10 ** 8
    assert open(paths[1]).read() == M.tum_text(P, stamps) and open(paths[2]).read() == M.cov_text([cov * i for i in range(3)], stamps)
    assert np.allclose(api.kitti_read(paths[0]), P, atol=1e-6)
    with pytest.raises(L.CfearError):
        api.EvalTrajectory().Save(str(tmp_path / "e"), str(tmp_path / "g"), "02.txt")
    with pytest.raises(L.CfearError):
        ev.CallbackGTEigen((np.zeros(5), None, 0))


def test_cpp_signature_compiles_and_writes(tmp_path):
    exe = str(tmp_path / "trajsync_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "trajsync_signature.cpp"), "-o", exe, "-L", so_dir, "-lcfear_hip",
                           "-Wl,-rpath," + so_dir])
    out = subprocess.check_output([exe, "refuse", str(tmp_path)]).decode().splitlines()
    assert out[0] == "%d pair 0: ground-truth stamp 2 is earlier than the one before it" % L.ERR_INVALID_ARGUMENT
    assert out[1] == "3 2 2"                                          # estimates, ground-truth poses, GetSize
    # the collector's estimate-only Save through the C ABI: the formatters' bytes
    P = np.array([M.planar(0.5 * i, 0.25 * i, 0.1 * i) for i in range(3)])
    stamps = [1547000000 * 10 ** 9 + i * 250000000 for i in range(3)]
    covs = [np.arange(36.0) * (i + 1) * 1e-3 for i in range(3)]
    assert open(tmp_path / "est" / "tum_05.txt").read() == M.tum_text(P, stamps)
    assert open(tmp_path / "est" / "cov_05.txt").read() == M.cov_text(covs, stamps)
    assert np.allclose(api.kitti_read(str(tmp_path / "est" / "05.txt")), P, atol=1e-6) and not os.path.exists(tmp_path / "gt")
