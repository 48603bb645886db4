"""GPU: the frame policy of cfear_odometry (csrc/odometry.hip::process_frame = OdometryKeyframeFuser::processFrame,
odometrykeyframefuser.cpp:143-259, + AddToGraph :428-445) on every branch and parameter, through process_clouds.

Every case of tests/fuser_cases.py runs against one CPU oracle fuser per stream, frame by frame: n_cells, keyframe_added,
the ok flag and outer_iters equal; the pose within the project's budget (BASELINE.json: 1e-4 m, 1e-5 rad) per frame;
cov_current as tests/test_gpu_covariance.py compares it; the odometry constraint after every frame.  An empty cloud is a
per-stream CFEAR_ERR_EMPTY_CLOUD that leaves the stream's state alone; the oracle is simply not fed that frame.
tests/test_fuser_cases_cpu.py shows that the cases reach the branches and that no decision sits near its threshold.

information is held to a NumPy restatement of AddToGraph :437-440 fed with the library's own covariance() and pose, so only
the 3 x 3 rotation and the inverse differ: full inverse where C has one, the planar (x, y, yaw) inverse where it is Register's
singular diagonal.  Deviation = the largest |I - I_numpy|[i, j] / sqrt(I_numpy[i, i] * I_numpy[j, j]).  Measured on an MI355X over all cases
(EXPERIMENTS.md, "Frame policy"): 2.461e-14 at worst (a full inverse of a sampled covariance; 8.5e-16 over the planar ones);
INFO_RTOL is ten times that, and must stay under 1e-6.
"""
import numpy as np
import pytest

from tests import fuser_cases as FC
from tests.test_fuser_cases_cpu import oracle_trace

pytestmark = pytest.mark.gpu

POS_TOL, ROT_TOL = 1e-4, 1e-5
INFO_RTOL = 2.5e-13
assert INFO_RTOL <= 1e-6
PLANAR = np.ix_([0, 1, 5], [0, 1, 5])


def _params(case):
    from tbv_slam_public_amd import api
    return api.odometry_params(**case["par"])


def _expected_information(cov, pose):
    """AddToGraph :437-440 in NumPy: C = Cov with its 3 x 3 block rotated by Tfrom^-1, information = C^-1 -- on the planar
    sub-space alone where C is singular (include/cfear_hip.h)."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])          # Tfrom.inverse().rotation()
    C = cov.copy()
    C[:3, :3] = R @ cov[:3, :3] @ R.T
    if np.linalg.det(C) != 0.0:
        return np.linalg.inv(C), False
    out = np.zeros((6, 6))
    out[PLANAR] = np.linalg.inv(C[PLANAR])
    return out, True


def _information_deviation(got, want):
    """Largest |got - want|[i, j] / sqrt(want[i, i] * want[j, j]): every entry on the scale of its own row and column (the
    yaw entries are 1e3 times the x, y ones).  Rows and columns that `want` leaves empty must be exactly zero."""
    d = np.sqrt(np.abs(np.diag(want)))
    on = d > 0
    assert not got[~on].any() and not got[:, ~on].any()
    return float((np.abs(got - want)[np.ix_(on, on)] / np.outer(d[on], d[on])).max())


def _rel_pose(a, b):
    """Ta^-1 * Tb as (x, y, theta)."""
    c, s = np.cos(a[2]), np.sin(a[2])
    d = b[:2] - a[:2]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], b[2] - a[2]])


def run_case(name, only=None):
    """Runs the case (or its stream `only` alone) on the device against the oracle -> (info per frame, figures)."""
    from tbv_slam_public_amd import api
    from tbv_slam_public_amd import _lib as L
    case = FC.BY_NAME[name]
    idx = list(range(len(case["streams"]))) if only is None else [only]
    B, F, world = len(idx), case["streams"][0].shape[0], FC.WORLDS[case["world"]]
    od = api.OdometryKeyframeFuser(B, 32, 64, _params(case))
    infos = []
    last_pose = np.zeros((B, 3))
    last_cov = np.tile(np.eye(6), (B, 1, 1))
    keyframes = [[] for _ in idx]                          # reported pose of every keyframe, in order
    worst = dict(xy=0.0, th=0.0, info=0.0, n_constraints=0, n_full=0, n_planar=0)
    for f in range(F):
        clouds = [FC.cloud(world, case["streams"][i][f], f) for i in idx]
        info = od.process_clouds(clouds)
        infos.append(info)
        cov, flag = od.covariance()
        for b, i in enumerate(idx):
            exp, at = oracle_trace(name, i)[f], (name, i, f)
            if exp is None:                                # empty cloud: this stream's own error, its state untouched
                assert info["reg_status"][b] == L.ERR_EMPTY_CLOUD, at
                assert info["n_points"][b] == 0 and info["n_cells"][b] == 0 and info["keyframe_added"][b] == 0, at
                np.testing.assert_array_equal(info["pose"][b], last_pose[b], err_msg=str(at))
                np.testing.assert_array_equal(cov[b], last_cov[b], err_msg=str(at))
                assert od.constraint(b) is None, at
                continue
            assert info["n_points"][b] == clouds[b].shape[0], at
            assert info["n_cells"][b] == exp["n_cells"], at
            assert info["keyframe_added"][b] == exp["keyframe"], at
            if not exp["first"]:
                assert (info["reg_status"][b] == 0) == bool(exp["ok"]), at
                assert info["outer_iters"][b] == exp["iters"], at
            d = np.abs(info["pose"][b] - exp["pose"])
            worst["xy"], worst["th"] = max(worst["xy"], d[:2].max()), max(worst["th"], d[2])
            assert d[:2].max() <= POS_TOL and d[2] <= ROT_TOL, (at, d)
            assert bool(flag[b]) == exp["sampled"], at
            if exp["sampled"]:
                np.testing.assert_allclose(cov[b][PLANAR], exp["cov"][PLANAR], rtol=1e-4, atol=1e-14, err_msg=str(at))
                rest = cov[b].copy()
                rest[PLANAR] = 0
                np.testing.assert_array_equal(rest, np.diag([0, 0, 1.0, 1.0, 1.0, 0]), err_msg=str(at))
            else:
                np.testing.assert_array_equal(cov[b], exp["cov"], err_msg=str(at))
            last_pose[b], last_cov[b] = info["pose"][b], cov[b]
            # ---- AddToGraph: a constraint after every keyframe but the first, and after nothing else
            c = od.constraint(b)
            if not info["keyframe_added"][b]:
                assert c is None, at
                continue
            keyframes[b].append(info["pose"][b].copy())
            if len(keyframes[b]) == 1:
                assert c is None, at
                continue
            assert (c["id_begin"], c["id_end"], c["type"]) == (len(keyframes[b]) - 1, len(keyframes[b]) - 2, 0), at
            rel = _rel_pose(keyframes[b][-1], keyframes[b][-2])                   # Tfrom^-1 * Tto of the two reported poses
            got = np.array([c["t_be"][0], c["t_be"][1], 2 * np.arctan2(c["t_be"][5], c["t_be"][6])])
            np.testing.assert_allclose(got, rel, rtol=0, atol=1e-12, err_msg=str(at))
            assert c["t_be"][2] == 0 and c["t_be"][3] == 0 and c["t_be"][4] == 0, at
            want, planar = _expected_information(cov[b], info["pose"][b])
            dev = _information_deviation(c["information"], want)
            worst["info"] = max(worst["info"], dev)
            worst["n_constraints"] += 1
            worst["n_planar" if planar else "n_full"] += 1
            assert dev <= INFO_RTOL, (at, dev)
    od.close()
    print("%s%s: worst pose deviation %.3e m %.3e rad; information %.3e over %d constraints (%d full, %d planar inverses)"
          % (name, "" if only is None else "[%d alone]" % only, worst["xy"], worst["th"], worst["info"], worst["n_constraints"],
             worst["n_full"], worst["n_planar"]))
    return infos, worst


def test_case_defaults_are_the_library_defaults():
    from tbv_slam_public_amd import api
    p = api.odometry_params()
    for k, v in FC.DEFAULTS.items():
        for prefix, sub in (("reg_", p.reg), ("cov_sampling_", p.cov_sampling)):
            if k.startswith(prefix):
                assert getattr(sub, k[len(prefix):]) == v, k
                break
        else:
            assert getattr(p, k) == v, k
    # kRegMaxScans: a window of REG_MAX_SCANS - 1 keyframes is the longest that create accepts
    api.OdometryKeyframeFuser(1, 32, 64, api.odometry_params(submap_scan_size=FC.REG_MAX_SCANS - 1)).close()
    with pytest.raises(Exception):
        api.OdometryKeyframeFuser(1, 32, 64, api.odometry_params(submap_scan_size=FC.REG_MAX_SCANS))


@pytest.mark.parametrize("name", [c["name"] for c in FC.CASES])
def test_case_matches_oracle(name):
    _, w = run_case(name)
    if name == "sampled_constraints":                      # both kinds of information, the full inverse past 1 rad of heading
        assert w["n_full"] >= 4 and w["n_planar"] >= 1
    if name == "failed_registration_keyframe":             # Identity has an inverse: one full one among the planar ones
        assert w["n_full"] == 1 and w["n_planar"] >= 4


def test_failed_frame_leaves_no_constraint_behind():
    """cfear_odometry_get_constraint speaks of the LAST processed frame: after a keyframe with a constraint, an empty cloud
    is a processed frame that added nothing."""
    from tbv_slam_public_amd import api
    from tbv_slam_public_amd import _lib as L
    w = FC.WORLDS["unit"]
    od = api.OdometryKeyframeFuser(2, 32, 64, api.odometry_params(use_keyframe=0))
    for f in range(2):
        info = od.process_clouds([FC.cloud(w, FC.STRAIGHT[f], f)] * 2)
    assert info["keyframe_added"].all() and od.constraint(0) is not None and od.constraint(1) is not None
    info = od.process_clouds([np.zeros((0, 4), np.float32), FC.cloud(w, FC.STRAIGHT[2], 2)])
    assert info["reg_status"][0] == L.ERR_EMPTY_CLOUD and info["keyframe_added"][1] == 1
    assert od.constraint(0) is None
    c = od.constraint(1)
    assert c is not None and (c["id_begin"], c["id_end"]) == (2, 1)


def test_diverging_streams_equal_the_same_streams_run_alone():
    """Nine streams (the registration batch is ordered in five classes from eight on) on different drives: on a frame some
    register and fuse, some register and do not, one fails to register, one has no job because its first cloud was empty.
    Every stream's frame info equals the same stream run alone, bit for bit in every field."""
    name = "diverging_streams"
    batch, _ = run_case(name)
    for i in range(len(FC.BY_NAME[name]["streams"])):
        alone, _ = run_case(name, only=i)
        for f, (a, b) in enumerate(zip(batch, alone)):
            for field in a.dtype.names:
                np.testing.assert_array_equal(a[field][i], b[field][0], err_msg="%s stream %d frame %d" % (field, i, f))
