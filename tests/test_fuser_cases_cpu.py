"""CPU: the frame-policy cases of tests/fuser_cases.py, kept honest with the oracle alone.  Every case must show the
events it declares in the oracle's own run, and no decision of any frame may sit so near its threshold that a device
within the pose budget (1e-4 m, 1e-5 rad) could legally decide the other way:
  |acc - 200| >= 1 and |vel - 200| >= 1  (a pose deviation of 1e-4 m moves acc by 1e-4 / 0.25^2 = 1.6e-3),
  ||t| - min_keyframe_dist| >= 1e-3 m and ||rot| - min_keyframe_rot| >= 1e-4 rad  (ten times the pose budget).
tests/test_gpu_fuser_policy.py runs the same cases on the device against oracle_trace()."""
import functools

import numpy as np
import pytest

from tests import fuser_cases as FC


def make_oracle(par):
    """One O.Fuser with the defaults of cfear_odometry_params_default and the case's overrides."""
    from oracle import pyoracle as O
    p = dict(FC.DEFAULTS)
    p.update(par)
    reg = O.reg_params(cost=p["reg_cost"], loss=p["reg_loss"], loss_limit=p["reg_loss_limit"], weight_opt=p["reg_weight_opt"],
                       max_outer=p["reg_max_itr_association"], max_inner=p["reg_max_itr_solver"], min_outer=p["reg_min_itr"],
                       radius=p["reg_radius"], cov_scale=p["reg_cov_scale"], regularization=p["reg_regularization"])
    return O.Fuser(reg, res=p["res"], submap_scan_size=p["submap_scan_size"], weight_intensity=bool(p["weight_intensity"]),
                   use_guess=bool(p["use_guess"]), compensate=bool(p["compensate"]), radar_ccw=bool(p["radar_ccw"]),
                   use_keyframe=bool(p["use_keyframe"]), min_keyframe_dist=p["min_keyframe_dist"],
                   min_keyframe_rot_deg=p["min_keyframe_rot_deg"], downsample_factor=p["downsample_factor"],
                   estimate_cov_by_sampling=bool(p["estimate_cov_by_sampling"]), cov_xy_range=p["cov_sampling_xy_range"],
                   cov_yaw_range=p["cov_sampling_yaw_range"], cov_samples_per_axis=p["cov_sampling_samples_per_axis"],
                   cov_scaler=p["cov_sampling_covariance_scaler"])


def _trace(par, world, poses):
    fz = make_oracle(par)
    out = []
    for f, pose in enumerate(poses):
        c = FC.cloud(FC.WORLDS[world], pose, f)
        if c.shape[0] == 0:                  # the oracle is simply not fed an empty cloud
            out.append(None)
            continue
        assert 400 <= c.shape[0] <= 700
        r = fz.process(c)
        assert r != -1
        cov, flag = fz.last_cov()
        out.append(dict(pose=r[0].copy(), n_cells=int(r[1][0]), keyframe=int(r[1][1]), ok=int(r[1][2]), iters=int(r[1][3]),
                        cov=cov, sampled=flag, first=not any(o is not None for o in out), **fz.last_decision()))
    return out


@functools.lru_cache(maxsize=None)
def oracle_trace(name, b, defaults=False):
    """The oracle's run of stream b of case `name`, frame by frame (None where the cloud is empty); computed once."""
    case = FC.BY_NAME[name]
    par = case["par"]
    if defaults:                             # the scaled world keeps the three settings that make it registrable at all
        par = FC.SCALED if case["world"] == "scaled" else {}
    return _trace(par, case["world"], case["streams"][b])


def _frames(name):
    """(stream, frame, record) of every frame of the case that took a decision (not empty, not a first frame)."""
    case = FC.BY_NAME[name]
    return [(b, f, r) for b in range(len(case["streams"])) for f, r in enumerate(oracle_trace(name, b))
            if r is not None and not r["first"]]


def _par(name):
    p = dict(FC.DEFAULTS)
    p.update(FC.BY_NAME[name]["par"])
    return p


NAMES = [c["name"] for c in FC.CASES]


def test_case_list_is_within_its_limits():
    assert len(set(NAMES)) == len(NAMES)
    for c in FC.CASES:
        assert 1 <= len(c["streams"]) <= 16 and all(s.shape[0] <= 20 for s in c["streams"])
        assert c["events"], c["name"]
    assert FC.BY_NAME["longest_window"]["par"]["submap_scan_size"] == FC.REG_MAX_SCANS - 1
    assert len(FC.BY_NAME["diverging_streams"]["streams"]) >= 8


@pytest.mark.parametrize("name", NAMES)
def test_no_decision_sits_near_a_threshold(name):
    p = _par(name)
    rot_thr = p["min_keyframe_rot_deg"] * np.pi / 180.0
    for b, f, r in _frames(name):
        assert abs(r["acc"] - 200.0) >= 1.0 and abs(r["vel"] - 200.0) >= 1.0, (b, f, r["acc"], r["vel"])
        if p["use_keyframe"]:
            assert abs(r["key_t"] - p["min_keyframe_dist"]) >= 1e-3, (b, f, r["key_t"])
            assert abs(r["key_rot"] - rot_thr) >= 1e-4, (b, f, r["key_rot"])


def _has_failed_then_good(tr):
    seq = [r["ok"] for r in tr if r is not None and not r["first"]]
    return any(a == 0 and b == 1 for a, b in zip(seq, seq[1:]))


def _event(name, ev):
    case, p, fr = FC.BY_NAME[name], _par(name), _frames(name)
    B = len(case["streams"])
    if ev == "keyframe_and_not":
        return {r["keyframe"] for _, _, r in fr} == {0, 1}
    if ev == "every_frame_evicts":           # every frame is a keyframe, and the window is full from frame submap_scan_size on
        return all(r["keyframe"] for _, _, r in fr) and case["streams"][0].shape[0] >= p["submap_scan_size"] + 3
    if ev == "only_first_keyframe":
        return not any(r["keyframe"] for _, _, r in fr)
    if ev == "keyframe_below_dist":          # a keyframe on rotation alone
        return any(r["keyframe"] and r["key_t"] < p["min_keyframe_dist"] for _, _, r in fr)
    if ev == "full_window":                  # the window reaches kRegMaxScans - 1 scans and then evicts three times
        return p["submap_scan_size"] == FC.REG_MAX_SCANS - 1 and sum(r["keyframe"] for _, _, r in fr) + 1 >= p["submap_scan_size"] + 3
    if ev == "failed_then_good":
        return any(_has_failed_then_good(oracle_trace(name, b)) for b in range(B))
    if ev == "failed_keyframe":
        return any(r["keyframe"] and not r["ok"] for _, _, r in fr)
    if ev == "rejected_jump":                # the registration moved the pose by metres and the guess took it back
        return any(r["replaced"] and r["ok"] and r["iters"] > 1 for _, _, r in fr)
    if ev == "accepted_jump":
        tr = oracle_trace(name, 0)
        return any(not r["replaced"] and np.hypot(*(r["pose"][:2] - tr[f - 1]["pose"][:2])) > 5.0 for _, f, r in fr)
    if ev == "acc_branch":
        return any(r["replaced"] and r["acc"] > 200.0 for _, _, r in fr)
    if ev == "vel_branch":                   # acceleration is tested first: the velocity branch is the one with acc <= 200
        return any(r["replaced"] and r["acc"] <= 200.0 and r["vel"] > 200.0 for _, _, r in fr)
    if ev == "empty_first":                  # a stream whose first cloud is empty beside streams that start
        first = [np.isnan(s[0, 0]) for s in case["streams"]]
        return any(first) and not all(first)
    if ev in ("empty_on_plain_frame", "empty_on_keyframe_frame"):
        # the same drive with every cloud delivered says what the missing frame would have done
        full = _trace(case["par"], case["world"], FC.STRAIGHT)
        b, want = (1, 0) if ev == "empty_on_plain_frame" else (2, 1)
        f = int(np.flatnonzero(np.isnan(case["streams"][b][:, 0]))[0])
        same = np.array_equal(np.delete(case["streams"][b], f, 0), np.delete(FC.STRAIGHT, f, 0))
        return same and f > 0 and full[f]["keyframe"] == want
    if ev == "starved":                      # submap_scan_size + 3 empty frames in a row, then good ones
        e = np.isnan(case["streams"][0][:, 0]).astype(int)
        run = max(len(x) for x in "".join(map(str, e)).split("0"))
        return run >= p["submap_scan_size"] + 3 and e[-1] == 0 and e[0] == 0
    if ev == "mixed_fusing":                 # on one frame some streams add a keyframe and some do not
        F = case["streams"][0].shape[0]
        for f in range(1, F):
            ks = {r["keyframe"] for b in range(B) for r in [oracle_trace(name, b)[f]] if r is not None and not r["first"]}
            if ks == {0, 1}:
                return True
        return False
    if ev == "sampled_keyframes":            # keyframes behind another one whose cov_current is the sampled one, past 1 rad
        k = [r for _, _, r in fr if r["keyframe"] and r["sampled"]]
        return len(k) >= 4 and max(abs(r["pose"][2]) for r in k) >= 1.0
    raise KeyError(ev)


@pytest.mark.parametrize("name,ev", [(c["name"], ev) for c in FC.CASES for ev in c["events"]])
def test_case_shows_its_declared_event(name, ev):
    assert _event(name, ev), (name, ev)


@pytest.mark.parametrize("name", [c["name"] for c in FC.CASES if c["differs"]])
def test_parameter_changes_the_outcome_against_the_defaults(name):
    a, d = oracle_trace(name, 0), oracle_trace(name, 0, True)
    same = all(x["keyframe"] == y["keyframe"] and x["iters"] == y["iters"] and x["n_cells"] == y["n_cells"] and
               np.array_equal(x["pose"], y["pose"]) for x, y in zip(a, d))
    assert not same


def test_fuser_process_returns_a_failed_frame():
    """orc_fuser_process answers -1 where the frame itself fails; Fuser.process hands that on instead of asserting.  (An
    empty cloud is no such failure in the oracle: it makes a scan without cells, which is why the cases never feed one.)"""
    fz = make_oracle({})
    r = fz.process(FC.cloud(FC.WORLDS["unit"], FC.STRAIGHT[0], 0))
    assert r != -1 and r[1][1] == 1 and np.isnan(fz.last_decision()["acc"])
    r = fz.process(FC.cloud(FC.WORLDS["unit"], FC.STRAIGHT[1], 1))
    d = fz.last_decision()
    assert r != -1 and not d["replaced"] and np.array_equal(d["registered"], r[0])
