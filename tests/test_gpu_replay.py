"""GPU: cfear_odometry_replay_clouds -- every frame registered from the recorded pose of the frame before it and the
recorded keyframe set -- on the hand-built wall world of tests/fuser_cases.py (about 550 points and 60 cells per frame),
against live OdometryKeyframeFuser.process_clouds, against the CPU restatement tests/replay_cpu.py, and against itself
(locality, several sequences, chunks, holes).  Bounds: a replay of the library's own trace meets the live poses within
1e-9 m / 1e-10 rad -- a hundred times the 1e-11 to which the matcher's forms agree when a batch size changes the form
(include/cfear_hip.h) --, the restatement within the project's 1e-4 m / 1e-5 rad."""
import ctypes as C

import numpy as np
import pytest

from tests import fuser_cases as FC
from tests import replay_cpu as RC

pytestmark = pytest.mark.gpu

OWN_XY, OWN_TH = 1e-9, 1e-10
POS_TOL, ROT_TOL = 1e-4, 1e-5
FAST_KF = dict(min_keyframe_dist=1.0)         # STRAIGHT: a keyframe every second frame, the window slides from frame 8 on
SLOW_KF = dict(min_keyframe_dist=2.0)         # straight(12, 0.6): keyframes 0, 4, 8
DRIVES = {"fast": (FC.STRAIGHT, FAST_KF), "slow": (FC.straight(12, 0.6), SLOW_KF), "turn": (FC.TURN[:7], FAST_KF),
          "mid": (FC.straight(8, 0.7, 0.2, -2.0), FAST_KF),
          "lap": (None, {})}                  # 8 sweeps of synth.scene_v1 through the k-strongest filter: scans that hold ties
BEND = (0.05, 0.0, 0.002)
_CACHE = {}


def _live(name):
    """Live odometry over the drive -> (clouds, FRAMEINFO records [frames], trace [frames, 3]); run once."""
    if name not in _CACHE:
        from tbv_slam_public_amd import api
        poses, over = DRIVES[name]
        if poses is None:
            from tbv_slam_public_amd import synth
            r = api.filter_kstrongest(synth.scene_v1(5, 8)[0], 40, 60, 0.0438, 2.5)
            clouds = [r["xyzi"][f, :int(r["n_points"][f])].copy() for f in range(8)]
        else:
            clouds = [FC.cloud(FC.WORLDS["unit"], p, f) for f, p in enumerate(poses)]
        od = api.OdometryKeyframeFuser(1, *((400, 3360) if poses is None else (32, 64)), api.odometry_params(**over))
        infos = np.concatenate([od.process_clouds([c]).copy() for c in clouds])
        _CACHE[name] = (clouds, infos, infos["pose"].copy())
    return _CACHE[name]


def _replay(name, trace=None, clouds=None, **kw):
    from tbv_slam_public_amd import api
    c, _, t = _live(name)
    return api.odometry_replay(c if clouds is None else clouds, t if trace is None else trace, api.odometry_params(**DRIVES[name][1]), **kw)


def _base(name):
    if ("replay", name) not in _CACHE:
        _CACHE[("replay", name)] = _replay(name)
    return _CACHE[("replay", name)]


def _flags(trace, over):
    """The keyframe chain of a trace on the host, with the library's own cfear_keyframe_based_fuse."""
    from tbv_slam_public_amd import _lib as L
    p = RC.params(over)
    flags, last = [1], 0
    for t in range(1, len(trace)):
        d = (C.c_double * 3)(*RC.xyt(RC.mul(RC.inv(RC.aff(trace[last])), RC.aff(trace[t]))))
        k = int(L.lib().cfear_keyframe_based_fuse(d, p["use_keyframe"], p["min_keyframe_dist"], p["min_keyframe_rot_deg"]))
        flags.append(k)
        last = t if k else last
    return flags


def _close(a, b):
    d = np.abs(np.asarray(a) - np.asarray(b))
    return bool(d[..., :2].max() <= OWN_XY and d[..., 2].max() <= OWN_TH)


@pytest.mark.parametrize("name", ["fast", "slow"])
def test_own_trace(name):
    """The replay of the library's own trace has the live run's counts and statuses, and meets its poses."""
    _, info, trace = _live(name)
    rec = _base(name)
    assert rec.dtype.itemsize == 160 and len(rec) == len(trace)
    for f in ("reg_status", "n_cells", "outer_iters", "lm_iters", "n_points"):
        assert np.array_equal(rec[f], info[f]), f
    assert np.array_equal(rec["is_keyframe"], info["keyframe_added"]) and rec["is_keyframe"].sum() >= 3
    assert rec["reg_status"][0] == 1 and rec["n_targets"][0] == 0 and not rec["dev"][0].any()
    assert np.array_equal(rec["pose"][0], trace[0]) and np.array_equal(rec["guess"][0], trace[0])
    assert np.array_equal(rec["score"][1:], info["score"][1:]) or np.allclose(rec["score"][1:], info["score"][1:], rtol=1e-9)
    assert (rec["sanity_ok"] == 1).all() and (rec["num_residuals"][1:] > 0).all()             # every job ran
    assert list(rec["n_targets"][1:]) == [min(4, int(rec["is_keyframe"][:t].sum())) for t in range(1, len(rec))]
    assert (rec["exposed"] == -1).all() and (rec["n_tied_start"] == -1).all() and (rec["n_voxels_exposed"] == -1).all()
    print(name, "max |dev| xy %.3g theta %.3g" % (np.abs(rec["dev"][:, :2]).max(), np.abs(rec["dev"][:, 2]).max()),
          "frames with dev exactly 0:", int((~rec["dev"].any(axis=1)).sum()), "of", len(rec))
    assert np.abs(rec["dev"][:, :2]).max() <= OWN_XY and np.abs(rec["dev"][:, 2]).max() <= OWN_TH
    assert _close(rec["pose"][1:], trace[1:])


def test_against_the_restatement():
    clouds, _, trace = _live("fast")
    rec, want = _base("fast"), RC.replay(clouds, trace, FAST_KF)
    for t, w in enumerate(want):
        at = (t, rec[t], w)
        assert rec["n_cells"][t] == w["n_cells"] and rec["is_keyframe"][t] == w["is_keyframe"] and rec["n_targets"][t] == w["n_targets"], at
        for f, tol in ((slice(0, 2), POS_TOL), (slice(2, 3), ROT_TOL)):
            assert np.abs(rec["pose"][t][f] - w["pose"][f]).max() <= tol and np.abs(rec["guess"][t][f] - w["guess"][f]).max() <= tol, at
        if t:
            assert (rec["reg_status"][t] == 0) == (w["ok"] == 1) and rec["outer_iters"][t] == w["outer_iters"], at
            assert rec["sanity_ok"][t] == w["sanity_ok"], at


def test_locality():
    """A perturbed NON-keyframe pose P_j (j + 1 and j + 2 no keyframes either: their compensated scans enter no window)
    changes frame j's dev and frames j + 1 and j + 2; a perturbed keyframe P_k its own dev and every frame whose window
    holds it.  Every other frame is bit-identical."""
    _, _, trace = _live("slow")
    base = _base("slow")
    flags = _flags(trace, SLOW_KF)
    assert flags == list(base["is_keyframe"]) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    j = 5
    bent = trace.copy()
    bent[j] += BEND
    assert _flags(bent, SLOW_KF) == flags
    got = _replay("slow", trace=bent)
    for t in range(len(trace)):
        if t == j:
            assert np.array_equal(got["pose"][t], base["pose"][t]) and not np.array_equal(got["dev"][t], base["dev"][t])
            assert np.abs(got["dev"][t] + BEND).max() < 1e-3            # the registration did not move: dev is the bend, undone
        elif t in (j + 1, j + 2):
            assert not np.array_equal(got["pose"][t], base["pose"][t]) and not np.array_equal(got["guess"][t], base["guess"][t]), t
        else:
            assert got[t].tobytes() == base[t].tobytes(), t
    k = 4
    bent = trace.copy()
    bent[k] += BEND
    assert _flags(bent, SLOW_KF) == flags
    got = _replay("slow", trace=bent)
    for t in range(len(trace)):
        if t < k:
            assert got[t].tobytes() == base[t].tobytes(), t
        elif t == k:
            assert np.array_equal(got["pose"][t], base["pose"][t]) and not np.array_equal(got["dev"][t], base["dev"][t])
        else:                                                             # 5 .. 11: keyframe 4 is in every window
            assert not np.array_equal(got["pose"][t], base["pose"][t]), t


def _same(a, b):
    for f in ("reg_status", "n_cells", "n_points", "is_keyframe", "n_targets", "outer_iters", "lm_iters", "num_residuals", "sanity_ok"):
        assert np.array_equal(a[f], b[f]), f
    assert _close(a["pose"], b["pose"]) and _close(a["guess"], b["guess"]) and _close(a["dev"], b["dev"])


def test_several_sequences_and_chunks():
    """Three sequences of different lengths in one call equal the three single calls, also with three frames per chunk:
    chunk boundaries then fall inside a window and inside a sequence."""
    from tbv_slam_public_amd import _lib as L, api
    names = ["fast", "turn", "mid"]                                       # 10 + 7 + 8 frames, one set of parameters
    clouds = sum([_live(n)[0] for n in names], [])
    trace = np.concatenate([_live(n)[2] for n in names])
    single = np.concatenate([_base(n) for n in names])
    offs = np.cumsum([0] + [len(_live(n)[2]) for n in names])
    par = api.odometry_params(**FAST_KF)
    _same(api.odometry_replay(clouds, trace, par, seq_offsets=offs), single)
    ctx = api.default_context()
    assert ctx.get_option(L.OPT_REPLAY_CHUNK) == 0
    for chunk in (3, 1):
        ctx.set_option(L.OPT_REPLAY_CHUNK, chunk)
        try:
            assert ctx.get_option(L.OPT_REPLAY_CHUNK) == chunk
            _same(api.odometry_replay(clouds, trace, par, seq_offsets=offs), single)
        finally:
            ctx.set_option(L.OPT_REPLAY_CHUNK, 0)
    import torch
    dev = api.odometry_replay([torch.from_numpy(c).cuda() for c in clouds], trace, par, seq_offsets=offs)   # clouds on the device
    assert dev.tobytes() == api.odometry_replay(clouds, trace, par, seq_offsets=offs).tobytes()


@pytest.mark.parametrize("hole", [3, 4], ids=["plain_frame", "keyframe"])
def test_failures_stay_local(hole):
    """An empty cloud is that frame's CFEAR_ERR_EMPTY_CLOUD and no job; where the frame is a keyframe of the trace, the frames
    whose window holds it report the status too.  Every other frame is bit-identical to the run without the hole."""
    from tbv_slam_public_amd import _lib as L
    clouds, _, trace = _live("fast")
    base = _base("fast")
    assert base["is_keyframe"][4] == 1 and base["is_keyframe"][3] == 0
    holed = list(clouds)
    holed[hole] = np.zeros((0, 4), np.float32)
    got = _replay("fast", clouds=holed)
    hit = {hole} | ({t for t in range(5, 10)} if hole == 4 else set())       # frames 5 .. 9 hold keyframe 4 in their windows
    for t in range(len(trace)):
        if t in hit:
            assert got["reg_status"][t] == L.ERR_EMPTY_CLOUD and got["n_targets"][t] == 0 and got["outer_iters"][t] == 0, t
            assert got["is_keyframe"][t] == base["is_keyframe"][t] and np.array_equal(got["guess"][t], base["guess"][t]), t
        else:
            assert got[t].tobytes() == base[t].tobytes(), t
    assert got["n_points"][hole] == 0 and got["n_cells"][hole] == 0


def test_refusals():
    from tbv_slam_public_amd import _lib as L, api
    clouds, _, trace = _live("fast")
    par = api.odometry_params(**FAST_KF)
    ctx = api.default_context()

    def refused(seq=None, tr=None):
        with pytest.raises(L.CfearError) as e:
            api.odometry_replay(clouds, trace if tr is None else tr, par, seq_offsets=seq)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        return str(e.value)
    assert "sequence 1" in refused(seq=[0, 6, 4, 10])                      # not ascending
    assert "sequence 1" in refused(seq=[0, 5, 5, 10])                      # a sequence of length 0
    assert "sequence 0" in refused(seq=[1, 10])
    bad = trace.copy()
    bad[7, 1] = np.nan
    assert "frame 7" in refused(tr=bad)
    arr = (L.ScCloud * 10)()
    out = np.zeros(10, L.REPLAY_FRAME_DTYPE)
    seq = np.array([0, 10], np.int32)
    lib = ctx._lib
    assert lib.cfear_odometry_replay_clouds(ctx.h, arr, C.byref(par), None, seq.ctypes.data, 1, 0, out.ctypes.data) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_odometry_replay_clouds(ctx.h, arr, C.byref(par), trace.ctypes.data, seq.ctypes.data, 0, 0, out.ctypes.data) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_odometry_replay_clouds(ctx.h, arr, C.byref(par), trace.ctypes.data, seq.ctypes.data, 1, 2, out.ctypes.data) == L.ERR_INVALID_ARGUMENT   # an unknown flag
    assert not out.view(np.uint8).any()                                    # nothing was launched or written
    big = api.odometry_params(submap_scan_size=16)
    assert lib.cfear_odometry_replay_clouds(ctx.h, arr, C.byref(big), trace.ctypes.data, seq.ctypes.data, 1, 0, out.ctypes.data) == L.ERR_INVALID_ARGUMENT


def test_summary_counts_the_classes():
    from tbv_slam_public_amd import api
    rec = _base("fast").copy()
    s = api.replay_summary(rec, 1e-6, 1e-7)
    assert (s["n_frames"], s["n_no_job"], s["n_equal"], s["n_differ_exposed"], s["n_differ_not_exposed"]) == (10, 1, 9, 0, 0)
    assert s["first_not_exposed"] == [-1]
    rec["dev"][6] = (0.01, 0.0, 0.0)
    rec["dev"][8] = (0.0, 0.0, 0.02)
    rec["exposed"][8] = 1
    s = api.replay_summary(rec, 1e-6, 1e-7, seq_offsets=[0, 5, 10])
    assert (s["n_equal"], s["n_differ_exposed"], s["n_differ_not_exposed"]) == (7, 1, 1)
    assert s["first_not_exposed"] == [-1, 6] and s["worst_dev_differ_not_exposed"][0] == 0.01 and s["worst_dev_differ_exposed"][2] == 0.02


@pytest.mark.parametrize("name", ["fast", "lap"])
def test_audit_fields_equal_the_direct_audits(name):
    """With CFEAR_REPLAY_AUDIT the tie fields are api.association_ties on the same jobs at the guess (itr = 1) and at the
    registered pose (itr = 2), the voxel fields api.voxel_order_audit on the compensated clouds, summed over the job's scans;
    without it they are -1 and every other field is the same bits."""
    from tbv_slam_public_amd import api
    clouds, _, trace = _live(name)
    over = DRIVES[name][1]
    p = RC.params(over)
    base = _base(name)
    got = _replay(name, audit=True)
    plain = got.copy()
    for f in ("n_tied_start", "n_tied_effective_start", "n_tied_end", "n_tied_effective_end", "n_voxels_exposed", "n_voxels_changed_reversed", "exposed"):
        plain[f] = -1
    assert plain.tobytes() == base.tobytes()
    T = [RC.aff(q) for q in trace]
    mots = np.array([RC.xyt(RC.IDENTITY if t < 2 else RC.mul(RC.inv(T[t - 2]), T[t - 1])) for t in range(len(trace))])
    comp = [api.Compensate(c.copy(), mots[t], bool(p["radar_ccw"])) for t, c in enumerate(clouds)]
    vox = api.voxel_order_audit(comp, p["res"], p["downsample_factor"])
    scans = api.scan_create_batch(clouds, p["res"], (0.0, 0.0), bool(p["weight_intensity"]), compensate=mots, ccw=bool(p["radar_ccw"]))
    keyframes, windows = [], []
    for t in range(len(trace)):
        windows.append(list(keyframes))
        if got["is_keyframe"][t]:
            keyframes = (keyframes + [t])[-p["submap_scan_size"]:]
    frames = list(range(1, len(trace)))
    window_poses = lambda t: [RC.xyt(T[k]) for k in windows[t]]
    jobs = lambda key: [([scans[k] for k in windows[t]] + [scans[t]], np.vstack(window_poses(t) + [got[key][t]])) for t in frames]
    reg = api.n_scan_normal_reg(ctx=api.default_context())
    reg.par = api.odometry_params(**over).reg
    start, end = api.association_ties(jobs("guess"), reg, 1), api.association_ties(jobs("pose"), reg, 2)
    for i, t in enumerate(frames):
        assert (got["n_tied_start"][t], got["n_tied_effective_start"][t]) == (start["n_tied"][i], start["n_tied_effective"][i]), t
        assert (got["n_tied_end"][t], got["n_tied_effective_end"][t]) == (end["n_tied"][i], end["n_tied_effective"][i]), t
        job_scans = windows[t] + [t]
        assert got["n_voxels_exposed"][t] == vox["n_voxels_exposed"][job_scans].sum(), t
        assert got["n_voxels_changed_reversed"][t] == vox["n_voxels_changed_reversed"][job_scans].sum(), t
        want = int(start["n_tied_effective"][i] > 0 or end["n_tied_effective"][i] > 0 or got["n_voxels_exposed"][t] > 0)
        assert got["exposed"][t] == want, t
    assert got["n_tied_start"][0] == 0 and got["n_voxels_exposed"][0] == vox["n_voxels_exposed"][0]
    if name == "lap":                                                      # the comparison is not of zeros with zeros
        assert got["n_tied_start"].sum() > 0 and got["n_voxels_exposed"].sum() > 0 and (got["exposed"] == 1).any()
    print(name, "exposed frames:", int((got["exposed"] == 1).sum()), "of", len(got), "tied (start, end):", got["n_tied_start"].tolist(), got["n_tied_end"].tolist(),
          "voxels exposed:", got["n_voxels_exposed"].tolist())


SWEEP_PARS = {"cfear3": dict(),
              "kvarntorp_cacfar": dict(filter_type=1, cacfar_range_res=0.175, cacfar_z_min=20.0, cacfar_nb_guard_cells=10, cacfar_window_size=40,
                                       cacfar_false_alarm_rate=0.01, radar_ccw=1, kstrong_range_res=0.175)}


@pytest.mark.parametrize("name", sorted(SWEEP_PARS))
def test_sweep_entry(name):
    """Two 8-frame scene_v1 sequences through cfear_odometry_replay along the trace live cfear_odometry_process made of the
    same sweeps: counts and statuses equal, the poses within the own-trace bound."""
    from tbv_slam_public_amd import _lib as L, api, synth
    n = 8
    scene = dict(range_res=0.175, ccw=True) if name == "kvarntorp_cacfar" else {}
    seqs = [synth.scene_v1(sd, n, **scene)[0] for sd in (21, 22)]
    par = api.odometry_params(**SWEEP_PARS[name])
    od = api.OdometryKeyframeFuser(2, seqs[0].shape[1], seqs[0].shape[2], par)
    info = np.stack([od.process(np.stack([s[f] for s in seqs])).copy() for f in range(n)])      # [frame][stream]
    live = np.concatenate([info[:, b] for b in range(2)])
    sweeps = np.ascontiguousarray(np.concatenate(seqs))
    rec = api.odometry_replay(sweeps, live["pose"], par, seq_offsets=[0, n, 2 * n])
    for f in ("reg_status", "n_cells", "n_points", "outer_iters", "lm_iters"):
        assert np.array_equal(rec[f], live[f]), (f, rec[f], live[f])
    assert np.array_equal(rec["is_keyframe"], live["keyframe_added"]) and (rec["reg_status"][[0, n]] == 1).all()
    print(name, "max |dev| xy %.3g theta %.3g" % (np.abs(rec["dev"][:, :2]).max(), np.abs(rec["dev"][:, 2]).max()),
          "frames with dev exactly 0:", int((~rec["dev"].any(axis=1)).sum()), "of", len(rec))
    assert np.abs(rec["dev"][:, :2]).max() <= OWN_XY and np.abs(rec["dev"][:, 2]).max() <= OWN_TH
    import torch
    assert api.odometry_replay(torch.from_numpy(sweeps).cuda(), live["pose"], par, seq_offsets=[0, n, 2 * n]).tobytes() == rec.tobytes()
    if name == "cfear3":                                                   # a desc.batch other than the frame count
        with pytest.raises(L.CfearError) as e:
            api.odometry_replay(sweeps[:-1], live["pose"], par, seq_offsets=[0, n, 2 * n])
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "desc.batch" in str(e.value)
