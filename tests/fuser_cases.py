"""Hand-built frame sequences that take OdometryKeyframeFuser::processFrame (odometrykeyframefuser.cpp:143-259) through
every branch and parameter of its frame policy.  NumPy only: no GPU, no oracle.

A world is a fixed set of points on straight walls; cloud(world, pose, frame) is what a sensor at `pose` sees of it: every
world point within reach, in the sensor frame, with a little noise -- float32 [n, 4] (x, y, 0, intensity), 400-700 points,
~65 surface cells at res = 3.  No sweep is rendered and no filter runs: the clouds enter through process_clouds.  The
clouds are NOT distorted by the sensor's motion, so with compensate = 1 the registration sees a warp of the size of the
motion; both sides of a comparison see the same warp.

A case = dict(name, par = odometry_params overrides (C field names), world = "unit" | "scaled", streams = list of pose
sequences ([F, 3] float64; a frame whose pose is NaN delivers an EMPTY cloud), events = what the oracle's run of the case
must show (tests/test_fuser_cases_cpu.py keeps them honest), differs = True where the parameter must change the outcome
against the defaults on the same drive).  At most 16 streams and 20 frames each.
"""
import numpy as np

# cfear_odometry_params_default, the fields the frame policy reads (the GPU test holds them to the library's own)
DEFAULTS = dict(res=3.0, submap_scan_size=4, weight_intensity=1, use_guess=1, compensate=1, radar_ccw=0, use_keyframe=1,
                min_keyframe_dist=1.5, min_keyframe_rot_deg=5.0, downsample_factor=1.0, estimate_cov_by_sampling=0,
                reg_cost=0, reg_loss=1, reg_loss_limit=0.1, reg_weight_opt=4, reg_max_itr_association=8,
                reg_max_itr_solver=20, reg_min_itr=3, reg_radius=2.0, reg_cov_scale=1.0, reg_regularization=0.0,
                cov_sampling_xy_range=0.4, cov_sampling_yaw_range=0.0043625, cov_sampling_samples_per_axis=3,
                cov_sampling_covariance_scaler=4.0)
REG_MAX_SCANS = 16                     # kRegMaxScans: the longest window is one less (the GPU test checks the value)

_WALLS = 12
_POINTS = 550


def make_world(seed, scale=1.0):
    """_POINTS points on _WALLS straight walls of 12 to 18 m, centred inside a 36 m box and at least 5 m beside the x axis
    the drives run along (all times `scale`), + reach and noise of the sensor
    -> dict(points [n, 2], intensity [n], reach, noise, seed)."""
    rng = np.random.default_rng(seed)
    pts = []
    per_wall = _POINTS // _WALLS
    for w in range(_WALLS):
        while True:
            c = rng.uniform(-18.0, 18.0, 2)
            if abs(c[1]) > 5.0:                         # the drives run along y ~ 0
                break
        ang = rng.uniform(0.0, np.pi)
        half = rng.uniform(6.0, 9.0)
        n = per_wall + (1 if w < _POINTS - per_wall * _WALLS else 0)
        s = np.linspace(-half, half, n)
        pts.append(c[None, :] + s[:, None] * np.array([np.cos(ang), np.sin(ang)])[None, :])
    pts = np.concatenate(pts) * scale
    inten = rng.integers(60, 256, pts.shape[0]).astype(np.float64)
    return dict(points=pts, intensity=inten, reach=45.0 * scale, noise=0.02 * scale, seed=seed)


WORLDS = {"unit": make_world(7), "scaled": make_world(7, 10.0)}


def cloud(world, pose, frame):
    """The cloud a sensor at pose (x, y, theta) sees on frame number `frame` -> float32 [n, 4]; a NaN pose sees nothing."""
    pose = np.asarray(pose, np.float64)
    if not np.isfinite(pose).all():
        return np.zeros((0, 4), np.float32)
    rng = np.random.default_rng([world["seed"], int(frame), int(abs(pose[0]) * 1e3) % 100003])
    d = world["points"] - pose[None, :2]
    keep = np.hypot(d[:, 0], d[:, 1]) < world["reach"]
    d = d[keep]
    c, s = np.cos(pose[2]), np.sin(pose[2])
    loc = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], 1)
    loc += rng.normal(0.0, world["noise"], loc.shape)
    out = np.zeros((loc.shape[0], 4), np.float32)
    out[:, :2] = loc
    out[:, 3] = world["intensity"][keep]
    return out


# ---- drives: pose sequences [F, 3] ------------------------------------------------------------------------------------
def straight(n, step, heading=0.0, x0=0.0):
    """n frames along `heading` from (x0, 0), `step` metres per frame."""
    s = step * np.arange(n)
    return np.stack([x0 + s * np.cos(heading), s * np.sin(heading), np.full(n, heading)], 1)


def turn_in_place(n, rate):
    p = np.zeros((n, 3))
    p[:, 2] = rate * np.arange(n)
    return p


def arc(n, step, rate):
    """`step` metres forward and `rate` radians of heading per frame."""
    p = np.zeros((n, 3))
    for f in range(1, n):
        th = p[f - 1, 2] + rate
        p[f] = [p[f - 1, 0] + step * np.cos(th), p[f - 1, 1] + step * np.sin(th), th]
    return p


def along_x(xs):
    p = np.zeros((len(xs), 3))
    p[:, 0] = xs
    return p


def with_empty(poses, frames):
    p = np.array(poses, np.float64)
    p[list(frames)] = np.nan
    return p


def glitch(poses, frame, dy):
    """One frame seen from `dy` metres beside the track: nothing associates within the default 2 m radius."""
    p = np.array(poses, np.float64)
    p[frame, 1] += dy
    return p


STRAIGHT = straight(10, 0.6)              # a keyframe every third frame at the default 1.5 m
TURN = turn_in_place(10, 0.035)           # 2 deg per frame: a keyframe every third frame at the default 5 deg, never on distance
FAST = straight(8, 1.2, 0.3, -4.0)        # 1.2 m per frame: a keyframe every second frame, and a compensation that matters
LONG_ARC = arc(13, 0.5, 0.12)             # the heading reaches 1.44 rad; a keyframe every frame (0.12 rad > 5 deg)
ARC = LONG_ARC[:10]
GLITCH = glitch(STRAIGHT, 4, 20.0)        # frame 4 (no keyframe due) fails to register, frame 5 registers again
# acceleration branch, scaled world: standing, a 16 m jump (acc 256 > 200: rejected, the estimate stays), then the sensor
# 8 m from the estimate (acc 128: accepted) and standing there (the guess overshoots by 8 m: acc 128 again, accepted)
JUMPS = along_x([0, 0, 0, 16, 8, 8, 8, 8])
# velocity branch, scaled world: the step grows by 8 m per frame (acc 128 on every frame) until it passes 50 m per frame
# (vel > 200) on frame 7 -- acc is tested first, so only a ramp under 12.5 m per frame gets there with the estimate tracking
RAMP = along_x(np.cumsum(8.0 * np.arange(9)) - 120.0)
SCALED = dict(res=30.0, reg_radius=30.0, compensate=0)
# submap_scan_size + 3 = 7 consecutive empty frames after three good ones, then the drive goes on where it stood
STARVED = np.concatenate([STRAIGHT[:3], np.full((7, 3), np.nan), STRAIGHT[3:6]])


def _case(name, par, streams, events=(), world="unit", differs=False):
    streams = [np.array(s, np.float64) for s in streams]
    assert len(streams) <= 16 and all(s.shape[0] <= 20 for s in streams) and len({s.shape[0] for s in streams}) == 1
    return dict(name=name, par=dict(par), streams=streams, events=tuple(events), world=world, differs=differs)


CASES = [
    _case("default", {}, [STRAIGHT, TURN, np.concatenate([FAST, FAST[-1:], FAST[-1:]])], ["keyframe_and_not"]),
    # ---- parameter matrix: each must change the oracle's outcome against the defaults on the same drive
    _case("use_guess_0", dict(use_guess=0), [FAST], ["keyframe_and_not"], differs=True),
    _case("compensate_0", dict(compensate=0), [FAST], ["keyframe_and_not"], differs=True),
    _case("radar_ccw_1", dict(radar_ccw=1), [FAST], ["keyframe_and_not"], differs=True),
    _case("no_keyframe_window_1", dict(use_keyframe=0, submap_scan_size=1), [STRAIGHT[:6]], ["every_frame_evicts"], differs=True),
    _case("no_keyframe_window_2", dict(use_keyframe=0, submap_scan_size=2), [STRAIGHT[:6]], ["every_frame_evicts"], differs=True),
    _case("keyframe_dist_0.5", dict(min_keyframe_dist=0.5), [STRAIGHT], ["keyframe_and_not"], differs=True),
    _case("keyframe_dist_1e9", dict(min_keyframe_dist=1e9), [STRAIGHT], ["only_first_keyframe"], differs=True),
    _case("keyframe_rot_1deg", dict(min_keyframe_rot_deg=1.0), [TURN], ["keyframe_below_dist"], differs=True),
    _case("downsample_2", dict(downsample_factor=2.0), [STRAIGHT], ["keyframe_and_not"], differs=True),
    _case("longest_window", dict(use_keyframe=0, submap_scan_size=REG_MAX_SCANS - 1), [straight(REG_MAX_SCANS + 2, 0.3)],
          ["full_window"], differs=True),
    # ---- branches
    _case("failed_registration", {}, [GLITCH], ["failed_then_good", "keyframe_and_not"]),
    # ... and on a frame that becomes a keyframe all the same: its constraint carries the Identity of the failed Register
    _case("failed_registration_keyframe", dict(use_keyframe=0), [glitch(STRAIGHT, 6, 20.0)], ["failed_then_good", "failed_keyframe"]),
    _case("sanity_acceleration", SCALED, [JUMPS], ["rejected_jump", "accepted_jump", "acc_branch"], world="scaled"),
    _case("sanity_velocity", SCALED, [RAMP], ["vel_branch"], world="scaled"),
    _case("empty_clouds", {},
          [with_empty(STRAIGHT, [0]),       # the first cloud is empty while the others start
           with_empty(STRAIGHT, [4]),       # mid-sequence, on a frame that adds no keyframe
           with_empty(STRAIGHT, [3]),       # on a frame that would have added one
           STRAIGHT],
          ["empty_first", "empty_on_plain_frame", "empty_on_keyframe_frame"]),
    _case("starved", {}, [STARVED, np.concatenate([STRAIGHT, STRAIGHT[-1:], STRAIGHT[-1:], STRAIGHT[-1:]])], ["starved"]),
    # >= 8 streams: the registration batch is ordered in five classes; some streams fuse on a frame and some do not, one
    # fails to register, one starts a frame late
    _case("diverging_streams", {},
          [STRAIGHT, TURN, ARC, GLITCH, with_empty(STRAIGHT, [0]), straight(10, -0.6), straight(10, 0.0),
           straight(10, 0.9, 0.5, -3.0), with_empty(TURN, [5])],
          ["keyframe_and_not", "failed_then_good", "empty_first", "mixed_fusing"]),
    # ---- AddToGraph with a sampled (anisotropic, non-singular) covariance at headings beyond 1 rad
    _case("sampled_constraints", dict(estimate_cov_by_sampling=1), [LONG_ARC, straight(13, 0.8, 0.3, -4.0)], ["sampled_keyframes"]),
]
BY_NAME = {c["name"]: c for c in CASES}
