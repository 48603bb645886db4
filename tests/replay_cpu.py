"""The replay's state rules (include/cfear_hip.h, cfear_odometry_replay_clouds) restated on the CPU from the oracle's
primitives: compensate, surface_points, register.  One sequence: frame t is registered from the TRACE pose of frame t - 1
and the trace's keyframe set; no frame reads another frame's result.  The poses are composed as the fuser composes them --
2 x 2 affine matrices in the operation order of Eigen's product and inverse (oracle/cfear_oracle.cpp: aff_mul, aff_inv;
csrc/pose2d.hpp) -- because xyt_compose / xyt_inverse, which add angles, differ from that in the last bit (measured: 2.2e-16 m
on frame 3 of the drive of tests/test_replay_cpu.py), and a replay of the fuser's own trace is to meet it exactly.

  frame 0    first keyframe at P_0, no job
  motion     M_1 = identity, M_t = P_t-2^-1 P_t-1; the cloud is compensated by M_t, the guess is P_t-1 M_t
  keyframes  frame t is one iff |t| > min_keyframe_dist or |rot| > min_keyframe_rot of P_lastkf^-1 P_t (or !use_keyframe)
  window     the last submap_scan_size keyframes before t, at their trace poses
  sanity     acc / vel of P_t-1^-1 pose against M_t (4 Hz, 200 m/s, 200 m/s^2; acceleration first)
  dev        P_t^-1 final on (x, y, theta) (xyt_inverse, xyt_compose), final = pose or, where the check fails, the guess

NumPy + the oracle only; used by tests/test_replay_cpu.py (against the oracle's own fuser) and tests/test_gpu_replay.py."""
import numpy as np

from tests import fuser_cases as FC


def params(overrides=None):
    p = dict(FC.DEFAULTS)
    p.update(overrides or {})
    return p


def aff(p):
    """(x, y, theta) -> (l0, l1, l2, l3, t0, t1): vectorToAffine3d."""
    c, s = np.cos(p[2]), np.sin(p[2])
    return (c, -s, s, c, float(p[0]), float(p[1]))


IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def mul(a, b):
    return (a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3],
            a[0] * b[4] + a[1] * b[5] + a[4], a[2] * b[4] + a[3] * b[5] + a[5])


def inv(a):
    invdet = 1.0 / (a[0] * a[3] - a[2] * a[1])
    l0, l1, l2, l3 = a[3] * invdet, -a[1] * invdet, -a[2] * invdet, a[0] * invdet
    return (l0, l1, l2, l3, -(l0 * a[4] + l1 * a[5]), -(l2 * a[4] + l3 * a[5]))


def xyt(a):
    """Affine3dToVectorXYeZ."""
    return np.array([a[4], a[5], np.arctan2(a[2], a[3])], np.float64)


def sane(prev_xy, curr_xy):
    dt, vel_limit, acc_limit = 0.25, 200.0, 200.0
    vel = np.sqrt((curr_xy[0] / dt) ** 2 + (curr_xy[1] / dt) ** 2)
    ax, ay = (curr_xy[0] - prev_xy[0]) / (dt * dt), (curr_xy[1] - prev_xy[1]) / (dt * dt)
    return not (np.sqrt(ax * ax + ay * ay) > acc_limit or vel > vel_limit)


def is_keyframe(diff, p):
    if not p["use_keyframe"]:
        return True
    return bool(np.sqrt(diff[0] * diff[0] + diff[1] * diff[1]) > p["min_keyframe_dist"] or abs(diff[2]) > p["min_keyframe_rot_deg"] * np.pi / 180.0)


def keyframe_flags(trace, p):
    """The keyframe chain of a trace alone -> int [frames]."""
    flags, last = [1], 0
    for t in range(1, len(trace)):
        k = is_keyframe(xyt(mul(inv(aff(trace[last])), aff(trace[t]))), p)
        flags.append(int(k))
        if k:
            last = t
    return np.array(flags)


def replay(clouds, trace, overrides=None):
    """-> one dict per frame: pose, guess, dev, is_keyframe, first, n_points, n_cells, n_targets, ok (the oracle's Register
    status: 1 = solved), outer_iters, lm_iters, num_residuals, sanity_ok.  An empty cloud gives dict(empty=True, ...) and
    no job, and so does a frame whose window holds one (window_empty=True)."""
    from oracle import pyoracle as O
    p = params(overrides)
    reg = O.reg_params(cost=p["reg_cost"], loss=p["reg_loss"], loss_limit=p["reg_loss_limit"], weight_opt=p["reg_weight_opt"],
                       max_outer=p["reg_max_itr_association"], max_inner=p["reg_max_itr_solver"], min_outer=p["reg_min_itr"],
                       radius=p["reg_radius"], cov_scale=p["reg_cov_scale"], regularization=p["reg_regularization"])
    P = np.asarray(trace, np.float64).reshape(-1, 3)
    T = [aff(q) for q in P]
    cells, keyframes, out = {}, [], []
    for t in range(len(P)):
        Tmot = IDENTITY if t < 2 else mul(inv(T[t - 2]), T[t - 1])
        M = xyt(Tmot)
        c = np.ascontiguousarray(clouds[t], np.float32)
        empty = c.shape[0] == 0
        if not empty:
            if p["compensate"]:
                c = O.compensate(c, M, p["radar_ccw"])
            cells[t] = O.surface_points(c, p["res"], p["downsample_factor"], (0.0, 0.0), bool(p["weight_intensity"]))
        window = list(keyframes)
        rec = dict(empty=empty, window_empty=any(k not in cells for k in window), first=t == 0, n_points=int(c.shape[0]),
                   n_cells=0 if empty else int(cells[t].shape[0]), n_targets=0, window=window)
        if t == 0:
            rec.update(pose=P[0].copy(), guess=P[0].copy(), dev=np.zeros(3), is_keyframe=1)
            keyframes.append(0)
            out.append(rec)
            continue
        Tguess = mul(T[t - 1], Tmot) if p["use_guess"] else T[t - 1]
        guess = xyt(Tguess)
        rec.update(guess=guess, pose=guess.copy(), dev=np.zeros(3))
        if not empty and not rec["window_empty"]:
            _, poses, res = O.register([cells[k] for k in window] + [cells[t]], np.vstack([xyt(T[k]) for k in window] + [guess]), reg)
            pose = poses[-1].copy()
            Tcurrent = aff(pose)
            ok = sane(Tmot[4:], mul(inv(T[t - 1]), Tcurrent)[4:])
            # dev on (x, y, theta) itself (xyt_inverse, xyt_compose): exactly zero iff the final pose IS the trace pose
            rec.update(pose=pose, dev=O.xyt_compose(O.xyt_inverse(P[t]), pose if ok else guess), n_targets=len(window), ok=int(res.status),
                       outer_iters=int(res.outer_iters), lm_iters=int(res.lm_iters), num_residuals=int(res.num_residuals),
                       sanity_ok=int(ok))
        k = is_keyframe(xyt(mul(inv(T[keyframes[-1]]), T[t])), p)
        rec["is_keyframe"] = int(k)
        if k:
            keyframes.append(t)
            if len(keyframes) > p["submap_scan_size"]:
                keyframes.pop(0)
        out.append(rec)
    return out
