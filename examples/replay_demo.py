"""Replay of a recorded odometry trace (api.odometry_replay).  One synthetic lap through live odometry gives trace A; the
replay of A registers every frame from A's own state in one batch and meets A.  Trace B is the same lap through a fuser
that decides every nearest-neighbour tie of every keyframe the OTHER way (api.flip_ties on the window's scans) -- what a
build with another tie rule would record.  B is replayed with the audit: the frames whose replayed pose differs from B
are exactly those where this library's rule and B's disagree from B's own state, and the audit says for how many of them
a tie or a voxel order was there to be seen at the two snapshots.  A tie that exists only at an association pass in
between is legally invisible to them: that class is reported by count, not gated.

  python examples/replay_demo.py --frames 24
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def aff(p):
    c, s = np.cos(p[2]), np.sin(p[2])
    return (c, -s, s, c, float(p[0]), float(p[1]))


def mul(a, b):
    return (a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3],
            a[0] * b[4] + a[1] * b[5] + a[4], a[2] * b[4] + a[3] * b[5] + a[5])


def inv(a):
    d = 1.0 / (a[0] * a[3] - a[2] * a[1])
    l0, l1, l2, l3 = a[3] * d, -a[1] * d, -a[2] * d, a[0] * d
    return (l0, l1, l2, l3, -(l0 * a[4] + l1 * a[5]), -(l2 * a[4] + l3 * a[5]))


def xyt(a):
    return np.array([a[4], a[5], np.arctan2(a[2], a[3])])


IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def flipped_fuser(clouds, par, api, L):
    """OdometryKeyframeFuser::processFrame (odometrykeyframefuser.cpp:143-259) in Python over the library's primitives, every
    window scan handed to Register with its cells reversed (api.flip_ties) -> the trace [frames, 3]."""
    lib = L.lib()
    reg = api.n_scan_normal_reg()
    reg.par = par.reg
    T_prev = Tmot = Tcur = IDENTITY
    keyframes, trace = [], []
    for cloud in clouds:
        scan = api.MapPointNormal(cloud.clone(), par.res, (0.0, 0.0), bool(par.weight_intensity),
                                  compensate=tuple(xyt(Tmot)) if par.compensate else None, ccw=bool(par.radar_ccw))
        Tguess = mul(T_prev, Tmot) if par.use_guess else T_prev
        if not keyframes:
            keyframes.append((IDENTITY, api.flip_ties(scan)))
            trace.append(xyt(Tcur))
            continue
        _, poses, _ = reg.Register([k[1] for k in keyframes] + [scan], np.vstack([xyt(k[0]) for k in keyframes] + [xyt(Tguess)]))
        Tcur = aff(poses[-1])
        now = mul(inv(T_prev), Tcur)
        if not lib.cfear_acc_vel_sanity_check((C.c_double * 2)(Tmot[4], Tmot[5]), (C.c_double * 2)(now[4], now[5])):
            Tcur = Tguess
        Tmot = mul(inv(T_prev), Tcur)
        kd = (C.c_double * 3)(*xyt(mul(inv(keyframes[-1][0]), Tcur)))
        if lib.cfear_keyframe_based_fuse(kd, par.use_keyframe, par.min_keyframe_dist, par.min_keyframe_rot_deg):
            keyframes = (keyframes + [(Tcur, api.flip_ties(scan))])[-par.submap_scan_size:]
        T_prev = Tcur
        trace.append(xyt(Tcur))
    return np.array(trace)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--tol-xy", type=float, default=1e-9)
    ap.add_argument("--tol-theta", type=float, default=1e-10)
    a = ap.parse_args()
    import torch
    from tbv_slam_public_amd import api, synth, _lib as L
    imgs, _, _ = synth.scene_v1(0, a.frames)
    par = api.odometry_params()
    dev = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    od = api.OdometryKeyframeFuser(1, imgs.shape[1], imgs.shape[2], par)
    live = np.concatenate([od.process(dev[f:f + 1]).copy() for f in range(a.frames)])
    trace_a = live["pose"].copy()
    r = api.filter_kstrongest(dev, par.kstrong.k_strongest, par.kstrong.z_min, par.kstrong.range_res, par.kstrong.min_distance)
    n = r["n_points"].cpu().numpy()
    clouds = [r["xyzi"][f, :int(n[f])] for f in range(a.frames)]

    def show(name, rec):
        s = api.replay_summary(rec, a.tol_xy, a.tol_theta)
        print("%s: %d frames, %d without a job, %d equal, %d differing and flagged, %d differing and NOT flagged" %
              (name, s["n_frames"], s["n_no_job"], s["n_equal"], s["n_differ_exposed"], s["n_differ_not_exposed"]))
        print("  worst |dev|: equal %s, flagged %s, not flagged %s; first not flagged: %s" %
              tuple([np.array2string(s[k], precision=3) for k in ("worst_dev_equal", "worst_dev_differ_exposed", "worst_dev_differ_not_exposed")] +
                    [s["first_not_exposed"]]))
        return s
    rec_a = api.odometry_replay(clouds, trace_a, par)
    show("trace A (this library's own), replayed", rec_a)
    rec_sweeps = api.odometry_replay(dev, trace_a, par)
    print("  the sweep entry gives the same records:", rec_sweeps.tobytes() == rec_a.tobytes(),
          "; keyframes and counts equal to the live run:", bool(np.array_equal(rec_a["is_keyframe"], live["keyframe_added"]) and
                                                                np.array_equal(rec_a["n_cells"], live["n_cells"]) and
                                                                np.array_equal(rec_a["outer_iters"], live["outer_iters"])))
    trace_b = flipped_fuser(clouds, par, api, L)
    d = np.abs(trace_b - trace_a)
    print("trace B (every keyframe's ties decided the other way): |B - A| at the last frame %s, worst %s" %
          (np.array2string(d[-1], precision=3), np.array2string(d.max(axis=0), precision=3)))
    rec_b = api.odometry_replay(clouds, trace_b, par, audit=True)
    s = show("trace B, replayed with the audit", rec_b)
    differing = s["n_differ_exposed"] + s["n_differ_not_exposed"]
    print("  frames the audit flags: %d of %d; of the %d differing frames it flags %d (%.0f %%); differing without a flag (a tie at an "
          "intermediate association pass only, or none at the snapshots): %d" %
          (int((rec_b["exposed"] == 1).sum()), len(rec_b), differing, s["n_differ_exposed"],
           100.0 * s["n_differ_exposed"] / max(differing, 1), s["n_differ_not_exposed"]))


if __name__ == "__main__":
    main()
