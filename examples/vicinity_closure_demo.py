#!/usr/bin/env python
"""Loop candidates from poses and odometry alone: TBV's GTVicinityClosure and MiniClosure on one synthetic lap.

  radar sweeps  -> CFEAR-3 odometry (OdometryKeyframeFuser); every keyframe leaves a graph node and the odometry
                   constraint of cfear_odometry_get_constraint                  as examples/slam_batch_demo.py
  the graph     -> api.closure_candidates, once per mode: for every origin node the later node that is nearby and has the
                   smallest distance / travelled-distance ratio, with its odometry bound   loopclosure.cpp:394-552, 776-806
  candidates    -> api.closure_verify_jobs -> api.verify_loop_candidates: registered, scored and classified in one call

GTVicinityClosure is how the reference finds the pairs it trains and evaluates its loop classifiers on; MiniClosure
(--miniloop-enabled) is its only generator that needs no descriptors.  The sensor drives a closed circle, so the last nodes
revisit the first ones; the accepted pairs are printed with their distance from the ground truth.
    python examples/vicinity_closure_demo.py [--frames 68] [--yaw-rate 0.45]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_closure_demo as demo          # noqa: E402


def run(n_frames=68, yaw_rate=0.45, log=None, **thresholds):
    """-> dict(poses [node, 3], gt [node, 3], constraints, modes = {mode: dict(candidates, jobs, results)}); keyword
    arguments override the closure thresholds of both modes."""
    from tbv_slam_public_amd import api
    sc = demo.circle_scene(yaw_rate=yaw_rate)
    gt = np.stack([sc.pose_at(f, n_frames) for f in range(n_frames)])
    gt = np.array([demo.xyt_compose(demo.xyt_inverse(gt[0]), g) for g in gt])
    od = api.OdometryKeyframeFuser(1, sc.rows, sc.cols, api.odometry_preset("CFEAR-3", "oxford", keep_nodes=1))
    poses, nodes, cons, kf = [], [], [], []
    for f in range(n_frames):
        info = od.process(sc.render(f, n_frames)[None])
        if not info["keyframe_added"][0]:
            continue
        nd = od.node(0)
        nodes.append(dict(scan=nd["scan"], peaks=nd["peaks"]))
        poses.append(info["pose"][0].copy())
        kf.append(f)
        c = od.constraint(0)                                                     # None for the first keyframe
        if c is not None:
            cons.append(c)
    od.close()
    poses, gt = np.array(poses), gt[kf]
    modes = {}
    for mode in ("gtvicinity", "mini"):
        cands = api.closure_candidates([(poses, cons)], mode=mode, **thresholds)[0]
        jobs = api.closure_verify_jobs(cands, nodes, poses)
        res = api.verify_loop_candidates(jobs)
        modes[mode] = dict(candidates=cands, jobs=jobs, results=res)
        if log:
            log("%s: %d of %d origins have a candidate, %d accepted" % (mode, len(jobs), len(poses), int(res["accepted"].sum())))
            for j, r in zip(jobs, res):
                if r["accepted"]:
                    true = demo.xyt_compose(demo.xyt_inverse(gt[j["from"]]), gt[j["to"]])
                    d = r["t_be"] - true
                    log("  loop %2d -> %2d  odom-bounds %.3f  p = %.3f  error vs ground truth %.2f m" % (
                        j["from"], j["to"], j["odom_bounds"], r["probability"], np.hypot(d[0], d[1])))
    return dict(poses=poses, gt=gt, constraints=cons, modes=modes)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=68)
    ap.add_argument("--yaw-rate", type=float, default=0.45)
    a = ap.parse_args()
    run(a.frames, a.yaw_rate, log=print)
