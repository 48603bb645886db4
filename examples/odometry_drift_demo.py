#!/usr/bin/env python
"""Odometry drift of a handful of synthetic streams, scored the way the reference scores itself.

Every stream is one synth.Scene; OdometryKeyframeFuser advances all of them per call, the poses go through
api.kitti_from_xyt, and ONE api.eval_trajectories call returns the KITTI odometry figures of every stream
(radar_kitti_benchmark/python/eval_odom.py --align 6dof): drift in % and deg / 100 m over the 100 ... 800 m segments, ATE and
RPE.  The ground truth is synth.Scene.pose_at.  A stream shorter than 100 m has no segment: its drift figures are 0 and only
ATE / RPE say something -- raise --frames (about 1.6 m per frame) to get segments.

    python examples/odometry_drift_demo.py --streams 4 --frames 12"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--alignment", default="6dof", choices=["none", "6dof"])
    args = ap.parse_args()
    import torch
    from tbv_slam_public_amd import api, synth
    scenes = [synth.Scene(seed) for seed in range(args.streams)]
    od = api.OdometryKeyframeFuser(args.streams, scenes[0].rows, scenes[0].cols)
    est = np.zeros((args.streams, args.frames, 3))
    for f in range(args.frames):
        imgs = np.stack([sc.render(f, args.frames) for sc in scenes])
        est[:, f] = od.process(torch.from_numpy(imgs).cuda())["pose"]
    gt = np.stack([[sc.pose_at(f, args.frames) for f in range(args.frames)] for sc in scenes])
    summaries, rows = api.eval_trajectories(list(api.kitti_from_xyt(est)), list(api.kitti_from_xyt(gt)), alignment=args.alignment)
    print("stream  poses  rows  transl.err(%)  rot.err(deg/100m)   ATE(m)   RPE(m)  RPE(deg)")
    for k, s in enumerate(summaries):
        print("%6d %6d %5d %14.5f %18.5f %8.5f %8.5f %9.5f" % (k, s["n_poses"], s["n_rows"], s["ave_t_err"] * 100,
              s["ave_r_err"] / np.pi * 180 * 100, s["ate"], s["rpe_trans"], s["rpe_rot"] * 180 / np.pi))


if __name__ == "__main__":
    main()
