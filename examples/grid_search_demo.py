#!/usr/bin/env python
"""A small parameter grid search, the way the reference runs its own (launch/oxford/eval/1_baseline and
params/grid_search/): every configuration on every sequence, scored with the KITTI odometry metric, one table row per
configuration.

Two synthetic laps x a grid over (k_strongest, z_min, res, loss_limit) go through ONE api.OdometryGrid: per frame each
lap's sweep is swept once for all of its configurations, the surface and matcher stages run once per group of equal
parameters, and one read-back returns every stream's pose.  ONE api.eval_trajectories call then scores every (sequence,
configuration) trajectory against synth.Scene.pose_at, and the table shows each configuration's drift averaged over the laps
(what evaluation/1_baseline tabulates per parameter set).  A lap shorter than 100 m has no KITTI segment: its drift figures
are 0 and ATE / RPE say something -- raise --frames (about 2.5 m per frame) to get segments.

    python examples/grid_search_demo.py --frames 12"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--alignment", default="6dof", choices=["none", "6dof"])
    args = ap.parse_args()
    import torch
    from tbv_slam_public_amd import api, synth
    grid_lists = dict(kstrong_k_strongest=[12, 40], kstrong_z_min=[60.0, 70.0], res=[3.0, 3.5], reg_loss_limit=[0.1, 0.3])
    configs = api.odometry_grid_configs("CFEAR-3", "oxford", **grid_lists)
    scenes = [synth.Scene(seed) for seed in (21, 22)]
    Q, K, F = len(scenes), len(configs), args.frames
    plan = api.odometry_grid_plan(scenes[0].rows, scenes[0].cols, configs, Q)["totals"]
    print("%d sequences x %d configurations = %d streams: %d sweeps per frame, %d filter classes, %d surface groups, %d matcher groups"
          % (Q, K, plan["n_streams"], plan["n_sweeps"], plan["n_classes"], plan["n_surface_groups"], plan["n_matcher_groups"]))
    grid = api.OdometryGrid(scenes[0].rows, scenes[0].cols, configs, Q)
    est = np.zeros((Q * K, F, 3))
    for f in range(F):
        imgs = np.stack([sc.render(f, F) for sc in scenes])
        est[:, f] = grid.process(torch.from_numpy(imgs).cuda())["pose"]          # stream s = sequence s // K, configuration s % K
    grid.close()
    gt = np.stack([[sc.pose_at(f, F) for f in range(F)] for sc in scenes])
    summaries, _ = api.eval_trajectories(list(api.kitti_from_xyt(est)), list(api.kitti_from_xyt(gt[np.arange(Q * K) // K])),
                                         alignment=args.alignment)
    print("  k  zmin  res  loss_limit  transl.err(%)  rot.err(deg/100m)   ATE(m)   RPE(m)  RPE(deg)")
    per = {name: np.asarray(summaries[name]).reshape(Q, K).mean(0) for name in ("ave_t_err", "ave_r_err", "ate", "rpe_trans", "rpe_rot")}
    for c, p in enumerate(configs):
        print("%3d %5.0f %4.1f %11.2f %14.5f %18.5f %8.5f %8.5f %9.5f" % (
            p.kstrong.k_strongest, p.kstrong.z_min, p.res, p.reg.loss_limit, per["ave_t_err"][c] * 100,
            per["ave_r_err"][c] / np.pi * 180 * 100, per["ate"][c], per["rpe_trans"][c], per["rpe_rot"][c] * 180 / np.pi))
    best = int(np.argmin(per["ate"]))
    print("lowest ATE: configuration %d (job_%d and job_%d of the reference's numbering)" % (best, best + 1, K + best + 1))


if __name__ == "__main__":
    main()
