#!/usr/bin/env python
"""Sweeps in, aligned trajectories, graph.txt and the map out: the end of the reference's SLAM run for N synthetic laps.

The stages of examples/slam_batch_demo.py (odometry of all laps at once, loop candidates per graph, one verification call, one
batched pose-graph solve), then what tbv_slam_offline ends in, per lap:

  all laps  -> PoseGraph::Align of the raw and of the solved graphs in ONE call (api.graph_align_batch): the mean distance
               to the ground truth before and after the solve
  per lap   -> graph.txt (PoseGraph.SaveGraphString) and est/00.txt, gt/00.txt (PoseGraph.OutputGraph) under --out/lap<k>/
  all laps  -> the map of every lap, each node's peak cloud carried into the world by its solved and aligned pose, and the
               ground-truth map beside it, in ONE call (api.graph_map_batch)

    python examples/slam_map_demo.py [--laps 3] [--frames 68] [--loop-scaling 1] [--skip-frames 1] [--out /tmp/slam_map_demo]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_closure_demo as demo          # noqa: E402


def solve_laps(n_laps, n_frames, loop_scaling):
    """slam_batch_demo's pipeline, keeping what the end of the run needs -> (raw, solved [lap][node, 7], gt [lap][node, 3],
    peaks [lap][node] float32 [k, 4], stamps [lap][node], loops [lap])."""
    from tbv_slam_public_amd import api
    backend = demo.HipBackend()
    scenes = [demo.circle_scene(seed=21 + lap) for lap in range(n_laps)]
    gt = []
    for sc in scenes:
        g = np.stack([sc.pose_at(f, n_frames) for f in range(n_frames)])
        gt.append(np.array([demo.xyt_compose(demo.xyt_inverse(g[0]), x) for x in g]))
    od = api.OdometryKeyframeFuser(n_laps, scenes[0].rows, scenes[0].cols, api.odometry_preset("CFEAR-3", "oxford", keep_nodes=1))
    raw = np.zeros((n_laps, n_frames, 3))
    kf, nodes, cons = [[] for _ in range(n_laps)], [[] for _ in range(n_laps)], [[] for _ in range(n_laps)]
    for f in range(n_frames):
        info = od.process(np.stack([sc.render(f, n_frames) for sc in scenes]))
        raw[:, f] = info["pose"]
        for lap in range(n_laps):
            if not info["keyframe_added"][lap]:
                continue
            nd = od.node(lap)
            nodes[lap].append(dict(scan=nd["scan"], peaks=nd["peaks"]))
            kf[lap].append(f)
            c = od.constraint(lap)
            if c is not None:
                cons[lap].append(c)
    od.close()
    poses = [raw[lap, kf[lap]] for lap in range(n_laps)]
    gt = [gt[lap][kf[lap]] for lap in range(n_laps)]
    cands, owner = [], []
    found_all = api.sc_detect_batch([([nd["peaks"] for nd in nodes[lap]], poses[lap]) for lap in range(n_laps)], n_aggregate=1,
                                    n_detect=[len(kf[lap]) - 1 for lap in range(n_laps)])
    for lap, found in enumerate(found_all):
        for i, group in enumerate(found):
            for c in group:
                to = c["nn_idx"]
                rel = [demo.xyt_compose(demo.xyt_inverse(poses[lap][k]), poses[lap][k + 1]) for k in range(to, i)]
                guess = demo.xyt_compose(demo.xyt_inverse(np.asarray(c["Taug"], np.float64)), np.array([0.0, 0.0, c["yaw_diff_rad"]]))
                cands.append({"from": i, "to": to, "from_pose": poses[lap][i], "t_be_guess": guess, "sc_sim": c["min_dist"],
                              "odom_bounds": backend.odom_bounds(np.array(rel).reshape(-1, 3))})
                owner.append(lap)
    jobs = [dict(from_scan=nodes[lap][c["from"]]["scan"], to_scan=nodes[lap][c["to"]]["scan"], from_peaks=nodes[lap][c["from"]]["peaks"],
                 to_peaks=nodes[lap][c["to"]]["peaks"], from_pose=c["from_pose"], t_be_guess=c["t_be_guess"], sc_sim=c["sc_sim"],
                 odom_bounds=c["odom_bounds"], group=lap * n_frames + c["from"]) for lap, c in zip(owner, cands)]
    res = api.verify_loop_candidates(jobs) if jobs else None
    loops = [[] for _ in range(n_laps)]
    for k, (lap, c) in enumerate(zip(owner, cands)):
        if res is not None and res["accepted"][k]:
            loops[lap].append(dict(id_begin=c["from"], id_end=c["to"], t_be=res["t_be"][k].copy(), information=np.eye(6), type=1))
    solved = api.pose_graph_optimize_batch([(poses[lap], np.arange(len(kf[lap])), cons[lap] + loops[lap]) for lap in range(n_laps)],
                                           loop_scaling=loop_scaling)
    to_host = lambda p: p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p)
    peaks = [[np.ascontiguousarray(to_host(nd["peaks"]), np.float32).reshape(-1, 4) for nd in nodes[lap]] for lap in range(n_laps)]
    stamps = [[1547131046000000000 + 250000000 * f for f in kf[lap]] for lap in range(n_laps)]       # 4 Hz sweeps
    return poses, [s[0] for s in solved], gt, peaks, stamps, loops


def run(n_laps=3, n_frames=68, loop_scaling=1.0, skip_frames=1, out_dir=None, log=None):
    """-> dict(ate_raw, ate_solved [lap], graphs [lap] aligned api.PoseGraph, map, map_gt, ranges)."""
    from tbv_slam_public_amd import api
    raw, solved, gt, peaks, stamps, loops = solve_laps(n_laps, n_frames, loop_scaling)
    # ---- Align: the raw and the solved graph of every lap in one call ---------------------------------------------------
    aligned = api.graph_align_batch([(raw[lap], gt[lap]) for lap in range(n_laps)] + [(solved[lap], gt[lap]) for lap in range(n_laps)])
    graphs = []
    for lap in range(n_laps):
        d = os.path.join(out_dir, "lap%d" % lap) if out_dir else None
        g = api.PoseGraph(poses=aligned[n_laps + lap][0], gt=gt[lap], stamps=stamps[lap], clouds=peaks[lap],
                          est_output_dir=os.path.join(d, "est") if d else ".", gt_output_dir=os.path.join(d, "gt") if d else ".")
        if d:
            os.makedirs(d, exist_ok=True)
            g.SaveGraphString(os.path.join(d, "graph.txt"))
            g.OutputGraph()
        graphs.append(g)
    # ---- the maps of all laps in one call ----------------------------------------------------------------------------------
    m, mg, ranges = api.graph_map_batch(graphs, skip_frames=skip_frames)
    if log:
        log("lap  nodes  loops  ATE raw -> solved (m, mean, after Align)  map points  extent x (m)        extent y (m)")
        for lap in range(n_laps):
            r = ranges[lap]
            pts = m[r["map_offset"]:r["map_offset"] + r["map_points"]]
            ext = (pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()) if len(pts) else (0.0,) * 4
            log("%3d %6d %6d %12.3f -> %.3f %32d  %8.1f .. %-8.1f %8.1f .. %-8.1f" % (
                lap, graphs[lap].size(), len(loops[lap]), aligned[lap][1]["ate"], aligned[n_laps + lap][1]["ate"], len(pts), *ext))
        if out_dir:
            log("graph.txt, est/00.txt and gt/00.txt of every lap are under %s" % out_dir)
    return dict(ate_raw=[aligned[lap][1]["ate"] for lap in range(n_laps)], ate_solved=[aligned[n_laps + lap][1]["ate"] for lap in range(n_laps)],
                graphs=graphs, map=m, map_gt=mg, ranges=ranges)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=68)
    ap.add_argument("--loop-scaling", type=float, default=1.0)
    ap.add_argument("--skip-frames", type=int, default=1)
    ap.add_argument("--out", default="/tmp/slam_map_demo")
    a = ap.parse_args()
    run(a.laps, a.frames, a.loop_scaling, a.skip_frames, a.out, log=print)
