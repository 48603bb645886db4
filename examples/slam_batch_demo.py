#!/usr/bin/env python
"""Sweeps in, corrected and scored trajectories out: N synthetic laps, every stage one batched device call.

  radar sweeps  -> CFEAR-3 odometry of all laps at once (OdometryKeyframeFuser, one stream per lap); every keyframe
                   leaves a graph node and the odometry constraint of cfear_odometry_get_constraint
  all laps      -> the Scan Context loop candidates of every graph in ONE call (api.sc_detect_batch)
  all laps      -> every candidate registered, scored and classified in one call (api.verify_loop_candidates)
  all laps      -> every pose graph solved in ONE call (api.pose_graph_optimize_batch, one wavefront per graph)
  all laps      -> raw and corrected trajectories scored by ONE api.eval_trajectories call (KITTI odometry metric)

The laps are the closed circle of examples/loop_closure_demo.py with different landmark seeds.  --loop-scaling weighs the
loops: the reference's 500000 leaves the graph leaning on odometry, 1 trusts the verified loops as much as a step.
--device-rows keeps the detector's rows in HBM and lets api.verify_sc_rows turn them into verified candidates there (the row
mapping, the guess, the odometry bound, registration and verification in one call): detect -> verify -> solve, no candidate
crosses to the host before it is verified.  --sampled-covariances (with --device-rows) adds api.verify_sample_covariances
behind it -- use_covariance_sampling_in_loop_closure, sampled and fitted on the device -- so that an accepted loop carries
information = inv(cov), and solves with the constraints' own information (replace_cov_by_identity = 0).
    python examples/slam_batch_demo.py [--laps 3] [--frames 68] [--loop-scaling 1] [--device-rows [--sampled-covariances]]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_closure_demo as demo          # noqa: E402


def _verify_device_rows(api, nodes, poses, n_detect, sampled=False):
    """detect -> verify with the rows left on the device [-> sampled covariances] -> (candidates [(lap, from, to)], accepted loops
    per lap, how many of them carry a sampled covariance)."""
    n_laps = len(nodes)
    flat = api.sc_flatten_graphs([([nd["peaks"] for nd in nodes[lap]], poses[lap]) for lap in range(n_laps)])
    rows, n_out, _ = api.sc_detect_batch(flat=flat, n_aggregate=1, n_detect=n_detect, device_out=True)
    all_poses = np.concatenate(poses)
    graphs = dict(node_off=flat["node_off"], table=api.ScanTable([nd["scan"] for lap in range(n_laps) for nd in nodes[lap]]),
                  xyzi=flat["xyzi"], point_off=flat["point_off"], poses=all_poses,
                  rel=api.loop_relative_motions(all_poses, flat["node_off"]))
    out = api.verify_sc_rows(graphs, rows, n_out, n_detect)
    if sampled:
        api.verify_sample_covariances(graphs, out)
    loops = [[] for _ in range(n_laps)]
    n_sampled = 0
    for c, r in zip(out["list"], out["results"]):
        if r["accepted"]:
            # the reference stores information = Cov.inverse().  Register's constant covariance has no inverse and keeps the
            # identity; so does a sampled one that the reference's rotation (the x-y-z block alone, loopclosure.cpp:93) has left
            # indefinite, which the solver would refuse
            use = bool(r["cov_sampled"]) and np.linalg.eigvalsh(r["cov"]).min() > 0
            info = np.linalg.inv(r["cov"]) if use else np.eye(6)
            n_sampled += int(use)
            loops[c["graph"]].append(dict(id_begin=int(c["from"]), id_end=int(c["to"]), t_be=r["t_be"].copy(), information=info, type=1))
    return [(int(c["graph"]), int(c["from"]), int(c["to"])) for c in out["list"]], loops, n_sampled


def run(n_laps=3, n_frames=68, loop_scaling=1.0, log=None, per_lap_scan_context=False, device_rows=False, narrow_sc_sim=False,
        sampled_covariances=False):
    """-> dict(raw, corrected, gt [lap][node, 3], keyframes [lap] frame indices, candidates [(lap, from, to)], loops [lap] accepted
    constraints, pgo [lap] summaries, before, after).  per_lap_scan_context: one api.sc_detect_sequence call per lap, the loop the
    batch call replaced (the candidates are the same).  device_rows: the rows stay on the device and api.verify_sc_rows verifies them
    there.  narrow_sc_sim: the host loop passes (double)(float)min_dist as the reference does (loopclosure.cpp:677) and as
    verify_sc_rows always does.  sampled_covariances (device_rows only): the accepted loops carry the inverse of their sampled
    covariance and the solve uses every constraint's own information; the dict gains n_sampled."""
    from tbv_slam_public_amd import api
    if sampled_covariances and not device_rows:
        raise ValueError("sampled_covariances needs device_rows")
    backend = demo.HipBackend()
    scenes = [demo.circle_scene(seed=21 + lap) for lap in range(n_laps)]
    gt = []
    for sc in scenes:
        g = np.stack([sc.pose_at(f, n_frames) for f in range(n_frames)])
        gt.append(np.array([demo.xyt_compose(demo.xyt_inverse(g[0]), x) for x in g]))
    # ---- odometry of all laps, one stream each; nodes and odometry constraints as the keyframes arrive ------------------
    od = api.OdometryKeyframeFuser(n_laps, scenes[0].rows, scenes[0].cols, api.odometry_preset("CFEAR-3", "oxford", keep_nodes=1))
    raw = np.zeros((n_laps, n_frames, 3))
    kf = [[] for _ in range(n_laps)]                                             # the frames that became keyframes = graph nodes
    nodes = [[] for _ in range(n_laps)]
    cons = [[] for _ in range(n_laps)]
    for f in range(n_frames):
        imgs = np.stack([sc.render(f, n_frames) for sc in scenes])
        info = od.process(imgs)
        raw[:, f] = info["pose"]
        for lap in range(n_laps):
            if not info["keyframe_added"][lap]:
                continue
            nd = od.node(lap)
            nodes[lap].append(dict(scan=nd["scan"], peaks=nd["peaks"]))
            kf[lap].append(f)
            c = od.constraint(lap)                                               # None for a stream's first keyframe
            if c is not None:
                cons[lap].append(c)
    od.close()
    poses = [raw[lap, kf[lap]] for lap in range(n_laps)]                         # node poses; ids = keyframe ordinals 0, 1, 2, ...
    gt = [gt[lap][kf[lap]] for lap in range(n_laps)]
    # ---- loop candidates of all graphs in ONE call, then ONE verification call for all laps ------------------------------
    cands, owner = [], []
    n_detect = [len(kf[lap]) - 1 for lap in range(n_laps)]
    if device_rows:
        found_all = []
        cand_ids, loops, n_sampled = _verify_device_rows(api, nodes, poses, n_detect, sampled_covariances)
    elif per_lap_scan_context:
        found_all = [api.sc_detect_sequence([nd["peaks"] for nd in nodes[lap]], poses[lap], n_aggregate=1, n_detect=n_detect[lap])
                     for lap in range(n_laps)]
    else:
        found_all = api.sc_detect_batch([([nd["peaks"] for nd in nodes[lap]], poses[lap]) for lap in range(n_laps)], n_aggregate=1,
                                        n_detect=n_detect)
    for lap, found in enumerate(found_all):
        for i, group in enumerate(found):
            for c in group:
                to = c["nn_idx"]
                rel = [demo.xyt_compose(demo.xyt_inverse(poses[lap][k]), poses[lap][k + 1]) for k in range(to, i)]
                guess = demo.xyt_compose(demo.xyt_inverse(np.asarray(c["Taug"], np.float64)), np.array([0.0, 0.0, c["yaw_diff_rad"]]))
                sim = float(np.float32(c["min_dist"])) if narrow_sc_sim else c["min_dist"]
                cands.append({"from": i, "to": to, "from_pose": poses[lap][i], "t_be_guess": guess, "sc_sim": sim,
                              "odom_bounds": backend.odom_bounds(np.array(rel).reshape(-1, 3))})
                owner.append(lap)
    jobs = [dict(from_scan=nodes[lap][c["from"]]["scan"], to_scan=nodes[lap][c["to"]]["scan"], from_peaks=nodes[lap][c["from"]]["peaks"],
                 to_peaks=nodes[lap][c["to"]]["peaks"], from_pose=c["from_pose"], t_be_guess=c["t_be_guess"], sc_sim=c["sc_sim"],
                 odom_bounds=c["odom_bounds"], group=lap * n_frames + c["from"]) for lap, c in zip(owner, cands)]
    res = api.verify_loop_candidates(jobs) if jobs else None
    if not device_rows:
        loops = [[] for _ in range(n_laps)]
        cand_ids = [(lap, c["from"], c["to"]) for lap, c in zip(owner, cands)]
    for k, (lap, c) in enumerate(zip(owner, cands)):
        if res is not None and res["accepted"][k]:
            # the odometry constraints number the keyframes 0, 1, 2, ... per stream: so do the loops
            loops[lap].append(dict(id_begin=c["from"], id_end=c["to"], t_be=res["t_be"][k].copy(), information=np.eye(6), type=1))
    # ---- every graph in one solve, every trajectory in one evaluation ---------------------------------------------------
    graphs = [(poses[lap], np.arange(len(kf[lap])), cons[lap] + loops[lap]) for lap in range(n_laps)]
    own = {}
    if sampled_covariances:
        # every constraint's own information.  An odometry constraint's is the inverse of Register's constant covariance on
        # (x, y, yaw) and zero on z, roll and pitch, which a planar graph never moves: a unit weight there makes it definite
        own = dict(replace_cov_by_identity=0)
        for lap in range(n_laps):
            for c in cons[lap]:
                info = np.array(c["information"], np.float64)
                for k in (2, 3, 4):
                    if info[k, k] == 0.0:
                        info[k, k] = 1.0
                c["information"] = info
    solved = api.pose_graph_optimize_batch(graphs, loop_scaling=loop_scaling, **own)
    corrected = []
    for out, _ in solved:
        xyt = np.zeros((len(out), 3))
        for i, p in enumerate(out):
            xyt[i] = [p[0], p[1], 2.0 * np.arctan2(p[5], p[6])]
        corrected.append(xyt)
    est = [api.kitti_from_xyt(poses[lap]) for lap in range(n_laps)] + [api.kitti_from_xyt(c) for c in corrected]
    summaries, _ = api.eval_trajectories(est, [api.kitti_from_xyt(g) for g in gt] * 2, alignment="none", want_rows=False)
    if log:
        log("lap  nodes  odometry constraints  loops  LM iterations  end-point gap raw -> corrected (m)   ATE raw -> corrected (m)")
        for lap in range(n_laps):
            gap = [np.hypot(*(t[-1, :2] - gt[lap][-1, :2])) for t in (poses[lap], corrected[lap])]
            log("%3d %6d %21d %6d %14d %18.3f -> %.3f %22.3f -> %.3f" % (lap, len(kf[lap]), len(cons[lap]), len(loops[lap]), solved[lap][1]["iterations"],
                                                                   gap[0], gap[1], summaries[lap]["ate"], summaries[n_laps + lap]["ate"]))
    out = dict(raw=poses, keyframes=kf, corrected=corrected, gt=gt, candidates=cand_ids,
               loops=loops, pgo=[s for _, s in solved], before=summaries[:n_laps], after=summaries[n_laps:])
    if sampled_covariances:
        out["n_sampled"] = n_sampled
        if log:
            log("sampled covariances: %d of %d accepted loops carry information = inv(cov); mean ATE %.3f -> %.3f m" % (
                n_sampled, sum(len(l) for l in loops), np.mean([s["ate"] for s in summaries[:n_laps]]), np.mean([s["ate"] for s in summaries[n_laps:]])))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=68)
    ap.add_argument("--loop-scaling", type=float, default=1.0)
    ap.add_argument("--device-rows", action="store_true", help="keep the Scan Context rows on the device: detect -> verify_sc_rows -> solve")
    ap.add_argument("--sampled-covariances", action="store_true",
                    help="with --device-rows: sample the accepted loops' covariances on the device and solve with the constraints' own information")
    a = ap.parse_args()
    run(a.laps, a.frames, a.loop_scaling, log=print, device_rows=a.device_rows, sampled_covariances=a.sampled_covariances)
