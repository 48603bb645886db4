"""Timing probe of cfear_odometry_grid: --sequences synthetic sequences x the 486 configurations of the reference's CFEAR-3
grid search (launch/oxford/eval/params/grid_search/oxford_cfear-3: 3 submap_scan_size x 3 res x 3 kstrong x 3 zmin x 3
loss_limit x 2 weight_option, in the order of utils/worker's loops) = 3888 streams, --frames frames, through ONE grid object.
Prints one JSON line: ms per grid step (host clock around calls that end in their read-back, --reps runs), the per-kernel
times of one profiled run (cfear_ctx_profile_read), the plan's sweeps, classes and groups, and beside it
  per_config   the same frames through one plain odometry object per configuration (--sequences streams each), for
               --plain-configs of the configurations one after another, scaled to all 486: what a grid costs without the grid
  single       a plain odometry object of 3888 streams with ONE configuration (CFEAR-3) on the same images: what the grouped
               launches and the shared sweep cost or save against the batch the headline measures
  pose_diff    the largest pose difference between the grid's streams and those plain objects (the matcher picks its form by
               the batch, so records may differ in the last bits; with one form forced they are identical, tests/
               test_gpu_odometry_grid.py)
The sweeps are every second azimuth of a 400-azimuth synthetic sweep (row r of a sweep of n azimuths looks along
2 pi (r + 1) / n, so rows 1, 3, 5, ... ARE a 200-azimuth sweep): k = 50 of the grid then stays within the 16 384 points per
scan the fused row-key hand-over takes (400 x 50 is beyond it, and such a grid is refused).

  python tools/grid_probe.py [--sequences 8 --frames 16 --reps 3 --plain-configs 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# grid_search/oxford_cfear-3, outermost loop first (utils/worker); everything else is the CFEAR-3 preset
GRID = dict(submap_scan_size=[4, 5, 6], res=[2.5, 2.75, 3.0], kstrong_k_strongest=[30, 40, 50], kstrong_z_min=[50.0, 60.0, 70.0],
            reg_loss_limit=[0.1, 0.2, 0.3], reg_weight_opt=[0, 4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plain-configs", type=int, default=16)
    ap.add_argument("--no-single", action="store_true", help="skip the 3888-stream single-configuration yardstick")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe measures on an MI355X; there is nothing to time without one"
    from tbv_slam_public_amd import api, synth
    Q, F = a.sequences, a.frames
    dev = torch.device("cuda:0")
    ctx = api.Context(0)                # a stream of its own: the grid deals its matcher groups to side streams only behind one
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        rings = torch.stack([synth.render_frames_torch(synth.Scene(2000 + q, circle_frames=4 * F), list(range(F)), dev) for q in range(Q)])
    finally:
        torch.use_deterministic_algorithms(was)
    frames = rings[:, :, 1::2, :].transpose(0, 1).contiguous()          # [F][Q][200][cols]
    del rings
    rows, cols = int(frames.shape[2]), int(frames.shape[3])
    torch.cuda.synchronize()
    configs = api.odometry_grid_configs("CFEAR-3", "oxford", **GRID)
    plan = api.odometry_grid_plan(rows, cols, configs, Q)
    S = plan["totals"]["n_streams"]

    def run(obj, images):
        """All frames through obj.process -> (seconds, poses [F][streams][3]); every call ends in its read-back."""
        t0 = time.perf_counter()
        poses = [obj.process(images(f))["pose"].copy() for f in range(F)]
        return time.perf_counter() - t0, np.stack(poses)

    # ---- the grid ----
    def grid_run():
        g = api.OdometryGrid(rows, cols, configs, Q, ctx=ctx)
        out = run(g, lambda f: frames[f])
        g.close()
        return out
    grid_run()                                                           # warm-up: workspaces, code objects
    grid_ms, grid_poses = [], None
    for _ in range(a.reps):
        t, grid_poses = grid_run()
        grid_ms.append(t / F * 1e3)
    ctx.profile_enable(True); ctx.profile_read(reset=True)
    grid_run()
    prof = ctx.profile_read(reset=True); ctx.profile_enable(False)
    kernels = {name: {"ms_per_step": round(ms / F, 4), "launches_per_step": cnt / F} for name, (ms, cnt) in sorted(prof.items())}

    # ---- one plain object per configuration, a sample of them one after another ----
    pick = sorted(set(np.linspace(0, len(configs) - 1, a.plain_configs).round().astype(int).tolist()))
    per_ms, diff_xy, diff_th = [], 0.0, 0.0
    for rep in range(a.reps + 1):                                        # the first pass warms up
        total = 0.0
        for c in pick:
            od = api.OdometryKeyframeFuser(Q, rows, cols, configs[c], ctx=ctx)
            t, poses = run(od, lambda f: frames[f])
            od.close()
            total += t
            if rep == 0:
                d = np.abs(grid_poses[:, np.arange(Q) * len(configs) + c] - poses)
                diff_xy, diff_th = max(diff_xy, float(d[..., :2].max())), max(diff_th, float(d[..., 2].max()))
        if rep > 0:
            per_ms.append(total / F * 1e3 * len(configs) / len(pick))

    # ---- one plain object of all the streams, one configuration ----
    single_ms = []
    if not a.no_single:
        seq_of = torch.from_numpy(plan["streams"]["sequence"].astype(np.int64)).to(dev)
        for rep in range(a.reps + 1):
            od = api.OdometryKeyframeFuser(S, rows, cols, api.odometry_preset("CFEAR-3"), ctx=ctx)
            t = 0.0
            for f in range(F):
                batch = frames[f].index_select(0, seq_of)                # [S][rows][cols], built outside the clock
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                od.process(batch)
                t += time.perf_counter() - t0
                del batch
            od.close()
            if rep > 0:
                single_ms.append(t / F * 1e3)

    rng = lambda v: [round(min(v), 3), round(max(v), 3)] if v else None
    print(json.dumps({
        "probe": "odometry grid", "sequences": Q, "configurations": len(configs), "streams": S, "frames": F, "azimuths": rows, "bins": cols,
        "plan": plan["totals"],
        "grid_ms_per_step": rng(grid_ms), "grid_registrations_per_s": round(S / (min(grid_ms) * 1e-3)),
        "per_config_ms_per_step_scaled": rng(per_ms), "per_config_sampled": len(pick),
        "single_config_ms_per_step": rng(single_ms),
        "speedup_over_per_config": round(min(per_ms) / max(grid_ms), 2) if per_ms else None,
        "derivation_off_ms_per_step": None,                              # no switch: the classes' row stride is part of the plan
        "pose_diff_vs_plain": {"xy_m": diff_xy, "theta_rad": diff_th},
        "kernels": kernels}))


if __name__ == "__main__":
    main()
