"""Timing probe of cfear_odometry_replay_clouds: --seqs sequences x --frames frames of bench.py's synthetic worlds (one
synth.Scene ring per sequence, k-strongest clouds with k = 40, z_min = 60 kept on the device) replayed along the trace that
live odometry (--seqs streams, cfear_odometry_process frame by frame) produced on the same sweeps.  Prints the milliseconds
of the live run and of the replay from a host clock around calls that end in their read-back (median of --reps), the
library's own kernel event times of one replay, and how the replayed poses compare with the trace.

  python tools/replay_probe.py --seqs 64 --frames 64
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe measures on an MI355X; there is nothing to time without one"
    from tbv_slam_public_amd import api, synth, _lib as L
    S, F = a.seqs, a.frames
    dev = torch.device("cuda:0")
    ctx = api.default_context()
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        rings = torch.stack([synth.render_frames_torch(synth.Scene(1000 + s, circle_frames=F), list(range(F)), dev) for s in range(S)])
    finally:
        torch.use_deterministic_algorithms(was)
    rows, cols = int(rings.shape[2]), int(rings.shape[3])
    frames = rings.transpose(0, 1).contiguous()                 # [F][S][rows][cols]: one batch of S sweeps per frame
    torch.cuda.synchronize()
    par = api.odometry_params()

    def live():
        od = api.OdometryKeyframeFuser(S, rows, cols, par)
        return np.stack([od.process(frames[f])["pose"].copy() for f in range(F)])      # [F][S][3]
    live()
    t0 = time.perf_counter()
    poses = live()
    live_ms = (time.perf_counter() - t0) * 1e3
    trace = np.ascontiguousarray(poses.transpose(1, 0, 2)).reshape(S * F, 3)            # sequences one behind the other
    clouds = []
    for s in range(S):
        r = api.filter_kstrongest(rings[s], par.kstrong.k_strongest, par.kstrong.z_min, par.kstrong.range_res, par.kstrong.min_distance)
        n = r["n_points"].cpu().numpy()
        clouds += [r["xyzi"][f, :int(n[f])] for f in range(F)]
    offs = np.arange(S + 1, dtype=np.int32) * F
    torch.cuda.synchronize()
    rec = api.odometry_replay(clouds, trace, par, seq_offsets=offs)
    ctx.profile_enable(True)
    api.odometry_replay(clouds, trace, par, seq_offsets=offs)
    ctx.synchronize()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        api.odometry_replay(clouds, trace, par, seq_offsets=offs)
        ms.append((time.perf_counter() - t0) * 1e3)
    s = api.replay_summary(rec, 1e-9, 1e-10, seq_offsets=offs)
    print(json.dumps(dict(seqs=S, frames=F, mean_points=float(rec["n_points"].mean()), mean_cells=float(rec["n_cells"].mean()),
                          keyframes=int(rec["is_keyframe"].sum()), live_ms=round(live_ms, 2), live_ms_per_frame_batch=round(live_ms / F, 3),
                          replay_ms=round(float(np.median(ms)), 2), replay_ms_all=[round(v, 2) for v in ms],
                          kernel_ms={k: round(v[0], 3) for k, v in sorted(prof.items())},
                          kernel_launches={k: int(v[1]) for k, v in sorted(prof.items())},
                          equal_1e9=s["n_equal"], differ=s["n_differ_not_exposed"], no_job=s["n_no_job"],
                          worst_dev=[float(v) for v in np.abs(rec["dev"]).max(axis=0)],
                          statuses={int(k): int(v) for k, v in zip(*np.unique(rec["reg_status"], return_counts=True))})))


if __name__ == "__main__":
    main()
