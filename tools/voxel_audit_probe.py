"""Timing probe of cfear_voxel_order_audit_batch: --scans scans drawn from the k-strongest clouds (k = 40, z_min = 60) of one
scene_v1 ring of --frames sweeps -- the headline scene of bench.py -- through `offsets`, staged on the device once.  ms per
call from a host clock around calls that end in the read-back of their records (median of --reps after --warmup), and the
library's own kernel event times for the two launches.

  python tools/voxel_audit_probe.py --scans 4096 --reps 5
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe measures on an MI355X; there is nothing to time without one"
    from tbv_slam_public_amd import api, synth, _lib as L
    ctx = api.default_context()
    imgs, _, _ = synth.scene_v1(0, a.frames, circle_frames=a.frames)
    r = api.filter_kstrongest(torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), 40, 60, 0.0438, 2.5)
    n_pts = np.array([int(r["n_points"][b]) for b in range(a.frames)], np.int64)
    xyzi = torch.cat([r["xyzi"][b, :int(n_pts[b])] for b in range(a.frames)]).contiguous()
    starts = np.concatenate([[0], np.cumsum(n_pts)[:-1]]).astype(np.int64)
    pick = np.arange(a.scans) % a.frames
    offsets, lengths = np.ascontiguousarray(starts[pick]), np.ascontiguousarray(n_pts[pick].astype(np.int32))
    rec = np.zeros(a.scans, L.VOXEL_AUDIT_RECORD_DTYPE)
    par = L.VoxelAuditParams(3.0, 0.0, 1.0)
    rows = C.c_int64(0)
    torch.cuda.synchronize()

    def call():
        ctx.check(ctx._lib.cfear_voxel_order_audit_batch(ctx.h, xyzi.data_ptr(), offsets.ctypes.data, lengths.ctypes.data, a.scans, C.byref(par),
                                                         rec.ctypes.data, None, 0, C.byref(rows)))

    for _ in range(a.warmup):
        call()
    ctx.profile_enable(True)
    call()
    ctx.synchronize()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(scans=a.scans, mean_points=float(lengths.mean()), mean_voxels=float(rec["n_voxels"].mean()),
                          max_voxel_points=int(rec["max_voxel_points"].max()), ms_per_call=float(np.median(ms)), ms_all=ms,
                          kernel_event_ms={k: v[0] for k, v in prof.items()},
                          scans_exposed=int((rec["n_voxels_exposed"] > 0).sum()), scans_changed_reversed=int((rec["n_voxels_changed_reversed"] > 0).sum()),
                          max_halfwidth_median=float(np.median(rec["max_halfwidth"])), max_halfwidth_max=float(rec["max_halfwidth"].max()))))


if __name__ == "__main__":
    main()
