"""Which registrations of a lap hang on a nearest-neighbour tie, and by how much.

FLANN's 1-NN search returns ONE of several equidistant target cells; this library takes the lowest index, a reference build
may take another.  The demo drives one synthetic lap, makes the oriented surface points of every sweep
and runs api.tie_sensitivity on all consecutive pairs: each pair is audited at its start pose, registered as given,
registered again with every tie decided the other way, and audited at the registered pose -- four batched device calls for
the whole lap.  Once with the CFEAR-3 preset (P2P, Huber 0.1, weights from the cells' sample counts, directions and
planarity) and once with the loop-closure preset (P2L, uniform weights), for which a tie between cells that differ only in
their sample count cannot matter.

    python examples/tie_audit_demo.py [--seed 0] [--frames 24]

Prints the share of registrations with an effective tie -- a tie between cells that differ in something the residual or the
weight reads -- and the distribution of the spread between the two registered poses.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", type=int, default=24)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the demo runs on an MI355X; the library has no CPU path"
    from tbv_slam_public_amd import api, synth
    imgs, gt, _ = synth.scene_v1(a.seed, a.frames, circle_frames=a.frames)
    r = api.filter_kstrongest(torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), 40, 60, 0.0438, 2.5)
    scans = [api.MapPointNormal(r["xyzi"][b, :int(r["n_points"][b])].contiguous(), 3.0, (0.0, 0.0), True) for b in range(a.frames)]
    print("%d sweeps, %d .. %d cells each" % (a.frames, min(s.GetSize() for s in scans), max(s.GetSize() for s in scans)))
    jobs = []
    for i in range(a.frames - 1):                            # target at the origin, source at the true motion plus an error
        c, s = np.cos(gt[i][2]), np.sin(gt[i][2])
        d = gt[i + 1][:2] - gt[i][:2]
        guess = np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], gt[i + 1][2] - gt[i][2]]) + [0.3, -0.2, 0.01]
        jobs.append(([scans[i], scans[i + 1]], np.array([[0.0, 0.0, 0.0], guess])))
    for name, reg in (("CFEAR-3 (P2P, weight option 4)", api.n_scan_normal_reg("P2P", "Huber", 0.1, 4)),
                      ("loop closure (P2L, uniform weights)", api.n_scan_normal_reg("P2L", "Huber", 0.1, 0))):
        out = api.tie_sensitivity(jobs, reg)
        start, end = out["ties_start"], out["ties_end"]
        n = len(jobs)
        pos = out["delta"][:, :2].max(axis=1)
        print("%s: %d registrations" % (name, n))
        print("  queries with an exact tie: %.1f %% at the start pose, %.1f %% at the registered pose; largest group %d"
              % (100.0 * start["n_tied"].sum() / max(start["n_in_radius"].sum(), 1), 100.0 * end["n_tied"].sum() / max(end["n_in_radius"].sum(), 1),
                 max(int(start["max_group"].max()), int(end["max_group"].max()))))
        print("  registrations with an effective tie: %d (%.0f %%) at the start, %d (%.0f %%) at the end"
              % ((start["n_tied_effective"] > 0).sum(), 100.0 * (start["n_tied_effective"] > 0).mean(),
                 (end["n_tied_effective"] > 0).sum(), 100.0 * (end["n_tied_effective"] > 0).mean()))
        print("  spread between the two tie rules: median %.1e m, 90 %% %.1e m, worst %.1e m / %.1e rad; beyond 1e-6 m: %d, beyond 1e-4 m: %d"
              % (np.median(pos), np.quantile(pos, 0.9), pos.max(), out["delta"][:, 2].max(), (pos > 1e-6).sum(), (pos > 1e-4).sum()))


if __name__ == "__main__":
    main()
