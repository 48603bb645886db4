"""Which scans of a lap hang on the order in which pcl::VoxelGrid sums a voxel's points, and by how much.

PCL sorts (voxel, point) pairs with an unstable std::sort and sums each voxel's points sequentially in float; this library
sums them in input order, a reference build in whatever order libstdc++ leaves.  The demo drives one
synthetic lap, takes the k-strongest cloud of every sweep and audits all of them in one device call
(api.voxel_order_audit): per scan, whether ANY order of any voxel could move a point across the radius of a centroid
(n_voxels_exposed -- an upper bracket, from an enclosure of every order's centroid) and whether the reversed order does
(n_voxels_changed_reversed -- a lower bracket).  Every pair of consecutive sweeps with a flagged scan is then registered
twice, from the clouds as given and from the reversed clouds (api.voxel_order_spread).

    python examples/voxel_order_demo.py [--seed 0] [--frames 48]

Prints the share of scans no order can change, the share the reversed order does change, the distribution of the
enclosure's largest half-width and the spread of the flagged registrations.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", type=int, default=48)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the demo runs on an MI355X; the library has no CPU path"
    from tbv_slam_public_amd import api, synth
    imgs, gt, _ = synth.scene_v1(a.seed, a.frames, circle_frames=a.frames)
    r = api.filter_kstrongest(torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), 40, 60, 0.0438, 2.5)
    clouds = [r["xyzi"][b, :int(r["n_points"][b])].contiguous() for b in range(a.frames)]
    rec = api.voxel_order_audit(clouds, 3.0, 1.0)
    assert (rec["status"] == 0).all()
    n = len(rec)
    print("%d sweeps, %d .. %d points and %d .. %d voxels each, at most %d points in a voxel"
          % (n, rec["n_points"].min(), rec["n_points"].max(), rec["n_voxels"].min(), rec["n_voxels"].max(), rec["max_voxel_points"].max()))
    print("  no order can change a cell (n_voxels_exposed == 0): %d scans (%.0f %%)"
          % ((rec["n_voxels_exposed"] == 0).sum(), 100.0 * (rec["n_voxels_exposed"] == 0).mean()))
    print("  the reversed order changes a cell (n_voxels_changed_reversed > 0): %d scans (%.0f %%)"
          % ((rec["n_voxels_changed_reversed"] > 0).sum(), 100.0 * (rec["n_voxels_changed_reversed"] > 0).mean()))
    print("  exposed voxels per scan: median %d, worst %d of %d; at the six-point threshold: %d scans; centroids the reversed order moves: %.0f %%"
          % (np.median(rec["n_voxels_exposed"]), rec["n_voxels_exposed"].max(), rec["n_voxels"][rec["n_voxels_exposed"].argmax()],
             (rec["n_voxels_exposed_at_threshold"] > 0).sum(), 100.0 * rec["n_centroids_reversed_differ"].sum() / rec["n_voxels"].sum()))
    hw = rec["max_halfwidth"]
    print("  largest half-width of the enclosure per scan: min %.1e m, median %.1e m, 90 %% %.1e m, max %.1e m"
          % (hw.min(), np.median(hw), np.quantile(hw, 0.9), hw.max()))
    host = [c.cpu().numpy() for c in clouds]
    reg = api.n_scan_normal_reg("P2P", "Huber", 0.1, 4)      # CFEAR-3
    flagged = [i for i in range(n - 1) if rec["n_voxels_exposed"][i] > 0 or rec["n_voxels_exposed"][i + 1] > 0]
    deltas, witnessed = [], []
    for i in flagged:                                        # target at the origin, source at the true motion plus an error
        c, s = np.cos(gt[i][2]), np.sin(gt[i][2])
        d = gt[i + 1][:2] - gt[i][:2]
        guess = np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], gt[i + 1][2] - gt[i][2]]) + [0.3, -0.2, 0.01]
        out = api.voxel_order_spread(([host[i], host[i + 1]], np.array([[0.0, 0.0, 0.0], guess])), reg)
        deltas.append(out["delta"])
        witnessed.append(bool((out["audit"]["n_voxels_changed_reversed"] > 0).any()))
    print("  consecutive pairs with a flagged scan: %d of %d, %d of them with a witness" % (len(flagged), n - 1, sum(witnessed)))
    if deltas:
        deltas = np.array(deltas)
        pos = deltas[:, :2].max(axis=1)
        print("  spread between input order and its reverse (CFEAR-3): median %.1e m, 90 %% %.1e m, worst %.1e m / %.1e rad; beyond 1e-6 m: %d, "
              "beyond 1e-4 m: %d" % (np.median(pos), np.quantile(pos, 0.9), pos.max(), deltas[:, 2].max(), (pos > 1e-6).sum(), (pos > 1e-4).sum()))
        w = np.array(witnessed)
        if w.any():
            print("    with a witness: worst %.1e m;  without: worst %.1e m" % (pos[w].max(), pos[~w].max() if (~w).any() else 0.0))


if __name__ == "__main__":
    main()
