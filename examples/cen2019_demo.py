"""One synthetic sweep pair through the Cen and Newman 2019 landmark detector (cen2019features, coral_alignment_quality
Utils.cpp:436-594) on the GPU, then the P2P alignment quality of the pair at its true and at a perturbed relative pose
(cfear_p2p_quality_batch; the clouds stay on the device).

    python examples/cen2019_demo.py [--seed 0] [--max-points 10000]

The reference's max_points = 1000 leaves a few dozen landmarks on a synthetic sweep (a landmark needs a marked neighbour in
an adjacent azimuth); the demo asks for 10000.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-points", type=int, default=10000)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the demo runs on an MI355X; the library has no CPU path"
    from tbv_slam_public_amd import api, synth
    imgs, gt, _ = synth.scene_v1(a.seed, 2)
    sweeps = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    r = api.filter_cen2019(sweeps, max_points=a.max_points, min_range_bins=0, range_res=0.0438, cap_points=65536, want_stats=True,
                           want_counts=True)
    clouds = []
    for b in range(2):
        n = int(r["n_points"][b])
        clouds.append(r["xyzi"][b, :n].contiguous())          # stays on the device
        mean, maxg, mean_h, last_h = (float(v) for v in r["image_stats"][b])
        cand, fresh, done = (int(v) for v in r["counts"][b])
        print("sweep %d: %d landmarks; mean %.4f, max gradient %.4f, mean_h %+.5f; %d candidates, %d fresh, %d gone through (last h %.4f)"
              % (b, n, mean, maxg, mean_h, cand, fresh, done, last_h))
    gt = np.asarray(gt, np.float64)                          # the sweeps' true poses (x, y, theta)
    jobs = [(clouds[0], tuple(gt[0]), clouds[1], tuple(gt[1]), off) for off in ((0.0, 0.0, 0.0), (0.8, 0.8, 0.05))]
    out, _ = api.p2p_quality_batch(jobs, 3.0)
    for name, res in zip(("true pose", "perturbed"), out):
        print("P2P %s: mean nearest-neighbour distance %.4f m over %d matched landmarks" % (name, float(res["mean"]), int(res["matched"])))


if __name__ == "__main__":
    main()
