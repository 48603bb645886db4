"""One synthetic sweep pair through the Cen and Newman 2018 landmark detector (Cen2018Radar, coral_alignment_quality
ScanType.cpp:68-88) on the GPU, then the two stages that consume such a cloud: oriented surface points (cfear_scan_create)
and the CorAl alignment quality of the pair at its true and at a perturbed relative pose.

    python examples/cen2018_demo.py [--seed 0] [--zq 5.0]

The reference's zq = 3.0 gives about 20 000 landmarks on a synthetic sweep; one CorAl job holds 16 384 points for the pair,
so the demo raises the threshold (about 3 500 landmarks per sweep at 5.0).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--zq", type=float, default=5.0)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the demo runs on an MI355X; the library has no CPU path"
    from tbv_slam_public_amd import api, synth
    imgs, gt, _ = synth.scene_v1(a.seed, 2)
    sweeps = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    r = api.filter_cen2018(sweeps, zq=a.zq, sigma_gauss=17, min_range_bins=2, range_res=0.0438, cap_points=65536, want_stats=True)
    clouds = []
    for b in range(2):
        n = int(r["n_points"][b])
        clouds.append(r["xyzi"][b, :n].contiguous())          # stays on the device
        st = r["row_stats"][b]
        print("sweep %d: %d landmarks, row sigma %.4f .. %.4f" % (b, n, float(st[:, 1].min()), float(st[:, 1].max())))
        scan = api.MapPointNormal(clouds[b], 3.0)
        print("         %d oriented surface points" % scan.GetSize())
    gt = np.asarray(gt, np.float64)                          # the sweeps' true poses (x, y, theta)
    for name, pose in (("true pose", gt[1]), ("perturbed", gt[1] + np.array([0.8, 0.8, 0.05]))):
        q = api.CorAlRadarQuality(clouds[0], tuple(gt[0]), clouds[1], tuple(float(v) for v in pose))
        j, s, o = q.GetQualityMeasure()
        print("CorAl %s: joint %.4f  separate %.4f  overlap %.3f  (joint - separate = %+.4f)" % (name, j, s, o, j - s))


if __name__ == "__main__":
    main()
