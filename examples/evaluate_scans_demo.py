"""evaluate_scans on one synthetic lap: every sweep through the Cen and Newman 2018 landmark detector with its cloud left on
the device, then scanEvaluator with method "P2P" -- every consecutive pair at the aligned offset and at the misaligned
ones, all of them in ONE batched call -- and eval.txt as the reference's tool writes it.

    python examples/evaluate_scans_demo.py [--frames 12] [--zq 5.0] [--out eval.txt]

Prints the share of pairs whose aligned row has the smallest score1 (the mean nearest squared distance).

    python examples/evaluate_scans_demo.py --scan-type kstrongCart

scores the same lap as CartesianRadar scans instead (classify_oxford.sh's --scan-type kstrongCart): every sweep resampled
into a 300 x 300 Cartesian image on the device, CorAlCartQuality -- the sum of absolute differences between the reference
image and the source image warped by the offset -- as the measure, and the share of pairs in which the aligned offset has
the lowest abs_diff.  That measure reads no pose but the offset (both poses come from the source scan in the reference)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--zq", type=float, default=5.0)
    ap.add_argument("--steps", type=int, default=4, help="offset_rotation_steps: misaligned offsets per pair")
    ap.add_argument("--out", default="eval.txt")
    ap.add_argument("--scan-type", default="cen2018", choices=["cen2018", "kstrongCart"])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the demo runs on an MI355X; the library has no CPU path"
    from tbv_slam_public_amd import api, synth
    imgs, gt, _ = synth.scene_v1(a.seed, a.frames, circle_frames=a.frames)
    sweeps = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    if a.scan_type == "kstrongCart":
        return cartesian(a, api, sweeps, gt)
    r = api.filter_cen2018(sweeps, zq=a.zq, sigma_gauss=17, min_range_bins=2, range_res=0.0438, cap_points=api.L.P2P_MAX_REF_POINTS)
    n = [int(v) for v in r["n_points"]]
    scans = [{"T": tuple(float(v) for v in gt[b]), "cloud": r["xyzi"][b, :n[b]].contiguous(), "pose_id": b, "type": "Cen2018Radar"}
             for b in range(a.frames)]                                     # the clouds stay on the device
    print("%d sweeps, %d .. %d landmarks each" % (a.frames, min(n), max(n)))
    epar = api.scanEvaluatorParameters(scan_spacing=1, offset_rotation_steps=a.steps, theta_range=2 * np.pi)
    ev = api.scanEvaluator(scans, epar, api.AlignmentQualityParameters(method="P2P"))
    path = ev.SaveEvaluation(a.out)
    rows = a.steps + 1
    pairs = len(ev.datapoints_) // rows
    best = 0
    for p in range(pairs):
        score = [d["score"][0] for d in ev.datapoints_[p * rows:(p + 1) * rows]]
        best += int(score[0] == min(score))
    print("%d pairs x %d offsets -> %s" % (pairs, rows, path))
    print("aligned row has the smallest score1 in %d of %d pairs (%.0f %%)" % (best, pairs, 100.0 * best / pairs))


def cartesian(a, api, sweeps, gt):
    pars = api.PoseScanParameters()
    carts = api.polar_to_cartesian(sweeps)                                 # [frames, 300, 300] float32, left on the device
    scans = [{"T": tuple(float(v) for v in gt[b]), "cart": carts[b], "pose_id": b, "type": "CartesianRadar",
              "cart_resolution": pars.cart_resolution, "cart_pixel_width": pars.cart_pixel_width} for b in range(a.frames)]
    print("%d sweeps -> %d x %d Cartesian images" % (a.frames, carts.shape[1], carts.shape[2]))
    epar = api.scanEvaluatorParameters(scan_spacing=1, offset_rotation_steps=a.steps, theta_range=2 * np.pi)
    ev = api.scanEvaluator(scans, epar, api.AlignmentQualityParameters(method="P2P"))   # the factory ignores the method here
    path = ev.SaveEvaluation(a.out)
    rows = a.steps + 1
    pairs = len(ev.datapoints_) // rows
    best = 0
    for p in range(pairs):
        score = [d["score"][0] for d in ev.datapoints_[p * rows:(p + 1) * rows]]
        best += int(score[0] == min(score))
    print("%d pairs x %d offsets -> %s" % (pairs, rows, path))
    print("aligned offset has the lowest abs_diff in %d of %d pairs (%.0f %%)" % (best, pairs, 100.0 * best / pairs))


if __name__ == "__main__":
    main()
