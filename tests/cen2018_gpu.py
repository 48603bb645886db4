"""What the GPU tests of cfear_filter_cen2018 share: the call with every optional output, and the comparison with the
restatement (tests/cen2018_cpu.py) -- row_stats bit-equal; det_mask equal on every decided bin; targets, n_points and xyzi
equal on every row without an undecided bin, and such rows at most 0.5 % of a case's rows."""
import numpy as np


def run(imgs, par, cap, device=False, **kw):
    from tbv_slam_public_amd import api
    if device:
        import torch
        x = imgs if hasattr(imgs, "data_ptr") else torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
        r = api.filter_cen2018(x, cap_points=cap, want_targets=True, want_mask=True, want_stats=True, **par, **kw)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in r.items()}
    return api.filter_cen2018(imgs, cap_points=cap, want_targets=True, want_mask=True, want_stats=True, **par, **kw)


def compare(got, refs, imgs, name):
    """the three checks of one batch against the restatement's results `refs`, and the cap on rows with an undecided bin"""
    bad = total = 0
    for b, ref in enumerate(refs):
        rows, cols = imgs[b].shape
        assert np.array_equal(got["row_stats"][b, :, 0].view(np.uint32), ref["mean"].view(np.uint32)), (name, b, "mean")
        assert np.array_equal(got["row_stats"][b, :, 1].view(np.uint32), ref["sigma"].view(np.uint32)), (name, b, "sigma")
        dec = ~ref["undecided"]
        assert np.array_equal(got["det_mask"][b][dec], ref["mask"][dec]), (name, b, "mask")
        und_rows = ref["undecided"].any(axis=1)
        bad += int(und_rows.sum())
        total += rows
        n = int(got["n_points"][b])
        gt, gx = got["targets"][b, :n], got["xyzi"][b, :n]
        if not und_rows.any():
            assert n == len(ref["targets"]), (name, b, n, len(ref["targets"]))
        keep_g = ~und_rows[gt[:, 0]]
        keep_r = ~und_rows[ref["targets"][:, 0]]
        assert np.array_equal(gt[keep_g], ref["targets"][keep_r]), (name, b, "targets")
        assert np.array_equal(gx[keep_g].view(np.uint32), ref["xyzi"][keep_r].view(np.uint32)), (name, b, "xyzi")
    print("undecided rows %s: %d of %d" % (name, bad, total))
    assert bad <= 0.005 * total, (name, bad, total)
