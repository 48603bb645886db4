#!/usr/bin/env python
"""Raw-sweep Scan Context (cfear_sc_raw_descriptors) launch times: 1, 512 and 4096 sweeps of 400 x 3360 and 400 x 3768,
stored azimuth-major (read transposed) and bins-major.  Sweeps and descriptors stay in HBM; no keys.  Prints per
configuration the kernel time (sc_raw_descriptor, hipEvents on the context's stream), the whole call (host clock around
the synchronous C-ABI call: table upload + kernel) and image bytes / kernel time as a fraction of the 8 TB/s HBM spec.
    python tools/sc_raw_probe.py [--reps 20] [--batches 1,512,4096]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tbv_slam_public_amd import _lib as L  # noqa: E402
from tbv_slam_public_amd import api  # noqa: E402

HBM_SPEC = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,512,4096")
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    a = ap.parse_args()
    ctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    par = api.sc_params()
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for bins in (3360, 3768):
        for layout in ("azimuth-major", "bins-major"):
            shape = (400, bins) if layout == "azimuth-major" else (bins, 400)
            raw = api.sc_raw_params(transpose=1 if layout == "azimuth-major" else 0)
            for B in [int(b) for b in a.batches.split(",")]:
                imgs = torch.randint(0, 256, (B,) + shape, dtype=torch.uint8, device="cuda", generator=g)
                out = torch.empty((B, par.num_ring * par.num_sector), dtype=torch.float64, device="cuda")
                d, ptr, _keep = api._image_desc(imgs)
                torch.cuda.synchronize()

                def call():
                    ctx.check(ctx._lib.cfear_sc_raw_descriptors(ctx.h, ptr, C.byref(d), C.byref(par), C.byref(raw),
                                                                out.data_ptr(), None, None))
                for _ in range(3):
                    call()
                ctx.synchronize()
                ctx.profile_enable(True)
                ctx.profile_read(reset=True)
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    call()
                ctx.synchronize()
                wall = (time.perf_counter() - t0) * 1e3 / a.reps
                prof = ctx.profile_read(reset=True)
                ctx.profile_enable(False)
                kms = prof["sc_raw_descriptor"][0] / prof["sc_raw_descriptor"][1]
                nbytes = B * shape[0] * shape[1]
                r = dict(bins=bins, layout=layout, batch=B, kernel_ms=round(kms, 4), call_ms=round(wall, 4),
                         hbm_fraction=round(nbytes / (kms * 1e-3) / HBM_SPEC, 3))
                rows.append(r)
                print("%4d bins %-13s batch %4d: kernel %.4f ms  call %.4f ms  %.3f of 8 TB/s" %
                      (bins, layout, B, kms, wall, r["hbm_fraction"]), flush=True)
                del imgs, out
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()
    assert L.OK == 0


if __name__ == "__main__":
    main()
