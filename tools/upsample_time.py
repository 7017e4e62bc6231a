#!/usr/bin/env python3
"""svgf_upsample at 1920x1080 -> 3840x2160, modulate on, AoS and planar guides: device events around regions of 50 launches, each
case behind 0.25 s of its own launches (README round 6's rule), median / min / max of seven regions; us per launch and bytes/s
beside the byte count of DESIGN.md 5.4b (per hi pixel: the hi guide, 12 B written, 40 B of lo taps per four hi pixels).  With
--frames also the ordered full-SVGF frame at both sizes, the same way, for the sum "small frame + upsample" against the large
frame.  Prints one JSON line per case."""
import json
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
b = pkg.binding
WL, HL, WH, HH = 1920, 1080, 3840, 2160
LAUNCHES, REGIONS, WARM_S = 50, 7, 0.25


def timed(fn):
    """us per call: REGIONS regions of LAUNCHES calls between two events, behind WARM_S seconds of the same calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARM_S:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    us = []
    for _ in range(REGIONS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    return float(np.median(us)), float(min(us)), float(max(us))


def split(texels, n):
    """the planes of a device AoS G-buffer (float view: 13 floats per texel)"""
    t = texels.view(torch.float32).view(n, 13)
    return [t[:, 0:3].contiguous(), t[:, 3:6].contiguous(), t[:, 12].contiguous().view(torch.int32), (t[:, 6:9] * t[:, 9:12]).contiguous()]


cam = pkg.synth.camera_for_frame(0, False)
rgb_lo = torch.empty((HL, WL, 3), dtype=torch.float32, device="cuda")
rgb_hi = torch.empty((HH, WH, 3), dtype=torch.float32, device="cuda")
gb_lo = torch.empty((HL * WL * 52,), dtype=torch.uint8, device="cuda")
gb_hi = torch.empty((HH * WH * 52,), dtype=torch.uint8, device="cuda")
b.synth_render(rgb_lo, gb_lo, WL, HL, cam, 0, seed=1000)
b.synth_render(rgb_hi, gb_hi, WH, HH, cam, 0, seed=1000)
out = torch.empty((HH, WH, 3), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
pl_lo, pl_hi = split(gb_lo, WL * HL), split(gb_hi, WH * HH)
guides = {"aos": (b.guide(gbuffer=gb_hi), b.guide(gbuffer=gb_lo), 52 + 12 + 40 / 4),
          "planar": (b.guide(normal=pl_hi[0], position=pl_hi[1], geom_id=pl_hi[2], albedo=pl_hi[3]),
                     b.guide(normal=pl_lo[0], position=pl_lo[1], geom_id=pl_lo[2]), 40 + 12 + 40 / 4)}
for name, (hi, lo, bpp) in guides.items():
    med, lo_us, hi_us = timed(lambda: b.upsample(out, hi, WH, HH, rgb_lo, lo, WL, HL, 0.5, 0.5, 1))
    nbytes = bpp * WH * HH
    print("UPSAMPLE", json.dumps(dict(case=name, lo=[WL, HL], hi=[WH, HH], us=round(med, 2), us_min=round(lo_us, 2), us_max=round(hi_us, 2),
                                      bytes_per_hi_pixel=bpp, megabytes=round(nbytes / 1e6, 1), terabytes_per_s=round(nbytes / med / 1e6, 3))))

if "--frames" in sys.argv:
    for (W, H, rgb, gb) in ((WL, HL, rgb_lo, gb_lo), (WH, HH, rgb_hi, gb_hi)):
        d = pkg.Denoiser(W, H)
        p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, sepcolor=1, addcolor=0)
        o = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        med, lo_us, hi_us = timed(lambda: d.denoise(o, rgb, gb, cam, p))
        print("FRAME", json.dumps(dict(size=[W, H], us=round(med, 2), us_min=round(lo_us, 2), us_max=round(hi_us, 2),
                                       gigapixels_per_s=round(W * H / med / 1e3, 3))))
        d.sync()
        d.free()
