#!/usr/bin/env python3
"""svgf_transfer_history at 960x540 -> 1280x720 (the resample) and 1920x1080 -> 1920x1080 (the copy): each launch between two device
events, the median / min / max of 20 launches behind 0.25 s of frames on the source context (README round 6's rule: a number is
taken on a warm device).  Bytes moved are the algorithmic count of DESIGN.md 5.4c: 56 B per src pixel read (colour + variance 16,
moments 8, history length 4, normal 12, position 12, geomId 4) and 56 B per dst pixel written.  Prints one JSON line per case."""
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
LAUNCHES, WARM_S, BYTES_PER_PIXEL = 20, 0.25, 56

for (Ws, Hs), (Wd, Hd) in (((960, 540), (1280, 720)), ((1920, 1080), (1920, 1080))):
    cam = pkg.synth.camera_for_frame(0, False)
    rgb = torch.empty((Hs, Ws, 3), dtype=torch.float32, device="cuda")
    gb = torch.empty((Hs * Ws * 52,), dtype=torch.uint8, device="cuda")
    out = torch.empty((Hs, Ws, 3), dtype=torch.float32, device="cuda")
    b.synth_render(rgb, gb, Ws, Hs, cam, 0, seed=1000)
    src, dst = pkg.Denoiser(Ws, Hs), pkg.Denoiser(Wd, Hd)
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARM_S:
        for _ in range(10):
            src.denoise(out, rgb, gb, cam, p)
        torch.cuda.synchronize()
    us = []
    for _ in range(LAUNCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.transfer_history_from(src)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    med = float(np.median(us))
    nbytes = BYTES_PER_PIXEL * (Ws * Hs + Wd * Hd)
    print("TRANSFER", json.dumps(dict(src=[Ws, Hs], dst=[Wd, Hd], us=round(med, 2), us_min=round(min(us), 2), us_max=round(max(us), 2),
                                      megabytes=round(nbytes / 1e6, 1), terabytes_per_s=round(nbytes / med / 1e6, 3))))
    src.free()
    dst.free()
