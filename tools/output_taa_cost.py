#!/usr/bin/env python3
"""The output pass (svgf_set_output_taa) at 1920x1080: its own duration (svgf_profile_read, kind 7) beside the temporal pass's of
the same frames, median of 32 frames behind 40 warm-up frames, and the wall time of an ordered frame with the feature off and on;
static and moving camera, camera path and a PREV_COORD_F32 plane.  Prints one line per case."""
import os, sys, json, time
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import __graft_entry__ as ge
pkg = ge.load_package()
W, H = 1920, 1080
NF = 8
res = {}
for moving in (False, True):
    cams = [pkg.synth.camera_for_frame(f, moving) for f in range(NF)]
    d_in = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(NF)]
    d_g = [torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda") for _ in range(NF)]
    for f in range(NF):
        pkg.binding.synth_render(d_in[f], d_g[f], W, H, cams[f], f, seed=1000)
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=5, history_level=1)
    plx, ply = pkg.synth._pixel_length(W, H, 45.0)
    p.reproj_scale[0], p.reproj_scale[1] = float(plx) * W / 2.0, float(ply) * H / 2.0
    for name, alpha, plane in (("off", 0.0, False), ("on", 0.2, False), ("on+plane", 0.2, True)):
        d = pkg.Denoiser(W, H)
        d.set_output_taa(alpha, 1.0)
        mv = torch.empty((H, W, 2), dtype=torch.float32, device="cuda") if plane else None
        def frame(i):
            f = i % NF if moving else i % 4
            if plane:
                pkg.binding.motion_reproject(mv, W, H, cams[(f - 1) % NF if moving else f], gbuffer=d_g[f], reproj_scale=(p.reproj_scale[0], p.reproj_scale[1]))
            d.denoise(out, d_in[f], d_g[f], cams[f], p, motion=mv)
        for i in range(40):
            frame(i)
        d.sync()
        d.profile_stride(1); d.profile_enable(32)
        for i in range(32):
            frame(40 + i)
        d.sync()
        per = {}
        for s in range(32):
            row = d.profile_read(s)
            if alpha > 0:
                assert row[-1][0] == 7 and sum(1 for k, _ in row if k == 7) == 1, row
            for k, ms in row:
                per.setdefault(k, []).append(ms)
            per.setdefault("sum", []).append(sum(ms for _, ms in row))
        d.profile_enable(0)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(200):
            frame(i)
        torch.cuda.synchronize(); wall = (time.perf_counter() - t0) / 200 * 1e3
        res[f"{'moving' if moving else 'static'} {name}"] = dict(
            temporal_us=float(np.median(per[1])) * 1e3, taa_us=float(np.median(per[7])) * 1e3 if 7 in per else None,
            taa_min_max_us=[float(np.min(per[7])) * 1e3, float(np.max(per[7])) * 1e3] if 7 in per else None,
            atrous_us_per_level=float(np.median(per[3])) * 1e3, kernels_sum_us=float(np.median(per["sum"])) * 1e3, wall_ms_per_frame=wall)
        d.free()
for k, v in res.items():
    print("TAA", k, json.dumps(v))
