#!/usr/bin/env python3
"""What bounce k of a path costs (row f19), by the method of tools/traced_scene_time.py: svgf_trace_draw with one bounce
sample (k_scene_trace of libsvgf_trace.so) alternates with svgf_path_draw (k_scene_path of libsvgf_path.so) at max_depth 1, 2, 4 and 8
with rr_depth 0 and 2, and with svgf_path_draw_split at depth 4, REPEATS times, after a warm-up; the kernel time is the interval between
two device events around one call while the stream is still busy with earlier work (the host side of the call hides behind it),
averaged over the frames of at least MIN_SECONDS.

Inputs: the recorded reference scenes (tests/golden/ref_scenes), frame 0 of their recorded cameras, at 3840x2160; a parallelogram
light (half-edges 0.5 in x and z) at the scene's light, one shadow ray at the first hit and at every later vertex, one path per pixel.
Every draw is reported as a multiple of the svgf_trace_draw time of the same run.

    python tools/path_scene_time.py [out.txt]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_scenes")
CASES = [("room", "room128x72_static_sepcolor", 3840, 2160), ("bunny", "bunny128x72_static", 3840, 2160)]
DEPTHS, ROULETTE = (1, 2, 4, 8), (0, 2)
REPEATS, MIN_SECONDS = 3, 0.3


def main(out_path=None):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    b = pkg.binding
    lines = [f"# {torch.cuda.get_device_name(0)}; device events around one call behind ~2 ms of queued work, mean over the frames of >= {MIN_SECONDS} s "
             f"(200 at the most); {REPEATS} repeats, the draws alternating; all times in ms (min .. max over the repeats)"]
    st = torch.cuda.Stream()
    busy = torch.empty((1 << 26,), dtype=torch.float32, device="cuda")
    for scene, rec, W, H in CASES:
        z, pi = np.load(os.path.join(REF, rec + ".npz")), np.load(os.path.join(REF, scene + "_producer_inputs.npz"))
        c = z["cams"][0]
        cam = dict(right=c[0:3], up=c[3:6], view=c[6:9], position=c[9:12], fovy_deg=float(pi["fovy"]))
        light = pkg.scene.light_position(pi["geoms"])
        rgb, d_img, i_img = (torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(3))
        gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
        res = pkg.Scene.create(pi["geoms"], pi["geom_ids"], pi["tris"], pi["tri_ids"], pi["tri_albedo"])
        info = res.info()
        lt = b.SvgfSceneLight.make(light, (0.5, 0.0, 0.0), (0.0, 0.0, 0.5), 1)

        def kernel_ms(call, n):
            e = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for f in range(n):
                with torch.cuda.stream(st):
                    for _ in range(8):
                        busy.add_(1.0)          # ~2 ms of work ahead of the call
                    e[f][0].record()
                call(f)
                with torch.cuda.stream(st):
                    e[f][1].record()
            st.synchronize()
            return sum(a.elapsed_time(z_) for a, z_ in e) / n

        calls = {"svgf_trace_draw, 1 bounce sample": lambda f: res.draw_traced(rgb, gbt, W, H, cam, lt, f, bounce_samples=1, stream=st)}
        for K in DEPTHS:
            for R in ROULETTE:
                if K == 1 and R:
                    continue                    # roulette never acts at depth 1
                calls[f"svgf_path_draw, depth {K}, rr_depth {R}"] = \
                    lambda f, K=K, R=R: res.draw_path(rgb, gbt, W, H, cam, lt, f, paths=1, max_depth=K, rr_depth=R, stream=st)
        calls["svgf_path_draw_split, depth 4, rr_depth 2"] = \
            lambda f: res.draw_path_split(d_img, i_img, gbt, W, H, cam, lt, f, paths=1, max_depth=4, rr_depth=2, out_rgb=rgb, stream=st)
        n = {}
        for name, call in calls.items():        # warm-up, and how many frames make MIN_SECONDS
            kernel_ms(call, 3)
            n[name] = min(200, max(5, int(MIN_SECONDS * 1e3 / (kernel_ms(call, 5) + 2.0)) + 1))
        k = {name: [] for name in calls}
        for _ in range(REPEATS):
            for name, call in calls.items():
                k[name].append(kernel_ms(call, n[name]))
        res.free()
        fmt = lambda v: f"{np.mean(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"     # noqa: E731
        base = np.mean(k["svgf_trace_draw, 1 bounce sample"])
        lines.append(f"{scene} ({info['n_tris']} triangles, {info['n_geoms']} primitives; BVH {info['n_nodes']} nodes, depth {info['depth']}) at {W}x{H}")
        for name in calls:
            lines.append(f"  {name:46s} {fmt(k[name])}   {np.mean(k[name]) / base:5.2f}x svgf_trace_draw")
        print("\n".join(lines[-(len(calls) + 1):]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
