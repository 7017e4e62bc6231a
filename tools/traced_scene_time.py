#!/usr/bin/env python3
"""The path-traced draw (row f17) against the two draws it stands beside, in one process, by the method of
tools/shadowed_scene_time.py: svgf_scene_draw (k_scene_bvh<false>), svgf_scene_draw_shadowed (k_scene_bvh<true>, one shadow ray) and
svgf_trace_draw (k_scene_trace of libsvgf_trace.so) alternate, REPEATS times, after a warm-up; the kernel time is the interval
between two device events around one call while the stream is still busy with earlier work (the host side of the call hides behind
it), averaged over the frames of at least MIN_SECONDS.

Inputs: the recorded reference scenes (tests/golden/ref_scenes), frame 0 of their recorded cameras, at 3840x2160; a parallelogram
light (half-edges 0.5 in x and z) at the scene's light, one shadow ray at the first hit; bounce_samples 1 and 4, shadow_secondary 0
and 1.  What one bounce costs is reported as a multiple of the primary walk (the unshadowed draw): the traced draw minus the
shadowed draw with the same first-hit work, per bounce sample.

    python tools/traced_scene_time.py [out.txt]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_scenes")
CASES = [("room", "room128x72_static_sepcolor", 3840, 2160), ("bunny", "bunny128x72_static", 3840, 2160)]
BOUNCES, SECONDARY = (1, 4), (0, 1)
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
        rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
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

        calls = {"svgf_scene_draw": lambda f: res.draw(rgb, gbt, W, H, cam, light, f, stream=st),
                 "shadowed, 1 sample": lambda f: res.draw_shadowed(rgb, gbt, W, H, cam, lt, f, stream=st),
                 "traced, 0 bounce samples": lambda f: res.draw_traced(rgb, gbt, W, H, cam, lt, f, bounce_samples=0, stream=st)}
        for J in BOUNCES:
            for sec in SECONDARY:
                calls[f"traced, {J} bounce sample{'s' if J > 1 else ''}, secondary shadow {sec}"] = \
                    lambda f, J=J, sec=sec: res.draw_traced(rgb, gbt, W, H, cam, lt, f, bounce_samples=J, shadow_secondary=sec, stream=st)
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
        base, shadowed = np.mean(k["svgf_scene_draw"]), np.mean(k["shadowed, 1 sample"])
        lines.append(f"{scene} ({info['n_tris']} triangles, {info['n_geoms']} primitives; BVH {info['n_nodes']} nodes, depth {info['depth']}) at {W}x{H}")
        for name in calls:
            extra = "" if name == "svgf_scene_draw" else f"   {np.mean(k[name]) / base:5.2f}x the unshadowed draw"
            if "bounce sample" in name and not name.startswith("traced, 0"):
                J = int(name.split()[1])
                extra += f", {(np.mean(k[name]) - shadowed) / base / J:5.2f} primary walks per bounce sample"
            lines.append(f"  {name:46s} {fmt(k[name])}{extra}")
        print("\n".join(lines[-(len(calls) + 1):]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
