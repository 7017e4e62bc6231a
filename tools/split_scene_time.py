#!/usr/bin/env python3
"""The split draw (row f18) beside the traced draw it is an instantiation of, and the recomposition, in one process,
by the method of tools/traced_scene_time.py: the calls alternate, REPEATS times, after a warm-up; the kernel time is the interval
between two device events around one call while the stream is still busy with earlier work, averaged over the frames of at least
MIN_SECONDS.

Inputs: the recorded reference scenes (tests/golden/ref_scenes), frame 0 of their recorded cameras, at 3840x2160; a parallelogram
light (half-edges 0.5 in x and z) at the scene's light, one shadow ray at the first hit, one bounce sample with its shadow ray.
Timed: svgf_trace_draw; svgf_trace_draw_split with and without out_rgb; two svgf_trace_draw calls (what separate terms cost before
this row: every ray twice); svgf_trace_compose with an AoS and with a planar guide, in microseconds and in TB/s of the bytes it has to
move (24 B/px of terms in, 12 out, and 24 of each AoS texel or 12 of the albedo plane).

    python tools/split_scene_time.py [out.txt]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_scenes")
CASES = [("room", "room128x72_static_sepcolor", 3840, 2160), ("bunny", "bunny128x72_static", 3840, 2160)]
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

        direct, indirect, out = (torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(3))
        albedo = torch.rand((H, W, 3), dtype=torch.float32, device="cuda")
        planar = b.guide(albedo=albedo)

        def twice(f):
            res.draw_traced(rgb, gbt, W, H, cam, lt, f, stream=st)
            res.draw_traced(out, gbt, W, H, cam, lt, f, stream=st)

        calls = {"svgf_trace_draw": lambda f: res.draw_traced(rgb, gbt, W, H, cam, lt, f, stream=st),
                 "svgf_trace_draw_split": lambda f: res.draw_traced_split(direct, indirect, gbt, W, H, cam, lt, f, stream=st),
                 "svgf_trace_draw_split with out_rgb": lambda f: res.draw_traced_split(direct, indirect, gbt, W, H, cam, lt, f, out_rgb=rgb, stream=st),
                 "two svgf_trace_draw calls": twice,
                 "svgf_trace_compose, AoS guide": lambda f: pkg.trace_compose(out, direct, indirect, gbt, W, H, stream=st),
                 "svgf_trace_compose, planar guide": lambda f: pkg.trace_compose(out, direct, indirect, planar, W, H, stream=st)}
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
        base = np.mean(k["svgf_trace_draw"])
        lines.append(f"{scene} ({info['n_tris']} triangles, {info['n_geoms']} primitives; BVH {info['n_nodes']} nodes, depth {info['depth']}) at {W}x{H}")
        for name in calls:
            if "compose" in name:
                nbytes = W * H * (36 + (24 if "AoS" in name else 12))
                extra = f"   {1e3 * np.mean(k[name]):8.1f} us, {nbytes / (1e-3 * np.mean(k[name])) / 1e12:5.2f} TB/s of {nbytes / 1e6:.0f} MB counted"
            else:
                extra = "" if name == "svgf_trace_draw" else f"   {np.mean(k[name]) / base:5.3f}x one traced draw"
            lines.append(f"  {name:46s} {fmt(k[name])}{extra}")
        print("\n".join(lines[-(len(calls) + 1):]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
