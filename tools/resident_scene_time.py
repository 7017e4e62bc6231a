#!/usr/bin/env python3
"""The resident scene (row f14) against the path it stands beside, svgf_scene_render_mesh, in one process:

  (a) kernel time: k_scene_frame (every triangle for every pixel) vs k_scene_bvh, device events around one call while the stream is
      still busy with earlier work - svgf_scene_render_mesh's upload and host wait then run beside that work and the interval between
      the events is the kernel alone;
  (b) wall time per frame of a loop of calls, host clock from the first call to the end of a final synchronisation: what a renderer's
      loop pays, upload and host wait included.

Per case the two paths alternate, REPEATS times, after a warm-up; every timed stretch lasts at least MIN_SECONDS.  Inputs: the
recorded reference scenes (tests/golden/ref_scenes), frame 0 of their recorded cameras.

    python tools/resident_scene_time.py [out.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_scenes")
CASES = [("room", "room128x72_static_sepcolor", 1920, 1080), ("room", "room128x72_static_sepcolor", 3840, 2160),
         ("bunny", "bunny128x72_static", 3840, 2160)]
REPEATS, MIN_SECONDS = 3, 0.3


def main(out_path=None):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    b = pkg.binding
    lines = [f"# {torch.cuda.get_device_name(0)}; kernel: device events, mean over the frames of >= {MIN_SECONDS} s (200 at the most); loop: host wall time per frame; "
             f"{REPEATS} repeats, the two paths alternating; all times in ms (min .. max over the repeats)"]
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

        def mesh(f):
            b.scene_render_mesh(rgb, gbt, W, H, cam, pi["geoms"], pi["geom_ids"], pi["tris"], pi["tri_ids"], pi["tri_albedo"], frame=f, light=light, stream=st)

        def draw(f):
            res.draw(rgb, gbt, W, H, cam, light, f, stream=st)

        def kernel_ms(call, n):
            e = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for f in range(n):
                with torch.cuda.stream(st):
                    for _ in range(8):
                        busy.add_(1.0)          # ~2 ms of work ahead of the call: the host side of the call hides behind it
                    e[f][0].record()
                call(f)
                with torch.cuda.stream(st):
                    e[f][1].record()
            st.synchronize()
            return sum(a.elapsed_time(z_) for a, z_ in e) / n

        def loop_ms(call, n):
            st.synchronize()
            t0 = time.perf_counter()
            for f in range(n):
                call(f)
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        # warm-up, and how many frames make MIN_SECONDS
        n = {}
        for name, call in (("mesh", mesh), ("draw", draw)):
            loop_ms(call, 3)
            n[name] = max(5, int(MIN_SECONDS * 1e3 / loop_ms(call, 5)) + 1)
        k = {"mesh": [], "draw": []}
        w = {"mesh": [], "draw": []}
        for _ in range(REPEATS):
            for name, call in (("mesh", mesh), ("draw", draw)):
                k[name].append(kernel_ms(call, min(n[name], 200)))
                w[name].append(loop_ms(call, n[name]))
        res.free()
        fmt = lambda v: f"{np.mean(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"     # noqa: E731
        lines.append(f"{scene} ({info['n_tris']} triangles; BVH {info['n_nodes']} nodes, depth {info['depth']}, leaves <= {info['max_leaf_tris']}) at {W}x{H}")
        lines.append(f"  kernel  k_scene_frame          {fmt(k['mesh'])}   k_scene_bvh     {fmt(k['draw'])}   ratio {np.mean(k['mesh']) / np.mean(k['draw']):.1f}x")
        lines.append(f"  loop    svgf_scene_render_mesh {fmt(w['mesh'])}   svgf_scene_draw {fmt(w['draw'])}   ratio {np.mean(w['mesh']) / np.mean(w['draw']):.1f}x"
                     f"   ({n['mesh']} / {n['draw']} frames per stretch)")
        print("\n".join(lines[-3:]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
