#!/usr/bin/env python3
"""Row f28 (libsvgf_restir_gi.so) measured with the method of tools/restir_time.py: device events behind ~2 ms of queued work, mean
over 10 calls, REPEATS times after a warm-up; every figure also in units of svgf_trace_draw_split with bounce_samples = 1 and the
same shadow_secondary on the same frame and in the same session - the draw whose one independent sample per pixel this row resamples
(it also casts the primary ray and the first hit's shadow ray, which svgf_restir_gi_frame does not).

  one svgf_restir_gi_frame (its two launches together) by `candidates` (1, 4, 8; no reuse), with the history tap, and by `neighbours`
  (1, 3, 5, 8 with one candidate and the tap), on a static view whose previous-coordinate plane is the identity; shadow_secondary 1
  and, for the first and the last way, 0.

Inputs: the recorded room (2 810 triangles) and the recorded cornell, at 3840x2160.

    python tools/restir_gi_time.py [out.txt]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_pose_time as spt  # noqa: E402

REPEATS = 2


def main(out_path=None):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    W, H = 3840, 2160
    lines = [f"# {torch.cuda.get_device_name(0)}; {W}x{H}; device events behind ~2 ms of queued work, mean over 10 calls; {REPEATS} repeats; "
             f"min .. max over the repeats; x = in units of svgf_trace_draw_split with bounce_samples = 1 and the same shadow_secondary"]
    st = torch.cuda.Stream()
    busy = torch.empty((1 << 26,), dtype=torch.float32, device="cuda")
    rgb, D, I = (torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(3))      # noqa: E741
    gbt, gb2 = (torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda") for _ in range(2))
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32, device="cuda"), torch.arange(W, dtype=torch.float32, device="cuda"), indexing="ij")
    still = torch.stack([x, y], -1).contiguous()
    fmt = lambda v, unit: f"{np.mean(v):8.3f} ms ({min(v):.3f} .. {max(v):.3f}) = {np.mean(v) / unit:5.2f}x"     # noqa: E731

    def event_ms(call, n=10):
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

    for name, s in (("room", spt.recorded(pkg, "room", "room128x72_static_sepcolor")), ("cornell", spt.recorded(pkg, "cornell", "cornell96_static"))):
        scene = pkg.Scene.create(s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"], s["tri_albedo"])
        light = tuple(float(v) for v in s["light"])
        state = pkg.RestirGI(scene, W, H)
        one = pkg.binding.SvgfSceneLight.make(light, (0.5, 0, 0), (0, 0, 0.5), 1)
        scene.draw(rgb, gbt, W, H, s["cam"], light, 0, noise=0.0, fireflies=0.0, stream=st)           # the G-buffer every frame below reads
        split = lambda sec: (lambda f: scene.draw_traced_split(D, I, gb2, W, H, s["cam"], one, f, 1, 0.15, sec, seed=7, stream=st))      # noqa: E731
        frame = lambda gp: (lambda f: state.frame(one, gbt, I, f, 7, motion=still, gp=gp, stream=st))      # noqa: E731
        P = pkg.gi_params
        ways = [(f"candidates {c}, no reuse,          sec 1", P(c, 0, 20.0, 0)) for c in (1, 4, 8)]
        ways += [(f"candidates 1, tap, {k} neighbours, sec 1", P(1, 1, 20.0, k)) for k in (0, 1, 3, 5, 8)]
        ways += [("candidates 1, no reuse,          sec 0", P(1, 0, 20.0, 0, shadow_secondary=0)),
                 ("candidates 1, tap, 8 neighbours, sec 0", P(1, 1, 20.0, 8, shadow_secondary=0))]
        for call in [split(0), split(1)] + [frame(gp) for _, gp in ways]:
            event_ms(call, 2)
        unit = {sec: [event_ms(split(sec)) for _ in range(REPEATS)] for sec in (1, 0)}
        lines.append(f"{name} ({scene.info()['n_tris']} triangles): svgf_trace_draw_split, 1 bounce sample, sec 1 {np.mean(unit[1]):8.3f} ms "
                     f"({min(unit[1]):.3f} .. {max(unit[1]):.3f}); sec 0 {np.mean(unit[0]):8.3f} ms ({min(unit[0]):.3f} .. {max(unit[0]):.3f})")
        for label, gp in ways:
            lines.append(f"  svgf_restir_gi_frame, {label} {fmt([event_ms(frame(gp)) for _ in range(REPEATS)], float(np.mean(unit[gp.shadow_secondary])))}")
        state.free(); scene.free()
        print("\n".join(lines[-(len(ways) + 1):]), flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
