#!/usr/bin/env python3
"""Row f27 (libsvgf_restir.so) measured with the method of tools/deform_time.py: device events behind ~2 ms of queued work, mean
over 10 calls, REPEATS times after a warm-up; every figure also in units of svgf_scene_draw_shadowed with samples = 1 on the same
frame, which is what one shadow ray per pixel costs in this code base.

  (a) one svgf_restir_frame (its two launches together) by `candidates` (1, 4, 8, 32; no reuse) and by `neighbours` (0, 1, 3, 5, 8
      with 8 candidates and the history tap), on a static view whose previous-coordinate plane is the identity;
  (b) svgf_lights_draw_all at 64 lights, one sample per light.

64 lamps in an 8 x 8 grid of small parallelograms around the scene's own light.  Inputs: the recorded room (2 810 triangles) and the
recorded cornell, at 3840x2160.

    python tools/restir_time.py [out.txt]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_pose_time as spt  # noqa: E402

REPEATS = 2


def lamps(pkg, centre, spread):
    k = np.arange(64)
    c = np.stack([centre[0] + spread * ((k % 8) / 3.5 - 1.0), np.full(64, centre[1] - 0.05 * spread), centre[2] + spread * ((k // 8) / 3.5 - 1.0)], -1)
    e = 0.03 * spread
    return pkg.restir.lights(c, np.tile([e, 0, 0], (64, 1)), np.tile([0, 0, e], (64, 1)), 30.0 / 8.0)


def main(out_path=None):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    R = pkg.restir
    W, H = 3840, 2160
    lines = [f"# {torch.cuda.get_device_name(0)}; {W}x{H}; device events behind ~2 ms of queued work, mean over 10 calls; {REPEATS} repeats; "
             f"min .. max over the repeats; x = in units of svgf_scene_draw_shadowed with samples = 1"]
    st = torch.cuda.Stream()
    busy = torch.empty((1 << 26,), dtype=torch.float32, device="cuda")
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    D = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
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
        P = np.asarray(s["tris"], np.float32).reshape(-1, 8)[:, 0:3]
        spread = 0.25 * float((P.max(axis=0) - P.min(axis=0)).max()) if len(P) else 2.0
        table, state = R.LightTable(lamps(pkg, light, spread)), R.Restir(scene, W, H)
        one = pkg.binding.SvgfSceneLight.make(light, (0.03 * spread, 0, 0), (0, 0, 0.03 * spread), 1)
        scene.draw(rgb, gbt, W, H, s["cam"], light, 0, stream=st)           # the G-buffer every call below reads
        shadowed = lambda f: scene.draw_shadowed(rgb, gbt, W, H, s["cam"], one, f, stream=st)       # noqa: E731
        frame = lambda rp: (lambda f: state.frame(table, gbt, D, f, 7, motion=still, rp=rp, stream=st))      # noqa: E731
        ways = [(f"candidates {c:2d}, no reuse        ", R.params(c, 0, 20.0, 0)) for c in (1, 4, 8, 32)]
        ways += [(f"candidates  8, tap, {k} neighbours", R.params(8, 1, 20.0, k)) for k in (0, 1, 3, 5, 8)]
        for call in [shadowed] + [frame(rp) for _, rp in ways]:
            event_ms(call, 2)
        unit = [event_ms(shadowed) for _ in range(REPEATS)]
        u = float(np.mean(unit))
        lines.append(f"{name} ({scene.info()['n_tris']} triangles, 64 lamps): svgf_scene_draw_shadowed, 1 sample {np.mean(unit):8.3f} ms ({min(unit):.3f} .. {max(unit):.3f})")
        for label, rp in ways:
            lines.append(f"  svgf_restir_frame, {label} {fmt([event_ms(frame(rp)) for _ in range(REPEATS)], u)}")
        lines.append(f"  svgf_lights_draw_all, 64 lights x 1 sample       "
                     f"{fmt([event_ms(lambda f: table.draw_all(scene, gbt, W, H, D, f, 7, 1, stream=st), 3) for _ in range(REPEATS)], u)}")
        state.free(); table.free(); scene.free()
        print("\n".join(lines[-11:]), flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
