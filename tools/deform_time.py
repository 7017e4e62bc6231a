#!/usr/bin/env python3
"""Row f26 (libsvgf_deform.so) measured with the method of tools/sah_time.py: device events behind ~2 ms of queued work for single
calls, host wall time per frame for loops, the alternatives alternating, REPEATS times after a warm-up.

  (a) one svgf_deform_apply (device events), every triangle of the scene skinned by two bones;
  (b) svgf_deform_prev_positions beside svgf_scene_draw on the same frame (device events), at 3840x2160;
  (c) the loops deform + svgf_scene_refit + draw, deform + svgf_lbvh_build + draw and deform + svgf_sah_build + draw at bend angles
      0, 45 and 135 degrees: bone 0 holds the scene's lower third, bone 1 turns its upper third about the scene's centre, the weights
      cross over in between.  The refit keeps the topology of the tree built at rest; the two builders split the triangles as drawn.

Before the loops run at an angle, the three scenes' triangles as drawn are compared with each other on bytes.
Inputs: the recorded room (2 810 triangles) and scene_pose_time's grid at 2^20 triangles.

    python tools/deform_time.py [out.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_pose_time as spt  # noqa: E402

REPEATS = 2
ANGLES = (0.0, 45.0, 135.0)


def height_rig(tris):
    """Every triangle skinned: (tri_index, bone, weight), bone 1's weight rising from 0 to 1 over the middle third of the scene's height."""
    y = np.asarray(tris, np.float32).reshape(-1, 3, 8)[:, :, 1]
    h = (y - y.min()) / max(float(y.max() - y.min()), 1e-6)
    w1 = np.clip((h - 1.0 / 3.0) * 3.0, 0.0, 1.0).astype(np.float32)
    weight = np.zeros(y.shape + (4,), np.float32)
    weight[..., 0], weight[..., 1] = np.float32(1.0) - w1, w1
    bone = np.zeros(y.shape + (4,), np.uint16)
    bone[..., 1] = 1
    return np.arange(len(y), dtype=np.int32), bone, weight


def main(out_path=None):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    D = pkg.deform
    W, H = 3840, 2160
    lines = [f"# {torch.cuda.get_device_name(0)}; {W}x{H}; single calls: device events behind ~2 ms of queued work, mean over 10 calls; loops: host wall "
             f"time per frame; {REPEATS} repeats, the alternatives alternating; min .. max over the repeats"]
    st = torch.cuda.Stream()
    busy = torch.empty((1 << 26,), dtype=torch.float32, device="cuda")
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    pos = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gid = torch.empty((H, W), dtype=torch.int32, device="cuda")
    fmt = lambda v, u=1.0: f"{np.mean(v) * u:9.3f} ({min(v) * u:.3f} .. {max(v) * u:.3f})"     # noqa: E731
    for name, s in (("room", spt.recorded(pkg, "room", "room128x72_static_sepcolor")), ("grid20", spt.grid_scene())):
        ti, bone, weight = height_rig(s["tris"])
        centre = tuple(float(v) for v in np.asarray(s["tris"], np.float32).reshape(-1, 8)[:, 0:3].mean(axis=0))
        tables = {a: torch.from_numpy(D.bend_bones(np.deg2rad(a), centre).view(np.uint8).reshape(-1).copy()).cuda() for a in ANGLES}
        create = lambda: pkg.Scene.create(s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"], s["tri_albedo"])      # noqa: E731
        scenes = dict(refit=create(), lbvh=create(), sah=create())
        for sc in scenes.values():
            sc.enable_pose(s["n_objects"])
        rigs = {k: pkg.DeformRig(sc, ti, bone, weight, 2) for k, sc in scenes.items()}
        t_lbvh, t_sah = pkg.SceneTree.create(scenes["lbvh"], 4), pkg.SahTree(scenes["sah"], 4)
        t_lbvh.build(st); t_sah.build(st)
        st.synchronize()
        t_lbvh.attach(); t_sah.attach()
        trees = dict(refit=lambda: D.scene_refit(scenes["refit"], st), lbvh=lambda: t_lbvh.build(st), sah=lambda: t_sah.build(st))

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

        def loop(n, body):
            st.synchronize()
            t0 = time.perf_counter()
            for f in range(n):
                body(f)
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        def frame(which, angle):
            def body(f):
                rigs[which].apply(tables[angle], stream=st)
                trees[which]()
                scenes[which].draw(rgb, gbt, W, H, s["cam"], s["light"], f, stream=st)
            return body

        for which in scenes:
            loop(2, frame(which, 45.0))
        k_apply, k_draw, k_prev = [], [], []
        for _ in range(REPEATS):
            k_apply.append(event_ms(lambda f: rigs["refit"].apply(tables[45.0], stream=st)))
            k_draw.append(event_ms(lambda f: scenes["refit"].draw(rgb, gbt, W, H, s["cam"], s["light"], f, stream=st)))
            k_prev.append(event_ms(lambda f: rigs["refit"].prev_positions(pos, gid, W, H, s["cam"], stream=st)))
        lines.append(f"{name} ({len(ti)} triangles, all skinned by 2 bones; rig {rigs['refit'].info()['device_bytes'] / 2 ** 20:.1f} MiB)")
        lines.append(f"  svgf_deform_apply {fmt(k_apply, 1e3)} us   svgf_scene_draw {fmt(k_draw)} ms   svgf_deform_prev_positions {fmt(k_prev)} ms "
                     f"({np.mean(k_prev) / np.mean(k_draw):.3f}x the draw; tree refitted at 45 degrees)")
        for angle in ANGLES:
            for which in scenes:
                loop(2, frame(which, angle))
            drawn = [scenes[which].read(0).tobytes() for which in scenes]
            assert drawn[0] == drawn[1] == drawn[2], f"{name}: the three scenes hold different triangles at {angle} degrees"
            wl = {which: [] for which in scenes}
            for _ in range(REPEATS):
                for which in scenes:
                    wl[which].append(loop(16 if name == "room" else 6, frame(which, angle)))
            best = min(wl, key=lambda which: np.mean(wl[which]))
            lines.append(f"  loop at {angle:5.1f} degrees, ms per frame   deform + refit + draw {fmt(wl['refit'])}   deform + LBVH build + draw {fmt(wl['lbvh'])}   "
                         f"deform + SAH build + draw {fmt(wl['sah'])}   fastest: {best}")
        t_lbvh.detach(); t_sah.detach()
        t_lbvh.free(); t_sah.free()
        for which in scenes:
            rigs[which].free(); scenes[which].free()
        print("\n".join(lines[-5:]), flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
