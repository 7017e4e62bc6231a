#!/usr/bin/env python3
"""The device SAH build (row f25, libsvgf_sah.so) beside row f24's LBVH build and the scene's own tree, in one process, measured as
tools/lbvh_time.py measures row f24: device events behind ~2 ms of queued work for single calls, host wall time per frame for loops,
the alternatives alternating, REPEATS times after a warm-up.

  (a) one svgf_sah_build and one svgf_lbvh_build (device events), against svgf_bvh_build_host + the upload of its nodes and order on
      the same triangles (host wall time: it blocks the host);
  (b) svgf_scene_draw and svgf_path_draw (depth 4, one path) at 3840x2160 on three trees over the same triangles at rest: the scene's
      own, the device SAH tree (the same tree in the sparse layout; held on bytes) and the LBVH tree;
  (c) the loops pose + svgf_sah_build + draw, pose + svgf_lbvh_build + draw and pose (refit) + draw, for both draws.

Before a draw walks a device-built tree it is read back and compared: the SAH tree with the relaid svgf_bvh_build_host tree of the
triangles as drawn, the LBVH tree with svgf_lbvh_build_host.
Inputs: the recorded scenes room and bunny, and scene_pose_time's grid at 2^16 and 2^20 triangles.

    python tools/sah_time.py [out.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_pose_time as spt  # noqa: E402

REPEATS = 2


def main(out_path=None):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    import sah_model as sm
    pkg = ge.load_package()
    b = pkg.binding
    W, H = 3840, 2160
    lines = [f"# {torch.cuda.get_device_name(0)}; {W}x{H}; single calls: device events behind ~2 ms of queued work, mean over 10 calls; loops and the host "
             f"build: host wall time per frame; {REPEATS} repeats, the alternatives alternating; all times in ms (min .. max over the repeats)"]
    st = torch.cuda.Stream()
    busy = torch.empty((1 << 26,), dtype=torch.float32, device="cuda")
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    fmt = lambda v: f"{np.mean(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"     # noqa: E731
    for name, s in (("room", spt.recorded(pkg, "room", "room128x72_static_sepcolor")), ("bunny", spt.recorded(pkg, "bunny", "bunny128x72_static")),
                    ("grid16", spt.grid_scene(181)), ("grid20", spt.grid_scene())):
        n_obj = s["n_objects"]
        pivot = tuple(float(v) for v in s["tris"].reshape(-1, 8)[:, 0:3].mean(axis=0))
        light = b.SvgfSceneLight.make(tuple(float(c) for c in s["light"]), (0.4, 0.0, 0.0), (0.0, 0.0, 0.4), 1)

        def table(deg, slide):
            t = b.pose_identity(n_obj)
            t[:] = b.pose_rigid((0, 1, 0), np.deg2rad(deg), pivot, (slide, 0, 0))
            return t
        n_frames = 8 if name != "grid20" else 3
        dev = [torch.from_numpy(table(9.0 * f / n_frames, 0.25 * f / n_frames).view(np.uint8).reshape(-1).copy()).cuda() for f in range(n_frames)]
        create = lambda: pkg.Scene.create(s["geoms"], s["geom_ids"], s["tris"], s["tri_ids"], s["tri_albedo"])      # noqa: E731
        scenes = dict(own=create(), sah=create(), lbvh=create())
        for sc in scenes.values():
            sc.enable_pose(n_obj)
        t_sah, t_lbvh = pkg.SahTree(scenes["sah"], 4), pkg.SceneTree.create(scenes["lbvh"], 4)
        builders = dict(own=None, sah=t_sah, lbvh=t_lbvh)

        def checked_builds():
            t_sah.build(st); t_lbvh.build(st)
            st.synchronize()
            nodes, order, _ = pkg.bvh_build_host(scenes["sah"].read(0), 4, 0)
            sm.same_tree(t_sah.read(0), t_sah.read(1), sm.relayout(nodes, len(order)), order, f"{name}: the device SAH tree vs svgf_bvh_build_host", bytes_too=True)
            nodes, order, _, _ = pkg.lbvh_build_host(scenes["lbvh"].read(1), 4)
            assert np.array_equal(t_lbvh.read(1), order) and t_lbvh.read(0).tobytes() == nodes.tobytes(), f"{name}: the device LBVH tree differs from svgf_lbvh_build_host"

        checked_builds()
        t_sah.attach(); t_lbvh.attach()
        draws = dict(scene=lambda sc, f: sc.draw(rgb, gbt, W, H, s["cam"], s["light"], f, stream=st),
                     path=lambda sc, f: sc.draw_path(rgb, gbt, W, H, s["cam"], light, f, paths=1, max_depth=4, stream=st))

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

        def host_build():
            st.synchronize()
            t0 = time.perf_counter()
            nodes, order, _ = pkg.bvh_build_host(s["tris"], 4, 0)
            keep = (torch.from_numpy(nodes.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(order).cuda())
            torch.cuda.synchronize()
            del keep
            return (time.perf_counter() - t0) * 1e3

        def loop(n, body):
            st.synchronize()
            t0 = time.perf_counter()
            for f in range(n):
                body(f)
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        def frame(which, draw):
            def body(f):
                scenes[which].pose(dev[f % n_frames], None, stream=st)
                if builders[which]:
                    builders[which].build(st)
                draws[draw](scenes[which], f)
            return body

        for which in scenes:
            for d in draws:
                loop(2, frame(which, d))
        rest = torch.from_numpy(b.pose_identity(n_obj).view(np.uint8).reshape(-1).copy()).cuda()
        for sc in scenes.values():               # the timed draws run AT REST: the device SAH tree is then the scene's own tree in the
            sc.pose(rest, None, stream=st)       # sparse layout (held below), so (b) prices the layout and nothing else
        checked_builds()
        same = sm.relayout(scenes["own"].read(2), len(scenes["own"].read(4))).tobytes() == t_sah.read(0).tobytes() and \
            scenes["own"].read(4).tobytes() == t_sah.read(1).tobytes()
        k = {key: [] for key in ("sah", "lbvh", "host")}
        kd = {(d, which): [] for d in draws for which in scenes}
        wl = {(d, which): [] for d in draws for which in scenes}
        for _ in range(REPEATS):
            k["sah"].append(event_ms(lambda f: t_sah.build(st)))
            k["lbvh"].append(event_ms(lambda f: t_lbvh.build(st)))
            k["host"].append(host_build())
            for d in draws:
                for which in scenes:
                    kd[d, which].append(event_ms(lambda f: draws[d](scenes[which], f)))
        for _ in range(REPEATS):
            for d in draws:
                for which in scenes:
                    wl[d, which].append(loop(4 * n_frames, frame(which, d)))
        si, li, c = t_sah.info(), t_lbvh.info(), t_sah.counts()
        lines.append(f"{name} ({si['n_tris']} triangles in {n_obj} objects; SAH tree {c['n_nodes']} nodes in {si['n_records']} records, depth {c['depth']}, "
                     f"{si['launches']} launches, {si['device_bytes'] / 2 ** 20:.1f} MiB; LBVH {li['n_nodes']} nodes, {li['launches']} launches)")
        lines.append(f"  build   svgf_sah_build {fmt(k['sah'])}   svgf_lbvh_build {fmt(k['lbvh'])}   svgf_bvh_build_host + upload {fmt(k['host'])}")
        for d in draws:
            own = np.mean(kd[d, "own"])
            lines.append(f"  draw {d:5s}  (at rest; device SAH == own tree relaid: {'yes' if same else 'NO'})  own tree {fmt(kd[d, 'own'])}   device SAH {fmt(kd[d, 'sah'])} ({np.mean(kd[d, 'sah']) / own:.3f}x)   "
                         f"LBVH {fmt(kd[d, 'lbvh'])} ({np.mean(kd[d, 'lbvh']) / own:.3f}x)")
        for d in draws:
            lines.append(f"  loop {d:5s}  pose (refit) + draw {fmt(wl[d, 'own'])}   pose + SAH build + draw {fmt(wl[d, 'sah'])}   pose + LBVH build + draw {fmt(wl[d, 'lbvh'])}")
        t_sah.detach(); t_lbvh.detach()
        t_sah.free(); t_lbvh.free()
        for sc in scenes.values():
            sc.free()
        print("\n".join(lines[-6:]), flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
