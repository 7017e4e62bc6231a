#!/usr/bin/env python3
"""The device BVH rebuild (row f24, libsvgf_lbvh.so) against what the library had before it, in one process, measured as
tools/scene_pose_time.py measures row f15: device events behind ~2 ms of queued work for single calls, host wall time
per frame for loops, the alternatives alternating, REPEATS times after a warm-up.

  (a) one svgf_lbvh_build (device events), against svgf_bvh_build_host + the upload of its nodes and order on the same triangles
      (host wall time: it blocks the host);
  (b) the loop pose + build + draw (LBVH tree attached), against pose (refit) + draw and against destroy + create + draw;
  (c) k_scene_bvh at 3840x2160 on the LBVH tree against the scene's own SAH tree: at rest, and after row f15's 170 degree turn, where
      the LBVH tree is rebuilt at the pose and the SAH tree refitted.

Before a draw walks a device-built tree it is read back and compared with svgf_lbvh_build_host on the same boxes.
Inputs: the recorded scenes room and bunny, and scene_pose_time's grid of 2^20 triangles.

    python tools/lbvh_time.py [out.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_pose_time as spt  # noqa: E402

REPEATS = 3


def main(out_path=None):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    b = pkg.binding
    W, H = 3840, 2160
    lines = [f"# {torch.cuda.get_device_name(0)}; {W}x{H}; single calls: device events behind ~2 ms of queued work, mean over 20 calls; loops and the host "
             f"build: host wall time per frame; {REPEATS} repeats, the alternatives alternating; all times in ms (min .. max over the repeats)"]
    st = torch.cuda.Stream()
    busy = torch.empty((1 << 26,), dtype=torch.float32, device="cuda")
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    fmt = lambda v: f"{np.mean(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"     # noqa: E731
    for name, s in (("room", spt.recorded(pkg, "room", "room128x72_static_sepcolor")), ("bunny", spt.recorded(pkg, "bunny", "bunny128x72_static")),
                    ("grid", spt.grid_scene())):
        n_obj = s["n_objects"]
        pivot = tuple(float(v) for v in s["tris"].reshape(-1, 8)[:, 0:3].mean(axis=0))

        def table(deg, slide):
            t = b.pose_identity(n_obj)
            t[:] = b.pose_rigid((0, 1, 0) if deg < 90 else (0.3, -0.5, 0.8), np.deg2rad(deg), pivot, (slide, 0, 0))
            return t
        n_frames = 8 if name != "grid" else 3
        tables = [table(9.0 * f / n_frames, 0.25 * f / n_frames) for f in range(n_frames)]
        dev = [torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).cuda() for t in tables]
        host_moved = [spt.moved(s["tris"], s["tri_ids"], t) for t in tables]
        create = lambda tris: pkg.Scene.create(s["geoms"], s["geom_ids"], tris, s["tri_ids"], s["tri_albedo"])      # noqa: E731
        sah, lb = create(s["tris"]), create(s["tris"])
        sah.enable_pose(n_obj); lb.enable_pose(n_obj)
        tree = pkg.SceneTree.create(lb, 4)
        info, ti = sah.info(), tree.info()

        def checked_build():
            tree.build(st)
            st.synchronize()
            nodes, order, _, _ = pkg.lbvh_build_host(lb.read(1), 4)
            got_n, got_o = tree.read(0), tree.read(1)
            assert np.array_equal(got_o, order) and all(np.array_equal(got_n[f], nodes[f]) for f in ("lo", "first", "hi", "count")), \
                f"{name}: the device tree differs from svgf_lbvh_build_host"

        checked_build()
        tree.attach()

        def draw(scene, f):
            scene.draw(rgb, gbt, W, H, s["cam"], s["light"], f, stream=st)

        def event_ms(call, n=20):
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

        def lbvh_frame(f):
            lb.pose(dev[f % n_frames], None, stream=st)
            tree.build(st)
            draw(lb, f)

        def refit_frame(f):
            sah.pose(dev[f % n_frames], None, stream=st)
            draw(sah, f)

        def recreate_frame(f):
            sc = create(host_moved[f % n_frames])
            draw(sc, f)
            sc.free()                           # waits for the device

        loop(3, lbvh_frame); loop(3, refit_frame); loop(1, recreate_frame)
        k_build, w_host, w_lbvh, w_refit, w_rec = [], [], [], [], []
        for _ in range(REPEATS):
            k_build.append(event_ms(lambda f: tree.build(st)))
            w_host.append(host_build())
            w_lbvh.append(loop(10 * n_frames, lbvh_frame))
            w_refit.append(loop(10 * n_frames, refit_frame))
            w_rec.append(loop(n_frames, recreate_frame))
        lines.append(f"{name} ({info['n_tris']} triangles in {n_obj} objects; SAH {info['n_nodes']} nodes, depth {info['depth']}; LBVH {ti['n_nodes']} nodes, "
                     f"key_bits {ti['key_bits']}, depth_bound {ti['depth_bound']}, {ti['launches']} launches, {ti['device_bytes'] / 2 ** 20:.1f} MiB)")
        lines.append(f"  svgf_lbvh_build                       {fmt(k_build)}   svgf_bvh_build_host + upload {fmt(w_host)}   ratio {np.mean(w_host) / np.mean(k_build):.1f}x")
        lines.append(f"  loop  pose + build + draw             {fmt(w_lbvh)}   pose (refit) + draw {fmt(w_refit)}   destroy + create + draw {fmt(w_rec)}")
        for deg in (0.0, 170.0):
            td = torch.from_numpy(table(deg, 0.25 if deg else 0.0).view(np.uint8).reshape(-1).copy()).cuda()
            sah.pose(td, None, stream=st)
            lb.pose(td, None, stream=st)
            checked_build()
            k_lbvh, k_sah = [], []
            for _ in range(REPEATS):
                k_lbvh.append(event_ms(lambda f: draw(lb, f)))
                k_sah.append(event_ms(lambda f: draw(sah, f)))
            what = "at rest:            LBVH" if not deg else f"after {deg:5.1f} deg:    LBVH rebuilt"
            lines.append(f"  k_scene_bvh {what} {fmt(k_lbvh)}   SAH{' refitted' if deg else ''} {fmt(k_sah)}   ratio {np.mean(k_lbvh) / np.mean(k_sah):.2f}x")
        tree.detach()
        tree.free(); sah.free(); lb.free()
        print("\n".join(lines[-5:]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
