#!/usr/bin/env python3
"""The animated resident scene (row f15) against the only alternative the library had before it, in one process:

  (a) one svgf_scene_pose (pose + refit, two or three launches): device events around the call while the stream is still busy with
      earlier work, so the host side of the call hides behind that work;
  (b) wall time per frame of a loop "pose + draw", host clock from the first call to the end of a final synchronisation, against
      the loop "svgf_scene_destroy + svgf_scene_create on triangles moved on the host + svgf_scene_draw" (the triangles are moved
      before the clock starts: the loop pays the build, the allocation, the upload and the waits, not the numpy arithmetic);
  (c) k_scene_bvh on the REFITTED tree after a 9 degree and a 170 degree pose, against a tree rebuilt at that pose: the price of
      not re-splitting.

The two loops of (b) alternate, REPEATS times, after a warm-up.  Inputs: the recorded reference scenes room and bunny
(tests/golden/ref_scenes, every mesh object posed) at 3840x2160, and a synthetic grid of 2^20 triangles in 16 objects.

    python tools/scene_pose_time.py [out.txt]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_scenes")
REPEATS = 3
F = np.float32


def grid_scene(side=724, n_objects=16):
    """side x side quads (2 triangles each, 2 * 724^2 = 1 048 352 <= 2^20 triangles) in the plane z = 0, facing +z, cut into
    n_objects vertical bands; a camera in front of it."""
    ys, xs = np.mgrid[0:side, 0:side].astype(F)
    s = F(8.0 / side)
    x0, y0 = (xs.reshape(-1) * s - 4).astype(F), (ys.reshape(-1) * s - 4).astype(F)
    n = 2 * side * side
    tris = np.zeros((n, 3, 8), F)
    tris[:, :, 5] = 1.0
    corners = [((0, 0), (1, 0), (0, 1)), ((1, 0), (1, 1), (0, 1))]
    for h, tri in enumerate(corners):
        for v, (dx, dy) in enumerate(tri):
            tris[h::2, v, 0], tris[h::2, v, 1] = x0 + dx * s, y0 + dy * s
    ids = np.repeat((xs.reshape(-1) * n_objects // side).astype(np.int32), 2)
    alb = np.random.default_rng(15).uniform(0.2, 0.9, (n, 3)).astype(F)
    cam = dict(right=(-1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), view=(0.0, 0.0, -1.0), position=(0.0, 0.0, 10.0), fovy_deg=45.0)
    return dict(geoms=None, geom_ids=None, tris=tris, tri_ids=ids, tri_albedo=alb, cam=cam, light=(0.0, 3.0, 8.0), n_objects=n_objects)


def recorded(pkg, scene, rec):
    z, pi = np.load(os.path.join(REF, rec + ".npz")), np.load(os.path.join(REF, scene + "_producer_inputs.npz"))
    c = z["cams"][0]
    cam = dict(right=c[0:3], up=c[3:6], view=c[6:9], position=c[9:12], fovy_deg=float(pi["fovy"]))
    return dict(geoms=pi["geoms"], geom_ids=pi["geom_ids"], tris=pi["tris"], tri_ids=pi["tri_ids"], tri_albedo=pi["tri_albedo"], cam=cam,
                light=pkg.scene.light_position(pi["geoms"]), n_objects=int(pi["tri_ids"].max()) + 1)


def moved(tris, ids, table):
    """The triangles moved on the host (float32 matmul: the timing does not need the library's rounding)."""
    T = np.array(tris, F).reshape(-1, 3, 8)
    M = table["xf"][ids].reshape(-1, 3, 4)
    T[:, :, 0:3] = np.einsum("nrc,nvc->nvr", M[:, :, 0:3], T[:, :, 0:3]) + M[:, None, :, 3]
    T[:, :, 3:6] = np.einsum("nrc,nvc->nvr", M[:, :, 0:3], T[:, :, 3:6])
    return T


def main(out_path=None):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    b = pkg.binding
    W, H = 3840, 2160
    lines = [f"# {torch.cuda.get_device_name(0)}; {W}x{H}; pose: device events around one svgf_scene_pose behind ~2 ms of queued work, mean over 50 calls; "
             f"loops: host wall time per frame; {REPEATS} repeats, the two loops alternating; all times in ms (min .. max over the repeats)"]
    st = torch.cuda.Stream()
    busy = torch.empty((1 << 26,), dtype=torch.float32, device="cuda")
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    fmt = lambda v: f"{np.mean(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"     # noqa: E731
    for name, s in (("room", recorded(pkg, "room", "room128x72_static_sepcolor")), ("bunny", recorded(pkg, "bunny", "bunny128x72_static")),
                    ("grid", grid_scene())):
        n_obj = s["n_objects"]
        pivot = tuple(float(v) for v in s["tris"].reshape(-1, 8)[:, 0:3].mean(axis=0))

        def table(deg, slide):
            t = b.pose_identity(n_obj)
            t[:] = b.pose_rigid((0, 1, 0) if deg < 90 else (0.3, -0.5, 0.8), np.deg2rad(deg), pivot, (slide, 0, 0))
            return t
        n_frames = 8 if name != "grid" else 3
        tables = [table(9.0 * f / n_frames, 0.25 * f / n_frames) for f in range(n_frames)]
        dev = [torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).cuda() for t in tables]
        host_moved = [moved(s["tris"], s["tri_ids"], t) for t in tables]
        motion = torch.empty((n_obj, 12), dtype=torch.float32, device="cuda")
        create = lambda tris: pkg.Scene.create(s["geoms"], s["geom_ids"], tris, s["tri_ids"], s["tri_albedo"])      # noqa: E731
        res = create(s["tris"])
        res.enable_pose(n_obj)
        info = res.info()

        def draw(scene, f):
            scene.draw(rgb, gbt, W, H, s["cam"], s["light"], f, stream=st)

        def event_ms(call, n):
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

        def pose_loop(n):
            st.synchronize()
            t0 = time.perf_counter()
            for f in range(n):
                res.pose(dev[f % n_frames], motion, stream=st)
                draw(res, f)
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        def recreate_loop(n):
            st.synchronize()
            t0 = time.perf_counter()
            for f in range(n):
                sc = create(host_moved[f % n_frames])
                draw(sc, f)
                sc.free()                       # waits for the device
            st.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

        pose_loop(3); recreate_loop(1)
        k_pose, w_pose, w_rec = [], [], []
        for _ in range(REPEATS):
            k_pose.append(event_ms(lambda f: res.pose(dev[f % n_frames], motion, stream=st), 50))
            w_pose.append(pose_loop(10 * n_frames))
            w_rec.append(recreate_loop(n_frames))
        lines.append(f"{name} ({info['n_tris']} triangles in {n_obj} objects; BVH {info['n_nodes']} nodes, depth {info['depth']})")
        lines.append(f"  svgf_scene_pose                       {fmt(k_pose)}")
        lines.append(f"  loop  pose + draw                     {fmt(w_pose)}   destroy + create + draw {fmt(w_rec)}   ratio {np.mean(w_rec) / np.mean(w_pose):.1f}x")
        for deg in (9.0, 170.0):
            t = table(deg, 0.25)
            td = torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).cuda()
            res.pose(td, None, stream=st)
            rebuilt = create(moved(s["tris"], s["tri_ids"], t))
            k_refit, k_rebuilt = [], []
            for _ in range(REPEATS):
                k_refit.append(event_ms(lambda f: draw(res, f), 20))
                k_rebuilt.append(event_ms(lambda f: draw(rebuilt, f), 20))
            rebuilt.free()
            lines.append(f"  k_scene_bvh after {deg:5.1f} deg: refitted {fmt(k_refit)}   rebuilt {fmt(k_rebuilt)}   ratio {np.mean(k_refit) / np.mean(k_rebuilt):.2f}x")
        res.free()
        print("\n".join(lines[-5:]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
