#!/usr/bin/env python3
"""What the rough lobe costs (row f22), by the method of tools/virtual_scene_time.py: at max_depth 1, 4 and 8
svgf_virtual_draw_split (k_scene_gloss<SceneVirtualSplitArgs> of libsvgf_virtual.so, the yardstick: the parent's code in the same
process) alternates with svgf_rough_draw_split (the same text with the lobe, libsvgf_rough.so), with no roughness table (the same D, I,
colour and G-buffer on bits) and with the scene's own (scene.roughness_table of cornell.txt: SPECEX 5 on its two mirror objects,
alpha 0.53), REPEATS times, after a warm-up; the kernel time is the interval between two device events around one call while the
stream is still busy with earlier work (the host side of the call hides behind it), averaged over the frames of at least MIN_SECONDS.

Input: the recorded cornell (tests/golden/ref_scenes), frame 0 of its recorded cameras, at 1920x1080, with scene.surface_table of its
file; a parallelogram light (half-edges 0.5 in x and z) at the scene's light, one shadow ray at the first hit and at every later
vertex, one path per pixel, roulette from bounce 2 on; max_chain 4, guide_alpha 0, out_chain given.  Every draw is reported as a
multiple of the svgf_virtual_draw_split time of the same depth and run.

    python tools/rough_scene_time.py [out.txt]
"""
import os
import sys
import tarfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_scenes")
SCENE, REC, W, H = "cornell", "cornell96_static", 1920, 1080
DEPTHS, RR = (1, 4, 8), 2
REPEATS, MIN_SECONDS, MAX_CHAIN = 3, 0.3, 4


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
    z, pi = np.load(os.path.join(REF, REC + ".npz")), np.load(os.path.join(REF, SCENE + "_producer_inputs.npz"))
    with tarfile.open(os.path.join(REF, "scene_files.tar.gz")) as tar:
        parsed = pkg.scene.parse_scene(tar.extractfile(SCENE + ".txt").read().decode())
    surfaces, alphas = pkg.scene.surface_table(parsed), pkg.scene.roughness_table(parsed)
    c = z["cams"][0]
    cam = dict(right=c[0:3], up=c[3:6], view=c[6:9], position=c[9:12], fovy_deg=float(pi["fovy"]))
    light = pkg.scene.light_position(pi["geoms"])
    rgb, d_img, i_img = (torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(3))
    chain = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    res = pkg.Scene.create(pi["geoms"], pi["geom_ids"], pi["tris"], pi["tri_ids"], pi["tri_albedo"])
    info = res.info()
    lt = b.SvgfSceneLight.make(light, (0.5, 0.0, 0.0), (0.0, 0.0, 0.5), 1)
    table, rough = pkg.GlossTable(surfaces), pkg.RoughTable(alphas)

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

    calls = {}
    for K in DEPTHS:
        calls[f"svgf_virtual_draw_split, depth {K}"] = \
            lambda f, K=K: res.draw_virtual_split(d_img, i_img, gbt, W, H, cam, lt, f, table=table, paths=1, max_depth=K, rr_depth=RR, out_rgb=rgb,
                                                  stream=st, max_chain=MAX_CHAIN, out_chain=chain)
        for rname, rt in (("no roughness table", None), ("cornell's roughness", rough)):
            calls[f"svgf_rough_draw_split, {rname}, depth {K}"] = \
                lambda f, K=K, rt=rt: res.draw_rough_split(d_img, i_img, gbt, W, H, cam, lt, f, table=table, paths=1, max_depth=K, rr_depth=RR,
                                                           out_rgb=rgb, stream=st, max_chain=MAX_CHAIN, out_chain=chain, rough=rt, guide_alpha=0.0)
    n = {}
    for name, call in calls.items():        # warm-up, and how many frames make MIN_SECONDS
        kernel_ms(call, 3)
        n[name] = min(200, max(5, int(MIN_SECONDS * 1e3 / (kernel_ms(call, 5) + 2.0)) + 1))
    k = {name: [] for name in calls}
    for _ in range(REPEATS):
        for name, call in calls.items():
            k[name].append(kernel_ms(call, n[name]))
    table.free(); rough.free(); res.free()
    fmt = lambda v: f"{np.mean(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"     # noqa: E731
    lines.append(f"{SCENE} ({info['n_tris']} triangles, {info['n_geoms']} primitives; BVH {info['n_nodes']} nodes, depth {info['depth']}) at {W}x{H}, "
                 f"{int((surfaces['reflect'] > 0).sum())} mirror and {int((surfaces['refract'] > 0).sum())} glass objects of {len(surfaces)}; "
                 f"roughness {[round(float(a), 4) for a in alphas]}")
    for name in calls:
        base = np.mean(k["svgf_virtual_draw_split, depth " + name.split("depth ")[1]])
        lines.append(f"  {name:56s} {fmt(k[name])}   {np.mean(k[name]) / base:5.3f}x svgf_virtual_draw_split of that depth")
    print("\n".join(lines), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
