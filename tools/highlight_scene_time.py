#!/usr/bin/env python3
"""What the light's term at rough vertices costs (row f23), by the method of tools/rough_scene_time.py: at max_depth 1
and 4 svgf_rough_draw_split (k_scene_gloss<SceneRoughSplitArgs> of libsvgf_rough.so, the yardstick: the parent's code object,
instruction for instruction, in the same process) alternates with svgf_highlight_draw_split (the same text with the light's term,
libsvgf_highlight.so) with enable 0 (the same D, I, colour and G-buffer on bits) and with enable 1, REPEATS times, after a warm-up; the
kernel time is the interval between two device events around one call while the stream is still busy with earlier work (the host side
of the call hides behind it), averaged over the frames of at least MIN_SECONDS.

Two inputs at 3840x2160, a parallelogram light, one shadow ray at the first hit and at every later vertex, one path per pixel, roulette
from bounce 2 on, max_chain 4, guide_alpha 0, out_chain given:
  cornell      the recorded cornell (tests/golden/ref_scenes), frame 0 of its recorded cameras, scene.surface_table and
               scene.roughness_table of its file (SPECEX 5 on its two mirror objects, alpha 0.53); light half-edges 0.5
  rough floor  the room of examples/highlight_scene.cpp at rest (floor a full mirror of alpha 0.1, a mirror sphere, a glass cube, the
               block), the synthetic scene's camera; light half-edges 1.5: most pixels' first hit is rough
Every draw is reported as a multiple of the svgf_rough_draw_split time of the same input, depth and run.

    python tools/highlight_scene_time.py [out.txt]
"""
import os
import sys
import tarfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "tests", "golden", "ref_scenes")
SCENE, REC, W, H = "cornell", "cornell96_static", 3840, 2160
DEPTHS, RR = (1, 4), 2
REPEATS, MIN_SECONDS, MAX_CHAIN = 3, 0.3, 4


def room(pkg):
    """(geoms, surfaces, alphas, camera, light centre, half-edge) of the rough-floor room."""
    z = (0, 0, 0)
    recs = ((0, (0, 0, 0), z, (12, 0.2, 12), (0.8, 0.8, 0.8), 0.0), (0, (0, 5, -6), z, (12, 10, 0.2), (0.8, 0.8, 0.7), 0.0),
            (0, (-6, 5, 0), z, (0.2, 10, 12), (0.8, 0.3, 0.3), 0.0), (0, (6, 5, 0), z, (0.2, 10, 12), (0.3, 0.8, 0.3), 0.0),
            (0, (0, 9.9, 0), z, (3, 0.1, 3), (1, 1, 1), 5.0), (0, (-2.5, 1.1, 0), z, (2, 2, 2), (0.3, 0.4, 0.9), 0.0),
            (1, (0.5, 1.6, -2.5), z, (3, 3, 3), (1, 1, 1), 0.0), (0, (3.2, 1.1, 0.5), z, (2, 2, 2), (1, 1, 1), 0.0))
    geoms = np.zeros(len(recs), dtype=pkg.scene.SCENE_GEOM_DTYPE)
    for g, (kind, trans, rotat, scale, albedo, emit) in zip(geoms, recs):
        xf, inv, invT = pkg.scene._transform(trans, rotat, scale)
        g["type"], g["material"], g["albedo"], g["emittance"] = kind, 0, np.array(albedo, np.float32), np.float32(emit)
        g["xf"], g["inv"], g["invT"] = xf.reshape(-1), inv.reshape(-1), invT.reshape(-1)
    surfaces = np.zeros(len(recs), dtype=[("reflect", "<f4"), ("refract", "<f4"), ("ior", "<f4"), ("spec", "<f4", 3)])
    surfaces["ior"] = 1.0
    surfaces[0] = (1.0, 0.0, 1.0, (0.9, 0.9, 0.9))
    surfaces[6] = (1.0, 0.0, 1.0, (0.95, 0.95, 0.95))
    surfaces[7] = (0.0, 1.0, 1.5, (1.0, 1.0, 1.0))
    alphas = np.zeros(len(recs), np.float32)
    alphas[0] = 0.1
    return geoms, surfaces, alphas, pkg.synth.camera_for_frame(0, False), (0.0, 9.5, 0.0), 1.5


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
    rgb, d_img, i_img = (torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(3))
    chain = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")

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

    z, pi = np.load(os.path.join(REF, REC + ".npz")), np.load(os.path.join(REF, SCENE + "_producer_inputs.npz"))
    with tarfile.open(os.path.join(REF, "scene_files.tar.gz")) as tar:
        parsed = pkg.scene.parse_scene(tar.extractfile(SCENE + ".txt").read().decode())
    c = z["cams"][0]
    rg, rs, ra, rcam, rcentre, redge = room(pkg)
    inputs = {
        "cornell": (pkg.Scene.create(pi["geoms"], pi["geom_ids"], pi["tris"], pi["tri_ids"], pi["tri_albedo"]), pkg.scene.surface_table(parsed),
                    pkg.scene.roughness_table(parsed), dict(right=c[0:3], up=c[3:6], view=c[6:9], position=c[9:12], fovy_deg=float(pi["fovy"])),
                    pkg.scene.light_position(pi["geoms"]), 0.5),
        "rough floor": (pkg.Scene.create(rg, None, None, None, None), rs, ra, rcam, rcentre, redge),
    }
    for iname, (res, surfaces, alphas, cam, centre, edge) in inputs.items():
        info = res.info()
        lt = b.SvgfSceneLight.make(centre, (edge, 0.0, 0.0), (0.0, 0.0, edge), 1)
        table, rough = pkg.GlossTable(surfaces), pkg.RoughTable(alphas)
        calls = {}
        for K in DEPTHS:
            kw = dict(table=table, paths=1, max_depth=K, rr_depth=RR, out_rgb=rgb, stream=st, max_chain=MAX_CHAIN, out_chain=chain, rough=rough, guide_alpha=0.0)
            calls[f"svgf_rough_draw_split, depth {K}"] = lambda f, kw=kw: res.draw_rough_split(d_img, i_img, gbt, W, H, cam, lt, f, **kw)
            for en in (0, 1):
                calls[f"svgf_highlight_draw_split, enable {en}, depth {K}"] = \
                    lambda f, kw=kw, en=en: res.draw_highlight_split(d_img, i_img, gbt, W, H, cam, lt, f, enable=en, clamp=0.0, **kw)
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
        lines.append(f"{iname} ({info['n_tris']} triangles, {info['n_geoms']} primitives; BVH {info['n_nodes']} nodes, depth {info['depth']}) at {W}x{H}, "
                     f"{int((surfaces['reflect'] > 0).sum())} mirror and {int((surfaces['refract'] > 0).sum())} glass objects of {len(surfaces)}; "
                     f"roughness {[round(float(a), 4) for a in alphas]}")
        for name in calls:
            base = np.mean(k["svgf_rough_draw_split, depth " + name.split("depth ")[1]])
            lines.append(f"  {name:56s} {fmt(k[name])}   {np.mean(k[name]) / base:5.3f}x svgf_rough_draw_split of that depth")
    print("\n".join(lines), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
