#!/usr/bin/env python3
"""Developer tool (GPU box): what the history clamp (svgf_set_history_clamp) buys on a lighting change — the figure of
INTEGRATION.md 5b.

box_room at 96x96, static camera, the turned block moving as in tests/test_motion_vectors.py, temporal pass only, history through
svgf_motion_reproject's plane.  The scene renderer shades without shadow rays, so nothing in this sequence changes the lighting of
a surface that stays put; the change is made here: from frame --switch on, the light is `--dim` times as bright.  Reported per
setting and frame: the mean absolute error of the accumulated colour against the noise-free render of that frame, over the floor
pixels (geomId of the floor, same object in both frames, so their history passes every geometric test).

  python tools/history_clamp_quality.py [--frames 9] [--switch 5] [--dim 0.4]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

MOVING_OBJECT, STEP_X, SIDE = 7, 0.4, 96


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--switch", type=int, default=5)
    ap.add_argument("--dim", type=float, default=0.4)
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    F = np.float32
    sc = pkg.scene.parse_scene(open(os.path.join(ROOT, "tests", "golden", "scenes", "box_room.txt")).read())
    cam = pkg.scene.camera_for_frame(sc, 0, False)
    x0 = sc.objects[MOVING_OBJECT]["trans"][0]
    W = H = SIDE
    frames, prev = [], None
    for f in range(a.frames):
        o = sc.objects[MOVING_OBJECT]
        o["trans"] = (x0 + STEP_X * f,) + tuple(o["trans"][1:])
        g = pkg.scene.geom_array(sc)
        gain = F(a.dim if f >= a.switch else 1.0)
        col, gb = pkg.scene.render_scene(W, H, f, g, cam, seed=3)
        clean, _ = pkg.scene.render_scene(W, H, f, g, cam, seed=3, noise=0.0, fireflies=0.0)
        lit = (gb["geomId"] >= 0) & ~(g["emittance"][np.maximum(gb["geomId"], 0)] > 0)      # the light itself stays as it is
        col = np.where(lit[..., None], col * gain, col).astype(F)
        clean = np.where(lit[..., None], clean * gain, clean).astype(F)
        X = np.tile(np.eye(3, 4).reshape(-1), (len(g), 1))
        if prev is not None:
            for k in range(len(g)):
                m0 = np.vstack([prev[k]["xf"].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
                m1 = np.vstack([g[k]["inv"].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
                X[k] = (m0 @ m1)[:3].reshape(-1)
        frames.append((col, gb, X.astype(F), clean))
        prev = g
    # the floor: of the objects seen from above only (every normal up), the lowest
    gb0 = frames[0][1]
    up = [(float(gb0["position"][gb0["geomId"] == k][:, 1].mean()), k) for k in range(len(prev))
          if np.count_nonzero(gb0["geomId"] == k) and gb0["normal"][gb0["geomId"] == k][:, 1].min() > 0.99]
    floor = min(up)[1]
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=0)
    print(f"box_room {W}x{H}, {a.frames} frames, light x{a.dim} from frame {a.switch} on; floor = object {floor}; "
          f"mean |accumulated - noise-free| over the floor pixels, per frame from the switch on")
    for name, (r, k) in (("clamp off", (0, 0.0)), ("r = 1, k = 1", (1, 1.0)), ("r = 2, k = 1", (2, 1.0)), ("r = 2, k = 2", (2, 2.0)), ("r = 3, k = 1", (3, 1.0))):
        den = pkg.Denoiser(W, H)
        den.set_capture(True)
        den.set_history_clamp(r, k)
        mv = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        errs = []
        for f, (col, gb, X, clean) in enumerate(frames):
            t_c = torch.from_numpy(np.ascontiguousarray(col)).cuda()
            t_g = torch.from_numpy(gb.view(np.uint8).reshape(-1).copy()).cuda()
            t_x = torch.from_numpy(X).cuda()
            pkg.binding.motion_reproject(mv, W, H, cam, gbuffer=t_g, geom_xf=t_x)
            den.denoise(out, t_c, t_g, cam, p, motion=mv)
            den.sync()
            acc = den.read_state(pkg.binding.STATE_COLOR_ACC)
            m = gb["geomId"] == floor
            errs.append(float(np.abs(acc[m].astype(np.float64) - clean.reshape(H, W, 3)[m]).mean()))
        den.free()
        print(f"{name:14s} before the switch (frame {a.switch - 1}): {errs[a.switch - 1]:.4f}; from it on: " + " ".join(f"{e:.4f}" for e in errs[a.switch:]))


if __name__ == "__main__":
    main()
