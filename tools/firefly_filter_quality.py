#!/usr/bin/env python3
"""Developer tool (GPU box): what the firefly filter (svgf_set_firefly_filter) buys on the project's own noise model — the figures
of INTEGRATION.md 5d.

The synthetic scene at 96x96 under a static camera, noise_model "hash" (multiplicative noise, 2 % of the pixels 6x brighter).
Reported per setting: mean absolute error and mean ratio against the noise-free render, of the input image of the last frame (raw,
and filtered by the library: a non-temporal pass-through frame returns F(in_rgb)) and of the accumulated colour of the temporal
pass after --frames frames; and the price on an input without fireflies (pixels touched, mean ratio).

  python tools/firefly_filter_quality.py [--frames 8] [--size 96] [--scale 1.0]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=31)
    a = ap.parse_args()
    pkg = ge.load_package()
    F = np.float32
    W = H = a.size
    render = lambda f, **kw: pkg.synth.render_frame(W, H, f, seed=a.seed, moving=False, noise_model="hash", **kw)      # noqa: E731
    frames = [render(f) for f in range(a.frames)]
    no_flies = np.asarray(render(a.frames - 1, fireflies=0.0)[0], F).reshape(H, W, 3)
    clean = np.asarray(render(a.frames - 1, noise=0.0, fireflies=0.0)[0], F).reshape(H, W, 3).astype(np.float64)
    mae = lambda x: float(np.abs(np.asarray(x, np.float64).reshape(H, W, 3) - clean).mean())      # noqa: E731
    ratio = lambda x: float(np.asarray(x, np.float64).mean() / clean.mean())      # noqa: E731
    temporal = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=0)
    through = pkg.reference_defaults().set(temporal_enable=0, spatial_enable=0)      # prepare pass + copy: the output is F(in_rgb)
    print(f"synthetic scene {W}x{H}, static camera, {a.frames} frames, scale {a.scale}: MAE / mean ratio against the noise-free render")
    print(f"{'':10s} {'input':>16s} {'accumulated':>16s}   on an input without fireflies")
    for rank in (0, 1, 2, 3):
        d = pkg.Denoiser(W, H)
        d.set_capture(True)
        d.set_firefly_filter(rank, a.scale)
        for c, g, cam in frames:
            d.denoise_host(c, g, cam, temporal)
        acc = d.read_state(pkg.binding.STATE_COLOR_ACC)
        d.free()
        e = pkg.Denoiser(W, H)
        e.set_firefly_filter(rank, a.scale)
        c, g, cam = frames[-1]
        fin = e.denoise_host(c, g, cam, through)
        fno = e.denoise_host(no_flies, g, cam, through)
        e.free()
        touched = float((np.asarray(fno).reshape(H, W, 3) != no_flies).any(axis=-1).mean())
        name = "filter off" if rank == 0 else f"rank {rank}"
        print(f"{name:10s} {mae(fin):8.4f} {ratio(fin):7.3f} {mae(acc):8.4f} {ratio(acc):7.3f}   "
              f"{100 * touched:5.1f} % of the pixels touched, mean x{float(np.asarray(fno, np.float64).mean() / no_flies.astype(np.float64).mean()):.3f}")


if __name__ == "__main__":
    main()
