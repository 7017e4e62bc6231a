#!/usr/bin/env python3
"""svgf_quality_meter at 1920x1080 and 3840x2160, both maps off and on, measured the way 5.4d measured the
histogram: kernel begin / end timestamps of a kernel trace, inputs rotated through more than 400 MB so that no image is still in the
cache when its turn comes again.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o q -- python tools/quality_time.py      # four cases x (6 + 42) meterings
    python tools/quality_time.py --summarize DIR                                                    # one JSON line per case

The cases run one after the other in CASES' order, WARM + LAUNCHES meterings each; --summarize takes the k_quality_tile /
k_quality_resolve rows of the trace in start order, cuts them into the cases, drops each case's first WARM and prints the mean, min
and max of the rest beside the counted bytes (24 B per pixel read, + 4 B per pixel and + 0.25 B per pixel for the maps)."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1920, 1080, False), (1920, 1080, True), (3840, 2160, False), (3840, 2160, True)]
WARM, LAUNCHES, ROTATE_BYTES = 6, 42, 420e6


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {d}")
    rows = {"k_quality_tile": [], "k_quality_resolve": []}
    for row in csv.DictReader(open(files[0])):
        for k in rows:
            if k in row["Kernel_Name"]:
                rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    per = WARM + LAUNCHES
    for k in rows:
        rows[k].sort()
        if len(rows[k]) != per * len(CASES):
            sys.exit(f"{k}: {len(rows[k])} launches in the trace, expected {per * len(CASES)}")
    for c, (W, H, maps) in enumerate(CASES):
        out = dict(size=[W, H], maps=maps)
        for k, name in (("k_quality_tile", "tile"), ("k_quality_resolve", "resolve")):
            us = [(e - s) / 1e3 for s, e in rows[k][c * per + WARM:(c + 1) * per]]
            out[name + "_us"] = round(sum(us) / len(us), 2)
            out[name + "_us_min"], out[name + "_us_max"] = round(min(us), 2), round(max(us), 2)
        nwx, nwy = (W - 8) // 4 + 1, (H - 8) // 4 + 1
        nbytes = 24 * W * H + (4 * W * H + 4 * nwx * nwy if maps else 0)
        out["megabytes"] = round(nbytes / 1e6, 1)
        out["tile_terabytes_per_s"] = round(nbytes / out["tile_us"] / 1e6, 3)
        out["meter_us"] = round(out["tile_us"] + out["resolve_us"], 2)
        print("QUALITY", json.dumps(out))


def run():
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge
    b = ge.load_package().binding
    for W, H, maps in CASES:
        n_pairs = int(ROTATE_BYTES // (24 * W * H)) + 1
        gen = torch.Generator(device="cuda").manual_seed(W)
        pairs = []
        for _ in range(n_pairs):
            ref = torch.rand((H, W, 3), dtype=torch.float32, device="cuda", generator=gen) * 1.5
            pairs.append((ref * (0.9 + 0.2 * torch.rand((H, W, 3), dtype=torch.float32, device="cuda", generator=gen)), ref))
        state = b.quality_state(W, H)
        nwx, nwy = b.quality_windows(W, H)
        se = torch.empty((H, W), dtype=torch.float32, device="cuda") if maps else None
        ss = torch.empty((nwy, nwx), dtype=torch.float32, device="cuda") if maps else None
        torch.cuda.synchronize()
        for i in range(WARM + LAUNCHES):
            a, ref = pairs[i % n_pairs]
            b.quality_meter(state, a, ref, W, H, se_map=se, ssim_map=ss)
        r = b.quality_read(state)
        print(f"{W}x{H} maps {maps}: {n_pairs} pairs rotated, PSNR {r['psnr_db']:.2f} dB, mean SSIM {r['mean_ssim']:.4f}", flush=True)
        del pairs, state, se, ss
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        run()
