"""Which a-trous kernel each level runs, and with which segment geometry — pinned against the CPU oracle level by level.

With kernel_variant 0 every level at steps 2-32 runs the lane-marching kernel (svgf_atrous_lane_impl.h) or the LDS strip kernel
(svgf_atrous_strip.hip), whichever the launch-geometry cost model (csrc/svgf_atrous_geometry.hip; memoised per context by lane_pays,
csrc/svgf_frame.hip) estimates cheaper; each kernel then cuts the image into (strip, y-phase, segment) workgroups by the segment-length
search of the same file (tests/test_kernel_geometry.py holds that arithmetic to a table, and CHOICE_256 below, without a GPU).  The experiments build records
the kernel of every level of the last frame (Denoiser.level_kernels); these tests hold that record to a committed table, tie it
to what the product library computes (bit-identical outputs), and compare EVERY level, not only the last, with the oracle.

The segment-length sweep forces every segment length 1 .. 13 through svgf_exp_set("lane_segrows" / "strip_segrows"): every level
of every length meets the oracle bar, and two lengths differ by no more than rounding (TOL_ACROSS_L).

The frames here run with the reference's default sigmas, on which levels 4 and 5 give their taps next to no weight: the coarse levels
are held to the oracle on frames they act on by tests/test_coarse_levels_gpu.py (inputs and conditions: tests/test_coarse_levels_coverage.py)."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5       # the suite's bar for the lane / strip kernels (test_parity_gpu.TOL_STRIP), here on every level
LEVELS = 5

# Per-level kernel of the automatic choice (kernel_variant 0) on a 256-CU device, steps 2, 4, 8, 16, 32: L lane, s strip.  Taken
# from the library's own estimates (atrous_lane_estimate_us / atrous_strip_estimate_us with n_cu = 256, as lane_pays compares
# them; a frame whose phases are shorter than the segment searches' range is costed as one segment per phase).
CHOICE_256 = {
    (1280, 720): "LLLsL",
    (2560, 1440): "LLLsL",
    (1280, 300): "LLLsL",
    (800, 600): "LLLLs",
    (2560, 240): "sssLL",
    (1024, 768): "sssss",
    (2048, 300): "sssss",
    (1920, 200): "LLLLL",
    (3840, 200): "LLLLL",
    # short frames (H / step < 6 at the coarse steps: one segment per phase).  Before the one-segment costing the empty search
    # range's -1 made these choices: 300x48 was LLLsL, 640x40 LLssL, 64x16 LsLLL; 3840x48 keeps LLLsL, now by the estimates
    (3840, 48): "LLLsL",
    (300, 48): "LLLss",
    (640, 40): "LLsss",
    (64, 16): "Lssss",
}
KIND_LETTER = {"fused": "L", "lane": "L", "strip": "s"}


def with_(params, **kw):
    """A copy of `params` with `kw` set (SvgfParams.set changes the structure in place)."""
    return type(params).from_buffer_copy(params).set(**kw)


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_levels(engine, frames, params):
    """Colour history after the frames, once per history_level 1 .. LEVELS: the output of every level of the last frame."""
    outs = []
    for k in range(1, LEVELS + 1):
        engine.reset()
        for c, g, cam in frames:
            engine.denoise(c, g, cam, with_(params, history_level=k))
        outs.append(engine.read_state(2))
    return outs


class _Host:
    """Denoiser.denoise_host under the Oracle's call names."""

    def __init__(self, d):
        self.d = d

    def reset(self):
        self.d.reset()

    def denoise(self, c, g, cam, p):
        return self.d.denoise_host(c, g, cam, p)

    def read_state(self, which):
        return self.d.read_state(which)


def oracle_levels(o, frames, params):
    """The oracle's output of every level: level k alone needs only the first k levels (atrous_nlevel = k)."""
    outs = []
    for k in range(1, LEVELS + 1):
        o.reset()
        for c, g, cam in frames:
            o.denoise(c, g, cam, with_(params, atrous_nlevel=k, history_level=k))
        outs.append(o.read_state(2))
    return outs


def assert_levels_match_oracle(got, ref, what):
    for k, (a, b) in enumerate(zip(got, ref), start=1):
        e = relerr(a, b).max()
        assert e <= TOL, f"{what}: level {k} vs oracle {e:.3e}"


@pytest.mark.experiments
@pytest.mark.parametrize("temporal", [1, 0], ids=["temporal", "nontemporal"])
@pytest.mark.parametrize("size", list(CHOICE_256), ids=[f"{w}x{h}" for w, h in CHOICE_256])
def test_automatic_choice_per_level_matches_table_and_oracle(pkg, orc, size, temporal):
    W, H = size
    table = CHOICE_256[size]
    pkg.binding.exp_clear()
    frames = [pkg.synth.render_frame(W, H, f, seed=61, moving=True) for f in range(2 if temporal else 1)]
    p = pkg.reference_defaults().set(temporal_enable=temporal, spatial_enable=1, atrous_nlevel=LEVELS, kernel_variant=0)

    # the record of the experiments build
    de = pkg.Denoiser(W, H, 0, experiments=True)
    exp_outs, records = [], []
    for k in range(1, LEVELS + 1):
        de.reset()
        for c, g, cam in frames:
            de.denoise_host(c, g, cam, with_(p, history_level=k))
        exp_outs.append(de.read_state(2))
        records.append(de.level_kernels())
    de.free()
    rec = records[0]
    assert all(r == rec for r in records), f"{W}x{H}: the kernels depend on history_level: {records}"
    assert [s for _, s, _, _ in rec] == [2, 4, 8, 16, 32]
    for kind, step, lane_us, strip_us in rec:
        assert kind in KIND_LETTER, f"{W}x{H} step {step}: {kind}"
        assert lane_us is not None and strip_us is not None, f"{W}x{H} step {step}: the choice was not made from the estimates"
        assert lane_us > 0 and strip_us > 0, f"{W}x{H} step {step}: estimates lane {lane_us} strip {strip_us} us"
        assert (kind != "strip") == (lane_us <= strip_us), f"{W}x{H} step {step}: {kind} against lane {lane_us} strip {strip_us} us"
    # the prepare pass of a non-temporal frame rides in the first level exactly when that level runs the lane kernel
    assert (rec[0][0] == "fused") == (not temporal and rec[0][0] != "strip"), rec
    if device_cus() == 256:
        got = "".join(KIND_LETTER[kind] for kind, _, _, _ in rec)
        assert got == table, f"{W}x{H}: per-level kernels {got}, table {table}"

    # the product library computes what the record describes
    d = pkg.Denoiser(W, H, 0)
    prod_outs = run_levels(_Host(d), frames, p)
    for k in range(LEVELS):
        assert np.array_equal(prod_outs[k], exp_outs[k], equal_nan=True), f"{W}x{H}: level {k + 1}, product != experiments build"
    # a uniform cascade is the forced kernel's cascade, bit for bit (the fused prepare pass equals the prepare kernel)
    kinds = {KIND_LETTER[kind] for kind, _, _, _ in rec}
    if len(kinds) == 1:
        forced = run_levels(_Host(d), frames, with_(p, kernel_variant=4 if kinds == {"L"} else 2))
        for k in range(LEVELS):
            assert np.array_equal(prod_outs[k], forced[k], equal_nan=True), f"{W}x{H}: level {k + 1}, variant 0 != forced {kinds}"
    d.free()

    o = orc.Oracle(pkg, W, H, threads=16)
    ref = oracle_levels(o, frames, p)
    o.free()
    assert_levels_match_oracle(prod_outs, ref, f"{W}x{H} {'temporal' if temporal else 'non-temporal'} {''.join(table)}")


# Segment-length sweep: widths one past a strip / chunk boundary (256-column strips; 480 columns of the lane kernel at steps <= 8,
# 60 lattice columns x 16 at step 16, x 32 at step 32), H = 193: 97 / 49 / 25 / 13 / 7 lattice rows at steps 2 .. 32, so the
# y-phases have unequal lengths and every residue of every segment length occurs.
SWEEP_WIDTHS = (257, 481, 961, 1921)
SWEEP_H = 193
SWEEP_L = range(1, 14)
SWEEP_CFGS = [dict(blur_variance=1), dict(blur_variance=0), dict(blur_variance=1, paper_steps=1)]
SWEEP_KERNELS = [(4, "lane", "lane_segrows"), (2, "strip", "strip_segrows")]
TOL_ACROSS_L = 1e-6      # largest difference between two segment lengths, per level


@pytest.mark.experiments
@pytest.mark.parametrize("W", SWEEP_WIDTHS)
def test_every_segment_length_gives_the_same_levels(pkg, orc, W, experiments_lib):
    H = SWEEP_H
    o = orc.Oracle(pkg, W, H, threads=16)
    worst, spread = {}, {}
    for ci, kw in enumerate(SWEEP_CFGS):
        c, g = pkg.synth.random_frame(W, H, seed=70 + ci)
        cam = pkg.synth.render_frame(8, 8, 0, seed=1, moving=False)[2]
        frames = [(c, g, cam)]
        p = pkg.reference_defaults().set(temporal_enable=0, spatial_enable=1, atrous_nlevel=LEVELS, **kw)
        ref = oracle_levels(o, frames, p)
        steps = [1 << (k - 1 if kw.get("paper_steps") else k) for k in range(1, LEVELS + 1)]
        for variant, kind, knob in SWEEP_KERNELS:
            first = None
            for L in SWEEP_L:
                experiments_lib.exp_set(knob, L)
                d = pkg.Denoiser(W, H, 0)
                outs = run_levels(_Host(d), frames, with_(p, kernel_variant=variant))
                rec = d.level_kernels()
                d.free()
                what = f"{W}x{H} {kind} L={L} {kw}"
                assert [(r[0], r[1]) for r in rec] == [(kind, s) for s in steps], f"{what}: {rec}"
                assert_levels_match_oracle(outs, ref, what)
                for k in range(LEVELS):
                    worst[kind] = max(worst.get(kind, 0.0), float(relerr(outs[k], ref[k]).max()))
                if first is None:
                    first = outs
                    continue
                # not bit for bit: both kernels round an isolated pixel of a segment's last row differently (one ulp at the level
                # that computes it, carried by the levels after it) — far inside the oracle bar, far above what a wrong row gives
                for k in range(LEVELS):
                    e = float(relerr(outs[k], first[k]).max())
                    spread[kind] = max(spread.get(kind, 0.0), e)
                    assert e <= TOL_ACROSS_L, f"{what}: level {k + 1} (step {steps[k]}) vs segment length {SWEEP_L[0]}: {e:.3e}"
            experiments_lib.exp_clear()
    o.free()
    print(f"{W}x{H}: largest per-level error vs oracle {worst}, across segment lengths {spread}")
