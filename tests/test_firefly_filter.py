"""Firefly filter of the input colour (include/svgf.h: svgf_set_firefly_filter / svgf_get_firefly_filter).

The statement of the feature is one sentence: with the filter on, a frame runs exactly as if in_rgb had been F(in_rgb).  So the
yardstick is tests/firefly_model.py (F in float32 numpy) in front of tests/temporal_model.py (the whole temporal pass), and, for
whole frames, the library itself with the filter off on the model-filtered input.

Bounds: every comparison of a kernel with the model, and of a filtered frame with the unfiltered frame on filtered input, is on
the bits of every pixel (NaNs in the same place count as equal).  Both sides perform the same correctly rounded float32
operations in the same order without contraction: there is no arithmetic that may differ, so there is no tolerance to choose.
The one tolerance in this file, 1e-5 on kernel_variant 0's non-temporal frame, is the project's existing gate between its a-trous
kernels (tests/test_parity_gpu.py): there the filtered frame runs the prepare kernel and the lane kernel where the unfiltered
frame runs the prepare pass inside the first level.  The one tolerance on the model alone, 4 * 2^-24 relative on the luminance
of a clamped pixel, is three roundings: the quotient s, the product c * s, and the luminance of the result."""
import ctypes

import numpy as np
import pytest

import firefly_model as ff
import temporal_model as tm
from conftest import relerr
from temporal_harness import (MOVING_FRAMES, SIDE, _whole_frames, assert_frames_equal, moving_block_sequence, run_gpu, same_bits,
                              scales, synth_params, synth_sequence, temporal_only)

F = np.float32
COORD, D32, D16 = tm.COORD, tm.D32, tm.D16
NEW_SYMBOLS = ("svgf_set_firefly_filter", "svgf_get_firefly_filter")
RANKS = (1, 2, 3)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def camera_planes(pkg, seq, fmt):
    """Per frame the plane svgf_motion_reproject writes for the previous frame's camera and synth_params' reproj_scale (frame 0: its
    own camera; never looked at)."""
    H, W = seq[0][1].shape
    sx, sy = scales(pkg, W, H)
    return [tm.motion_plane(seq[max(f - 1, 0)][3], W, H, seq[f][1], None, fmt, F(sx), F(sy)) for f in range(len(seq))]


def filtered(frames, rank, scale):
    """[(colour, texels, ...)] with every colour replaced by F(colour)."""
    return [(ff.firefly_filter(fr[0], rank, scale),) + tuple(fr[1:]) for fr in frames]


def model_on(pkg, seq, fmt, rank, scale, radius, k, tag):
    """The model of the temporal pass on the FILTERED frames of a synthetic sequence, history looked up through the camera plane of
    format `fmt` converted as the header says, clamp (radius, k) — whose statistics are then the filtered colour's."""
    cache = model_on.__dict__.setdefault("cache", {})
    key = (tag, fmt, rank, scale, radius, k)
    if key not in cache:
        H, W = seq[0][1].shape
        coords = [tm.coord_plane(pl, fmt, W, H) for pl in camera_planes(pkg, seq, fmt)]
        cache[key] = tm.run_sequence(filtered([(c, g) for c, g, _, _ in seq], rank, scale), coords, radius=radius, k=k)
    return cache[key]


def grey(H, W, v=0.5):
    return np.full((H, W, 3), v, F)


# ---- 1. CPU: symbols and the NULL context ----------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_a_null_context_is_invalid(pkg):
    lib = pkg.load_library()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in pkg.binding.EXPORTS, n
    assert lib.svgf_set_firefly_filter(None, 1, 1.0) == -1
    assert lib.svgf_set_firefly_filter(None, 0, 0.0) == -1
    r, k = ctypes.c_int(7), ctypes.c_float(7.0)
    assert lib.svgf_get_firefly_filter(None, ctypes.byref(r), ctypes.byref(k)) == -1
    assert lib.svgf_get_firefly_filter(None, None, None) == -1
    assert (r.value, k.value) == (7, 7.0), "nothing is written on failure"
    assert hasattr(pkg.Denoiser, "set_firefly_filter") and hasattr(pkg.Denoiser, "firefly_filter")


# ---- 2. CPU: the model's properties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", RANKS)
def test_model_a_constant_image_comes_back_with_identical_bits(rank):
    img = np.tile(np.array([0.3, 0.7, 0.1], F), (7, 9, 1))
    for scale in (1.0, 1.5):
        assert same_bits(ff.firefly_filter(img, rank, scale), img)
    assert same_bits(ff.firefly_filter(img, 0, 1.0), img), "rank 0 is the identity"


@pytest.mark.parametrize("scale", [1.0, 1.5])
@pytest.mark.parametrize("rank", RANKS)
def test_model_one_spike_on_grey_is_brought_to_the_bound_and_nothing_else_changes(rank, scale):
    img = grey(7, 9)
    img[3, 4] = (5.0, 3.0, 8.0)
    out = ff.firefly_filter(img, rank, scale)
    changed = (out != img).any(axis=-1)
    want = np.zeros((7, 9), bool)
    want[3, 4] = True
    assert np.array_equal(changed, want)
    bound = float(F(scale) * tm.luminance(grey(1, 1))[0, 0])
    got = float(tm.luminance(out)[3, 4])
    assert abs(got - bound) <= 4 * 2.0 ** -24 * bound, (got, bound)


def test_model_two_adjacent_spikes_survive_rank_1_and_fall_to_rank_2():
    img = grey(7, 9)
    img[3, 4] = img[3, 5] = (6.0, 6.0, 6.0)
    assert same_bits(ff.firefly_filter(img, 1, 1.0), img), "each is the other's largest neighbour"
    out = ff.firefly_filter(img, 2, 1.0)
    changed = (out != img).any(axis=-1)
    assert changed[3, 4] and changed[3, 5] and np.count_nonzero(changed) == 2
    bound = float(tm.luminance(grey(1, 1))[0, 0])
    for x in (4, 5):
        assert abs(float(tm.luminance(out)[3, x]) - bound) <= 4 * 2.0 ** -24 * bound


def test_model_image_edges_nan_and_scale_zero():
    one = np.array([[[3.0, 2.0, 1.0]]], F)
    for rank in RANKS:
        assert same_bits(ff.firefly_filter(one, rank, 0.0), one), "1x1: no neighbour, unchanged"
    # 1 x N: an end has one neighbour, which is its bound at every rank (B = t[min(rank, n) - 1])
    row = np.array([1.0, 5.0, 1.0, 9.0], F)[None, :, None] * np.ones(3, F)
    for rank in RANKS:
        out = ff.firefly_filter(row, rank, 1.0)
        assert same_bits(out[0, 0], row[0, 0]), "the dark end stays"
        l3 = float(tm.luminance(out)[0, 3])
        assert abs(l3 - 1.0) <= 4 * 2.0 ** -24, (rank, l3)
    assert abs(float(tm.luminance(ff.firefly_filter(row, 1, 1.0))[0, 1]) - 1.0) <= 4 * 2.0 ** -24
    # N x 1 likewise
    col = np.transpose(row, (1, 0, 2)).copy()
    assert same_bits(np.transpose(ff.firefly_filter(col, 2, 1.0), (1, 0, 2)), ff.firefly_filter(row, 2, 1.0))
    # a NaN neighbour is not counted: the centre's only counted neighbour is 1, at rank 2 too (counted, n would be 2 and B = -inf)
    nn = np.array([np.nan, 5.0, 1.0], F)[None, :, None] * np.ones(3, F)
    for rank in RANKS:
        out = ff.firefly_filter(nn, rank, 1.0)
        assert abs(float(tm.luminance(out)[0, 1]) - 1.0) <= 4 * 2.0 ** -24, rank
        assert np.isnan(out[0, 0]).all(), "a NaN centre is unchanged"
        assert same_bits(out[0, 0], nn[0, 0]) and same_bits(out[0, 2], nn[0, 2])
    # one NaN channel makes the centre's luminance NaN: unchanged, bit for bit
    part = grey(3, 3)
    part[1, 1] = (np.nan, 50.0, 50.0)
    assert same_bits(ff.firefly_filter(part, 1, 1.0)[1, 1], part[1, 1])
    # scale 0: every pixel with a counted neighbour and positive luminance becomes 0
    rng = np.random.default_rng(3)
    img = rng.uniform(0.1, 2.0, (6, 5, 3)).astype(F)
    for rank in RANKS:
        assert (ff.firefly_filter(img, rank, 0.0) == 0).all()
    # the arithmetic runs as written: an infinite centre over a finite bound gives s = 0 and inf * 0 = NaN
    inf = grey(3, 3)
    inf[1, 1] = (np.inf, 1.0, 1.0)
    out = ff.firefly_filter(inf, 1, 1.0)[1, 1]
    assert np.isnan(out[0]) and out[1] == 0 and out[2] == 0


# ---- 3. CPU: what it is for ------------------------------------------------------------------------------------------------------------------
def test_model_rank_1_scale_1_brings_the_project_s_noisy_frame_closer_to_the_noise_free_render(pkg):
    """synth.render_frame(96, 96, 2, seed=31, noise_model="hash"): two strict inequalities, no threshold."""
    W = H = 96
    noisy = np.asarray(pkg.synth.render_frame(W, H, 2, seed=31, noise_model="hash")[0], F).reshape(H, W, 3)
    clean = np.asarray(pkg.synth.render_frame(W, H, 2, seed=31, noise_model="hash", noise=0.0, fireflies=0.0)[0], F).reshape(H, W, 3)
    out = ff.firefly_filter(noisy, 1, 1.0)
    mae = lambda a: float(np.abs(a.astype(np.float64) - clean).mean())      # noqa: E731
    bias = lambda a: abs(float(a.astype(np.float64).mean() / clean.astype(np.float64).mean()) - 1.0)      # noqa: E731
    print(f"MAE raw {mae(noisy):.4f} filtered {mae(out):.4f}; |mean ratio - 1| raw {bias(noisy):.4f} filtered {bias(out):.4f}")
    assert mae(out) < mae(noisy)
    assert bias(out) < bias(noisy)


# ---- 4. GPU: the temporal pass equals the model, bit for bit, on every pixel ------------------------------------------------------------------
# 65x5 and 130x9 cross the 64-column and 4-row tile seams and put the R + 1 margin off every image edge; 1x1 and 5x3 are all edge
SIZES = [(1, 1), (5, 3), (65, 5), (130, 9)]
LEGS = ["aos", "planar", "promised", "coord_f32", "delta_f32", "delta_f16"]
# (rank, scale, clamp radius, clamp k): every rank, every scale of {0, 1, 1.5} and both radii; the seam sizes run all six
SETTINGS = [(1, 1.0, 0, 0.0), (2, 1.5, 2, 1.0), (3, 0.0, 0, 0.0), (1, 0.0, 2, 1.0), (2, 1.0, 0, 0.0), (3, 1.5, 2, 2.5)]


@pytest.mark.gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("W,H", SIZES)
def test_hip_equals_the_model_on_every_pixel(pkg, orc, W, H, leg):
    """Four frames under the moving camera; one context per leg, reset between the runs (the settings are given anew each time)."""
    seq = synth_sequence(pkg, orc, W, H)
    frames, cams = [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]
    fmt = {"coord_f32": COORD, "delta_f32": D32, "delta_f16": D16}.get(leg, COORD)
    planes = camera_planes(pkg, seq, fmt) if leg in ("coord_f32", "delta_f32", "delta_f16") else None
    params = synth_params(pkg, W, H)
    den = pkg.Denoiser(W, H, 0, pipelined=leg == "promised")
    try:
        if leg == "promised":
            if den.pipeline_status() == 2:
                pytest.skip("the context's two streams share a hardware queue: the promise is refused")
            params.inputs_ready = 1
        for rank, scale, radius, k in (SETTINGS if W >= 64 else SETTINGS[:3]):
            den.reset()
            den.set_firefly_filter(rank, scale)
            den.set_history_clamp(radius, k)
            got = run_gpu(pkg, den, frames, params, leg="planar" if leg == "planar" else "aos", planes=planes, fmt=fmt, cams=cams)
            ref = model_on(pkg, seq, fmt, rank, scale, radius, k, (W, H))
            assert_frames_equal(got, ref, f"{W}x{H} {leg} rank {rank} scale {scale} radius {radius} k {k}")
        if W >= 64:
            raw = model_on(pkg, seq, fmt, 0, 1.0, 0, 0.0, (W, H))
            on = model_on(pkg, seq, fmt, 1, 1.0, 0, 0.0, (W, H))
            assert not same_bits(raw[-1]["color"], on[-1]["color"]), "the filter acts on this sequence"
            assert on[-1]["hlen"].max() == len(frames), "some history survives the moving camera"
    finally:
        den.free()


# ---- 5. GPU: the identity on whole frames -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("promised", [False, True], ids=["ordered", "promised"])
@pytest.mark.parametrize("variant", [0, 1, 4])
def test_whole_frames_are_the_unfiltered_frames_of_the_filtered_input(pkg, variant, promised):
    """box_room's moving block, six frames, temporal pass and five levels: the filter on the raw input against the filter off on
    the model-filtered input, two contexts.  Every frame's output and states 0 to 2, bit for bit."""
    cam, frames = moving_block_sequence(pkg)
    rank, scale = 2, 1.0
    pre = filtered(frames, rank, scale)
    assert not same_bits(pre[0][0], frames[0][0]), "the filter acts on this sequence"
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=5, history_level=1, kernel_variant=variant)
    res = []
    for on in (True, False):
        d = pkg.Denoiser(SIDE, SIDE, 0, pipelined=promised)
        try:
            if promised:
                if d.pipeline_status() == 2:
                    pytest.skip("the context's two streams share a hardware queue: the promise is refused")
                p.inputs_ready = 1
            if on:
                d.set_firefly_filter(rank, scale)
            res.append(_whole_frames(pkg, d, p, frames if on else pre, cam))
            if promised:
                assert d.is_pipelined()
        finally:
            d.free()
    for f in range(MOVING_FRAMES):
        assert same_bits(res[0][0][f], res[1][0][f]), f"output, frame {f}"
    for k in range(3):
        assert same_bits(res[0][1][k], res[1][1][k]), f"state {k}"


# ---- 6. GPU: non-temporal frames ---------------------------------------------------------------------------------------------------------------
def _non_temporal(pkg, W, H, frames, variant, rank, scale):
    """Frames with temporal_enable = 0 and five levels, profiled.  Returns per frame (output, colour history, kernel kinds)."""
    d = pkg.Denoiser(W, H)
    d.set_firefly_filter(rank, scale)
    d.profile_stride(1)
    d.profile_enable(len(frames))
    p = pkg.reference_defaults().set(temporal_enable=0, spatial_enable=1, atrous_nlevel=5, kernel_variant=variant)
    res = []
    for c, g, cam in frames:
        out = d.denoise_host(c, g, cam, p)
        res.append([out, d.read_state(2)])
    d.sync()
    for s in range(len(frames)):
        res[s].append([kk for kk, _ in d.profile_read(s)])
    d.free()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("variant,W,H", [(1, 67, 41), (4, 67, 41), (4, 130, 9), (4, 481, 64)])
def test_non_temporal_frames_are_the_unfiltered_frames_of_the_filtered_input(pkg, variant, W, H):
    b = pkg.binding
    frames = [pkg.synth.render_frame(W, H, f, seed=17, moving=True) for f in range(2)]
    rank, scale = 1, 1.0
    pre = [(ff.firefly_filter(np.asarray(c, F).reshape(H, W, 3), rank, scale), g, cam) for c, g, cam in frames]
    assert not same_bits(pre[0][0], np.asarray(frames[0][0], F).reshape(H, W, 3)), "the filter acts on these frames"
    on, off = _non_temporal(pkg, W, H, frames, variant, rank, scale), _non_temporal(pkg, W, H, pre, variant, 0, 1.0)
    for f in range(len(frames)):
        assert on[f][2] == off[f][2] == [b.KERNEL_PREPARE] + [b.KERNEL_ATROUS] * 5, (on[f][2], off[f][2])
        assert same_bits(on[f][0], off[f][0]), f"output, frame {f}"
        assert same_bits(on[f][1], off[f][1]), f"colour history, frame {f}"


@pytest.mark.gpu
def test_non_temporal_default_choice_gives_up_the_fused_prepare_for_one_launch(pkg):
    """kernel_variant 0 at 481x64, where the unfiltered frame runs its prepare pass inside the first level
    (tests/test_prepare_fused_gpu.py): the filtered frame launches the prepare kernel and five levels."""
    b = pkg.binding
    W, H = 481, 64
    frames = [pkg.synth.render_frame(W, H, f, seed=17, moving=True) for f in range(2)]
    rank, scale = 1, 1.0
    pre = [(ff.firefly_filter(np.asarray(c, F).reshape(H, W, 3), rank, scale), g, cam) for c, g, cam in frames]
    on, off = _non_temporal(pkg, W, H, frames, 0, rank, scale), _non_temporal(pkg, W, H, pre, 0, 0, 1.0)
    for f in range(len(frames)):
        assert off[f][2] == [b.KERNEL_FUSED] + [b.KERNEL_ATROUS] * 4, off[f][2]
        assert on[f][2] == [b.KERNEL_PREPARE] + [b.KERNEL_ATROUS] * 5, on[f][2]
        err = float(relerr(on[f][0], off[f][0]).max())
        print(f"frame {f}: filtered frame against the fused frame of the filtered input, max relative error {err:.3e}")
        assert err <= 1e-5, f"frame {f}"


# ---- 7. GPU: off is off -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_is_off_and_the_pass_stays_one_temporal_kernel(pkg, orc):
    W, H = 67, 41
    seq = synth_sequence(pkg, orc, W, H)
    frames, cams = [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]
    params = synth_params(pkg, W, H)
    fresh, toggled = pkg.Denoiser(W, H), pkg.Denoiser(W, H)
    assert fresh.firefly_filter() == (0, 0.0)
    toggled.set_firefly_filter(2, 1.0)
    toggled.set_firefly_filter(0, 1.0)
    a, b = run_gpu(pkg, fresh, frames, params, cams=cams), run_gpu(pkg, toggled, frames, params, cams=cams)
    fresh.free(); toggled.free()
    ref = model_on(pkg, seq, COORD, 0, 1.0, 0, 0.0, (W, H))      # rank 0: the model of the unfiltered frames
    assert_frames_equal(a, ref, "never configured")
    assert_frames_equal(b, ref, "rank 2, then 0")
    # whole frames, profiled: the same kernel kinds, one TEMPORAL per frame, filter on or off
    full = synth_params(pkg, W, H, spatial_enable=1, atrous_nlevel=5, history_level=1)
    kinds = {}
    for rank in (0, 2):
        d = pkg.Denoiser(W, H)
        d.set_firefly_filter(rank, 1.0)
        d.profile_stride(1)
        d.profile_enable(len(frames))
        for (col, gb), cam in zip(frames, cams):
            d.denoise_host(col, gb, cam, full)
        d.sync()
        assert d.profile_frames() == len(frames)
        kinds[rank] = [[kk for kk, _ in d.profile_read(s)] for s in range(len(frames))]
        d.free()
    assert kinds[0] == kinds[2]
    for row in kinds[2]:
        assert row == [pkg.binding.KERNEL_TEMPORAL] + [pkg.binding.KERNEL_ATROUS] * 5, row


# ---- 8. GPU: every value is a defined input ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rank,scale,radius,k", [(1, 1.0, 0, 0.0), (2, 1.0, 2, 1.0), (3, 1.5, 0, 0.0)])
def test_non_finite_colours_are_defined_inputs(pkg, orc, rank, scale, radius, k):
    """NaN / +-inf / 1e38 colours sprinkled into frame 1, singly and in adjacent pairs: centres, neighbours and (from frame 2 on)
    the history hold non-finite values.  Frame 1 and the two frames behind it equal the model."""
    W, H = 67, 41
    seq = synth_sequence(pkg, orc, W, H)
    bad_values = [F(np.nan), F(np.inf), F(-np.inf), F(1e38), F(-1e38)]
    col1 = seq[1][0].copy()
    flat = col1.reshape(-1, 3)
    pick = np.linspace(0, W * H - 2, 9 * len(bad_values)).astype(int)
    for j, i in enumerate(pick):
        v, where = bad_values[j % len(bad_values)], (j // len(bad_values)) % 3      # one channel, two, all three
        flat[i, :where + 1] = v
        if j % 2:                                                                    # and its right-hand neighbour: another value
            flat[i + 1, :] = bad_values[(j + 1) % len(bad_values)]
    frames = [(c, g) for c, g, _, _ in seq]
    frames[1] = (col1, frames[1][1])
    cams = [c for _, _, c, _ in seq]
    coords = camera_planes(pkg, seq, COORD)
    ref = tm.run_sequence(filtered(frames, rank, scale), coords, radius=radius, k=k)
    assert np.isnan(ref[1]["color"]).any() and np.isnan(ref[3]["color"]).any(), "non-finite values reach the history"
    assert np.isfinite(ref[3]["color"]).sum() > ref[3]["color"].size // 2
    den = pkg.Denoiser(W, H)
    den.set_firefly_filter(rank, scale)
    den.set_history_clamp(radius, k)
    got = run_gpu(pkg, den, frames, synth_params(pkg, W, H), cams=cams)
    den.free()
    assert_frames_equal(got, ref, f"non-finite colours, rank {rank}")


# ---- 9. GPU: contract -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_contract_of_the_setting(pkg, orc):
    W, H = 67, 41
    seq = synth_sequence(pkg, orc, W, H)
    frames, cams = [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]
    lib = pkg.load_library()
    d = pkg.Denoiser(W, H)
    d.set_firefly_filter(2, 1.5)
    for rank, scale, word in ((-1, 1.0, "rank"), (4, 1.0, "rank"), (1, -0.5, "scale"), (1, float("nan"), "scale"),
                              (1, float("inf"), "scale"), (1, float("-inf"), "scale")):
        assert lib.svgf_set_firefly_filter(d.h, rank, scale) == -1, (rank, scale)
        assert word in d.last_error(), d.last_error()
        with pytest.raises(pkg.SvgfError, match="-> -1"):
            d.set_firefly_filter(rank, scale)
        assert d.firefly_filter() == (2, 1.5), "a refused call changes nothing"
    r = ctypes.c_int(-7)
    assert lib.svgf_get_firefly_filter(d.h, ctypes.byref(r), None) == 0 and r.value == 2, "either pointer may be NULL"
    s = ctypes.c_float(-7.0)
    assert lib.svgf_get_firefly_filter(d.h, None, ctypes.byref(s)) == 0 and s.value == 1.5
    d.set_firefly_filter(3, 0.0)
    assert d.firefly_filter() == (3, 0.0)
    d.set_firefly_filter(1, 2.5)
    assert d.firefly_filter() == (1, 2.5)
    assert d.history_clamp() == (0, 0.0), "the clamp is a setting of its own"
    # the setting survives svgf_reset: frames behind a reset are the model's with the filter on
    run_gpu(pkg, d, frames[:2], synth_params(pkg, W, H), cams=cams)
    d.reset()
    assert d.firefly_filter() == (1, 2.5)
    assert_frames_equal(run_gpu(pkg, d, frames, synth_params(pkg, W, H), cams=cams), model_on(pkg, seq, COORD, 1, 2.5, 0, 0.0, (W, H)), "behind svgf_reset")
    d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("temporal", [1, 0], ids=["temporal", "non-temporal"])
def test_an_image_taller_than_the_tiled_grid_is_refused_not_launched(pkg, temporal):
    """The filtered kernels' grid has one row of workgroups per four image rows, at most 65535 of them: 1 x 262144 is one tile row
    too tall.  Refused when the frame is planned; with the filter off, and at 1 x 262140 with it on, the frame runs."""
    import torch
    cam = pkg.synth.camera_for_frame(0, False)
    p = temporal_only(pkg, temporal_enable=temporal)
    for H, ok in ((262144, False), (262140, True)):
        rgb = torch.ones((H, 1, 3), dtype=torch.float32, device="cuda")
        gbt = torch.zeros((H * 52,), dtype=torch.uint8, device="cuda")
        out = torch.empty_like(rgb)
        d = pkg.Denoiser(1, H)
        d.denoise(out, rgb, gbt, cam, temporal_only(pkg))
        d.sync()
        d.set_firefly_filter(3, 1.0)
        if ok:
            d.denoise(out, rgb, gbt, cam, p)
            d.sync()
            assert (out.cpu().numpy() == 1.0).all(), "constant colour in, constant colour out"
        else:
            with pytest.raises(pkg.SvgfError, match="-> -5"):
                d.denoise(out, rgb, gbt, cam, p)
            assert "262140" in d.last_error() and "firefly" in d.last_error()
            d.sync()
            assert (d.read_state(0) == 1).all(), "a refused frame enqueues nothing"
        d.free()


@pytest.mark.gpu
@pytest.mark.experiments
@pytest.mark.parametrize("which", ["kernel_variant_6", "split_fused"])
def test_parked_fused_temporal_kernels_refuse_a_filtered_frame(pkg, experiments_lib, which):
    import torch
    W, H = 64, 48
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    gbt = torch.zeros((H * W * 52,), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(rgb)
    cam = pkg.synth.camera_for_frame(0, False)
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    if which == "split_fused":
        experiments_lib.exp_set("split_fused", 1)      # read by svgf_create
    else:
        p.kernel_variant = 6
    e = pkg.Denoiser(W, H, experiments=True)
    e.denoise(out, rgb, gbt, cam, p)                   # unfiltered: runs
    e.sync()
    before = e.read_state(0).copy()
    e.set_firefly_filter(1, 1.0)
    with pytest.raises(pkg.SvgfError, match="-> -5"):
        e.denoise(out, rgb, gbt, cam, p)
    assert "firefly filter" in e.last_error()
    e.sync()
    assert np.array_equal(e.read_state(0), before), "a refused frame enqueues nothing"
    e.set_firefly_filter(0, 1.0)
    e.denoise(out, rgb, gbt, cam, p)                   # off again: runs
    e.sync()
    e.free()
