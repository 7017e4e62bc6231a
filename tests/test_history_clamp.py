"""History clamp of the temporal pass (include/svgf.h: svgf_set_history_clamp / svgf_get_history_clamp).

The yardstick is tests/temporal_model.py, the float32 numpy model of the whole temporal pass.  The oracle knows no clamp;
test 2 pins the model to the oracle with the clamp off, bit for bit, so that with the clamp on any difference is the clamp's.

Bounds: every comparison of the kernel with the model is on the bits of every pixel (NaNs in the same place count as equal).
Both sides perform the same float32 operations in the same order without contraction, and division and square root are
correctly rounded on both: there is no arithmetic that may differ, so there is no tolerance to choose.  The one tolerance in
this file, 1e-5 between kernel_variant 0 and 1 on whole frames, is the project's existing gate between its a-trous kernels
(tests/test_parity_gpu.py): the clamp changes their input, not them."""
import ctypes

import numpy as np
import pytest

import temporal_model as tm
from conftest import relerr
from temporal_harness import (MOVING_FRAMES, SIDE, _whole_frames, assert_frames_equal, moving_block_sequence, read_states, run_gpu,
                              same_bits, scales, synth_params, synth_sequence, temporal_only)

F = np.float32
COORD, D32, D16 = tm.COORD, tm.D32, tm.D16
NEW_SYMBOLS = ("svgf_set_history_clamp", "svgf_get_history_clamp")
RADII, KS = (1, 2, 3), (0.0, 1.0, 2.5)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def camera_planes(pkg, seq, fmt):
    """Per frame the plane svgf_motion_reproject writes for the previous frame's camera and synth_params' reproj_scale (frame 0: its
    own camera; never looked at)."""
    H, W = seq[0][1].shape
    sx, sy = scales(pkg, W, H)
    return [tm.motion_plane(seq[max(f - 1, 0)][3], W, H, seq[f][1], None, fmt, F(sx), F(sy)) for f in range(len(seq))]


def moving_block_model(pkg, orc, radius, k):
    cache = moving_block_model.__dict__.setdefault("cache", {})
    if (radius, k) not in cache:
        cam, frames = moving_block_sequence(pkg)
        M = orc.view_matrix(pkg, cam)
        coords = [tm.motion_plane(M, SIDE, SIDE, gb, X, COORD) for _, gb, X in frames]
        cache[(radius, k)] = tm.run_sequence([(c, g) for c, g, _ in frames], coords, radius=radius, k=k)
    return cache[(radius, k)]


def model_on(pkg, seq, fmt, radius, k, tag):
    """The model on a synthetic sequence, history looked up through the camera plane of format `fmt` converted as the header says."""
    cache = model_on.__dict__.setdefault("cache", {})
    key = (tag, fmt, radius, k)
    if key not in cache:
        H, W = seq[0][1].shape
        coords = [tm.coord_plane(pl, fmt, W, H) for pl in camera_planes(pkg, seq, fmt)]
        cache[key] = tm.run_sequence([(c, g) for c, g, _, _ in seq], coords, radius=radius, k=k)
    return cache[key]


FEATURE_W, FEATURE_H, FEATURE_EDGE = 40, 24, 20
C0, C1 = np.array([0.5, 0.25, 1.0], F), np.array([2.0, 1.0, 0.25], F)


def feature_sequence(pkg):
    """Test 3's sequence: a uniform G-buffer, frames 0-3 all C0, frame 4 has columns x < 20 at C1.  [(colour, texels)], 5 frames."""
    W, H = FEATURE_W, FEATURE_H
    gb = np.zeros((H, W), dtype=pkg.synth.GBUFFER_DTYPE)
    gb["normal"] = (0.0, 1.0, 0.0)
    gb["albedo"] = gb["ialbedo"] = 1.0
    gb["geomId"] = 0
    ys, xs = np.mgrid[0:H, 0:W]
    gb["position"] = np.stack([xs * 0.1, np.zeros_like(xs), ys * 0.1], axis=-1).astype(F)
    frames = []
    for f in range(5):
        col = np.tile(C0, (H, W, 1)).astype(F)
        if f >= 4:
            col[:, :FEATURE_EDGE] = C1
        frames.append((col, gb))
    return frames


def assert_feature(last, radius):
    """The exact statement of the feature on frame 4 (`last`: dict with color and hlen)."""
    col, r = last["color"], radius
    blend = (F(0.25) * C1 + F(0.75) * C0).astype(F)
    left = col[:, :FEATURE_EDGE - r] if r else col[:, :FEATURE_EDGE]
    assert left.shape[1] == FEATURE_EDGE - r and left.shape[0] == FEATURE_H
    assert (left == (C1 if r else blend)).all(), f"radius {r}: columns x <= {FEATURE_EDGE - 1 - r}"
    assert (col[:, FEATURE_EDGE + r:] == C0).all(), f"radius {r}: columns x >= {FEATURE_EDGE + r}"
    assert (last["hlen"] == 5).all()


# ---- 1. CPU: symbols and the NULL context ----------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_a_null_context_is_invalid(pkg):
    lib = pkg.load_library()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in pkg.binding.EXPORTS, n
    assert lib.svgf_set_history_clamp(None, 1, 1.0) == -1
    assert lib.svgf_set_history_clamp(None, 0, 0.0) == -1
    r, k = ctypes.c_int(7), ctypes.c_float(7.0)
    assert lib.svgf_get_history_clamp(None, ctypes.byref(r), ctypes.byref(k)) == -1
    assert lib.svgf_get_history_clamp(None, None, None) == -1
    assert (r.value, k.value) == (7, 7.0), "nothing is written on failure"
    assert hasattr(pkg.Denoiser, "set_history_clamp") and hasattr(pkg.Denoiser, "history_clamp")


# ---- 2. CPU: the model is a model --------------------------------------------------------------------------------------------------------
def test_model_without_clamp_is_the_oracle_on_the_moving_block(pkg, orc):
    """Radius 0 on the six box_room frames (substituted positions, alpha defaults, temporal only): history length, moments and
    colour history of the C oracle, bit for bit, on every frame."""
    cam, frames = moving_block_sequence(pkg)
    ref = moving_block_model(pkg, orc, 0, 0.0)
    o = orc.Oracle(pkg, SIDE, SIDE, threads=4)
    try:
        for f, (col, gb, X) in enumerate(frames):
            sub = gb.copy()
            sub["position"] = tm.apply_xf(X, gb["geomId"], gb["position"])
            o.denoise(col, sub, cam, temporal_only(pkg))
            assert same_bits(o.read_state(0), ref[f]["hlen"]), f"history length, frame {f}"
            assert same_bits(o.read_state(1), ref[f]["mom"]), f"moments, frame {f}"
            assert same_bits(o.read_state(2), ref[f]["color"]), f"colour history, frame {f}"
    finally:
        o.free()
    hl = ref[-1]["hlen"]
    assert hl.max() == MOVING_FRAMES and hl.min() == 1, "the sequence keeps some history and loses some"


# ---- 3. CPU: the statement of the feature, on the model alone ------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_model_a_lighting_change_inside_a_constant_window_is_taken_at_once(pkg, radius):
    frames = feature_sequence(pkg)
    coords = [tm.pixel_grid(FEATURE_W, FEATURE_H)] * len(frames)
    for k in ((0.0,) if radius == 0 else (0.0, 1.0, 7.5)):      # any k: sd is 0 where the window is constant
        res = tm.run_sequence(frames, coords, color_alpha=0.25, moment_alpha=0.25, radius=radius, k=k)
        assert (res[3]["color"] == C0).all() and (res[3]["hlen"] == 4).all(), "frames 0-3 accumulate exactly C0"
        assert_feature(res[4], radius)


# ---- 4. GPU: HIP equals the model, bit for bit, on every pixel ----------------------------------------------------------------------------
SIZES = [(1, 1), (5, 3), (67, 41), (257, 131), (300, 9)]
LEGS = ["aos", "planar", "promised", "coord_f32", "delta_f32", "delta_f16"]


@pytest.mark.gpu
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("W,H", SIZES)
def test_hip_equals_the_model_on_every_pixel(pkg, orc, W, H, leg):
    """Four frames under the moving camera (bilinear taps, fallback taps, off-screen taps and misses all occur), every radius
    and k in {0, 1, 2.5}; one context per leg, reset between the runs (the setting is given anew each time)."""
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
        for radius in RADII:
            for k in KS:
                den.reset()
                den.set_history_clamp(radius, k)
                got = run_gpu(pkg, den, frames, params, leg="planar" if leg == "planar" else "aos", planes=planes, fmt=fmt, cams=cams)
                ref = model_on(pkg, seq, fmt, radius, k, (W, H))
                assert_frames_equal(got, ref, f"{W}x{H} {leg} radius {radius} k {k}")
        hl = ref[-1]["hlen"]
        assert hl.max() == len(frames), "some history survives the moving camera"
        assert hl.min() == 1 or W * H < 1000, "and some is lost"
    finally:
        den.free()


@pytest.mark.gpu
@pytest.mark.parametrize("radius,k", [(1, 1.0), (2, 1.0), (3, 2.5)])
def test_hip_equals_the_model_on_the_moving_block(pkg, orc, radius, k):
    """box_room's moving block at 96x96, the plane written by svgf_motion_reproject with the object maps."""
    import torch
    cam, frames = moving_block_sequence(pkg)
    ref = moving_block_model(pkg, orc, radius, k)
    W = H = SIDE
    den = pkg.Denoiser(W, H)
    den.set_capture(True)
    den.set_history_clamp(radius, k)
    mv = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    got = []
    for col, gb, X in frames:
        t_c = torch.from_numpy(col).cuda()
        t_g = torch.from_numpy(gb.view(np.uint8).reshape(-1).copy()).cuda()
        t_x = torch.from_numpy(X).cuda()
        pkg.binding.motion_reproject(mv, W, H, cam, gbuffer=t_g, geom_xf=t_x)
        den.denoise(out, t_c, t_g, cam, temporal_only(pkg), motion=mv)
        torch.cuda.synchronize()
        got.append(read_states(den))
    den.free()
    assert_frames_equal(got, ref, f"moving block radius {radius} k {k}")
    off = moving_block_model(pkg, orc, 0, 0.0)
    assert not np.array_equal(off[-1]["color"], ref[-1]["color"]), "the clamp acts on this sequence"


# ---- 5. GPU: off is off -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_is_off_and_the_pass_stays_one_temporal_kernel(pkg, orc):
    W, H = 67, 41
    seq = synth_sequence(pkg, orc, W, H)
    frames, cams = [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]
    params = synth_params(pkg, W, H)
    fresh, toggled = pkg.Denoiser(W, H), pkg.Denoiser(W, H)
    assert fresh.history_clamp() == (0, 0.0)
    toggled.set_history_clamp(2, 1.0)
    toggled.set_history_clamp(0, 1.0)
    a, b = run_gpu(pkg, fresh, frames, params, cams=cams), run_gpu(pkg, toggled, frames, params, cams=cams)
    fresh.free(); toggled.free()
    ref = model_on(pkg, seq, COORD, 0, 0.0, (W, H))
    assert_frames_equal(a, ref, "never configured")
    assert_frames_equal(b, ref, "radius 2, then 0")
    # whole frames, profiled: the same kernel kinds, one TEMPORAL per frame, clamp on or off
    full = synth_params(pkg, W, H, spatial_enable=1, atrous_nlevel=5, history_level=1)
    kinds = {}
    for radius in (0, 2):
        d = pkg.Denoiser(W, H)
        d.set_history_clamp(radius, 1.0)
        d.profile_stride(1)
        d.profile_enable(len(frames))
        for (col, gb), cam in zip(frames, cams):
            d.denoise_host(col, gb, cam, full)
        d.sync()
        assert d.profile_frames() == len(frames)
        kinds[radius] = [[kk for kk, _ in d.profile_read(s)] for s in range(len(frames))]
        d.free()
    assert kinds[0] == kinds[2]
    for row in kinds[2]:
        assert row == [pkg.binding.KERNEL_TEMPORAL] + [pkg.binding.KERNEL_ATROUS] * 5, row


# ---- 6. GPU: the feature -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_gpu_a_lighting_change_inside_a_constant_window_is_taken_at_once(pkg, radius):
    W, H = FEATURE_W, FEATURE_H
    frames = feature_sequence(pkg)
    cam = pkg.synth.camera_for_frame(0, False)
    planes = [tm.pixel_grid(W, H)] * len(frames)
    params = temporal_only(pkg, color_alpha=0.25, moment_alpha=0.25)
    den = pkg.Denoiser(W, H)
    den.set_history_clamp(radius, 1.0)
    got = run_gpu(pkg, den, frames, params, planes=planes, fmt=COORD, cams=[cam] * len(frames))
    den.free()
    assert (got[3]["color"] == C0).all() and (got[3]["hlen"] == 4).all(), "frames 0-3 accumulate exactly C0"
    assert_feature(got[4], radius)
    assert same_bits(got[4]["acc"], got[4]["color"])


# ---- 7. GPU: every value is a defined input ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("radius,k", [(1, 1.0), (3, 2.5)])
def test_non_finite_colours_are_defined_inputs(pkg, orc, radius, k):
    """NaN / +-inf / huge colours sprinkled into frame 1: windows, centres and (from frame 2 on) the history hold non-finite
    values.  Frame 1 and the two frames behind it equal the model."""
    W, H = 67, 41
    seq = synth_sequence(pkg, orc, W, H)
    bad_values = [F(np.nan), F(np.inf), F(-np.inf), F(1e30), F(-1e30)]
    col1 = seq[1][0].copy()
    flat = col1.reshape(-1, 3)
    pick = np.linspace(0, W * H - 1, 9 * len(bad_values)).astype(int)
    for j, i in enumerate(pick):
        v, where = bad_values[j % len(bad_values)], (j // len(bad_values)) % 3      # one channel, two, all three
        flat[i, :where + 1] = v
    frames = [(c, g) for c, g, _, _ in seq]
    frames[1] = (col1, frames[1][1])
    cams = [c for _, _, c, _ in seq]
    coords = camera_planes(pkg, seq, COORD)
    ref = tm.run_sequence(frames, coords, radius=radius, k=k)
    assert np.isnan(ref[1]["color"]).any() and np.isnan(ref[3]["color"]).any(), "non-finite values reach the history"
    assert np.isfinite(ref[3]["color"]).sum() > ref[3]["color"].size // 2
    den = pkg.Denoiser(W, H)
    den.set_history_clamp(radius, k)
    got = run_gpu(pkg, den, frames, synth_params(pkg, W, H), cams=cams)
    den.free()
    assert_frames_equal(got, ref, f"non-finite colours, radius {radius}")


# ---- 8. GPU: whole frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_whole_frames_ordered_promised_and_strict_gather_agree(pkg):
    cam, frames = moving_block_sequence(pkg)
    full = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=5, history_level=1)

    def run(variant=0, promised=False):
        d = pkg.Denoiser(SIDE, SIDE, 0, pipelined=promised)
        p = pkg.SvgfParams.from_buffer_copy(full).set(kernel_variant=variant)
        if promised:
            if d.pipeline_status() == 2:
                d.free()
                return None
            p.inputs_ready = 1
        d.set_history_clamp(2, 1.0)
        try:
            res = _whole_frames(pkg, d, p, frames, cam)
            if promised:
                assert d.is_pipelined()
            return res
        finally:
            d.free()

    ordered, strict, promised = run(), run(variant=1), run(promised=True)
    for f in range(MOVING_FRAMES):
        err = float(relerr(ordered[0][f], strict[0][f]).max())
        print(f"frame {f}: kernel_variant 0 against 1, max relative error {err:.3e}")
        assert err <= 1e-5, f"frame {f}"
    if promised is None:
        pytest.skip("the context's two streams share a hardware queue: the promise is refused (variants 0 and 1 agreed)")
    for f in range(MOVING_FRAMES):
        assert same_bits(ordered[0][f], promised[0][f]), f"output, frame {f}"
    for k in range(3):
        assert same_bits(ordered[1][k], promised[1][k]), f"state {k}"


# ---- 9. GPU: contract -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_contract_of_the_setting(pkg, orc):
    W, H = 67, 41
    seq = synth_sequence(pkg, orc, W, H)
    frames, cams = [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]
    lib = pkg.load_library()
    d = pkg.Denoiser(W, H)
    d.set_history_clamp(2, 1.5)
    for radius, k, word in ((-1, 1.0, "radius"), (4, 1.0, "radius"), (1, -0.5, "sigma_scale"), (1, float("nan"), "sigma_scale"),
                            (1, float("inf"), "sigma_scale"), (1, float("-inf"), "sigma_scale")):
        assert lib.svgf_set_history_clamp(d.h, radius, k) == -1, (radius, k)
        assert word in d.last_error(), d.last_error()
        with pytest.raises(pkg.SvgfError, match="-> -1"):
            d.set_history_clamp(radius, k)
        assert d.history_clamp() == (2, 1.5), "a refused call changes nothing"
    d.set_history_clamp(3, 0.0)
    assert d.history_clamp() == (3, 0.0)
    d.set_history_clamp(1, 2.5)
    assert d.history_clamp() == (1, 2.5)
    # the setting survives svgf_reset: frames behind a reset are the model's with the clamp on
    run_gpu(pkg, d, frames[:2], synth_params(pkg, W, H), cams=cams)
    d.reset()
    assert d.history_clamp() == (1, 2.5)
    assert_frames_equal(run_gpu(pkg, d, frames, synth_params(pkg, W, H), cams=cams), model_on(pkg, seq, COORD, 1, 2.5, (W, H)), "behind svgf_reset")
    d.free()
    # a non-temporal frame ignores it
    spatial = pkg.reference_defaults().set(temporal_enable=0, spatial_enable=1)
    outs = []
    for radius in (0, 2):
        e = pkg.Denoiser(W, H)
        e.set_history_clamp(radius, 1.0)
        outs.append([e.denoise_host(c, g, cam, spatial) for (c, g), cam in zip(frames[:2], cams)])
        e.free()
    for x, y in zip(*outs):
        assert same_bits(x, y)


@pytest.mark.gpu
def test_an_image_taller_than_the_clamped_grid_is_refused_not_launched(pkg):
    """The clamped kernels' grid has one row of workgroups per four image rows, at most 65535 of them: 1 x 262144 is one tile row
    too tall.  Refused when the frame is planned; with the clamp off, and at 1 x 262140 with it on, the frame runs."""
    import torch
    cam = pkg.synth.camera_for_frame(0, False)
    p = temporal_only(pkg)
    for H, ok in ((262144, False), (262140, True)):
        rgb = torch.ones((H, 1, 3), dtype=torch.float32, device="cuda")
        gbt = torch.zeros((H * 52,), dtype=torch.uint8, device="cuda")
        out = torch.empty_like(rgb)
        d = pkg.Denoiser(1, H)
        d.denoise(out, rgb, gbt, cam, p)
        d.sync()
        d.set_history_clamp(3, 1.0)
        if ok:
            d.denoise(out, rgb, gbt, cam, p)
            d.sync()
            assert (out.cpu().numpy() == 1.0).all(), "constant colour in, constant colour out (alpha 1/2 is exact)"
        else:
            with pytest.raises(pkg.SvgfError, match="-> -5"):
                d.denoise(out, rgb, gbt, cam, p)
            assert "262140" in d.last_error()
            d.sync()
            assert (d.read_state(0) == 1).all(), "a refused frame enqueues nothing"
        d.free()


@pytest.mark.gpu
@pytest.mark.experiments
@pytest.mark.parametrize("which", ["kernel_variant_6", "split_fused"])
def test_parked_fused_temporal_kernels_refuse_a_clamped_frame(pkg, experiments_lib, which):
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
    e.denoise(out, rgb, gbt, cam, p)                   # unclamped: runs
    e.sync()
    before = e.read_state(0).copy()
    e.set_history_clamp(2, 1.0)
    with pytest.raises(pkg.SvgfError, match="-> -5"):
        e.denoise(out, rgb, gbt, cam, p)
    assert "history clamp" in e.last_error()
    e.sync()
    assert np.array_equal(e.read_state(0), before), "a refused frame enqueues nothing"
    e.denoise(out, rgb, gbt, cam, pkg.SvgfParams.from_buffer_copy(p).set(temporal_enable=0))      # no temporal pass: not refused
    e.sync()
    e.free()
