"""Per-pixel motion vectors for the temporal pass (include/svgf.h: svgf_denoise_motion, svgf_denoise_planar_motion,
svgf_motion_reproject).

The CPU oracle does not know motion vectors.  It reprojects `gbuffer.position`, and with spatial_enable = 0 and
reproj_position_tol = 0 the position is used for nothing else — so the oracle fed texels whose position is X[g] * p (the point
moved back into the previous frame's world space) IS the motion path fed true positions plus svgf_motion_reproject(X), bit for
bit.  That substitution is the reference of the moving-object test; the camera-path tests need no oracle at all: a plane written
by svgf_motion_reproject with no object maps must reproduce svgf_denoise exactly.

Bounds: every comparison here is np.array_equal.  The helper and the camera path share one device function for the projection,
the numpy replica (tests/temporal_model.py) performs the same float32 operations in the same order without contraction, and
everything behind the coordinate is the same kernel code; there is no arithmetic that may differ, so there is no tolerance to
choose.  The two history fractions (<= 0.10 without motion, >= 0.95 with) are the statement of what the feature is for; the
oracle gives 0.00 and 1.00."""
import ctypes

import numpy as np
import pytest

from conftest import denoiser_for
from temporal_harness import BLOCK, MOVING_FRAMES, SIDE, moving_block_sequence, scales, temporal_only
from temporal_model import COORD, D16, D32, apply_xf, motion_plane

F = np.float32
NEW_SYMBOLS = ("svgf_denoise_motion", "svgf_denoise_planar_motion", "svgf_motion_reproject")


# ---- the moving block of box_room.txt (checks 1 and 5) ---------------------------------------------------------------------------
def substituted(gb, X):
    out = gb.copy()
    out["position"] = apply_xf(X, gb["geomId"], gb["position"])
    return out


def full_history_fraction(hlen, gb):
    block = gb["geomId"] == BLOCK
    assert np.count_nonzero(block) > 150
    return float(np.count_nonzero(hlen[block] == MOVING_FRAMES)) / float(np.count_nonzero(block))


def oracle_moving_block(pkg, orc, substitute):
    """Per frame (output, history length, moments, colour history) of the oracle on the true or the substituted texels."""
    key = ("oracle", substitute)
    cache = oracle_moving_block.__dict__.setdefault("cache", {})
    if key not in cache:
        cam, frames = moving_block_sequence(pkg)
        o = orc.Oracle(pkg, SIDE, SIDE, threads=4)
        res = []
        for col, gb, X in frames:
            out = o.denoise(col, substituted(gb, X) if substitute else gb, cam, temporal_only(pkg))
            res.append((out, o.read_state(0), o.read_state(1), o.read_state(2)))
        o.free()
        cache[key] = res
    return cache[key]


# ---- 1. CPU: symbols, error paths, and what the feature is for --------------------------------------------------------------------
def test_symbols_are_exported_and_null_or_unknown_arguments_are_invalid(pkg):
    lib = pkg.load_library()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in pkg.binding.EXPORTS, n
    cam = pkg.SvgfCamera()
    assert lib.svgf_denoise_motion(None, None, None, None, None, COORD, None, None, None) == -1
    assert lib.svgf_denoise_planar_motion(None, None, None, None, COORD, None, None, None) == -1
    assert lib.svgf_denoise_motion(None, None, None, None, None, 99, None, None, None) == -1
    # an unknown format (and 0, which names no format) is refused before the device or any pointer is touched
    for fmt in (0, 4, 99, -1):
        assert lib.svgf_motion_reproject(0, 64, fmt, 64, None, None, 4, 4, ctypes.byref(cam), None, None, 0, None) == -1
    assert lib.svgf_motion_reproject(0, None, COORD, 64, None, None, 4, 4, ctypes.byref(cam), None, None, 0, None) == -1
    assert lib.svgf_motion_reproject(0, 64, COORD, None, 64, None, 4, 4, ctypes.byref(cam), None, None, 0, None) == -1
    assert lib.svgf_motion_reproject(0, 64, COORD, 64, None, None, 4, 4, None, None, None, 0, None) == -1
    assert (pkg.binding.MOTION_PREV_COORD_F32, pkg.binding.MOTION_DELTA_F32, pkg.binding.MOTION_DELTA_F16) == (COORD, D32, D16)


def test_oracle_loses_the_moving_block_and_keeps_it_with_its_previous_position(pkg, orc):
    """The statement of the feature, on the oracle alone (it pins the inputs of the GPU test below; none of the new code runs):
    through the previous camera the block's pixels never keep their history; given the point's previous position, all do."""
    _, frames = moving_block_sequence(pkg)
    gb = frames[-1][1]
    lost = full_history_fraction(oracle_moving_block(pkg, orc, False)[-1][1], gb)
    kept = full_history_fraction(oracle_moving_block(pkg, orc, True)[-1][1], gb)
    print(f"block pixels {np.count_nonzero(gb['geomId'] == BLOCK)}: full history on {lost:.3f} (true positions), {kept:.3f} (substituted)")
    assert lost <= 0.10
    assert kept >= 0.95


# ---- 2. the helper against numpy --------------------------------------------------------------------------------------------------
def _texels_for_helper(pkg, W, H):
    """Synthetic texels with ray misses, ids beyond the map table and a few non-finite / behind-the-camera positions."""
    _, gb, _ = pkg.synth.render_frame(W, H, 3, seed=11, moving=True, noise_model="hash")
    gb = gb.copy().reshape(H, W)
    rng = np.random.default_rng(W * 1000 + H)
    flat = gb.reshape(-1)
    n = flat.size
    flat["geomId"][rng.integers(0, n, max(1, n // 7))] = -1
    flat["geomId"][rng.integers(0, n, max(1, n // 9))] = 40             # beyond every table used below: unmoved
    if n > 4:
        flat["position"][rng.integers(0, n, 3)] = (np.nan, np.inf, -1e30)
        flat["position"][rng.integers(0, n, 2)] = (0.0, 5.0, 60.0)      # behind the camera
    return gb


@pytest.mark.gpu
@pytest.mark.parametrize("planes", [False, True], ids=["aos", "planes"])
@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (67, 41), (200, 200)])
def test_motion_reproject_matches_numpy_bit_for_bit(pkg, orc, W, H, planes):
    import torch
    gb = _texels_for_helper(pkg, W, H)
    cam = pkg.synth.camera_for_frame(2, True)
    M = orc.view_matrix(pkg, cam)
    rng = np.random.default_rng(5)
    X = (np.tile(np.eye(3, 4), (9, 1, 1)) + rng.uniform(-0.3, 0.3, (9, 3, 4))).astype(F).reshape(9, 12)
    t_g = torch.from_numpy(gb.view(np.uint8).reshape(-1).copy()).cuda()
    t_pos = torch.from_numpy(np.ascontiguousarray(gb["position"])).cuda()
    t_gid = torch.from_numpy(np.ascontiguousarray(gb["geomId"])).cuda()
    t_x = torch.from_numpy(X).cuda()
    src = dict(position=t_pos, geom_id=t_gid) if planes else dict(gbuffer=t_g)
    for fmt in (COORD, D32, D16):
        for xf in (None, X):
            for sx, sy in ((0.0, 0.0), scales(pkg, W, H)):
                out = torch.full((H, W, 2), 7.0, dtype=torch.float16 if fmt == D16 else torch.float32, device="cuda")
                pkg.binding.motion_reproject(out, W, H, cam, motion_format=fmt, reproj_scale=(sx, sy),
                                             geom_xf=None if xf is None else t_x, **src)
                torch.cuda.synchronize()
                got, ref = out.cpu().numpy(), motion_plane(M, W, H, gb, xf, fmt, sx, sy)
                assert np.isnan(got[gb["geomId"] == -1]).all(), "ray misses are NaN"
                bits = np.uint16 if fmt == D16 else np.uint32
                nan = np.isnan(ref)
                assert np.array_equal(np.isnan(got), nan)
                assert np.array_equal(got.view(bits)[~nan], ref.view(bits)[~nan]), f"format {fmt}, maps {xf is not None}, scale {sx}"


# ---- 3. the camera path reproduced through the motion plane -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["aos", "planar", "promised", "pipelined_ordered", "reproj_scale"])
@pytest.mark.parametrize("W,H", [(1, 1), (96, 64), (257, 131)])
def test_plane_of_the_previous_camera_reproduces_svgf_denoise(pkg, W, H, leg):
    """Context A: svgf_denoise.  Context B: svgf_motion_reproject(previous camera) -> svgf_denoise_motion (PREV_COORD_F32).  Full
    SVGF, 5 levels, history from level 1, a moving camera, 5 frames: output and history equal on every frame."""
    import torch
    N = 5
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=5, history_level=1)
    if leg == "reproj_scale":
        p.reproj_scale[0], p.reproj_scale[1] = scales(pkg, W, H)
    rs = (p.reproj_scale[0], p.reproj_scale[1])
    a = pkg.Denoiser(W, H, 0)
    b = pkg.Denoiser(W, H, 0, pipelined=leg in ("promised", "pipelined_ordered"))
    pb = pkg.SvgfParams.from_buffer_copy(p)
    if leg == "pipelined_ordered":      # the pipeline without the promise: two plane sets, frames ordered on the caller's stream
        pb.inputs_ready = 2
    if leg == "promised":
        if b.pipeline_status() == 2:
            a.free(); b.free()
            pytest.skip("the context's two streams share a hardware queue: the promise is refused")
        pb.inputs_ready = 1
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    # the promise: inputs complete at call time and untouched until the frame is done — one set of inputs per frame
    ins = [(torch.empty_like(rgb), torch.empty_like(gbt), torch.empty((H, W, 2), dtype=torch.float32, device="cuda")) for _ in range(N)]
    out_a = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    out_b = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    cams = [pkg.synth.camera_for_frame(f, True) for f in range(N)]
    for f in range(N):
        prev_cam = cams[max(f - 1, 0)]      # (frame 0 has no history: its plane is never looked at)
        pkg.binding.synth_render(rgb, gbt, W, H, cams[f], f, seed=21)
        a.denoise(out_a, rgb, gbt, cams[f], p)
        rgb_b, gbt_b, mv = ins[f]
        if leg == "planar":
            planes = b.planar_gbuffer()
            pkg.binding.synth_render_planar(rgb_b, planes, W, H, cams[f], f, seed=21)
            pkg.binding.motion_reproject(mv, W, H, prev_cam, position=planes.position, geom_id=planes.geom_id, reproj_scale=rs)
            torch.cuda.synchronize()
            b.denoise_planar(out_b, rgb_b, cams[f], pb, motion=mv)
        else:
            pkg.binding.synth_render(rgb_b, gbt_b, W, H, cams[f], f, seed=21)
            pkg.binding.motion_reproject(mv, W, H, prev_cam, gbuffer=gbt_b, reproj_scale=rs)
            torch.cuda.synchronize()
            b.denoise(out_b, rgb_b, gbt_b, cams[f], pb, motion=mv, motion_format=COORD)
        torch.cuda.synchronize()
        assert np.array_equal(out_a.cpu().numpy(), out_b.cpu().numpy(), equal_nan=True), f"output, frame {f}"
        for which in (0, 1, 2):
            assert np.array_equal(a.read_state(which), b.read_state(which), equal_nan=True), f"state {which}, frame {f}"
    if leg in ("promised", "pipelined_ordered"):
        assert b.is_pipelined()
    assert a.read_state(0).max() > 1 or W * H == 1, "some history survives the moving camera"
    a.free(); b.free()


# ---- 4. the three formats -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_three_formats_agree(pkg):
    """Deltas in multiples of 1/8 within +-3 pixels are exact in float16, and x + d is exact in float32: the same field in the
    three formats must give the same frames."""
    W, H, N = 67, 41, 3
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=5, history_level=1)
    frames = [pkg.synth.render_frame(W, H, f, seed=8, moving=False, noise_model="hash") for f in range(N)]
    rng = np.random.default_rng(17)
    d = (rng.integers(-24, 25, (N, H, W, 2)) / 8.0).astype(F)
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs, ys], axis=-1).astype(F)
    res = {}
    for fmt in (COORD, D32, D16):
        den = pkg.Denoiser(W, H)
        res[fmt] = []
        for f, (c, g, cam) in enumerate(frames):
            m = {COORD: xy + d[f], D32: d[f], D16: d[f].astype(np.float16)}[fmt]
            out = den.denoise_host(c, g, cam, p, motion=m, motion_format=fmt)
            res[fmt].append((out, den.read_state(0), den.read_state(1), den.read_state(2)))
        den.free()
    assert res[COORD][-1][1].max() == N and res[COORD][-1][1].min() == 1, "the field keeps some history and loses some"
    for fmt in (D32, D16):
        for f in range(N):
            for x, y in zip(res[COORD][f], res[fmt][f]):
                assert np.array_equal(x, y, equal_nan=True), f"format {fmt}, frame {f}"


# ---- 5. a moving object ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_moving_block_keeps_its_history_and_equals_the_oracle_on_substituted_positions(pkg, orc):
    import torch
    cam, frames = moving_block_sequence(pkg)
    ref = oracle_moving_block(pkg, orc, True)
    W = H = SIDE
    p = temporal_only(pkg)
    den, plain = pkg.Denoiser(W, H), pkg.Denoiser(W, H)
    mv = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    for f, (col, gb, X) in enumerate(frames):
        t_c = torch.from_numpy(col).cuda()
        t_g = torch.from_numpy(gb.view(np.uint8).reshape(-1).copy()).cuda()
        t_x = torch.from_numpy(X).cuda()
        pkg.binding.motion_reproject(mv, W, H, cam, gbuffer=t_g, geom_xf=t_x)
        den.denoise(out, t_c, t_g, cam, p, motion=mv)
        plain.denoise(out.clone(), t_c, t_g, cam, p)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref[f][0]), f"output, frame {f}"
        for which in (0, 1, 2):
            assert np.array_equal(den.read_state(which), ref[f][1 + which]), f"state {which}, frame {f}"
    gb = frames[-1][1]
    kept, lost = full_history_fraction(den.read_state(0), gb), full_history_fraction(plain.read_state(0), gb)
    print(f"block pixels with full history: {kept:.3f} with motion vectors, {lost:.3f} through the previous camera")
    den.free(); plain.free()
    assert kept >= 0.95
    assert lost <= 0.10


# ---- 6. every value is a defined input ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [COORD, D32])
def test_non_finite_and_huge_coordinates_mean_no_history(pkg, orc, fmt):
    W, H = 67, 41
    p = temporal_only(pkg)
    sx, sy = scales(pkg, W, H)      # (at this aspect the reference's own mapping loses most of a static frame's history)
    p.reproj_scale[0], p.reproj_scale[1] = sx, sy
    frames = [pkg.synth.render_frame(W, H, f, seed=13, moving=False, noise_model="hash") for f in range(2)]
    cam = frames[0][2]
    M = orc.view_matrix(pkg, cam)
    clean = motion_plane(M, W, H, frames[1][1].reshape(H, W), None, fmt, F(sx), F(sy))
    bad_values = [F(np.nan), F(np.inf), F(-np.inf), F(1e30), F(-1e30)]
    runs = {}
    for tag in ("clean", "bad"):
        den = pkg.Denoiser(W, H)
        den.set_capture(True)
        den.denoise_host(*frames[0][:2], cam, p)
        m = clean.copy()
        if tag == "bad":
            hl = runs["clean"][0]
            ys, xs = np.nonzero(hl == 2)                              # pixels that DO find their history otherwise
            pick = np.linspace(0, len(ys) - 1, 3 * len(bad_values)).astype(int)
            hit = np.zeros((H, W), dtype=bool)
            for k, i in enumerate(pick):
                v, where = bad_values[k % len(bad_values)], k // len(bad_values)      # in x, in y, in both
                if where != 1:
                    m[ys[i], xs[i], 0] = v
                if where != 0:
                    m[ys[i], xs[i], 1] = v
                hit[ys[i], xs[i]] = True
            assert np.count_nonzero(hit) == 3 * len(bad_values)
        den.denoise_host(*frames[1][:2], cam, p, motion=m, motion_format=fmt)
        runs[tag] = tuple(den.read_state(k) for k in (0, 1, 2, 3, 4))
        den.free()
    assert (runs["bad"][0][hit] == 1).all(), "history length 1"
    assert (runs["bad"][3][hit] == 100.0).all(), "variance 100"
    assert np.array_equal(runs["bad"][4][hit], frames[1][0].reshape(H, W, 3)[hit]), "accumulated colour = input"
    for k in range(5):
        assert np.array_equal(runs["bad"][k][~hit], runs["clean"][k][~hit], equal_nan=True), f"state {k} of the untouched pixels"


# ---- 7. nothing else moved ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_null_plane_is_svgf_denoise_and_non_temporal_frames_ignore_the_plane(pkg):
    import torch
    W, H, N = 96, 64, 3
    lib = pkg.load_library()
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gbt = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    junk = torch.full((H, W, 2), 3.5, dtype=torch.float32, device="cuda")
    for temporal in (1, 0):
        p = pkg.reference_defaults().set(temporal_enable=temporal, spatial_enable=1)
        a, b = pkg.Denoiser(W, H), pkg.Denoiser(W, H)
        out_a, out_b = torch.empty_like(rgb), torch.empty_like(rgb)
        for f in range(N):
            cam = pkg.SvgfCamera.from_dict(pkg.synth.camera_for_frame(f, True))
            pkg.binding.synth_render(rgb, gbt, W, H, cam, f, seed=2)
            a.denoise(out_a, rgb, gbt, cam, p)
            if temporal:      # NULL plane: exactly svgf_denoise (the format is not looked at)
                rc = lib.svgf_denoise_motion(b.h, out_b.data_ptr(), rgb.data_ptr(), gbt.data_ptr(), None, 99, ctypes.byref(cam), ctypes.byref(p), None)
                assert rc == 0, b.last_error()
            else:             # no temporal pass: the plane is not read
                b.denoise(out_b, rgb, gbt, cam, p, motion=junk, motion_format=D32)
            torch.cuda.synchronize()
            assert np.array_equal(out_a.cpu().numpy(), out_b.cpu().numpy()), f"temporal {temporal}, frame {f}"
            for which in (0, 1, 2):
                assert np.array_equal(a.read_state(which), b.read_state(which)), f"temporal {temporal}, state {which}, frame {f}"
        a.free(); b.free()


@pytest.mark.gpu
def test_unknown_format_and_parked_fused_kernels_are_refused_before_anything_runs(pkg):
    import torch
    W, H = 64, 48
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    gbt = torch.zeros((H * W * 52,), dtype=torch.uint8, device="cuda")
    mv = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    out = torch.empty_like(rgb)
    cam = pkg.synth.camera_for_frame(0, False)
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    d = pkg.Denoiser(W, H)
    d.denoise(out, rgb, gbt, cam, p)
    before = d.read_state(0).copy()
    for fmt in (0, 4, -1):
        with pytest.raises(pkg.SvgfError, match="-> -1"):
            d.denoise(out, rgb, gbt, cam, p, motion=mv, motion_format=fmt)
        with pytest.raises(pkg.SvgfError, match="-> -1"):
            d.planar_gbuffer()
            d.denoise_planar(out, rgb, cam, p, motion=mv, motion_format=fmt)
    assert np.array_equal(d.read_state(0), before), "a refused frame changes nothing"
    d.free()
    e = denoiser_for(pkg, W, H, 6)      # the experiments build: the fused temporal kernel has no motion input
    with pytest.raises(pkg.SvgfError, match="-> -5"):
        e.denoise(out, rgb, gbt, cam, pkg.SvgfParams.from_buffer_copy(p).set(kernel_variant=6), motion=mv)
    e.free()
