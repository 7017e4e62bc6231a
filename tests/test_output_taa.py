"""Output TAA (include/svgf.h: svgf_set_output_taa / svgf_get_output_taa): the frame's image blended with the
previous frame's output, reprojected like the temporal pass's history and clipped to the image's 3x3 neighbourhood.

The yardstick is tests/taa_model.py, fed the image C a twin context with the feature off writes for the same frames, the frame's
geomId and the PREV_COORD_F32 plane the kernel derives (temporal_model.coord_plane / motion_plane).

Bounds: every comparison of the kernel with the model, and of two contexts with each other, is on the bits of every pixel (NaNs in
the same place count as equal).  Both sides perform the same correctly rounded float32 operations in the same order without
contraction: there is no arithmetic that may differ, so there is no tolerance to choose.  The one tolerance in this file, 10 % around
alpha / (2 - alpha) on the model's variance reduction, is a cap around the value derived for an exponential average of independent
samples, not a measurement (the bare recurrence gives 0.108, 0.112 and 0.112 for seeds 1, 7 and 31).

One statement of the flat-image case is narrower here than a reader might expect: with sigma_scale = 1e6 the blend
0.25 C1 + 0.75 C0 results where the 3x3 window holds both colours (column 19).  Where the window is flat (columns <= 18) sigma is
exactly 0, 1e6 * 0 = 0, and the clip collapses the history onto C1 whatever sigma_scale is - which is the case's other statement."""
import ctypes

import numpy as np
import pytest

import taa_model as taa
import temporal_model as tm
from temporal_harness import SIDE, _hip, block_sequence, device_table, same_bits, scales, synth_sequence

F = np.float32
COORD, D32, D16 = tm.COORD, tm.D32, tm.D16
NEW_SYMBOLS = ("svgf_set_output_taa", "svgf_get_output_taa")
C0, C1 = np.array([0.5, 0.25, 1.0], F), np.array([2.0, 1.0, 0.25], F)      # the clamp tests' colours: every product and sum below is exact
ALPHAS, SIGMAS = (0.2, 1.0), (0.0, 1.0, 1e6)
NFRAMES = 6


# ---- 1. CPU: symbols and binding (fails without the feature) -------------------------------------------------------------------------
def test_symbols_are_exported_and_a_null_context_is_invalid(pkg):
    lib = pkg.load_library()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in pkg.binding.EXPORTS, n
    assert lib.svgf_set_output_taa(None, 0.2, 1.0) == -1
    assert lib.svgf_set_output_taa(None, 0.0, 0.0) == -1
    a, k = ctypes.c_float(7.0), ctypes.c_float(7.0)
    assert lib.svgf_get_output_taa(None, ctypes.byref(a), ctypes.byref(k)) == -1
    assert lib.svgf_get_output_taa(None, None, None) == -1
    assert (a.value, k.value) == (7.0, 7.0), "nothing is written on failure"
    assert hasattr(pkg.Denoiser, "set_output_taa") and hasattr(pkg.Denoiser, "output_taa")
    assert pkg.binding.KERNEL_OUTPUT_TAA == 7


# ---- 2. CPU: the model's statement on a flat image -------------------------------------------------------------------------------------
def _flat_sequence(W=40, H=24, other_gid=False):
    imgs = [np.tile(C0, (H, W, 1)) for _ in range(4)]
    imgs[3][:, :20] = C1
    gids = [np.zeros((H, W), np.int32) for _ in range(4)]
    if other_gid:
        gids[3][:, :20] = 5
    return imgs, gids, [tm.pixel_grid(W, H)] * 4


@pytest.mark.parametrize("k", SIGMAS)
def test_model_flat_image_any_sigma_scale(k):
    imgs, gids, coords = _flat_sequence()
    out = taa.run_sequence(imgs, gids, coords, 0.25, k)
    for f in range(3):
        assert same_bits(out[f], imgs[f]), f"frame {f}: a constant sequence comes back with identical bits"
    assert same_bits(out[3][:, :19], np.broadcast_to(C1, out[3][:, :19].shape).copy()), "flat window: the clip collapses the history onto C1"
    assert same_bits(out[3][:, 21:], np.broadcast_to(C0, out[3][:, 21:].shape).copy())


def test_model_flat_image_inert_clip_blends_and_another_geom_id_does_not():
    imgs, gids, coords = _flat_sequence()
    out = taa.run_sequence(imgs, gids, coords, 0.25, 1e6)[3]
    blend = (F(0.25) * C1 + F(0.75) * C0).astype(F)
    assert same_bits(blend, np.array([0.875, 0.4375, 0.8125], F))
    assert same_bits(out[:, 19], np.broadcast_to(blend, out[:, 19].shape).copy()), "mixed window, sigma > 0, times 1e6: the clip is inert"
    assert same_bits(out[:, 20], np.broadcast_to(C0, out[:, 20].shape).copy())
    assert same_bits(out[:, :19], np.broadcast_to(C1, out[:, :19].shape).copy()), "sigma == 0 exactly: 1e6 * 0 = 0"
    imgs, gids, coords = _flat_sequence(other_gid=True)
    out = taa.run_sequence(imgs, gids, coords, 0.25, 1e6)[3]
    assert same_bits(out[:, :20], np.broadcast_to(C1, out[:, :20].shape).copy()), "no tap counted: no history"
    assert same_bits(out[:, 20:], np.broadcast_to(C0, out[:, 20:].shape).copy())


# ---- 3. CPU: the model accumulates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 7, 31])
def test_model_accumulates(seed):
    W = H = 64
    alpha, n = 0.2, 40
    rng = np.random.default_rng(seed)
    gid, coord = np.zeros((H, W), np.int32), tm.pixel_grid(W, H)
    prev = None
    for _ in range(n):
        img = (1.0 + 0.5 * rng.standard_normal((H, W, 3))).astype(F)
        o, prev = taa.output_taa(img, gid, coord, prev, alpha, 1e3)
    ratio = float(np.var(o.astype(np.float64)) / np.var(img.astype(np.float64)))
    want = alpha / (2.0 - alpha)
    print(f"seed {seed}: variance of the output / variance of the input {ratio:.4f}, alpha / (2 - alpha) = {want:.4f}")
    assert abs(ratio - want) <= 0.1 * want


# ---- 4. CPU: non-finite inputs in the model ---------------------------------------------------------------------------------------------
def test_model_non_finite_inputs_follow_the_arithmetic():
    W, H = 9, 7
    rng = np.random.default_rng(5)
    prev_col = rng.uniform(0.1, 2.0, (H, W, 3)).astype(F)
    img = rng.uniform(0.1, 2.0, (H, W, 3)).astype(F)
    gid = np.zeros((H, W), np.int32)
    gid[0, 0] = -1
    prev = (prev_col, np.zeros((H, W), np.int32))
    coord = (tm.pixel_grid(W, H) + F(0.25)).astype(F)
    bad = {(1, 1): (np.nan, 1.0), (2, 1): (1.0, np.nan), (3, 1): (np.inf, 1.0), (4, 1): (1.0, -np.inf), (5, 1): (-3.0, 2.0),
           (6, 1): (2.0, float(H)), (7, 1): (3e38, 1.0), (1, 2): (-0.5, 2.0)}
    for (x, y), v in bad.items():
        coord[y, x] = v
    o, hist = taa.output_taa(img, gid, coord, prev, 0.2, 1.0)
    have = taa.has_history(img, gid, coord, prev, 0.2, 1.0)
    want = np.ones((H, W), bool)
    want[0, 0] = False                      # geomId == -1
    for (x, y) in bad:
        want[y, x] = False                  # floor off the screen, NaN, +-inf
    assert np.array_equal(have, want)
    assert same_bits(o[~have], img[~have]), "no history: the output is the image"
    assert np.isfinite(o).all() and same_bits(hist[0], o) and np.array_equal(hist[1], gid)
    # the last column and row look at taps outside the image: not counted, the remaining weights renormalise
    assert have[3, W - 1] and have[H - 1, 3]
    # NaN / inf in C: the window statistics are NaN, the comparisons false, h unchanged; the blend runs as written
    img2 = img.copy()
    img2[3, 4] = (np.nan, np.inf, 1.0)
    o2 = taa.output_taa(img2, gid, coord, prev, 0.2, 1.0)[0]
    assert np.isnan(o2[3, 4, 0]) and np.isinf(o2[3, 4, 1]) and np.isfinite(o2[3, 4, 2])
    assert np.isfinite(o2[0:2, 0:3]).all(), "pixels whose window does not hold the texel are untouched"
    # NaN / inf in the history: taps carry it into h; h = NaN passes the clip unchanged, +inf is clipped to hi
    prev3 = (prev_col.copy(), prev[1])
    prev3[0][3, 4] = (np.nan, np.inf, 1.0)
    o3 = taa.output_taa(img, gid, coord, prev3, 0.2, 1e6)[0]
    assert np.isnan(o3[3, 4, 0]) and np.isfinite(o3[3, 4, 1]) and np.isfinite(o3[3, 4, 2])
    assert taa.has_history(img, gid, coord, prev3, 0.2, 1e6)[3, 4]
    # all of it without a history: the image, bit for bit
    assert same_bits(taa.output_taa(img2, gid, coord, None, 0.2, 1.0)[0], img2)


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------
def _upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _texels(gb):
    import torch
    return torch.from_numpy(np.ascontiguousarray(gb).view(np.uint8).reshape(-1).copy()).cuda()


def _fill_planes(den, gb):
    g = den.planar_gbuffer()
    hip = _hip()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    flat = np.ascontiguousarray(gb).reshape(-1)
    for dst, arr in ((g.normal, flat["normal"]), (g.position, flat["position"]), (g.geom_id, flat["geomId"]),
                     (g.albedo, (flat["albedo"] * flat["ialbedo"]).astype(F))):
        arr = np.ascontiguousarray(arr)
        assert hip.hipMemcpy(dst, arr.ctypes.data, arr.nbytes, 1) == 0


def run_outputs(pkg, den, frames, params, cams, leg="aos", planes=None, fmt=COORD, tables=None, device_planes=None, plist=None):
    """frames: [(colour, texels)]; per frame the output.  planes: per frame a host motion plane of format `fmt`; device_planes: the
    format svgf_motion_reproject writes the plane in on the device (for the previous frame's camera, params' reproj_scale and the
    frame's table); tables: per frame X, set as the context's object motion table before the frame; plist: per frame the parameters."""
    import torch
    H, W = frames[0][1].shape
    res, keep = [], []
    for f, (col, gb) in enumerate(frames):
        p = plist[f] if plist is not None else params
        t_c, t_g = _upload(np.asarray(col, F)), _texels(gb)
        t_x = device_table(tables[f]) if tables is not None else None
        mv = None if planes is None else _upload(planes[f])
        if device_planes is not None:
            fmt = device_planes
            mv = torch.empty((H, W, 2), dtype=torch.float16 if fmt == D16 else torch.float32, device="cuda")
            pkg.binding.motion_reproject(mv, W, H, cams[max(f - 1, 0)], gbuffer=t_g, motion_format=fmt,
                                         reproj_scale=(p.reproj_scale[0], p.reproj_scale[1]), geom_xf=t_x)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        keep.append((t_c, t_g, t_x, mv, out))
        torch.cuda.synchronize()
        if tables is not None:
            den.set_object_motion(t_x, tables[f].shape[0])
        if leg == "planar":
            _fill_planes(den, gb)
            den.denoise_planar(out, t_c, cams[f], p, motion=mv, motion_format=fmt)
        else:
            den.denoise(out, t_c, t_g, cams[f], p, motion=mv, motion_format=fmt)
        den.sync()
        res.append(out.cpu().numpy())
    return res


def synth_coords(pkg, seq, fmt, W, H):
    """(host planes of format fmt, the PREV_COORD_F32 planes the kernel derives from them): the camera path's own projection of every
    frame's positions through the previous frame's view matrix (frame 0: its own; no history there)."""
    sx, sy = scales(pkg, W, H)
    planes = [tm.motion_plane(seq[max(f - 1, 0)][3], W, H, seq[f][1], None, fmt, F(sx), F(sy)) for f in range(len(seq))]
    return planes, [tm.coord_plane(pl, fmt, W, H) for pl in planes]


def full_params(pkg, W, H, **kw):
    p = pkg.reference_defaults().set(**{**dict(temporal_enable=1, spatial_enable=1, atrous_nlevel=5, history_level=1), **kw})
    p.reproj_scale[0], p.reproj_scale[1] = scales(pkg, W, H)
    return p


# ---- 5. GPU: the kernel equals the model, bit for bit, on every pixel -------------------------------------------------------------------
# 65x5 and 130x9 cross the 64-column and 4-row tile seams; neither width nor height of 37x23 is a multiple of the tile; 1x1 and 5x3
# are all edge
SIZES = [(1, 1), (5, 3), (65, 5), (130, 9), (37, 23)]
MODES = {"cascade": dict(), "copy": dict(spatial_enable=0), "modulate": dict(sepcolor=1, addcolor=1)}


def _configs():
    """(name, motion format or None, SvgfParams fields, (clamp radius, k), (firefly rank, scale), [(alpha, sigma_scale)])"""
    every = [(a, k) for a in ALPHAS for k in SIGMAS]
    out = []
    for fmt in (None, COORD, D32, D16):
        for temporal in (1, 0):
            for mode, kw in MODES.items():
                out.append((f"motion {fmt} temporal {temporal} {mode}", fmt, dict(temporal_enable=temporal, **kw), (0, 0.0), (0, 0.0), every))
    out.append(("history clamp 2 + firefly filter", None, dict(), (2, 1.0), (1, 1.0), [(0.2, 1.0)]))
    out.append(("kernel_variant 1", COORD, dict(kernel_variant=1), (0, 0.0), (0, 0.0), [(0.2, 1.0)]))
    out.append(("kernel_variant 4", None, dict(kernel_variant=4), (0, 0.0), (0, 0.0), [(0.2, 1.0)]))
    out.append(("history_level == atrous_nlevel", D32, dict(history_level=5), (0, 0.0), (0, 0.0), [(0.2, 1.0)]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["aos", "planar"])
@pytest.mark.parametrize("W,H", SIZES)
def test_hip_equals_the_model_on_every_pixel(pkg, orc, W, H, leg):
    """Six frames under the moving camera.  C is the output of a twin context with the feature off, fed the same frames."""
    seq = synth_sequence(pkg, orc, W, H, n=NFRAMES)
    frames, cams = [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]
    gids = [g["geomId"] for _, g in frames]
    twin, den = pkg.Denoiser(W, H), pkg.Denoiser(W, H)
    acted = blended = False
    try:
        for name, fmt, kw, clamp, firefly, settings in _configs():
            planes, coords = synth_coords(pkg, seq, fmt or COORD, W, H)
            if fmt is None:
                planes = None
            params = full_params(pkg, W, H, **kw)
            for d in (twin, den):
                d.set_history_clamp(*clamp)
                d.set_firefly_filter(*firefly)
            twin.reset()
            C = run_outputs(pkg, twin, frames, params, cams, leg, planes, fmt or COORD)
            for alpha, k in settings:
                den.reset()
                den.set_output_taa(alpha, k)
                got = run_outputs(pkg, den, frames, params, cams, leg, planes, fmt or COORD)
                ref = taa.run_sequence(C, gids, coords, alpha, k)
                for f in range(NFRAMES):
                    assert same_bits(got[f], ref[f]), f"{W}x{H} {leg} {name} alpha {alpha} sigma_scale {k}: frame {f}"
                acted = acted or not same_bits(ref[-1], C[-1])
                blended = blended or bool(taa.has_history(C[-1], gids[-1], coords[-1], (ref[-2], gids[-2]), alpha, k).any())
    finally:
        twin.free(); den.free()
    if W >= 37:
        assert acted and blended, "the pass acts on this sequence: some history survives the moving camera"


# ---- 6. GPU: the camera path equals the plane path ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_camera_path_equals_the_plane_svgf_motion_reproject_writes(pkg, orc):
    """No motion plane against the PREV_COORD_F32 plane svgf_motion_reproject writes on the device for the previous camera, under
    the moving camera."""
    W, H = 65, 5
    seq = synth_sequence(pkg, orc, W, H, n=NFRAMES)
    frames, cams = [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]
    params = full_params(pkg, W, H)
    res = {}
    for how in ("camera", "plane"):
        d = pkg.Denoiser(W, H)
        d.set_output_taa(0.2, 1.0)
        res[how] = run_outputs(pkg, d, frames, params, cams, device_planes=COORD if how == "plane" else None)
        d.free()
    for f in range(NFRAMES):
        assert same_bits(res["camera"][f], res["plane"][f]), f"frame {f}"


@pytest.mark.gpu
@pytest.mark.parametrize("table", [False, True], ids=["no table", "object table"])
def test_camera_path_equals_the_plane_path_on_the_moving_block(pkg, table):
    """box_room's turned block sliding and turning under a static camera, temporal pass and five levels.  Without a table: no plane
    against the plane of the unmoved positions.  With the table: the table alone against the table plus the plane written with it."""
    cam, seq = block_sequence(pkg, NFRAMES, 0.4, 3.0)
    frames, tables = [(c, g) for c, g, _ in seq], [X for _, _, X in seq]
    cams = [cam] * NFRAMES
    params = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=5, history_level=1)
    res = {}
    for how in ("camera", "plane", "off"):
        d = pkg.Denoiser(SIDE, SIDE)
        if how != "off":
            d.set_output_taa(0.2, 1.0)
        res[how] = run_outputs(pkg, d, frames, params, cams, tables=tables if table else None,
                               device_planes=COORD if how == "plane" else None)
        d.free()
    for f in range(NFRAMES):
        assert same_bits(res["camera"][f], res["plane"][f]), f"frame {f}"
    assert not same_bits(res["camera"][-1], res["off"][-1]), "the pass acts on this sequence"


# ---- 7. GPU: off is off ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_is_off_and_on_is_one_launch_at_the_end(pkg, orc):
    W, H = 65, 5
    seq = synth_sequence(pkg, orc, W, H, n=NFRAMES)
    frames, cams = [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]
    params = full_params(pkg, W, H)
    b = pkg.binding
    res, kinds = {}, {}
    for how in ("never", "toggled", "on"):
        d = pkg.Denoiser(W, H)
        assert d.output_taa() == (0.0, 0.0)
        if how == "toggled":
            d.set_output_taa(0.2, 1.0)
            d.set_output_taa(0.0, 0.0)
        if how == "on":
            d.set_output_taa(0.2, 1.0)
        d.profile_stride(1)
        d.profile_enable(NFRAMES)
        res[how] = run_outputs(pkg, d, frames, params, cams)
        kinds[how] = [[kk for kk, _ in d.profile_read(s)] for s in range(NFRAMES)]
        d.free()
    for f in range(NFRAMES):
        assert same_bits(res["never"][f], res["toggled"][f]), f"frame {f}"
    assert kinds["never"] == kinds["toggled"] == [[b.KERNEL_TEMPORAL] + [b.KERNEL_ATROUS] * 5] * NFRAMES, kinds
    assert kinds["on"] == [[b.KERNEL_TEMPORAL] + [b.KERNEL_ATROUS] * 5 + [b.KERNEL_OUTPUT_TAA]] * NFRAMES, kinds["on"]
    assert not same_bits(res["never"][-1], res["on"][-1])


# ---- 8. GPU: the life of the output history ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_history_lifecycle(pkg, orc):
    """The twin (feature off) and the context run the same calls; a frame without an output history equals the twin's, bit for bit."""
    import torch
    W, H = 65, 5
    seq = synth_sequence(pkg, orc, W, H, n=NFRAMES)
    params, debug = full_params(pkg, W, H), full_params(pkg, W, H, right_view_option=1)
    twin, d = pkg.Denoiser(W, H), pkg.Denoiser(W, H)
    d.set_output_taa(0.25, 1.5)
    assert d.output_taa() == (0.25, 1.5)

    def frame(f, p=params):
        col, gb, cam, _ = seq[f]
        t_c, t_g = _upload(col), _texels(gb)
        outs = []
        for den in (twin, d):
            out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            den.denoise(out, t_c, t_g, cam, p)
            den.sync()
            outs.append(out.cpu().numpy())
        return outs

    c, o = frame(0)
    assert same_bits(c, o), "the first frame"
    c, o = frame(1)
    assert not same_bits(c, o), "the second frame blends"
    twin.reset(); d.reset()
    assert d.output_taa() == (0.25, 1.5), "svgf_reset keeps the setting"
    c, o = frame(2)
    assert same_bits(c, o), "the frame after svgf_reset"
    c, o = frame(3)
    assert not same_bits(c, o)
    c, o = frame(4, debug)
    assert same_bits(c, o), "a debug view is written as it is"
    c, o = frame(5)
    assert same_bits(c, o), "the frame after a debug view"
    c, o = frame(0)
    assert not same_bits(c, o)
    d.set_output_taa(0.0, 1.5)
    c, o = frame(1)
    assert same_bits(c, o), "the feature off"
    d.set_output_taa(0.25, 1.5)
    c, o = frame(2)
    assert same_bits(c, o), "the frame after a frame run with the feature off"
    c, o = frame(3)
    assert not same_bits(c, o)
    twin.free(); d.free()


# ---- 9. GPU: the frame pipeline ----------------------------------------------------------------------------------------------------------
def _pipeline_run(pkg, W, H, mode, leg, n, taa_on=True):
    """n frames under the moving camera; mode 0: ordered frames on a plain context; 1: the promise; 2: two caller streams in turn."""
    import torch
    d = pkg.Denoiser(W, H, 0, pipelined=mode != 0)
    if mode == 1 and d.pipeline_status() == 2:
        d.free()
        pytest.skip("the context's two streams share a hardware queue: the promise is refused")
    if taa_on:
        d.set_output_taa(0.2, 1.0)
    p = full_params(pkg, W, H, inputs_ready=mode)
    cams = [pkg.synth.camera_for_frame(f, True) for f in range(n)]
    st = [torch.cuda.Stream(), torch.cuda.Stream()]
    rgb = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(n)]
    gbt = [torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda") for _ in range(n)]
    outs = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    for f in range(n):
        s = st[f & 1] if mode == 2 else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            if leg == "planar":
                planes = d.planar_gbuffer(stream=s) if mode == 2 else d.planar_gbuffer()
                pkg.binding.synth_render_planar(rgb[f], planes, W, H, cams[f], f, seed=19, stream=s)
            else:
                pkg.binding.synth_render(rgb[f], gbt[f], W, H, cams[f], f, seed=19, stream=s)
            if mode == 1:
                torch.cuda.synchronize()      # the promise: the inputs are complete at call time
            if leg == "planar":
                d.denoise_planar(outs[f], rgb[f], cams[f], p, stream=s)
            else:
                d.denoise(outs[f], rgb[f], gbt[f], cams[f], p, stream=s)
    torch.cuda.synchronize()
    assert mode == 0 or d.is_pipelined()
    res = [o.cpu().numpy() for o in outs]
    d.free()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["aos", "planar"])
@pytest.mark.parametrize("mode", [1, 2], ids=["promised", "two streams"])
@pytest.mark.parametrize("W,H", [(130, 9), (65, 5)])
def test_pipelined_frames_are_bit_identical_to_ordered_frames(pkg, W, H, mode, leg):
    n = 12
    want = _pipeline_run(pkg, W, H, 0, leg, n)
    got = _pipeline_run(pkg, W, H, mode, leg, n)
    for f in range(n):
        assert same_bits(want[f], got[f]), f"frame {f}"
    off = _pipeline_run(pkg, W, H, 0, leg, n, taa_on=False)
    assert not same_bits(want[-1], off[-1]), "the pass acts on this sequence"


# ---- 10. GPU: graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_captured_pair_of_frames_replays_bit_identically(pkg):
    """Two eager frames, two frames captured on a stream, the graph replayed twice: six eager frames.  A static camera: the previous
    view matrix is a kernel argument (tests/test_stream_gpu.py)."""
    import torch
    hip = _hip()
    W, H = 130, 9
    fr = [pkg.synth.render_frame(W, H, f, seed=9, moving=False) for f in range(6)]
    cols, gbs, cam = [_upload(f[0]) for f in fr], [_texels(f[1]) for f in fr], pkg.SvgfCamera.from_dict(fr[0][2])
    p = full_params(pkg, W, H)
    d = pkg.Denoiser(W, H)
    d.set_output_taa(0.2, 1.0)
    want = []
    for f in range(6):
        o = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        d.denoise(o, cols[f], gbs[f], cam, p)
        d.sync()
        want.append(o.cpu().numpy())
    d.free()
    d = pkg.Denoiser(W, H)
    d.set_output_taa(0.2, 1.0)
    s = torch.cuda.Stream()
    cin, gin = [torch.empty_like(cols[0]) for _ in range(2)], [torch.empty_like(gbs[0]) for _ in range(2)]
    out = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)]

    def refresh(r):
        with torch.cuda.stream(s):
            for k in range(2):
                cin[k].copy_(cols[2 * r + k]); gin[k].copy_(gbs[2 * r + k])

    torch.cuda.synchronize()
    refresh(0)
    for k in range(2):
        d.denoise(out[k], cin[k], gin[k], cam, p, stream=s)
    d.sync_stream(s)
    got = [out[0].cpu().numpy(), out[1].cpu().numpy()]
    graph, gexec = ctypes.c_void_p(), ctypes.c_void_p()
    hip.hipStreamBeginCapture.argtypes = [ctypes.c_void_p, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    hip.hipGraphInstantiate.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    hip.hipGraphLaunch.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipGraphExecDestroy.argtypes = [ctypes.c_void_p]
    hip.hipGraphDestroy.argtypes = [ctypes.c_void_p]
    assert hip.hipStreamBeginCapture(s.cuda_stream, 2) == 0           # hipStreamCaptureModeRelaxed
    for k in range(2):
        d.denoise(out[k], cin[k], gin[k], cam, p, stream=s)           # recorded, not executed
    assert hip.hipStreamEndCapture(s.cuda_stream, ctypes.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, 0) == 0
    for r in (1, 2):
        refresh(r)
        assert hip.hipGraphLaunch(gexec, s.cuda_stream) == 0
        d.sync_stream(s)
        got += [out[0].cpu().numpy(), out[1].cpu().numpy()]
    hip.hipGraphExecDestroy(gexec); hip.hipGraphDestroy(graph)
    d.free()
    for f in range(6):
        assert same_bits(got[f], want[f]), f"frame {f}: graph replay differs from the eager run"


# ---- 11. GPU: svgf_denoise_host ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_denoise_host_honours_it(pkg, orc):
    W, H = 37, 23
    seq = synth_sequence(pkg, orc, W, H, n=NFRAMES)
    frames, cams = [(c, g) for c, g, _, _ in seq], [c for _, _, c, _ in seq]
    params = full_params(pkg, W, H)
    dev, host, off = pkg.Denoiser(W, H), pkg.Denoiser(W, H), pkg.Denoiser(W, H)
    dev.set_output_taa(0.2, 1.0)
    host.set_output_taa(0.2, 1.0)
    want = run_outputs(pkg, dev, frames, params, cams)
    plain = run_outputs(pkg, off, frames, params, cams)
    for f, (col, gb) in enumerate(frames):
        got = host.denoise_host(col, gb, cams[f], params).reshape(H, W, 3)
        assert same_bits(got, want[f]), f"frame {f}"
    assert not same_bits(want[-1], plain[-1]), "the pass acts on this sequence"
    dev.free(); host.free(); off.free()


# ---- 12. GPU: limits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_invalid_settings_are_refused_and_change_nothing(pkg):
    lib = pkg.load_library()
    d = pkg.Denoiser(8, 8)
    d.set_output_taa(0.5, 1.5)
    nan, inf = float("nan"), float("inf")
    for alpha, k, word in ((-0.1, 1.0, "alpha"), (1.5, 1.0, "alpha"), (nan, 1.0, "alpha"), (inf, 1.0, "alpha"), (-inf, 1.0, "alpha"),
                           (0.2, -0.5, "sigma_scale"), (0.2, nan, "sigma_scale"), (0.2, inf, "sigma_scale"), (0.2, -inf, "sigma_scale")):
        assert lib.svgf_set_output_taa(d.h, alpha, k) == -1, (alpha, k)
        assert word in d.last_error(), d.last_error()
        with pytest.raises(pkg.SvgfError, match="-> -1"):
            d.set_output_taa(alpha, k)
        assert d.output_taa() == (0.5, 1.5), "a refused call changes nothing"
    a = ctypes.c_float(-7.0)
    assert lib.svgf_get_output_taa(d.h, ctypes.byref(a), None) == 0 and a.value == 0.5, "either pointer may be NULL"
    k = ctypes.c_float(-7.0)
    assert lib.svgf_get_output_taa(d.h, None, ctypes.byref(k)) == 0 and k.value == 1.5
    d.set_output_taa(1.0, 0.0)
    assert d.output_taa() == (1.0, 0.0)
    assert d.history_clamp() == (0, 0.0) and d.firefly_filter() == (0, 0.0), "a setting of its own"
    d.free()


@pytest.mark.gpu
def test_an_image_taller_than_the_tiled_grid_is_refused_not_launched(pkg):
    """The pass's grid has one row of workgroups per four image rows, at most 65535 of them: 1 x 262141 is one tile row too tall.
    Refused when the frame is planned; with the feature off, and at 1 x 262140 with it on, the frame runs."""
    import torch
    cam = pkg.synth.camera_for_frame(0, False)
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=0)
    for H, ok in ((262141, False), (262140, True)):
        rgb = torch.ones((H, 1, 3), dtype=torch.float32, device="cuda")
        gbt = torch.zeros((H * 52,), dtype=torch.uint8, device="cuda")
        out = torch.empty_like(rgb)
        d = pkg.Denoiser(1, H)
        d.denoise(out, rgb, gbt, cam, p)
        d.sync()
        d.set_output_taa(0.2, 1.0)
        if ok:
            for _ in range(2):
                d.denoise(out, rgb, gbt, cam, p)
            d.sync()
            assert (out.cpu().numpy() == 1.0).all(), "constant colour in, constant colour out"
        else:
            with pytest.raises(pkg.SvgfError, match="-> -5"):
                d.denoise(out, rgb, gbt, cam, p)
            assert "262140" in d.last_error() and "svgf_set_output_taa" in d.last_error()
            d.sync()
            assert (d.read_state(0) == 1).all(), "a refused frame enqueues nothing"
            d.set_output_taa(0.0, 0.0)
            d.denoise(out, rgb, gbt, cam, p)      # off: the frame runs
            d.sync()
        d.free()


@pytest.mark.gpu
@pytest.mark.experiments
@pytest.mark.parametrize("which", ["kernel_variant_6", "split_fused"])
def test_parked_fused_temporal_kernels_refuse_a_frame_with_the_pass(pkg, experiments_lib, which):
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
    e.denoise(out, rgb, gbt, cam, p)                   # feature off: runs
    e.sync()
    before = e.read_state(0).copy()
    e.set_output_taa(0.2, 1.0)
    with pytest.raises(pkg.SvgfError, match="-> -5"):
        e.denoise(out, rgb, gbt, cam, p)
    assert "output pass" in e.last_error()
    e.sync()
    assert np.array_equal(e.read_state(0), before), "a refused frame enqueues nothing"
    e.set_output_taa(0.0, 1.0)
    e.denoise(out, rgb, gbt, cam, p)                   # off again: runs
    e.sync()
    e.free()
