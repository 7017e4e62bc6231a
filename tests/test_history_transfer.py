"""History transfer (include/svgf.h: svgf_transfer_history): the whole history of one context carried into a
context of a different (or the same) size.

The yardstick is tests/transfer_model.py.  Every comparison of the kernel with the model is on the bits of every pixel (NaNs in the
same place count as equal): both sides perform the same correctly rounded float32 operations in the same order without contraction,
so there is no tolerance to choose.  The statements about the model itself are exact too, except one: at the ratios 1.5 and 4/3,
whose weights are not dyadic, a flat state stays flat within 4 units in the last place - four rounded products, three sums and one
division.

"Earns its place" (test_model_transfer_beats_a_reset): the model alone, the synthetic scene under a static camera, six frames at
96x54, the transfer to 128x72 and one temporal frame there; the mean absolute error against the clean 128x72 frame with the
transfer over the same error after a reset.  Measured before the bound was fixed: 0.436 (0.0534 against 0.1225); the test asserts
ratio <= 2 x that.  0.436 is ABOVE the 0.35 this row set itself as the mark of a feature that has earned its place.  For scale: the
same figure for an equal-size transfer - the unbroken sequence, the most any transfer could keep - is 0.518 on this scene (the
resampled one is lower because the four-tap mean also averages noise), so the mark is out of reach of the temporal filter itself
after six frames at color_alpha 0.2, not of the transfer.  The condition on the inputs: with the transfer >= 50 % of the non-miss
pixels of that frame have history length >= 2 (measured 98 %), with a reset none."""
import ctypes

import numpy as np
import pytest

import firefly_model as ff
import taa_model as taa
import temporal_harness as th
import temporal_model as tm
import transfer_model as xm
from temporal_harness import same_bits, scales

F = np.float32
C0, C1 = np.array([0.5, 0.25, 1.0], F), np.array([2.0, 1.0, 0.25], F)      # tests/test_upsample.py's dyadic colours
INVALID, UNSUPPORTED = -1, -5
MEASURED_RATIO = 0.436
HIST = dict(hlen=0, mom=1, color=2, normal=5, position=6, gid=7)      # svgf_read_state kinds: what the next frame reads as history
PLANES = ("hlen", "mom", "color", "normal", "position", "gid")
DYADIC = [((8, 6), (16, 12)), ((16, 12), (8, 6)), ((16, 12), (4, 3)), ((5, 3), (10, 6)), ((12, 8), (3, 2))]      # ratios 1/2, 2, 4
OTHER = [((12, 9), (8, 6)), ((8, 6), (12, 9)), ((16, 12), (12, 9)), ((9, 6), (12, 8)), ((96, 54), (128, 72)), ((193, 11), (130, 7))]


# ---- 1. CPU: symbol, binding, argument checking (fails without the feature) ----------------------------------------------------------------
def test_symbol_is_exported_and_the_binding_exists(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "svgf_transfer_history")
    b = pkg.binding
    assert "svgf_transfer_history" in b.EXPORTS
    assert callable(b.Denoiser.transfer_history_from)
    assert (b.STATE_PREV_NORMAL, b.STATE_PREV_POSITION, b.STATE_PREV_GEOM_ID, b.STATE_OUTPUT_HISTORY) == (5, 6, 7, 8)
    assert (pkg.STATE_PREV_NORMAL, pkg.STATE_PREV_POSITION, pkg.STATE_PREV_GEOM_ID, pkg.STATE_OUTPUT_HISTORY) == (5, 6, 7, 8)


def test_a_null_context_is_invalid(pkg):
    """Answered before either pointer is looked at: the other one is a dummy that is never dereferenced."""
    lib = pkg.load_library()
    P = 0x1000
    assert lib.svgf_transfer_history(None, P, None) == INVALID
    assert lib.svgf_transfer_history(P, None, None) == INVALID
    assert lib.svgf_transfer_history(None, None, None) == INVALID


# ---- 2. CPU: what the model says ---------------------------------------------------------------------------------------------------------
def random_state(W, H, seed=3, nonfinite=True):
    rng = np.random.default_rng(seed)
    st = tm.empty_state(W, H)
    st["hlen"] = rng.integers(0, 9, (H, W)).astype(np.int32)
    st["mom"] = rng.uniform(0, 2, (H, W, 2)).astype(F)
    st["color"] = rng.uniform(0, 2, (H, W, 3)).astype(F)
    st["normal"] = rng.normal(size=(H, W, 3)).astype(F)
    st["position"] = rng.normal(size=(H, W, 3)).astype(F)
    st["gid"] = rng.integers(-1, 3, (H, W)).astype(np.int32)
    if nonfinite:
        flat = st["color"].reshape(-1)
        for val in (np.nan, np.inf, -np.inf):
            flat[rng.integers(0, flat.size, max(1, flat.size // 20))] = val
    return st


def two_objects(W, H):
    """Object 0 left of a slanted edge, object 1 right of it; colour C0 / C1, moments (1, 2) / (4, 0.5), history length 5."""
    ys, xs = np.mgrid[0:H, 0:W]
    gid = (xs + ys // 2 >= W // 2).astype(np.int32)
    st = tm.empty_state(W, H)
    st["gid"] = gid
    st["hlen"][:] = 5
    st["color"] = np.where(gid[..., None] == 1, C1, C0).astype(F)
    st["mom"] = np.where(gid[..., None] == 1, np.array([4.0, 0.5], F), np.array([1.0, 2.0], F)).astype(F)
    st["normal"][..., 2] = 1
    return st


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (64, 4)])
def test_model_equal_size_is_the_identity_on_every_bit(W, H):
    st = random_state(W, H)
    out = xm.transfer(st, W, H)
    for k in PLANES:
        assert out[k].dtype == st[k].dtype and np.array_equal(out[k].view(np.uint32), st[k].view(np.uint32)), k
        assert out[k] is not st[k]
    rgb, gid = xm.transfer_output_history((st["color"], st["gid"]), W, H)
    assert np.array_equal(rgb.view(np.uint32), st["color"].view(np.uint32)) and np.array_equal(gid, st["gid"])


@pytest.mark.parametrize("src,dst", DYADIC + OTHER)
def test_model_constant_history_length_and_true_texels(src, dst):
    """A constant history length stays constant; geomId, normal and position of every dst pixel are the bits of ONE src texel (the
    same one for the three planes and the history length), which lies within half a src texel (+ rounding) of the pixel's centre."""
    (Ws, Hs), (Wd, Hd) = src, dst
    st = random_state(Ws, Hs, seed=Ws + Hd)
    st["hlen"][:] = 7
    tag = np.arange(Ws * Hs, dtype=np.int32).reshape(Hs, Ws)
    st["position"][..., 0] = tag.astype(F)      # (exact: below 2^24) which texel a value came from
    out = xm.transfer(st, Wd, Hd)
    assert (out["hlen"] == 7).all()
    idx = out["position"][..., 0].astype(np.int64)
    ya, xa = idx // Ws, idx % Ws
    for k in ("gid", "normal", "position"):
        assert np.array_equal(out[k].view(np.uint32), st[k][ya, xa].view(np.uint32)), k
    cx = (np.arange(Wd) + 0.5) * Ws / Wd - 0.5
    cy = (np.arange(Hd) + 0.5) * Hs / Hd - 0.5
    assert (np.abs(xa - cx[None, :]) <= 0.5 + 1e-4).all() and (np.abs(ya - cy[:, None]) <= 0.5 + 1e-4).all()


@pytest.mark.parametrize("src,dst", DYADIC)
def test_model_never_mixes_across_geom_ids_exact_at_dyadic_ratios(src, dst):
    (Ws, Hs), (Wd, Hd) = src, dst
    st = two_objects(Ws, Hs)
    out = xm.transfer(st, Wd, Hd)
    g = out["gid"]
    assert set(np.unique(g)) == {0, 1}, "both objects survive"
    assert same_bits(out["color"], np.where(g[..., None] == 1, C1, C0).astype(F))
    assert same_bits(out["mom"], np.where(g[..., None] == 1, np.array([4.0, 0.5], F), np.array([1.0, 2.0], F)).astype(F))
    rgb, gh = xm.transfer_output_history((st["color"], st["gid"]), Wd, Hd)
    assert np.array_equal(gh, g) and same_bits(rgb, out["color"])


@pytest.mark.parametrize("src,dst", DYADIC + OTHER)
def test_model_flat_state_stays_flat(src, dst):
    """Exactly where weights and values are dyadic (ratios 1/2, 2, 4: every product and sum is exact); within 4 units in the last
    place for any value at any ratio (four rounded products, three sums and one division)."""
    (Ws, Hs), (Wd, Hd) = src, dst
    for exact, c, m in ((True, C0, np.array([1.0, 2.0], F)), (False, np.array([0.3, 1.7, 0.9], F), np.array([0.7, 1.3], F))):
        if exact and (src, dst) not in DYADIC:
            continue
        st = tm.empty_state(Ws, Hs)
        st["hlen"][:] = 3
        st["color"][:], st["mom"][:] = c, m
        out = xm.transfer(st, Wd, Hd)
        for got, want in ((out["color"], c), (out["mom"], m)):
            want = np.ascontiguousarray(np.broadcast_to(want, got.shape))
            if exact:
                assert same_bits(got, want)
            else:
                ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
                assert ulps.max() <= 4, ulps.max()


def test_model_two_objects_never_mix_at_any_ratio():
    """At 4/3 and 1.5 the colours are not exact, but every dst colour is within 4 units in the last place of ITS object's colour."""
    for (Ws, Hs), (Wd, Hd) in OTHER:
        out = xm.transfer(two_objects(Ws, Hs), Wd, Hd)
        want = np.where(out["gid"][..., None] == 1, C1, C0).astype(F)
        ulps = np.abs(out["color"].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 4, ((Ws, Hs), (Wd, Hd), ulps.max())


# ---- 3. CPU: the feature against a reset ---------------------------------------------------------------------------------------------------
def test_model_transfer_beats_a_reset(pkg, orc):
    """Measured 0.436 before the bound was fixed (module docstring): above the 0.35 mark; the unbroken sequence scores 0.518."""
    (Ws, Hs), (Wd, Hd), n, seed = (96, 54), (128, 72), 6, 31
    cam = pkg.synth.camera_for_frame(0, False)
    M = orc.view_matrix(pkg, cam)
    st = tm.empty_state(Ws, Hs)
    sx, sy = scales(pkg, Ws, Hs)
    for f in range(n):
        col, gb, _ = pkg.synth.render_frame(Ws, Hs, f, seed=seed, moving=False, noise_model="hash", cam=cam)
        gb = gb.reshape(Hs, Ws)
        st, _ = tm.temporal_pass(np.asarray(col, F).reshape(Hs, Ws, 3), gb["normal"], gb["position"], gb["geomId"], st,
                                 tm.project_prev(M, Ws, Hs, F(sx), F(sy), gb["position"]))
    col, gb, _ = pkg.synth.render_frame(Wd, Hd, n, seed=seed, moving=False, noise_model="hash", cam=cam)
    clean = pkg.synth.render_frame(Wd, Hd, n, seed=seed, moving=False, noise=0.0, fireflies=0.0, cam=cam)[0].reshape(Hd, Wd, 3).astype(np.float64)
    gb, col = gb.reshape(Hd, Wd), np.asarray(col, F).reshape(Hd, Wd, 3)
    sx, sy = scales(pkg, Wd, Hd)
    co = tm.project_prev(M, Wd, Hd, F(sx), F(sy), gb["position"])
    moved, _ = tm.temporal_pass(col, gb["normal"], gb["position"], gb["geomId"], xm.transfer(st, Wd, Hd), co)
    fresh, _ = tm.temporal_pass(col, gb["normal"], gb["position"], gb["geomId"], tm.empty_state(Wd, Hd), co)
    hit = gb["geomId"] != -1
    e_moved, e_fresh = np.abs(moved["color"] - clean)[hit].mean(), np.abs(fresh["color"] - clean)[hit].mean()
    share, share_fresh = (moved["hlen"][hit] >= 2).mean(), (fresh["hlen"][hit] >= 2).mean()
    print(f"mean absolute error against the clean frame: transfer {e_moved:.5f}, reset {e_fresh:.5f}, ratio {e_moved / e_fresh:.3f}; "
          f"history length >= 2 on {100 * share:.1f} % of the non-miss pixels with the transfer, {100 * share_fresh:.1f} % after a reset")
    assert share >= 0.5 and share_fresh == 0
    assert e_moved / e_fresh <= 2 * MEASURED_RATIO


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------
def read_history(den):
    return {name: den.read_state(k) for name, k in HIST.items()}


def assert_state(got, want, what):
    for k in PLANES:
        assert same_bits(got[k], want[k]), f"{what}: {k}"


def one_frame(pkg, den, col, gb, cam, params, leg="aos", plane=None, fmt=th.COORD):
    """One frame through the context (capture on): (output, the five states of temporal_harness.STATES)."""
    import torch
    H, W = gb.shape
    den.set_capture(True)
    t_c = torch.from_numpy(np.ascontiguousarray(col, dtype=F)).cuda()
    t_g = torch.from_numpy(np.ascontiguousarray(gb).view(np.uint8).reshape(-1).copy()).cuda()
    mv = None if plane is None else torch.from_numpy(np.ascontiguousarray(plane)).cuda()
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if leg == "planar":
        g = den.planar_gbuffer()
        hip = th._hip()
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        flat = np.ascontiguousarray(gb).reshape(-1)
        for dst, arr in ((g.normal, flat["normal"]), (g.position, flat["position"]), (g.geom_id, flat["geomId"]),
                         (g.albedo, (flat["albedo"] * flat["ialbedo"]).astype(F))):
            arr = np.ascontiguousarray(arr)
            assert hip.hipMemcpy(dst, arr.ctypes.data, arr.nbytes, 1) == 0
        den.denoise_planar(out, t_c, cam, params, motion=mv, motion_format=fmt)
    else:
        den.denoise(out, t_c, t_g, cam, params, motion=mv, motion_format=fmt)
    den.sync()
    return out.cpu().numpy(), th.read_states(den)


def run_frames(pkg, orc, den, W, H, frames, leg="aos", finite=False, **kw):
    """Frames `frames` of mixed_sequence at the context's size, temporal pass only (or **kw).  Returns the last (output, states)."""
    seq = th.mixed_sequence(pkg, orc, W, H, n=7 if max(frames) >= 4 else 4, finite=finite)
    p = th.synth_params(pkg, W, H, **kw)
    last = None
    for f in frames:
        col, gb, cam, _ = seq[f]
        last = one_frame(pkg, den, col, gb, cam, p, leg)
    return last


def model_next(pkg, orc, prev_state, Wd, Hd, f, fmt=None, radius=0, k=0.0, rank=0, scale=1.0):
    """The model's frame f of mixed_sequence at Wd x Hd on `prev_state`, the previous view being frame f - 1's: (state, variance, the
    PREV_COORD plane, the host motion plane or None)."""
    seq = th.mixed_sequence(pkg, orc, Wd, Hd, n=7 if f >= 4 else 4)
    col, gb, _, _ = seq[f]
    sx, sy = scales(pkg, Wd, Hd)
    plane = tm.motion_plane(seq[f - 1][3], Wd, Hd, gb, None, fmt or th.COORD, F(sx), F(sy))
    coord = tm.coord_plane(plane, fmt or th.COORD, Wd, Hd)
    st, var = tm.temporal_pass(ff.firefly_filter(col, rank, scale), gb["normal"], gb["position"], gb["geomId"], prev_state, coord,
                               radius=radius, k=k)
    return st, var, coord, (plane if fmt is not None else None)


def assert_next_frame(pkg, orc, dst, prev_state, Wd, Hd, f, leg, what, fmt=None, **model_kw):
    """Frame f on `dst` equals the model's frame on `prev_state`: history length, moments, colour, variance."""
    st, var, _, plane = model_next(pkg, orc, prev_state, Wd, Hd, f, fmt, **model_kw)
    col, gb, cam, _ = th.mixed_sequence(pkg, orc, Wd, Hd, n=7 if f >= 4 else 4)[f]
    _, got = one_frame(pkg, dst, col, gb, cam, th.synth_params(pkg, Wd, Hd), leg, plane, fmt or th.COORD)
    want = dict(hlen=st["hlen"], mom=st["mom"], color=st["color"], variance=var, acc=st["color"])
    for name in th.STATES:
        assert same_bits(got[name], want[name]), f"{what}: the next frame's {name}"
    return st


# 1x1 and 3x2 are all edge; 7x5 -> 7x5 is the copy; the last four cross 64-column / 4-row tile seams at ratios 3, 1/2, ~4/3, ~2/3
PAIRS = [((1, 1), (1, 1)), ((1, 1), (3, 2)), ((7, 5), (7, 5)), ((64, 4), (96, 6)), ((100, 3), (300, 9)), ((130, 9), (65, 5)),
         ((97, 13), (129, 17)), ((193, 11), (130, 7))]


# ---- 4. GPU: the planes equal the model, and so does the frame behind them ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["aos", "planar"])
@pytest.mark.parametrize("src,dst", PAIRS, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in PAIRS])
def test_hip_equals_the_model_on_every_pixel(pkg, orc, src, dst, leg):
    """Three frames with non-finite colours' positions, two objects and misses on src; the transfer; every plane of dst is the model on
    the same reads of src; then one frame on dst through the camera path (the previous view moved too) and, on a second dst, through a
    half-precision motion plane."""
    (Ws, Hs), (Wd, Hd) = src, dst
    s = pkg.Denoiser(Ws, Hs)
    ds = [pkg.Denoiser(Wd, Hd), pkg.Denoiser(Wd, Hd)]
    try:
        run_frames(pkg, orc, s, Ws, Hs, (0, 1, 2), leg)
        have = read_history(s)
        want = xm.transfer(have, Wd, Hd)
        for d, fmt in zip(ds, (None, th.D16)):
            d.transfer_history_from(s)
            assert_state(read_history(d), want, f"{src} -> {dst} {leg}")
            assert_next_frame(pkg, orc, d, want, Wd, Hd, 3, leg, f"{src} -> {dst} {leg} motion {fmt}", fmt)
        assert_state(read_history(s), have, "src is only read")
    finally:
        for d in [s] + ds:
            d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["src", "dst", "both"])
@pytest.mark.parametrize("src,dst", [((97, 13), (129, 17)), ((7, 5), (7, 5))], ids=["97x13-129x17", "7x5-7x5"])
def test_pipelined_contexts(pkg, orc, src, dst, which):
    """Contexts with pipeline resources alternate two plane sets: the planes written are the ones dst's next frame reads, whichever set
    they lie in (dst has run one frame or two before the transfer: both parities)."""
    (Ws, Hs), (Wd, Hd) = src, dst
    for before in ((0,), (0, 1)):
        s = pkg.Denoiser(Ws, Hs, pipelined=which in ("src", "both"))
        d = pkg.Denoiser(Wd, Hd, pipelined=which in ("dst", "both"))
        try:
            run_frames(pkg, orc, s, Ws, Hs, (0, 1, 2))
            run_frames(pkg, orc, d, Wd, Hd, before)
            want = xm.transfer(read_history(s), Wd, Hd)
            piped = d.is_pipelined()
            d.transfer_history_from(s)
            assert d.is_pipelined() == piped
            assert_state(read_history(d), want, f"{which} pipelined, {len(before)} frames before")
            st = assert_next_frame(pkg, orc, d, want, Wd, Hd, 3, "aos", f"{which} pipelined, {len(before)} frames before")
            assert_next_frame(pkg, orc, d, st, Wd, Hd, 4, "aos", f"{which} pipelined, {len(before)} frames before, second frame")
        finally:
            s.free(); d.free()


@pytest.mark.gpu
def test_configuration_of_dst_stays(pkg, orc):
    """History clamp and firefly filter set on dst before the transfer are in force after it."""
    (Ws, Hs), (Wd, Hd) = (97, 13), (129, 17)
    s, d = pkg.Denoiser(Ws, Hs), pkg.Denoiser(Wd, Hd)
    try:
        d.set_history_clamp(2, 1.0)
        d.set_firefly_filter(1, 1.0)
        run_frames(pkg, orc, s, Ws, Hs, (0, 1, 2))
        want = xm.transfer(read_history(s), Wd, Hd)
        d.transfer_history_from(s)
        assert d.history_clamp() == (2, 1.0) and d.firefly_filter() == (1, 1.0)
        assert s.history_clamp() == (0, 0.0) and s.firefly_filter() == (0, 0.0)
        assert_next_frame(pkg, orc, d, want, Wd, Hd, 3, "aos", "clamp + firefly", radius=2, k=1.0, rank=1, scale=1.0)
    finally:
        s.free(); d.free()


# ---- 5. GPU: the output history ---------------------------------------------------------------------------------------------------------
def split_output_history(a):
    return np.ascontiguousarray(a[..., :3]), np.ascontiguousarray(a[..., 3]).view(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", [((97, 13), (129, 17)), ((130, 9), (65, 5)), ((7, 5), (7, 5))], ids=["97x13-129x17", "130x9-65x5", "7x5-7x5"])
def test_output_history_moves_when_both_contexts_have_one(pkg, orc, src, dst):
    (Ws, Hs), (Wd, Hd) = src, dst
    alpha, k = 0.25, 1.5
    s, d = pkg.Denoiser(Ws, Hs), pkg.Denoiser(Wd, Hd)
    try:
        s.set_output_taa(0.2, 1.0)
        d.set_output_taa(alpha, k)
        run_frames(pkg, orc, s, Ws, Hs, (0, 1, 2))
        with pytest.raises(pkg.SvgfError, match=r"-1"):
            d.read_state(pkg.STATE_OUTPUT_HISTORY)
        want = xm.transfer(read_history(s), Wd, Hd)
        want_hist = xm.transfer_output_history(split_output_history(s.read_state(pkg.STATE_OUTPUT_HISTORY)), Wd, Hd)
        d.transfer_history_from(s)
        assert d.output_taa() == (alpha, k)
        rgb, gid = split_output_history(d.read_state(pkg.STATE_OUTPUT_HISTORY))
        assert same_bits(rgb, want_hist[0]) and np.array_equal(gid, want_hist[1])
        st, _, coord, _ = model_next(pkg, orc, want, Wd, Hd, 3)
        col, gb, cam, _ = th.mixed_sequence(pkg, orc, Wd, Hd)[3]
        out, got = one_frame(pkg, d, col, gb, cam, th.synth_params(pkg, Wd, Hd))
        assert same_bits(got["color"], st["color"])
        o, _ = taa.output_taa(st["color"], gb["geomId"], coord, want_hist, alpha, k)      # (spatial filter off: C is the accumulated colour)
        assert same_bits(out, o)
        if Wd >= 65:
            assert taa.has_history(st["color"], gb["geomId"], coord, want_hist, alpha, k).any(), "the transferred output history is used"
    finally:
        s.free(); d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("on", ["src", "dst"])
def test_no_output_history_unless_both_contexts_have_one(pkg, orc, on):
    (Ws, Hs), (Wd, Hd) = (97, 13), (129, 17)
    s, d = pkg.Denoiser(Ws, Hs), pkg.Denoiser(Wd, Hd)
    try:
        (s if on == "src" else d).set_output_taa(0.2, 1.0)
        run_frames(pkg, orc, s, Ws, Hs, (0, 1, 2))
        if on == "dst":
            run_frames(pkg, orc, d, Wd, Hd, (0, 1))      # dst holds an output history of its own: gone, as after svgf_reset
            d.read_state(pkg.STATE_OUTPUT_HISTORY)
        want = xm.transfer(read_history(s), Wd, Hd)
        d.transfer_history_from(s)
        with pytest.raises(pkg.SvgfError, match=r"-1"):
            d.read_state(pkg.STATE_OUTPUT_HISTORY)
        st, _, _, _ = model_next(pkg, orc, want, Wd, Hd, 3)
        col, gb, cam, _ = th.mixed_sequence(pkg, orc, Wd, Hd)[3]
        out, _ = one_frame(pkg, d, col, gb, cam, th.synth_params(pkg, Wd, Hd))
        assert same_bits(out, st["color"]), "a frame without an output history writes its image as it is"
    finally:
        s.free(); d.free()


# ---- 6. GPU: lifecycle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lifecycle(pkg, orc):
    (Ws, Hs), (Wd, Hd) = (97, 13), (129, 17)
    s, twin = pkg.Denoiser(Ws, Hs), pkg.Denoiser(Ws, Hs)
    fresh, used, again, cleared, never = (pkg.Denoiser(Wd, Hd) for _ in range(5))
    try:
        for c in (s, twin):
            run_frames(pkg, orc, c, Ws, Hs, (0, 1, 2))
        run_frames(pkg, orc, used, Wd, Hd, (2, 0))      # two unrelated frames first
        fresh.transfer_history_from(s)
        used.transfer_history_from(s)
        again.transfer_history_from(s)
        again.transfer_history_from(s)
        cleared.transfer_history_from(s)
        cleared.reset()
        want = read_history(fresh)
        assert_state(want, xm.transfer(read_history(s), Wd, Hd), "a fresh dst")
        assert_state(read_history(used), want, "a dst that ran two frames first")
        assert_state(read_history(again), want, "transfer twice")
        assert_state(read_history(cleared), read_history(never), "transfer, then svgf_reset")
        nxt = [run_frames(pkg, orc, c, Wd, Hd, (3,))[1] for c in (fresh, used, again)]
        for name in th.STATES:
            assert same_bits(nxt[1][name], nxt[0][name]) and same_bits(nxt[2][name], nxt[0][name]), name
        rst = [run_frames(pkg, orc, c, Wd, Hd, (3,))[1] for c in (cleared, never)]
        for name in th.STATES:
            assert same_bits(rst[0][name], rst[1][name]), name
        assert not same_bits(rst[0]["color"], nxt[0]["color"]), "the transferred history acts on this frame"
        a, b = run_frames(pkg, orc, s, Ws, Hs, (3,)), run_frames(pkg, orc, twin, Ws, Hs, (3,))
        assert same_bits(a[0], b[0])
        for name in th.STATES:
            assert same_bits(a[1][name], b[1][name]), f"src's next frame: {name}"
    finally:
        for c in (s, twin, fresh, used, again, cleared, never):
            c.free()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("piped", [False, True], ids=["ordered", "pipelined dst"])
def test_equal_size_transfer_clones_a_sequence(pkg, orc, variant, piped):
    """Three frames on src and its twin, the transfer, then four whole frames (the cascade on) on dst and on the twin: the same bits,
    outputs and states.  Finite texels: temporal_harness.mixed_sequence says why whole frames are compared on those only."""
    W, H = 130, 9
    kw = dict(spatial_enable=1, atrous_nlevel=5, history_level=1, kernel_variant=variant)
    s, twin, d = pkg.Denoiser(W, H), pkg.Denoiser(W, H), pkg.Denoiser(W, H, pipelined=piped)
    try:
        for c in (s, twin):
            run_frames(pkg, orc, c, W, H, (0, 1, 2), finite=True, **kw)
        d.transfer_history_from(s)
        for f in (3, 4, 5, 6):
            a, b = run_frames(pkg, orc, d, W, H, (f,), finite=True, **kw), run_frames(pkg, orc, twin, W, H, (f,), finite=True, **kw)
            assert same_bits(a[0], b[0]), f"frame {f}: output"
            for name in th.STATES:
                assert same_bits(a[1][name], b[1][name]), f"frame {f}: {name}"
    finally:
        s.free(); twin.free(); d.free()


# ---- 7. GPU: errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors(pkg, orc):
    import torch
    W, H = 7, 5
    s, d = pkg.Denoiser(W, H), pkg.Denoiser(W, H)
    lib = pkg.load_library()
    try:
        assert lib.svgf_transfer_history(d.h, d.h, None) == INVALID
        with pytest.raises(pkg.SvgfError, match=r"-1"):
            d.transfer_history_from(d)
        run_frames(pkg, orc, s, W, H, (0, 1))
        hip = th._hip()
        st = torch.cuda.Stream()
        graph = ctypes.c_void_p()
        hip.hipStreamBeginCapture.argtypes = [ctypes.c_void_p, ctypes.c_int]
        hip.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        hip.hipGraphDestroy.argtypes = [ctypes.c_void_p]
        torch.cuda.synchronize()
        before = read_history(d)
        assert hip.hipStreamBeginCapture(st.cuda_stream, 2) == 0           # hipStreamCaptureModeRelaxed
        rc = lib.svgf_transfer_history(d.h, s.h, st.cuda_stream)
        assert hip.hipStreamEndCapture(st.cuda_stream, ctypes.byref(graph)) == 0, "the capture ends cleanly"
        if graph.value:
            hip.hipGraphDestroy(graph)
        assert rc == UNSUPPORTED
        assert_state(read_history(d), before, "a refused call changes nothing")
        d.transfer_history_from(s, stream=st)      # and the same stream takes the call once the capture is over
        d.sync_stream(st)
        assert_state(read_history(d), read_history(s), "after the capture")
    finally:
        s.free(); d.free()
