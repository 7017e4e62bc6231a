"""Guided upsampling (include/svgf.h: svgf_upsample): the full-size image from a reduced-size denoise and the
full-size G-buffer.

The yardstick is tests/upsample_model.py.  Every comparison of the kernel with the model is on the bits of every pixel (NaNs in the
same place count as equal): both sides perform the same correctly rounded float32 operations in the same order without contraction,
so there is no tolerance to choose.  The statements about the model itself (identity, flat colours) are exact too.

Two bounds are not equalities.  "Earns its place": the mean absolute error of the upsampled image against the clean full-size
frame is at most 0.5 x that of a plain bilinear stretch of the small COLOUR image (the test prints the ratios; the arithmetic
restated in a scratch script gave 0.23, 0.19, 0.15 and 0.26 before the test existed, so the bound keeps a margin of 2).  The pass
shares of the GPU inputs (each of A, B, C taken by >= 3 % of the pixels of the three largest shapes) are a cap that keeps the
inputs honest, not a measurement."""
import ctypes

import numpy as np
import pytest

import upsample_model as um
from temporal_harness import same_bits, scales

F = np.float32
C0, C1 = np.array([0.5, 0.25, 1.0], F), np.array([2.0, 1.0, 0.25], F)      # the TAA tests' dyadic colours: every product and sum is exact
SIGMAS = ((0.0, 0.0), (0.5, 0.5), (0.05, 0.0))
INVALID, UNSUPPORTED = -1, -5


# ---- 1. CPU: symbol, binding, argument checking (fails without the feature) ----------------------------------------------------------------
def test_symbol_is_exported_and_the_binding_exists(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "svgf_upsample")
    assert "svgf_upsample" in pkg.binding.EXPORTS
    b = pkg.binding
    assert callable(b.upsample) and pkg.upsample is b.upsample
    assert pkg.SvgfGuide is b.SvgfGuide and pkg.SvgfUpsampleParams is b.SvgfUpsampleParams
    assert ctypes.sizeof(b.SvgfGuide) == 5 * ctypes.sizeof(ctypes.c_void_p) and ctypes.sizeof(b.SvgfUpsampleParams) == 12
    assert [n for n, _ in b.SvgfGuide._fields_] == ["gbuffer", "normal", "position", "geom_id", "albedo"]
    assert [n for n, _ in b.SvgfUpsampleParams._fields_] == ["sigma_n", "sigma_x", "modulate"]


def test_invalid_arguments_are_answered_before_any_device_work(pkg):
    """Device 0 and dummy non-NULL pointers: every case below returns its code before the first HIP call, with or without a GPU.
    (The valid call itself is not made here: it would launch on the dummy pointers.)"""
    b = pkg.binding
    lib = pkg.load_library()
    P = 0x1000      # never dereferenced
    aos = lambda: b.SvgfGuide(P, None, None, None, None)
    planes = lambda albedo=None: b.SvgfGuide(None, P, P, P, albedo)
    par = lambda sn=0.5, sx=0.5, m=1: b.SvgfUpsampleParams(sn, sx, m)

    def call(out=P, hi="aos", whi=8, hhi=6, rgb=P, lo="aos", wlo=4, hlo=3, up="par"):
        hi = aos() if hi == "aos" else hi
        lo = aos() if lo == "aos" else lo
        up = par() if up == "par" else up
        ref = lambda s: None if s is None else ctypes.byref(s)
        return lib.svgf_upsample(0, out, ref(hi), whi, hhi, rgb, ref(lo), wlo, hlo, ref(up), None)

    # NULL arguments
    assert call(out=None) == INVALID and call(rgb=None) == INVALID
    assert call(hi=None) == INVALID and call(lo=None) == INVALID and call(up=None) == INVALID
    # a guide with neither the texels nor all three planes
    for missing in range(3):
        ptrs = [P, P, P]
        ptrs[missing] = None
        g = b.SvgfGuide(None, ptrs[0], ptrs[1], ptrs[2], P)
        assert call(hi=g) == INVALID and call(lo=g) == INVALID, missing
    assert call(hi=b.SvgfGuide(None, None, None, None, None)) == INVALID
    # modulate with a planar hi guide without albedo; modulate that is not 0 or 1
    assert call(hi=planes(None), up=par(m=1)) == INVALID
    for m in (2, -1, 7):
        assert call(up=par(m=m)) == INVALID, m
    # sizes
    for kw in (dict(whi=0), dict(hhi=0), dict(wlo=0), dict(hlo=0), dict(whi=-8), dict(hlo=-3), dict(wlo=9), dict(hlo=7), dict(wlo=9, hlo=7)):
        assert call(**kw) == INVALID, kw
    # sigmas
    nan, inf = float("nan"), float("inf")
    for bad in (-0.5, nan, inf, -inf):
        assert call(up=par(sn=bad)) == INVALID and call(up=par(sx=bad)) == INVALID, bad
    # too many pixels: width_hi * height_hi >= 2^31 / 16
    assert call(whi=16384, hhi=8192) == UNSUPPORTED
    assert call(whi=1 << 27, hhi=1, hlo=1) == UNSUPPORTED
    assert call(whi=16384, hhi=8192, hi=planes(P), lo=planes()) == UNSUPPORTED
    # and the binding raises
    with pytest.raises(pkg.SvgfError, match=r"\(-1\)"):
        b.upsample(P, b.guide(gbuffer=P), 8, 6, P, b.guide(gbuffer=P), 9, 3, 0.5, 0.5, 1)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def make_hi(pkg, W, H, seed):
    """geomId in 8 x 3 patches drawn from 0..3, 5 % speckle of id 40 and 5 % of -1; per-patch unit normals with small jitter, a
    quarter of the pixels with a large one; small random positions; albedo and ialbedo away from 0 and 1."""
    rng = np.random.default_rng(seed)
    pw, ph = -(-W // 8), -(-H // 3)
    grow = lambda a: np.repeat(np.repeat(a, 3, axis=0), 8, axis=1)[:H, :W]
    gb = np.zeros((H, W), pkg.synth.GBUFFER_DTYPE)
    gid = grow(rng.integers(0, 4, (ph, pw))).astype(np.int32)
    r = rng.random((H, W))
    gid[r < 0.05] = 40
    gid[(r >= 0.05) & (r < 0.10)] = -1
    pn = rng.normal(size=(ph, pw, 3))
    pn /= np.linalg.norm(pn, axis=-1, keepdims=True)
    n = grow(pn) + 0.02 * rng.normal(size=(H, W, 3))
    n += np.where((rng.random((H, W)) < 0.25)[..., None], rng.normal(size=(H, W, 3)), 0.0)
    gb["geomId"], gb["normal"] = gid, n.astype(F)
    gb["position"] = rng.uniform(-0.05, 0.05, (H, W, 3)).astype(F)
    gb["albedo"] = rng.uniform(0.2, 1.0, (H, W, 3)).astype(F)
    gb["ialbedo"] = rng.uniform(0.5, 1.5, (H, W, 3)).astype(F)
    return gb


def make_case(pkg, Wh, Hh, Wl, Hl, seed=5, nonfinite=False):
    cache = make_case.__dict__.setdefault("cache", {})
    key = (Wh, Hh, Wl, Hl, seed, nonfinite)
    if key not in cache:
        rng = np.random.default_rng(seed + 1000)
        hi = make_hi(pkg, Wh, Hh, seed)
        if nonfinite:
            for field in ("normal", "position"):
                for val in (np.nan, np.inf, -np.inf):
                    k = rng.integers(0, hi.size, max(2, hi.size // 40))
                    hi[field].reshape(-1, 3)[k, rng.integers(0, 3, k.size)] = val
        lo = um.nearest_lo(hi, Wl, Hl)
        rgb = rng.uniform(0.05, 2.0, (Hl, Wl, 3)).astype(F)
        if nonfinite:
            for field in ("normal", "position"):
                for val in (np.nan, np.inf, -np.inf):
                    k = rng.integers(0, lo.size, 3)
                    lo[field].reshape(-1, 3)[k, rng.integers(0, 3, k.size)] = val
            for val in (np.nan, np.inf, -np.inf):
                k = rng.integers(0, lo.size, 6)
                rgb.reshape(-1, 3)[k, rng.integers(0, 3, k.size)] = val
        cache[key] = (hi, lo, rgb)
    return cache[key]


# ---- 2. CPU: what the model states, exactly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(64, 4), (67, 9)])
@pytest.mark.parametrize("sn,sx", SIGMAS)
def test_model_identity(pkg, W, H, sn, sx):
    hi, _, _ = make_case(pkg, W, H, W, H)
    rgb = np.random.default_rng(3).uniform(0.05, 2.0, (H, W, 3)).astype(F)
    out, took = um.upsample(rgb, hi, hi, sn, sx, 0)
    assert same_bits(out, rgb), "the same size and the same G-buffer: rgb_lo comes back bit for bit"
    assert (took == um.PASS_A).all()


def _flat_case(pkg):
    Wl, Hl, Wh, Hh = 20, 12, 40, 24
    hi = np.zeros((Hh, Wh), pkg.synth.GBUFFER_DTYPE)
    edge = 18 + 2 * ((np.arange(Hh) // 2) % 3)                         # a stepped edge on even coordinates: 18, 20, 22 ...
    hi["geomId"] = (np.arange(Wh)[None, :] >= edge[:, None]).astype(np.int32)
    hi["normal"] = (0.0, 1.0, 0.0)
    xs, zs = np.meshgrid(np.arange(Wh, dtype=F), np.arange(Hh, dtype=F))
    hi["position"][..., 0], hi["position"][..., 2] = xs * F(0.25), zs * F(0.25)      # in the plane: the distance term is exactly 1
    hi["albedo"] = hi["ialbedo"] = 1.0
    lo = np.ascontiguousarray(hi[::2, ::2])
    rgb = np.where((lo["geomId"] == 0)[..., None], C0, C1).astype(F)
    return hi, lo, rgb


@pytest.mark.parametrize("sn,sx", SIGMAS)
def test_model_flat_colours_do_not_cross_an_object_edge(pkg, sn, sx):
    hi, lo, rgb = _flat_case(pkg)
    out, took = um.upsample(rgb, lo, hi, sn, sx, 0)
    want = np.where((hi["geomId"] == 0)[..., None], C0, C1).astype(F)
    assert same_bits(out, want), "every hi pixel has exactly its own object's colour"
    assert (took == um.PASS_A).all()
    plain = um.bilinear(rgb, lo.shape, hi.shape)
    assert not same_bits(plain, want), "the plain stretch does cross the edge"


def test_model_non_finite_and_missing_taps_take_the_fallbacks(pkg):
    hi, lo, rgb = _flat_case(pkg)
    hi, lo = hi.copy(), lo.copy()
    hi["normal"][5, 7] = (np.nan, 1.0, 0.0)          # every guided weight is 0: pass B
    hi["position"][6, 9] = (0.0, np.inf, 0.0)        # the plane distance is inf: pass B
    hi["geomId"][9, 30] = 17                         # no lo tap of this object: pass C
    hi["geomId"][11, 3] = -1                         # a miss between hits: pass C
    out, took = um.upsample(rgb, lo, hi, 0.5, 0.5, 0)
    assert took[5, 7] == um.PASS_B and took[6, 9] == um.PASS_B
    assert took[9, 30] == um.PASS_C and took[11, 3] == um.PASS_C
    want = took.copy()
    want[5, 7] = want[6, 9] = want[9, 30] = want[11, 3] = um.PASS_A
    assert (want == um.PASS_A).all(), "and nothing else moved"
    assert same_bits(out[5, 7], C0) and same_bits(out[6, 9], C0), "pass B: the same object's colour, unguided"
    assert same_bits(out[9, 30], um.bilinear(rgb, lo.shape, hi.shape)[9, 30]), "pass C: the plain stretch"
    assert np.isfinite(out).all()
    # with the terms off nothing is guided: a NaN normal is not looked at
    out0, took0 = um.upsample(rgb, lo, hi, 0.0, 0.0, 0)
    assert took0[5, 7] == um.PASS_A and took0[6, 9] == um.PASS_A and took0[9, 30] == um.PASS_C
    # pass C always accepts with lo <= hi
    for (Wh, Hh, Wl, Hl) in [(67, 5, 1, 1), (300, 9, 100, 3), (193, 7, 129, 5), (7, 5, 3, 2)]:
        h, l, c = make_case(pkg, Wh, Hh, Wl, Hl)
        assert (um.upsample(c, l, h, 0.5, 0.5, 1)[1] != um.PASS_NONE).all()


# ---- 3. CPU: the feature earns its place ---------------------------------------------------------------------------------------------------
def test_model_halves_the_error_of_a_plain_stretch(pkg):
    Wh, Hh = 192, 108
    ratios = []
    for (Wl, Hl, moving, frame) in [(96, 54, False, 0), (96, 54, True, 3), (128, 72, True, 3), (64, 36, True, 3)]:
        cam = pkg.synth.camera_for_frame(frame, moving)
        clean, hi, _ = pkg.synth.render_frame(Wh, Hh, frame, moving=moving, noise=0.0, fireflies=0.0, cam=cam)
        small, lo, _ = pkg.synth.render_frame(Wl, Hl, frame, moving=moving, noise=0.0, fireflies=0.0, cam=cam)
        hit_lo = (lo["geomId"] != -1)[..., None]
        with np.errstate(all="ignore"):
            ill = np.where(hit_lo, small.reshape(Hl, Wl, 3) / lo["albedo"], F(0)).astype(F)
        got, _ = um.upsample(ill, lo, hi, 0.5, 0.5, 1)
        plain = um.bilinear(small.reshape(Hl, Wl, 3), lo.shape, hi.shape)
        hit = hi["geomId"] != -1
        clean = clean.reshape(Hh, Wh, 3).astype(np.float64)
        e_up, e_plain = np.abs(got - clean)[hit].mean(), np.abs(plain - clean)[hit].mean()
        ratios.append(e_up / e_plain)
        print(f"{Wl}x{Hl} -> {Wh}x{Hh} {'moving' if moving else 'static'}: guided {e_up:.5f}, plain {e_plain:.5f}, ratio {ratios[-1]:.3f}")
    print("ratios:", " ".join(f"{r:.3f}" for r in ratios))
    assert all(r <= 0.5 for r in ratios), ratios


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guides(pkg, gb):
    """{"aos": (guide, keep-alive), "planar": ...} of one G-buffer on the device"""
    b = pkg.binding
    texels = _dev(np.ascontiguousarray(gb).view(np.uint8).reshape(-1).copy())
    planes = [_dev(gb["normal"]), _dev(gb["position"]), _dev(gb["geomId"]), _dev((gb["albedo"] * gb["ialbedo"]).astype(F))]
    return {"aos": (b.guide(gbuffer=texels), texels),
            "planar": (b.guide(normal=planes[0], position=planes[1], geom_id=planes[2], albedo=planes[3]), planes)}


def _run_every_layout(pkg, hi, lo, rgb, what):
    """Every layout x modulate x sigma pair against the model; returns the pass map of (0.5, 0.5)."""
    import torch
    (Hh, Wh), (Hl, Wl) = hi.shape, lo.shape
    g_hi, g_lo, t_rgb = _guides(pkg, hi), _guides(pkg, lo), _dev(rgb)
    took = None
    for sn, sx in SIGMAS:
        ref = {m: um.upsample(rgb, lo, hi, sn, sx, m) for m in (0, 1)}
        if (sn, sx) == (0.5, 0.5):
            took = ref[0][1]
        for lh in ("aos", "planar"):
            for ll in ("aos", "planar"):
                for m in (0, 1):
                    out = torch.full((Hh, Wh, 3), -7.0, dtype=torch.float32, device="cuda")
                    pkg.binding.upsample(out, g_hi[lh][0], Wh, Hh, t_rgb, g_lo[ll][0], Wl, Hl, sn, sx, m)
                    torch.cuda.synchronize()
                    got = out.cpu().numpy()
                    assert same_bits(got, ref[m][0]), (f"{what}: hi {lh}, lo {ll}, modulate {m}, sigma ({sn}, {sx}): "
                                                      f"{np.count_nonzero(~np.isclose(got, ref[m][0], rtol=0, atol=0, equal_nan=True))} values differ")
    return took


# 1x1 and 67x5 <- 1x1: a footprint of one texel; 64x4 <- 64x4: ratio 1, exactly one tile; 130x9 <- 65x5, 193x7 <- 129x5 and
# 300x9 <- 100x3: tile seams in x and y, ratios 2, 1.5 (1.4 in y), 3, neither size a multiple of the tile
SHAPES = [(1, 1, 1, 1), (67, 5, 1, 1), (64, 4, 64, 4), (130, 9, 65, 5), (193, 7, 129, 5), (300, 9, 100, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("Wh,Hh,Wl,Hl", SHAPES, ids=[f"{a}x{b}<-{c}x{d}" for a, b, c, d in SHAPES])
def test_hip_equals_the_model_on_every_pixel(pkg, Wh, Hh, Wl, Hl):
    hi, lo, rgb = make_case(pkg, Wh, Hh, Wl, Hl)
    took = _run_every_layout(pkg, hi, lo, rgb, f"{Wh}x{Hh} <- {Wl}x{Hl}")
    share = [float((took == k).mean()) for k in (um.PASS_A, um.PASS_B, um.PASS_C)]
    print(f"{Wh}x{Hh} <- {Wl}x{Hl}: pass A {share[0]:.3f}, B {share[1]:.3f}, C {share[2]:.3f}")
    if Wh >= 130:
        assert min(share) >= 0.03, f"each pass is taken by at least 3 % of the pixels: {share}"


@pytest.mark.gpu
def test_hip_equals_the_model_on_non_finite_inputs(pkg):
    hi, lo, rgb = make_case(pkg, 130, 9, 65, 5, nonfinite=True)
    assert not np.isfinite(hi["normal"]).all() and not np.isfinite(lo["position"]).all() and not np.isfinite(rgb).all()
    _run_every_layout(pkg, hi, lo, rgb, "non-finite 130x9 <- 65x5")


@pytest.mark.gpu
def test_denoise_small_then_upsample(pkg):
    """The device producer at both sizes, four frames through a context at the small size (illumination out), then the upsample:
    bit for bit the model fed the context's own output, and closer to the clean full-size frame than the bilinear stretch of the
    small result (the small illumination times the small albedo, what the context would have written with addcolor = 1)."""
    import torch
    Wl, Hl, Wh, Hh, n = 96, 54, 192, 108, 4
    d = pkg.Denoiser(Wl, Hl)
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, sepcolor=1, addcolor=0)
    p.reproj_scale[0], p.reproj_scale[1] = scales(pkg, Wl, Hl)
    rgb_lo = torch.empty((Hl, Wl, 3), dtype=torch.float32, device="cuda")
    rgb_hi = torch.empty((Hh, Wh, 3), dtype=torch.float32, device="cuda")
    gb_lo = torch.empty((Hl * Wl * 52,), dtype=torch.uint8, device="cuda")
    gb_hi = torch.empty((Hh * Wh * 52,), dtype=torch.uint8, device="cuda")
    ill = torch.empty((Hl, Wl, 3), dtype=torch.float32, device="cuda")
    out = torch.full((Hh, Wh, 3), -7.0, dtype=torch.float32, device="cuda")
    try:
        for f in range(n):
            cam = pkg.synth.camera_for_frame(f, True)
            pkg.binding.synth_render(rgb_lo, gb_lo, Wl, Hl, cam, f, seed=19)
            pkg.binding.synth_render(rgb_hi, gb_hi, Wh, Hh, cam, f, seed=19)
            d.denoise(ill, rgb_lo, gb_lo, cam, p)
            pkg.binding.upsample(out, gb_hi, Wh, Hh, ill, gb_lo, Wl, Hl, 0.5, 0.5, 1)
        d.sync()
        torch.cuda.synchronize()
    finally:
        d.free()
    dt = pkg.synth.GBUFFER_DTYPE
    lo = gb_lo.cpu().numpy().view(dt).reshape(Hl, Wl)
    hi = gb_hi.cpu().numpy().view(dt).reshape(Hh, Wh)
    ill_h, got = ill.cpu().numpy(), out.cpu().numpy()
    ref, _ = um.upsample(ill_h, lo, hi, 0.5, 0.5, 1)
    assert same_bits(got, ref)
    clean = pkg.synth.render_frame(Wh, Hh, n - 1, moving=True, noise=0.0, fireflies=0.0, cam=cam)[0].reshape(Hh, Wh, 3).astype(np.float64)
    plain = um.bilinear((ill_h * (lo["albedo"] * lo["ialbedo"]).astype(F)).astype(F), lo.shape, hi.shape)
    hit = hi["geomId"] != -1
    e_up, e_plain = np.abs(got - clean)[hit].mean(), np.abs(plain - clean)[hit].mean()
    print(f"mean absolute error against the clean frame: guided {e_up:.5f}, bilinear stretch of the small result {e_plain:.5f}")
    assert np.isfinite(got).all() and e_up < e_plain
