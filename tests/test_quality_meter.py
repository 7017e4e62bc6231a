"""Image-quality meter (include/svgf.h row f13): svgf_quality_state_bytes, svgf_quality_windows, svgf_quality_meter,
svgf_quality_read.

The yardstick is tests/quality_model.py.  Every comparison of the kernels with the model is on the bits of both maps, the two counts,
max_abs, min_ssim, peak and the effective scale; the two sums are held to the header's derived bound against the model's exact
(math.fsum) totals: |sum - exact| <= n 2^-52 sum |term|, n the number of terms.  The state is filled with 0xFF bytes before every call
(it needs no initialisation) and both maps with a sentinel.

Launch geometry of k_quality_tile (svgf_quality.hip): one workgroup per tile of Q_TILE_W x Q_TILE_H = 64 x 32 pixels = 16 x 8 cells,
plus one cell column / row of halo read from the neighbouring tiles; the grid is one workgroup per tile (not grid-stride).  A lane takes
one cell row (four pixels) with three 16-byte loads per image when both images are 16-byte aligned AND the width is a multiple of 4,
with dword loads otherwise; the error map is stored 16 bytes at a time when it is 16-byte aligned on that path as well.  SHAPES
therefore holds the issue's list, then 63 / 64 / 65 wide and 31 / 32 / 33 high (one pixel below, at and above a tile edge), 129 x 65
(two tiles + 1 both ways), and 132 x 36 (16-byte loads on a partial last tile); 1921 x 9 and 9 x 515 cross every tile seam in x / y."""
import ctypes
import math

import numpy as np
import pytest

import quality_model as qm

F = np.float32
INVALID, UNSUPPORTED = -1, -5
NAMES = ("svgf_quality_state_bytes", "svgf_quality_windows", "svgf_quality_meter", "svgf_quality_read")
TILE_W, TILE_H = 64, 32
SENTINEL = 0x5A5A5A5A


# ---- 1. CPU: symbols, binding, layouts (fails without the feature) ------------------------------------------------------------------
def test_symbols_are_exported_and_the_binding_exists(pkg):
    lib, b = pkg.load_library(), pkg.binding
    for n in NAMES:
        assert hasattr(lib, n) and n in b.EXPORTS, n
    for n in ("quality_state", "quality_windows", "quality_meter", "quality_read"):
        assert callable(getattr(b, n)) and getattr(pkg, n) is getattr(b, n), n
    assert pkg.SvgfQualityParams is b.SvgfQualityParams and pkg.SvgfQualityResult is b.SvgfQualityResult
    assert ctypes.sizeof(b.SvgfQualityParams) == 12
    assert ctypes.sizeof(b.SvgfQualityResult) == 88, "two 64-bit counts and nine doubles: what include/svgf.h states"
    assert [n for n, _ in b.SvgfQualityParams._fields_] == ["peak", "scale", "clamp"]
    assert [n for n, _ in b.SvgfQualityResult._fields_] == ["n_pixels", "n_windows", "sum_se", "sum_ssim", "max_abs", "min_ssim", "peak",
                                                            "scale", "mse", "psnr_db", "mean_ssim"]
    for w, h in ((1, 1), (7, 9), (64, 32), (65, 33), (1920, 1080), (3840, 2160), (1 << 26, 1)):
        n = lib.svgf_quality_state_bytes(w, h)
        assert n >= 64 and n % 8 == 0, (w, h, n)
    for w, h in ((0, 5), (5, 0), (-1, 5), (5, -1), (16384, 8192), (1 << 27, 1)):
        assert lib.svgf_quality_state_bytes(w, h) == 0, (w, h)
    for d, n in ((1, 0), (7, 0), (8, 1), (11, 1), (12, 2), (1921, 479)):
        assert b.quality_windows(d, 8) == (n, 1) and b.quality_windows(8, d) == (1, n) and qm.windows(d) == n, d
    assert lib.svgf_version() == 9, "svgf_version stays 0.9: the symbols are probed"


# ---- 2. CPU: every error is answered before any device work ---------------------------------------------------------------------------
def test_invalid_arguments_are_answered_before_any_device_work(pkg):
    """Device 0 and dummy non-NULL pointers, as tests/test_hdr_display.py does: every case returns its code before the first HIP call,
    with or without a GPU.  (The valid calls are not made here: they would launch on the dummy pointers.)"""
    b, lib = pkg.binding, pkg.load_library()
    P = 0x1000      # never dereferenced
    nan, inf = float("nan"), float("inf")
    QP = lambda peak=1.0, scale=1.0, clamp=0: b.SvgfQualityParams(peak, scale, clamp)

    def meter(state=P, a=P, bb=P, w=8, h=6, qp="qp", exposure=None, se=None, ssim=None):
        return lib.svgf_quality_meter(0, state, a, bb, w, h, None if qp is None else ctypes.byref(QP() if qp == "qp" else qp), exposure,
                                      se, ssim, None)

    assert meter(state=None) == INVALID and meter(a=None) == INVALID and meter(bb=None) == INVALID and meter(qp=None) == INVALID
    for kw in (dict(w=0), dict(h=0), dict(w=-8), dict(h=-6)):
        assert meter(**kw) == INVALID and meter(exposure=P, se=P, ssim=P, **kw) == INVALID, kw
    for bad in (0.0, -1.0, nan, inf, -inf):
        assert meter(qp=QP(peak=bad)) == INVALID and meter(qp=QP(scale=bad)) == INVALID, bad
    for bad in (-1, 2, 7, 1 << 30):
        assert meter(qp=QP(clamp=bad)) == INVALID, bad
    assert meter(w=16384, h=8192) == UNSUPPORTED and meter(w=1 << 27, h=1, exposure=P, se=P, ssim=P) == UNSUPPORTED
    assert meter(w=16384, h=8192, qp=QP(peak=nan)) == INVALID, "the parameters are looked at before the size"

    out = b.SvgfQualityResult()
    assert lib.svgf_quality_read(0, None, ctypes.byref(out), None) == INVALID
    assert lib.svgf_quality_read(0, P, None, None) == INVALID
    nwx, nwy = ctypes.c_int(-7), ctypes.c_int(-7)
    for w, h in ((0, 8), (8, 0), (-8, 8), (8, -8)):
        assert lib.svgf_quality_windows(w, h, ctypes.byref(nwx), ctypes.byref(nwy)) == INVALID and nwx.value == nwy.value == -7
    assert lib.svgf_quality_windows(20, 9, None, None) == 0 and lib.svgf_quality_windows(20, 9, ctypes.byref(nwx), None) == 0 and nwx.value == 4
    # and the binding raises
    with pytest.raises(pkg.SvgfError, match=r"\(-1\)"):
        b.quality_meter(P, P, P, 8, 6, peak=0.0)
    with pytest.raises(pkg.SvgfError, match=r"\(-1\)"):
        b.quality_meter(P, P, P, 8, 6, clamp=2)
    with pytest.raises(pkg.SvgfError, match=r"\(-5\)"):
        b.quality_meter(P, P, P, 16384, 8192)
    with pytest.raises(pkg.SvgfError, match=r"\(-1\)"):
        b.quality_read(None)
    with pytest.raises(pkg.SvgfError, match=r"\(-1\)"):
        b.quality_windows(0, 8)
    with pytest.raises(pkg.SvgfError):
        b.quality_state(0, 8)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def hdr_pair(W, H, seed, peak=1.0, noise=0.3):
    """b: lognormal colours with a share of pixels at 40 x peak; a: b times lognormal noise"""
    rng = np.random.default_rng(seed)
    ref = (rng.lognormal(-1.5, 1.3, (H, W, 3)) * peak).astype(F)
    hot = rng.random((H, W)) < 0.02
    ref[hot] = F(40.0 * peak)
    test = (ref * rng.lognormal(0.0, noise, (H, W, 3))).astype(F)
    return test, ref


def with_specials(a, b):
    """NaN, +inf, -inf, a negative and a denormal pixel in either image: in a window's corner, on a cell seam, on the tile seam (pixels
    63 | 64 and rows 31 | 32) and in the margin no window covers (the images are 75 or 76 x 45: rows from 44, columns from 72 when 75
    wide)."""
    a, b = a.copy(), b.copy()
    H, W = a.shape[:2]
    assert W > TILE_W + 8 and H > TILE_H + 8 and qm.windows(H) * 4 + 4 == H - 1
    a[0, 0, 1] = np.nan                      # a window's corner: one window
    b[3, 4, 0] = np.inf                      # a cell seam in x
    a[4, 11, 2] = -np.inf                    # a cell seam in y
    b[TILE_H - 1, TILE_W - 1] = -b[TILE_H - 1, TILE_W - 1]      # negative: counted, and clamped to 0 with clamp = 1
    a[TILE_H, TILE_W, 0] = np.nan            # the first pixel of the fourth tile: four windows across the seams
    b[TILE_H - 1, TILE_W, 2] = -np.inf
    a[20, TILE_W - 1] = F(1e-40)             # denormal: counted
    b[H - 1, 5, 1] = np.nan                  # the margin below the last window: the error only
    a[H - 1, W - 1] = F(1e-41)
    if W % 4:
        a[10, W - 1, 0] = np.inf             # the margin right of the last window
    return a, b


# ---- 3. CPU: what the model states ------------------------------------------------------------------------------------------------------
def test_model_identical_images_score_one():
    a, _ = hdr_pair(37, 22, 1)
    m = qm.meter(a, a)
    assert m["n_windows"] == 8 * 4 and (m["ssim"] == 1.0).all() and m["min_ssim"] == 1.0 and m["mean_ssim"] == 1.0
    assert m["sum_se"] == 0 and m["max_abs"] == 0 and m["mse"] == 0 and m["psnr_db"] == math.inf and m["n_pixels"] == 37 * 22


def test_model_is_symmetric():
    for seed in range(20):
        a, b = hdr_pair(29, 19, 50 + seed, peak=(1.0, 4.0)[seed & 1])
        kw = dict(peak=(1.0, 4.0)[seed & 1], scale=(1.0, 0.37)[(seed >> 1) & 1], clamp=(seed >> 2) & 1)
        m, r = qm.meter(a, b, **kw), qm.meter(b, a, **kw)
        assert np.array_equal(m["ssim"].view(np.uint64), r["ssim"].view(np.uint64)), seed
        assert np.array_equal(m["se_map"].view(np.uint32), r["se_map"].view(np.uint32)), seed
        for k in ("n_pixels", "n_windows", "sum_se", "sum_ssim", "max_abs", "min_ssim", "mse", "psnr_db", "mean_ssim"):
            assert m[k] == r[k], (seed, k)


def test_model_flat_images():
    a, b = np.full((13, 18, 3), F(0.5), F), np.full((13, 18, 3), F(0.25), F)
    m = qm.meter(a, b, peak=1.0)
    assert m["n_windows"] == 3 * 2 and np.abs(m["ssim"] - (0.25 + 1e-4) / (0.3125 + 1e-4)).max() <= 1e-15
    assert m["mse"] == 0.0625 and m["max_abs"] == 0.25 and m["sum_se"] == 13 * 18 * 3 * 0.0625


def test_model_one_nan_pixel_uncounts_itself_and_its_windows():
    a, b = hdr_pair(30, 22, 3)
    clean = qm.meter(a, b)
    for x, y, n in ((0, 0, 1), (5, 2, 2), (5, 6, 4), (29, 21, 0), (13, 9, 4), (28, 3, 0), (27, 3, 1)):      # 30 wide: windows end at 28; 22 high: at 20
        a2 = a.copy()
        a2[y, x, 1] = np.nan
        m = qm.meter(a2, b)
        assert m["n_pixels"] == clean["n_pixels"] - 1 and m["se_map"].view(np.uint32)[y, x] == qm.NAN_BITS
        gone = clean["counted_windows"] & ~m["counted_windows"]
        want = np.zeros_like(gone)
        for j in range(gone.shape[0]):
            for i in range(gone.shape[1]):
                want[j, i] = 4 * i <= x < 4 * i + 8 and 4 * j <= y < 4 * j + 8
        assert np.array_equal(gone, want) and gone.sum() == n and m["n_windows"] == clean["n_windows"] - n, (x, y)
        assert (m["ssim_map"].view(np.uint32)[gone] == qm.NAN_BITS).all()
        assert np.array_equal(m["ssim"][~gone], clean["ssim"][~gone])


def test_model_clamp_and_the_upper_bound():
    m = qm.meter(np.full((9, 9, 3), F(40.0), F), np.full((9, 9, 3), F(2.0), F), peak=1.0, clamp=1)
    assert m["mse"] == 0 and m["psnr_db"] == math.inf and (m["ssim"] == 1.0).all()
    assert qm.meter(np.full((9, 9, 3), F(40.0), F), np.full((9, 9, 3), F(2.0), F), peak=1.0, clamp=0)["mse"] == 38.0 ** 2
    worst = 0.0
    for seed in range(10):
        a, b = hdr_pair(41, 27, 200 + seed, noise=(0.05, 0.3, 1.0)[seed % 3])
        for clamp in (0, 1):
            m = qm.meter(a, b, clamp=clamp)
            worst = max(worst, float(m["ssim"].max()))
            assert m["ssim"].max() <= 1 + 1e-12
    print(f"largest window of 20 random comparisons: {worst!r}")


# ---- 4. CPU: the use case on the CPU oracle ---------------------------------------------------------------------------------------------
CHAIN_W, CHAIN_H, CHAIN_FRAMES, CHAIN_SEED = 128, 72, 8, 3


def test_model_denoised_frame_scores_above_the_noisy_one_on_the_cpu_oracle(pkg, orc):
    """Synthetic static scene 128 x 72, eight frames, temporal + spatial on, defaults otherwise, against the clean frame (noise 0,
    fireflies 0), peak 1, no clamp.  Last frame, on the CPU oracle: noisy PSNR 13.084 dB, mean SSIM 0.6562; denoised PSNR 16.395 dB,
    mean SSIM 0.7364 (the library's own frames score the same to every printed digit: the chain test below)."""
    W, H = CHAIN_W, CHAIN_H
    o = orc.Oracle(pkg, W, H, threads=4)
    p = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    try:
        for f in range(CHAIN_FRAMES):
            noisy, gb, cam = pkg.synth.render_frame(W, H, f, seed=CHAIN_SEED, moving=False, noise_model="hash")
            out = o.denoise(noisy, gb, cam, p).reshape(H, W, 3)
    finally:
        o.free()
    clean = pkg.synth.render_frame(W, H, CHAIN_FRAMES - 1, seed=CHAIN_SEED, moving=False, noise=0.0, fireflies=0.0, noise_model="hash")[0]
    mn, md = qm.meter(noisy, clean), qm.meter(out, clean)
    print(f"noisy: PSNR {mn['psnr_db']:.3f} dB, mean SSIM {mn['mean_ssim']:.4f}; denoised: PSNR {md['psnr_db']:.3f} dB, mean SSIM {md['mean_ssim']:.4f}")
    assert mn["n_pixels"] == md["n_pixels"] == W * H and mn["n_windows"] == md["n_windows"] == 31 * 17
    assert md["psnr_db"] > mn["psnr_db"] and md["mean_ssim"] > mn["mean_ssim"]


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------
def _dev(a, offset_floats=0):
    """the array on the device, `offset_floats` floats behind a 16-byte boundary"""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.zeros((flat.numel() + 4,), dtype=flat.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset_floats:offset_floats + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4 * offset_floats
    return view


def run_meter(pkg, a, b, maps=(True, True), offset=0, map_offset=0, exposure_state=None, stream=None, **kw):
    """One metering on a state of 0xFF bytes -> (the eight result words as uint64, se_map or None, ssim_map or None)."""
    import torch
    bd = pkg.binding
    H, W = a.shape[:2]
    nwx, nwy = bd.quality_windows(W, H)
    state = bd.quality_state(W, H)
    assert state.numel() * 8 == pkg.load_library().svgf_quality_state_bytes(W, H)
    state.fill_(-1)
    se = _dev(np.full((H, W), SENTINEL, np.uint32).view(F), map_offset) if maps[0] else None
    ss = _dev(np.full((max(nwy, 1), max(nwx, 1)), SENTINEL, np.uint32).view(F)) if maps[1] else None
    torch.cuda.synchronize()
    bd.quality_meter(state, _dev(a, offset), _dev(b, offset), W, H, exposure_state=exposure_state, se_map=se, ssim_map=ss, stream=stream, **kw)
    torch.cuda.synchronize()
    words = state[:8].cpu().numpy().view(np.uint64)
    got_se = se.cpu().numpy().view(np.uint32).reshape(H, W) if maps[0] else None
    got_ss = ss.cpu().numpy().view(np.uint32).reshape(max(nwy, 1), max(nwx, 1)) if maps[1] else None
    return words, got_se, got_ss, state


def compare(words, got_se, got_ss, m, what):
    d = words.view(np.float64)
    print(f"{what}: n_pixels {words[0]} n_windows {words[1]} sum_se {d[2]!r} (exact {m['sum_se']!r}) sum_ssim {d[3]!r} (exact {m['sum_ssim']!r}) "
          f"max_abs {d[4]!r} min_ssim {d[5]!r}")
    assert int(words[0]) == m["n_pixels"] and int(words[1]) == m["n_windows"], what
    assert d[4] == m["max_abs"] and d[5] == m["min_ssim"] and d[6] == m["peak"] and d[7] == m["scale"], what
    assert abs(d[2] - m["sum_se"]) <= m["n_pixels"] * 2.0 ** -52 * m["abs_se"], (what, d[2], m["sum_se"])
    assert abs(d[3] - m["sum_ssim"]) <= m["n_windows"] * 2.0 ** -52 * m["abs_ssim"], (what, d[3], m["sum_ssim"])
    if got_se is not None:
        bad = np.argwhere(got_se != m["se_map"].view(np.uint32))
        assert bad.size == 0, f"{what}: se_map differs at {len(bad)} pixels, first (y, x) {bad[:4].tolist()}"
    if got_ss is not None:
        nwy, nwx = m["ssim_map"].shape
        if nwx and nwy:
            bad = np.argwhere(got_ss != m["ssim_map"].view(np.uint32))
            assert bad.size == 0, f"{what}: ssim_map differs at {len(bad)} windows, first (j, i) {bad[:4].tolist()}"
        else:
            assert (got_ss == SENTINEL).all(), f"{what}: no window, nothing written"


SHAPES = [(1, 1), (7, 9), (8, 8), (9, 8), (11, 12), (12, 8), (1921, 9), (9, 515),
          (63, 9), (64, 9), (65, 9), (9, 31), (9, 32), (9, 33), (129, 65), (132, 36)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_hip_meter_equals_the_model_on_every_shape(pkg, W, H):
    a, b = hdr_pair(W, H, 1000 + W + H)
    if W * H >= 500:
        a[H // 2, W // 3, 1] = np.nan
        b[H - 1, W - 1, 0] = np.inf
    m = qm.meter(a, b, peak=1.0, scale=1.0, clamp=0)
    assert (m["n_windows"] > 0) == (W >= 8 and H >= 8)
    compare(*run_meter(pkg, a, b, peak=1.0, scale=1.0, clamp=0)[:3], m, f"{W}x{H}")
    m1 = qm.meter(a, b, peak=1.0, scale=0.37, clamp=1)
    compare(*run_meter(pkg, a, b, peak=1.0, scale=0.37, clamp=1)[:3], m1, f"{W}x{H} clamped")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(65, 33), (132, 36), (8, 8)])
def test_hip_meter_of_images_that_are_not_16_byte_aligned(pkg, W, H):
    """The image pair 4 bytes behind a 16-byte boundary (dword loads whatever the width); then aligned images with the error map 4
    bytes behind one (16-byte loads, dword stores)."""
    a, b = hdr_pair(W, H, 77 + W)
    a[H // 2, W // 2, 0] = np.nan
    m = qm.meter(a, b, peak=4.0, scale=1.0, clamp=0)
    compare(*run_meter(pkg, a, b, offset=1, peak=4.0)[:3], m, f"misaligned {W}x{H}")
    compare(*run_meter(pkg, a, b, offset=3, map_offset=2, peak=4.0)[:3], m, f"misaligned by 12 bytes {W}x{H}")
    compare(*run_meter(pkg, a, b, map_offset=1, peak=4.0)[:3], m, f"misaligned map {W}x{H}")


@pytest.mark.gpu
@pytest.mark.parametrize("W", [75, 76])
def test_hip_meter_values(pkg, W):
    """HDR pairs with every kind of special pixel, every clamp / scale / peak, with and without each map."""
    H = 45
    for peak in (1.0, 4.0):
        a, b = with_specials(*hdr_pair(W, H, 500 + W, peak=peak))
        for clamp in (0, 1):
            for scale in (1.0, 0.37):
                m = qm.meter(a, b, peak=peak, scale=scale, clamp=clamp)
                assert 0 < m["n_pixels"] < W * H and 0 < m["n_windows"] < qm.windows(W) * qm.windows(H)
                compare(*run_meter(pkg, a, b, peak=peak, scale=scale, clamp=clamp)[:3], m, f"{W}x{H} peak {peak} clamp {clamp} scale {scale}")
        for maps in ((False, False), (True, False), (False, True)):
            compare(*run_meter(pkg, a, b, maps=maps, peak=peak, scale=0.37, clamp=1)[:3], m, f"{W}x{H} maps {maps}")


@pytest.mark.gpu
def test_hip_meter_of_dead_and_identical_images(pkg):
    W, H = 70, 37
    a, b = hdr_pair(W, H, 9)
    dead = np.full((H, W, 3), np.nan, F)
    for x, y, what in ((dead, b, "all-NaN a"), (a, dead, "all-NaN b")):
        m = qm.meter(x, y)
        assert m["n_pixels"] == 0 and m["n_windows"] == 0 and m["min_ssim"] == math.inf and m["max_abs"] == 0
        words, se, ss, state = run_meter(pkg, x, y)
        compare(words, se, ss, m, what)
        r = pkg.binding.quality_read(state)
        assert r["n_pixels"] == 0 and math.isnan(r["mse"]) and math.isnan(r["psnr_db"]) and math.isnan(r["mean_ssim"]) and r["min_ssim"] == math.inf
    m = qm.meter(a, a, peak=4.0)
    words, se, ss, state = run_meter(pkg, a, a, peak=4.0)
    compare(words, se, ss, m, "a == a")
    r = pkg.binding.quality_read(state)
    assert r["mse"] == 0 and r["psnr_db"] == math.inf and r["mean_ssim"] == 1.0 and r["min_ssim"] == 1.0 and r["peak"] == 4.0
    assert (ss.view(F) == 1.0).all() and (se == 0).all()
    # no window at all: the dependent value is NaN, the error is not
    a7, b7 = hdr_pair(7, 9, 4)
    words, se, ss, state = run_meter(pkg, a7, b7)
    m = qm.meter(a7, b7)
    compare(words, se, ss, m, "7x9")
    r = pkg.binding.quality_read(state)
    assert r["n_windows"] == 0 and math.isnan(r["mean_ssim"]) and r["mse"] == r["sum_se"] / (3.0 * 63) and r["psnr_db"] == 10.0 * math.log10(1.0 / r["mse"])


@pytest.mark.gpu
def test_hip_meter_with_a_metered_exposure(pkg):
    """exposure_state_dev from a real svgf_exposure_meter run: the model fed scale x word[516]."""
    import torch
    bd = pkg.binding
    W, H = 76, 45
    a, b = with_specials(*hdr_pair(W, H, 31, peak=3.0))
    est = bd.exposure_state()
    bd.exposure_meter(est, _dev(b), W, H, adapt=1.0)
    torch.cuda.synchronize()
    words = est.cpu().numpy().view(np.uint32)
    exposure = float(words[qm.EXPOSURE_WORD:qm.EXPOSURE_WORD + 1].view(F)[0])
    assert math.isfinite(exposure) and exposure not in (0.0, 1.0)
    for clamp in (0, 1):
        m = qm.meter(a, b, peak=1.0, scale=0.8, clamp=clamp, exposure_words=words)
        assert m["scale"] == float(F(0.8) * F(exposure))
        got = run_meter(pkg, a, b, exposure_state=est, peak=1.0, scale=0.8, clamp=clamp)
        compare(*got[:3], m, f"metered exposure {exposure}, clamp {clamp}")
        r = bd.quality_read(got[3])
        assert r["scale"] == m["scale"] and r["n_pixels"] == m["n_pixels"]
        assert r["mse"] == r["sum_se"] / (3.0 * r["n_pixels"]) and r["mean_ssim"] == r["sum_ssim"] / r["n_windows"]
        assert r["psnr_db"] == 10.0 * math.log10(1.0 / r["mse"])


@pytest.mark.gpu
def test_hip_meter_is_deterministic(pkg):
    """The same call twice, then on another stream: the same 64 bytes."""
    import torch
    W, H = 333, 131
    a, b = hdr_pair(W, H, 5)
    first = run_meter(pkg, a, b, peak=1.0, scale=0.37, clamp=0)[0]
    again = run_meter(pkg, a, b, peak=1.0, scale=0.37, clamp=0)[0]
    side = torch.cuda.Stream()
    other = run_meter(pkg, a, b, peak=1.0, scale=0.37, clamp=0, stream=side)[0]
    assert np.array_equal(first, again) and np.array_equal(first, other)
    compare(first, None, None, qm.meter(a, b, peak=1.0, scale=0.37, clamp=0), "333x131")


@pytest.mark.gpu
def test_hip_produce_denoise_meter_chain(pkg):
    """The frames of the CPU use case run by the library at 128 x 72: produce, denoise, then the meter of the noisy and of the denoised
    frame against the clean producer frame, equal to the model fed the downloaded images; the denoised frame scores strictly higher in
    PSNR and in mean SSIM; and the flicker figure (this output against the previous one) equals the model as well."""
    import torch
    bd = pkg.binding
    W, H = CHAIN_W, CHAIN_H
    den = pkg.Denoiser(W, H)
    params = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1)
    new = lambda: torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    noisy, clean, out, prev = new(), new(), new(), new()
    gb = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    gb_clean = torch.empty_like(gb)
    s = torch.cuda.current_stream()
    states = [bd.quality_state(W, H) for _ in range(3)]
    try:
        for f in range(CHAIN_FRAMES):
            cam = pkg.synth.camera_for_frame(f, False)
            prev.copy_(out)
            bd.synth_render(noisy, gb, W, H, cam, f, seed=CHAIN_SEED, stream=s)
            den.denoise(out, noisy, gb, cam, params, stream=s)
        bd.synth_render(clean, gb_clean, W, H, cam, CHAIN_FRAMES - 1, seed=CHAIN_SEED, noise=0.0, fireflies=0.0, stream=s)
        for st in states:
            st.fill_(-1)
        bd.quality_meter(states[0], noisy, clean, W, H, stream=s)
        bd.quality_meter(states[1], out, clean, W, H, stream=s)
        bd.quality_meter(states[2], out, prev, W, H, stream=s)
        rn, rd, rf = (bd.quality_read(st, stream=s) for st in states)
    finally:
        den.free()
    h_noisy, h_clean, h_out, h_prev = (t.cpu().numpy() for t in (noisy, clean, out, prev))
    for r, st, m, what in ((rn, states[0], qm.meter(h_noisy, h_clean), "noisy"), (rd, states[1], qm.meter(h_out, h_clean), "denoised"),
                           (rf, states[2], qm.meter(h_out, h_prev), "flicker")):
        compare(st[:8].cpu().numpy().view(np.uint64), None, None, m, what)
        assert r["n_pixels"] == W * H and r["n_windows"] == 31 * 17
        assert r["mse"] == r["sum_se"] / (3.0 * W * H) and r["mean_ssim"] == r["sum_ssim"] / (31 * 17)
        print(f"{what}: PSNR {r['psnr_db']:.3f} dB, mean SSIM {r['mean_ssim']:.4f}, largest error {r['max_abs']:.4f}, worst window {r['min_ssim']:.4f}")
    assert rd["psnr_db"] > rn["psnr_db"] and rd["mean_ssim"] > rn["mean_ssim"]
