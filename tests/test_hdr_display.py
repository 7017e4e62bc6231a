"""HDR display (include/svgf.h row f12): svgf_exposure_reset, svgf_exposure_meter, svgf_display_tonemap,
svgf_tonemap_srgb_table.

The yardstick is tests/tonemap_model.py.  Every comparison of a kernel with the model is on every state word / every byte: the
histogram is integer counts, the resolve integer sums and a handful of correctly rounded float32 operations, the pack float32
without contraction and no transcendental, so there is no tolerance to choose.

Two statements about the model are bounds, both derived and not measured.  Flat image of luminance L: the metered average is the
centre bit pattern of L's bin; a bin spans 1/8 of its octave's mantissa range, so centre / L lies in [1.0625 / 1.125, 1.0625] and
key / (t L) within 6.25 % of 1.  Lognormal image, no trim: the mean of bit patterns is the mean of a piecewise-linear log2 whose
worst error against log2 is 0.0861 (at mantissa 1 / ln 2 - 1), so the inverse differs from the geometric mean by at most 2^0.0861,
times the half bin: 1.0615 x 1.0625 < 1.13.

Launch geometry of k_luma_histogram (svgf_display.hip): 1024 threads, at most 256 workgroups, four pixels per thread and turn on a
16-byte aligned image: one grid-stride turn covers 256 x 1024 x 4 = 1 048 576 pixels.  1025 x 1025 = 1 050 625 pixels = 262 656
whole fours + 1: threads 0..511 take a second turn and one pixel goes down the one-pixel tail.  An image that is not 16-byte aligned
takes one pixel per thread and turn throughout: that path gets shapes of its own."""
import ctypes

import numpy as np
import pytest

import tonemap_model as tmm
from temporal_harness import same_bits
from test_display import pack_oracle

F = np.float32
INVALID, UNSUPPORTED = -1, -5
TRIMS = ((0, 0), (51, 51), (512, 511), (0, 1023), (1023, 0))
NAMES = ("svgf_exposure_reset", "svgf_exposure_meter", "svgf_display_tonemap", "svgf_tonemap_srgb_table")


# ---- 1. CPU: symbols, binding, layouts (fails without the feature) ------------------------------------------------------------------
def test_symbols_are_exported_and_the_binding_exists(pkg):
    lib, b = pkg.load_library(), pkg.binding
    for n in NAMES:
        assert hasattr(lib, n) and n in b.EXPORTS, n
    for n in ("exposure_state", "exposure_reset", "exposure_meter", "display_tonemap", "srgb_table"):
        assert callable(getattr(b, n)) and getattr(pkg, n) is getattr(b, n), n
    assert pkg.SvgfExposureParams is b.SvgfExposureParams and pkg.SvgfTonemapParams is b.SvgfTonemapParams
    assert ctypes.sizeof(b.SvgfExposureParams) == 24 and ctypes.sizeof(b.SvgfTonemapParams) == 16
    assert [n for n, _ in b.SvgfExposureParams._fields_] == ["key", "trim_low_1024", "trim_high_1024", "min_exposure", "max_exposure", "adapt"]
    assert [n for n, _ in b.SvgfTonemapParams._fields_] == ["op", "transfer", "exposure_bias", "white"]
    assert b.EXPOSURE_STATE_WORDS == tmm.STATE_WORDS == 520
    assert lib.svgf_version() == 9, "svgf_version stays 0.9: the symbols are probed"


# ---- 2. CPU: every error is answered before any device work ---------------------------------------------------------------------------
def test_invalid_arguments_are_answered_before_any_device_work(pkg):
    """Device 0 and dummy non-NULL pointers, as tests/test_upsample.py does: every case returns its code before the first HIP call,
    with or without a GPU.  (The valid calls are not made here: they would launch on the dummy pointers.)"""
    b, lib = pkg.binding, pkg.load_library()
    P = 0x1000      # never dereferenced
    nan, inf = float("nan"), float("inf")
    ref = lambda s: None if s is None else ctypes.byref(s)
    EP = lambda key=0.18, lo=51, hi=51, mn=1 / 64, mx=64.0, adapt=0.25: b.SvgfExposureParams(key, lo, hi, mn, mx, adapt)
    TP = lambda op=2, transfer=2, bias=1.0, white=0.0: b.SvgfTonemapParams(op, transfer, bias, white)

    assert lib.svgf_exposure_reset(0, None, None) == INVALID

    def meter(state=P, rgb=P, w=8, h=6, ep="ep"):
        return lib.svgf_exposure_meter(0, state, rgb, w, h, ref(EP() if ep == "ep" else ep), None)

    assert meter(state=None) == INVALID and meter(rgb=None) == INVALID and meter(ep=None) == INVALID
    for kw in (dict(w=0), dict(h=0), dict(w=-8), dict(h=-6)):
        assert meter(**kw) == INVALID, kw
    for bad in (0.0, -0.18, nan, inf, -inf):
        assert meter(ep=EP(key=bad)) == INVALID and meter(ep=EP(mn=bad)) == INVALID and meter(ep=EP(mx=bad)) == INVALID, bad
    assert meter(ep=EP(mn=2.0, mx=1.0)) == INVALID
    for bad in (0.0, -0.25, 1.0000001, 2.0, nan, inf, -inf):
        assert meter(ep=EP(adapt=bad)) == INVALID, bad
    for lo, hi in ((-1, 0), (0, -1), (1024, 0), (0, 1024), (512, 512), (1023, 1), (1, 1023), (1 << 30, 1 << 30), (-(1 << 31), 0)):
        assert meter(ep=EP(lo=lo, hi=hi)) == INVALID, (lo, hi)
    assert meter(w=16384, h=8192) == UNSUPPORTED and meter(w=1 << 27, h=1) == UNSUPPORTED

    def tone(pbo=P, left=P, right=P, w=8, h=6, tp="tp", state=P):
        return lib.svgf_display_tonemap(0, pbo, left, right, w, h, ref(TP() if tp == "tp" else tp), state, None)

    assert tone(pbo=None) == INVALID and tone(right=None) == INVALID and tone(tp=None) == INVALID
    assert tone(pbo=None, left=None, state=None) == INVALID      # a NULL left or state is no error in itself ...
    for kw in (dict(w=0), dict(h=0), dict(w=-8), dict(h=-6)):
        assert tone(**kw) == INVALID and tone(left=None, state=None, **kw) == INVALID, kw
    for bad in (-1, 3, 7):
        assert tone(tp=TP(op=bad)) == INVALID and tone(tp=TP(transfer=bad)) == INVALID, bad
    for bad in (-0.5, nan, inf, -inf):
        assert tone(tp=TP(bias=bad)) == INVALID and tone(tp=TP(white=bad)) == INVALID, bad
    assert tone(w=16384, h=8192) == UNSUPPORTED and tone(w=1 << 27, h=1, left=None, state=None) == UNSUPPORTED      # ... and reaches the size check

    assert lib.svgf_tonemap_srgb_table(None) == INVALID
    # and the binding raises
    with pytest.raises(pkg.SvgfError, match=r"\(-1\)"):
        b.exposure_meter(P, P, 8, 6, adapt=0.0)
    with pytest.raises(pkg.SvgfError, match=r"\(-1\)"):
        b.display_tonemap(P, None, P, 8, 6, op=3)
    with pytest.raises(pkg.SvgfError, match=r"\(-1\)"):
        b.exposure_reset(None)


# ---- 3. CPU: the table ------------------------------------------------------------------------------------------------------------------
def test_srgb_table_is_the_formula(pkg):
    T = pkg.binding.srgb_table()
    assert T.dtype == F and T.shape == (256,)
    assert same_bits(T, tmm.srgb_table()), "all 256 literals are the float32 nearest to the double formula"
    assert (np.diff(T) > 0).all(), "strictly increasing"
    assert T[0] == 0 and T[255] == 1


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def hdr_image(W, H, seed, special=True):
    """lognormal(-1.5, 1.2) colours; from 15 pixels up, NaN, +inf, -inf, negative, zero and denormal pixels sprinkled in (one of each,
    or 0.5 % of the pixels each)."""
    rng = np.random.default_rng(seed)
    img = rng.lognormal(-1.5, 1.2, (H, W, 3)).astype(F)
    px, n = img.reshape(-1, 3), W * H
    if special and n >= 15:
        k = max(1, n // 200)
        where = rng.choice(n, 6 * k, replace=False).reshape(6, k)
        px[where[0], rng.integers(0, 3, k)] = np.nan
        px[where[1], rng.integers(0, 3, k)] = np.inf
        px[where[2], rng.integers(0, 3, k)] = -np.inf
        px[where[3]] = -px[where[3]]
        px[where[4]] = 0.0
        px[where[5]] = F(1e-40)
    return img


def edge_image():
    """1e-7, 1e6 and, for the octaves at either end of the histogram and six in the middle, every bin boundary 2^k (1 + j / 8) and the
    float just below it, as grey pixels: the luminance of (v, v, v) is v (checked)."""
    v = [F(1e-7), F(1e6)]
    for k in (-18, -17, -16, -15, -3, -2, -1, 0, 1, 2, 14, 15, 16, 17):
        for j in range(8):
            edge = F(2.0 ** k * (1 + j / 8))
            v += [edge, np.nextafter(edge, F(0))]
    v = np.array(v, dtype=F)
    img = np.repeat(v[None, :, None], 3, axis=2)
    assert same_bits(tmm.luminance(img).reshape(-1), v)
    return np.ascontiguousarray(img)


# ---- 4. CPU: what the model states ------------------------------------------------------------------------------------------------------
def test_model_flat_image_meters_within_half_a_bin():
    worst = 0.0
    for L in np.geomspace(1e-4, 1e4, 200):
        img = np.full((9, 16, 3), F(L), F)
        Lf = float(tmm.luminance(img)[0, 0])
        s = tmm.meter(tmm.reset(), img, key=0.18, trim_low_1024=51, trim_high_1024=51, min_exposure=1e-6, max_exposure=1e6)
        t = float(tmm.as_float(s[tmm.TARGET]))
        assert s[tmm.N] == s[tmm.M] + ((144 * 51) >> 10) * 2 == 144 and s[tmm.EXPOSURE] == s[tmm.TARGET] and s[tmm.COUNT] == 1
        worst = max(worst, abs(0.18 / (t * Lf) - 1))
        assert abs(0.18 / (t * Lf) - 1) <= 0.0625, (L, t)
    print(f"flat images: key / (t L) is within {100 * worst:.2f} % of 1")


def test_model_lognormal_image_meters_the_geometric_mean():
    img = hdr_image(96, 54, 11, special=False)
    L = tmm.luminance(img).astype(np.float64)
    G = float(np.exp(np.log(L).mean()))
    for trims, bound in (((0, 0), 0.13), ((51, 51), None)):
        s = tmm.meter(tmm.reset(), img, key=0.18, trim_low_1024=trims[0], trim_high_1024=trims[1], min_exposure=1e-6, max_exposure=1e6)
        t = float(tmm.as_float(s[tmm.TARGET]))
        print(f"lognormal 96x54, trims {trims}: t = {t:.5f}, key / geometric mean = {0.18 / G:.5f}, off by {100 * abs(t * G / 0.18 - 1):.2f} %; "
              f"{np.count_nonzero(s[256:512])} bins populated")
        if bound is not None:
            assert abs(t * G / 0.18 - 1) <= bound


def test_model_no_counted_pixel_keeps_the_exposure():
    dead = np.full((3, 5, 3), np.nan, F)
    s = tmm.meter(tmm.reset(), dead)
    assert s[tmm.N] == s[tmm.M] == s[tmm.LBITS] == 0 and s[tmm.COUNT] == 1
    assert s[tmm.TARGET] == s[tmm.EXPOSURE] == tmm.ONE_BITS, "a first metering without a counted pixel: exposure 1"
    s1 = tmm.meter(tmm.reset(), hdr_image(16, 9, 2), adapt=0.25)
    s2 = tmm.meter(s1, dead, adapt=0.25)
    assert s2[tmm.M] == 0 and s2[tmm.TARGET] == s1[tmm.EXPOSURE] and s2[tmm.COUNT] == 2
    assert s2[tmm.EXPOSURE] == s1[tmm.EXPOSURE], "prev + (prev - prev) * adapt"
    # the clamps of the target, and the step towards it
    dark = np.full((2, 2, 3), F(1e-4), F)
    s3 = tmm.meter(s1, dark, adapt=0.25)
    assert tmm.as_float(s3[tmm.TARGET]) == F(64.0)
    prev = tmm.as_float(s1[tmm.EXPOSURE])
    assert tmm.as_float(s3[tmm.EXPOSURE]) == prev + (F(64.0) - prev) * F(0.25)
    assert (s3[:256] == 0).all() and s3[256:512].sum() == 4 and (s3[518:] == 0).all()


def test_model_identity_is_the_plain_pack():
    """op 0, transfer 0, bias 1, no state: svgf_display_pack's bytes (tests/test_display.py's pack_oracle)."""
    rng = np.random.default_rng(9)
    left = (rng.random((7, 13, 3), dtype=F) * 1.6 - 0.3).astype(F)
    right = (rng.random((7, 13, 3), dtype=F) * 3.0).astype(F)
    left.flat[0], left.flat[1], left.flat[2] = np.nan, np.inf, -np.inf
    right.flat[5], right.flat[6] = F(37.0 / 255.0), F(1.0)
    assert np.array_equal(tmm.display_tonemap(left, right, 0, 0), pack_oracle(left, right))
    assert np.array_equal(tmm.display_tonemap(None, right, 0, 0), pack_oracle(left, right)[:, 13:])


def test_model_table_search_is_the_count():
    """The model counts thresholds with a sorted search; the definition is the count itself."""
    T = tmm.srgb_table()
    y = np.concatenate([T, np.nextafter(T, F(-1)), np.nextafter(T, F(2)), [np.nan, np.inf, -np.inf, -0.0, 7.0]]).astype(F)
    want = np.array([sum(1 for k in range(1, 256) if v >= T[k]) for v in y], dtype=np.uint8)
    assert np.array_equal(tmm.tonemap_bytes(y, 1.0, 0, 2, 0.0, T), want)
    assert np.array_equal(want[:256], np.arange(256)) and np.array_equal(want[257:512], np.arange(255))


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(state):
    import torch
    torch.cuda.synchronize()
    return state.cpu().numpy().view(np.uint32)


def _diff(got, ref):
    bad = np.flatnonzero(got != ref)
    return f"{bad.size} words differ, first at {bad[:8].tolist()}: got {got[bad[:8]].tolist()}, want {ref[bad[:8]].tolist()}"


def _meter_every_trim(pkg, img, what, misaligned=False):
    """One metering per trim pair on a freshly reset state, all 520 words against the model."""
    import torch
    b = pkg.binding
    H, W = img.shape[:2]
    if misaligned:      # the image starts 4 bytes behind a 16-byte boundary
        buf = torch.zeros((W * H * 3 + 1,), dtype=torch.float32, device="cuda")
        buf[1:] = _dev(img).reshape(-1)
        dev = buf[1:]
        assert dev.data_ptr() % 16 == 4
    else:
        dev = _dev(img)
        assert dev.data_ptr() % 16 == 0
    state = b.exposure_state()
    assert np.array_equal(_words(state), tmm.reset())
    for lo, hi in TRIMS:
        b.exposure_reset(state)
        b.exposure_meter(state, dev, W, H, trim_low_1024=lo, trim_high_1024=hi, adapt=0.5)
        got, ref = _words(state), tmm.meter(tmm.reset(), img, trim_low_1024=lo, trim_high_1024=hi, adapt=0.5)
        assert np.array_equal(got, ref), f"{what}, trims ({lo}, {hi}): {_diff(got, ref)}"
        if ref[tmm.N] >= 1:
            assert ref[tmm.M] >= 1


HIST_SHAPES = [(1, 1), (5, 3), (257, 131), (1921, 7), (1025, 1025)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", HIST_SHAPES, ids=[f"{w}x{h}" for w, h in HIST_SHAPES])
def test_hip_histogram_and_resolve_equal_the_model(pkg, W, H):
    """1025 x 1025: some threads take a second grid-stride turn (the module docstring derives it)."""
    img = hdr_image(W, H, 100 + W)
    if W * H >= 257 * 131:
        h = tmm.histogram(img)
        print(f"{W}x{H}: {np.count_nonzero(h)} bins populated, {100.0 * h.sum() / (W * H):.1f} % of the pixels counted")
        assert np.count_nonzero(h) >= 60 and h.sum() >= 0.9 * W * H
    _meter_every_trim(pkg, img, f"{W}x{H}")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(5, 3), (257, 131), (515, 511)])
def test_hip_histogram_of_an_image_that_is_not_16_byte_aligned(pkg, W, H):
    """515 x 511 = 263 165 pixels: more than the 262 144 one turn of one pixel per thread covers."""
    _meter_every_trim(pkg, hdr_image(W, H, 300 + W), f"misaligned {W}x{H}", misaligned=True)


@pytest.mark.gpu
def test_hip_histogram_of_a_flat_image(pkg):
    """300 x 9 at 0.18: every lane of every wave lands on one bin."""
    img = np.full((9, 300, 3), F(0.18), F)
    assert np.count_nonzero(tmm.histogram(img)) == 1
    _meter_every_trim(pkg, img, "flat 300x9")


@pytest.mark.gpu
def test_hip_histogram_of_the_bin_edges(pkg):
    img = edge_image()
    h = tmm.histogram(img)
    assert h[0] >= 17 and h[255] >= 17 and h.sum() == img.shape[1]
    _meter_every_trim(pkg, img, "bin edges")


@pytest.mark.gpu
def test_hip_metering_sequence(pkg):
    """Five meterings of different images with adapt 0.25, an all-NaN image (the target is the previous exposure), a reset, an
    all-invalid first image (the exposure is 1): all 520 words after every step."""
    b = pkg.binding
    W, H = 67, 45
    state = b.exposure_state()
    ref = tmm.reset()
    assert np.array_equal(_words(state), ref)
    for i, gain in enumerate((1.0, 8.0, 0.05, 300.0, 1.0)):
        img = (hdr_image(W, H, 40 + i) * F(gain)).astype(F)
        b.exposure_meter(state, _dev(img), W, H, adapt=0.25)
        got, ref = _words(state), tmm.meter(ref, img, adapt=0.25)
        assert np.array_equal(got, ref), f"metering {i}: {_diff(got, ref)}"
        assert ref[tmm.COUNT] == i + 1 and (i == 0 or ref[tmm.EXPOSURE] != ref[tmm.TARGET])
    before = ref
    dead = np.full((H, W, 3), np.nan, F)
    b.exposure_meter(state, _dev(dead), W, H, adapt=0.25)
    got, ref = _words(state), tmm.meter(ref, dead, adapt=0.25)
    assert np.array_equal(got, ref), f"all-NaN image: {_diff(got, ref)}"
    assert ref[tmm.TARGET] == before[tmm.EXPOSURE] and ref[tmm.M] == 0
    b.exposure_reset(state)
    got = _words(state)
    assert np.array_equal(got, tmm.reset()) and got[tmm.EXPOSURE] == tmm.ONE_BITS and got[tmm.COUNT] == 0
    invalid = np.zeros((H, W, 3), F)
    invalid[::2] = -1.0
    invalid[1::3, :, 1] = np.inf
    invalid[2::5, :, 2] = -np.inf
    b.exposure_meter(state, _dev(invalid), W, H, adapt=0.25)
    got, ref = _words(state), tmm.meter(tmm.reset(), invalid, adapt=0.25)
    assert np.array_equal(got, ref), f"all-invalid first image: {_diff(got, ref)}"
    assert got[tmm.EXPOSURE] == tmm.ONE_BITS and got[tmm.N] == 0 and got[tmm.COUNT] == 1


def tone_image(W, H, seed):
    """0 to several hundred, negative, NaN and +-inf"""
    rng = np.random.default_rng(seed)
    img = rng.lognormal(-1.5, 1.2, (H, W, 3)).astype(F)
    v = img.reshape(-1)
    if v.size >= 15:
        k = max(1, v.size // 50)
        where = rng.choice(v.size, 6 * k, replace=False).reshape(6, k)
        v[where[0]] *= F(300.0)
        v[where[1]] *= F(-1.0)
        v[where[2]] = np.nan
        v[where[3]] = np.inf
        v[where[4]] = -np.inf
        v[where[5]] = 0.0
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (257, 131)])
def test_hip_tonemap_equals_the_model(pkg, W, H):
    import torch
    b = pkg.binding
    left, right = tone_image(W, H, 7 * W), tone_image(W, H, 7 * W + 1)
    T = b.srgb_table()
    words = tmm.meter(tmm.reset(), hdr_image(16, 9, 5), adapt=1.0)
    assert tmm.as_float(words[tmm.EXPOSURE]) not in (F(0), F(1))
    state = _dev(words.view(np.int32))
    t_left, t_right = _dev(left), _dev(right)
    two, one = torch.empty((H, 2 * W, 4), dtype=torch.uint8, device="cuda"), torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
    for op in (0, 1, 2):
        for transfer in (0, 1, 2):
            for st in (None, state):
                for white in (0.0, 4.0):
                    for bias in (0.0, 1.0, 2.5):
                        for has_left in (True, False):
                            pbo = two if has_left else one
                            pbo.fill_(0x5A)
                            b.display_tonemap(pbo, t_left if has_left else None, t_right, W, H, op=op, transfer=transfer,
                                              exposure_bias=bias, white=white, state=st)
                            torch.cuda.synchronize()
                            ref = tmm.display_tonemap(left if has_left else None, right, op, transfer, bias, white,
                                                      None if st is None else words, T)
                            got = pbo.cpu().numpy()
                            assert np.array_equal(got, ref), (f"op {op}, transfer {transfer}, state {st is not None}, white {white}, bias {bias}, "
                                                              f"left {has_left}: {np.count_nonzero(got != ref)} bytes differ")
    # op 0, transfer 0, bias 1, no state: svgf_display_pack's own output on the same tensors
    plain = torch.empty_like(two)
    b.display_pack(plain, t_left, t_right, W, H)
    b.display_tonemap(two, t_left, t_right, W, H, op=0, transfer=0, exposure_bias=1.0, white=0.0, state=None)
    torch.cuda.synchronize()
    assert torch.equal(plain, two)


@pytest.mark.gpu
def test_hip_srgb_transfer_on_every_threshold(pkg):
    """op 0, transfer 2: T[k] gives k and the float below it k - 1."""
    import torch
    b = pkg.binding
    T = b.srgb_table()
    below = np.nextafter(T, F(-1))
    img = np.concatenate([T, below, [F(0.5)]]).astype(F).reshape(1, 171, 3)
    pbo = torch.empty((1, 171, 4), dtype=torch.uint8, device="cuda")
    b.display_tonemap(pbo, None, _dev(img), 171, 1, op=0, transfer=2, exposure_bias=1.0, state=None)
    torch.cuda.synchronize()
    got = pbo.cpu().numpy()
    assert (got[..., 3] == 0).all()
    got = got[..., :3].reshape(-1)
    assert np.array_equal(got[:256], np.arange(256)), "T[k] -> k"
    assert np.array_equal(got[256:512], np.maximum(np.arange(256) - 1, 0)), "the float below T[k] -> k - 1"
    assert np.array_equal(pbo.cpu().numpy(), tmm.display_tonemap(None, img, 0, 2, 1.0, 0.0, None, T))


@pytest.mark.gpu
def test_hip_produce_denoise_meter_tonemap_chain(pkg):
    """320 x 180, six frames on one stream, the synth colours scaled x 8: after each frame the state and the bytes equal the model fed
    the context's downloaded output; on the last frame the plain pack saturates on a larger share of the bytes than the tone-mapped one.
    53 % of this frame are ray misses, which the cascade leaves at 1e-16 .. 1e-13, positive, so counted, in bin 0: the low trim is 60 %
    (trim the background's share away, as histogram metering commonly does).  With the 5 % starting value the
    dark half drags the average down to 0.0036 and the exposure up to 49.6, and the tone-mapped image clips MORE than the plain one
    (46.7 % against 41.1 % of the bytes, measured on the device before this test took its present form)."""
    import torch
    b = pkg.binding
    W, H = 320, 180
    den = pkg.Denoiser(W, H)
    params = pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=5, history_level=1)
    rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    gb = torch.empty((H * W * 52,), dtype=torch.uint8, device="cuda")
    out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    pbo = torch.empty((H, 2 * W, 4), dtype=torch.uint8, device="cuda")
    plain = torch.empty((H, 2 * W, 4), dtype=torch.uint8, device="cuda")
    T = b.srgb_table()
    s = torch.cuda.current_stream()
    state = b.exposure_state()
    ref = tmm.reset()
    try:
        for f in range(6):
            cam = pkg.synth.camera_for_frame(f, False)
            b.synth_render(rgb, gb, W, H, cam, f, seed=3, stream=s)
            rgb.mul_(8.0)
            den.denoise(out, rgb, gb, cam, params, stream=s)
            b.exposure_meter(state, out, W, H, trim_low_1024=614, trim_high_1024=51, adapt=0.25, stream=s)
            b.display_tonemap(pbo, rgb, out, W, H, op=2, transfer=2, exposure_bias=1.0, state=state, stream=s)
            b.display_pack(plain, rgb, out, W, H, stream=s)
            got = _words(state)
            h_rgb, h_out = rgb.cpu().numpy(), out.cpu().numpy()
            ref = tmm.meter(ref, h_out, trim_low_1024=614, trim_high_1024=51, adapt=0.25)
            assert np.array_equal(got, ref), f"frame {f}: {_diff(got, ref)}"
            assert np.array_equal(pbo.cpu().numpy(), tmm.display_tonemap(h_rgb, h_out, 2, 2, 1.0, 0.0, ref, T)), f"frame {f}"
    finally:
        den.free()
    share = lambda a: float((a[:, W:, :3] == 255).mean())
    sat_plain, sat_mapped = share(plain.cpu().numpy()), share(pbo.cpu().numpy())
    print(f"exposure {tmm.as_float(ref[tmm.EXPOSURE]):.4f}; bytes at 255 in the denoised half: plain pack {100 * sat_plain:.2f} %, tone-mapped {100 * sat_mapped:.2f} %")
    assert sat_plain > sat_mapped
