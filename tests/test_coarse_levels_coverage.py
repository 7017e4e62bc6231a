"""What the lane / strip kernels' coarse-level tests cover, pinned without a GPU.

The lane-marching kernel (csrc/svgf_atrous_lane_impl.h) and the strip kernel (csrc/svgf_atrous_strip.hip) run the a-trous levels of
steps 2 .. 32.  With the reference's default sigmas (0.45 / 0.35 / 0.2) the levels at steps 8, 16 and 32 give their taps next to no
weight on the frames the other modules use: on random_frame(257, 193, seed=70) level 4 moves 0.1 % of the pixels by more than 1e-3
when its 16 outer taps (|i| or |j| = 2) are dropped and level 5 none, sigma_l stops acting at level 3 (den_l = sqrt(10) 0.45 = 1.42
is far above what two levels leave of the luminance differences), and a non-temporal frame's variance is 10.0 at every level, so
that the variance plane a level writes, the 3x3 pre-blur and blur_variance are invisible.  A wrong outer-ring tap at step 16 or 32
would pass every one of those tests.  This module holds what tests/test_coarse_levels_gpu.py runs instead, and proves from the
reference side alone (the CPU oracle and a float64 numpy model of one level) that the coarse levels act on it:

  * cascade(): the oracle's exported single-level function (svgf_oracle_atrous) chained over the levels; it returns colour and
    variance after EVERY level from one run, and is pinned to Oracle.denoise bit for bit, level by level.
  * model_level(): one a-trous level in float64 numpy, written from atrous_pixel of oracle/svgf_oracle.c (5x5 binomial taps, the
    three exponentials, the `wsum > 10e-6` fall-through, the variance output, the optional 3x3 variance blur) with a `taps` mask,
    the one thing the oracle cannot do.  It models the operation, not a kernel; it is for finite frames only.  Pinned to the
    oracle level by level with the mask full (MODEL_TOL, MODEL_TOL_VARIANCE); the same figure is the reference's own rounding noise on these frames,
    which test_coarse_levels_gpu.py's bar refers to.
  * the inputs.  Non-temporal: random_frame(W, 193, seed=70) with the colours cubed, sigma_l = 0.45, sigma_n = 0.2 and, for a
    target level k, sigma_x = 0.1 * 2^k (one parameter set per target level: SvgfParams has one sigma_x for the whole cascade).
    Temporal: two frames under a static camera with the ray-cast scene's G-buffer (temporal_frames()), so that the second frame
    has an accumulated history and a variance that differs from pixel to pixel.
  * the conditions on those inputs (below), asserted at every size the GPU module uses.  They are conditions on the inputs, not
    tolerances on a kernel: where an input misses one, the input is changed, never the threshold.
  * GEOMETRY: the sizes, with the strips / segments of both kernels at steps 8, 16 and 32 on a 256-CU device, held to the library
    (binding.atrous_geometry; host arithmetic, no device), and the coverage conditions over that table.

Conditions, for every target level k in 3, 4, 5 with its parameter set, at level k itself:
  * the level moves at least 90 % of all pixels by more than 1e-3, and at least 80 % of the pixels of every image row and of
    every image column by more than 1e-4 (seams run along rows: segments, and along columns: strips and chunks);
  * each of sigma_l, sigma_n, sigma_x raised 2 % at level k alone moves at least 50 % of the pixels by more than 1e-4, ten times
    the kernels' bar;
  * dropping the 16 outer-ring taps at level k alone moves at least 50 % of the pixels by more than 1e-3 (model_level's mask).
Temporal leg, levels 4 and 5: the 90 % condition; at least 50 % of the pixels with a history longer than 1; blur_variance toggled
at level k alone moves at least 25 % of the pixels by more than 1e-4; sigma_l raised 2 % at level k + 1 alone, the only reader of
the variance level k writes, moves at least 25 % by more than 1e-4.

The ray-cast scene as it is does not reach the temporal conditions: see temporal_frames() for the figures and for what is used."""
import ctypes as C

import numpy as np
import pytest

from conftest import relerr

H = 193     # 13 lattice rows at step 16 and 7 at step 32 (y-phase 0; the last y-phases have one row less)
# (W, H) -> {kernel: {step: (n_strips, seg_rows, n_segs)}} on a 256-CU device.  Lane strips at steps 16 / 32 are (chunk of 60
# lattice columns, group of 8 x-phases) pairs: n_strips = chunks * step / 8.
GEOMETRY = {
    # two 256-column strips of the strip kernel; one lane strip
    (257, H): {"lane": {8: (1, 4, 7), 16: (2, 4, 4), 32: (4, 4, 2)}, "strip": {8: (2, 8, 4), 16: (2, 8, 2), 32: (2, 8, 1)}},
    # one column past a 480-column lane strip, steps <= 8
    (481, H): {"lane": {8: (2, 4, 7), 16: (2, 4, 4), 32: (4, 4, 2)}, "strip": {8: (2, 8, 4), 16: (2, 8, 2), 32: (2, 8, 1)}},
    # 61 lattice columns at step 16: the seam between two 60-column chunks
    (961, H): {"lane": {8: (3, 4, 7), 16: (4, 4, 4), 32: (4, 4, 2)}, "strip": {8: (4, 8, 4), 16: (4, 8, 2), 32: (4, 8, 1)}},
    # the same seam at step 32; five 480-column strips
    (1921, H): {"lane": {8: (5, 5, 5), 16: (6, 7, 2), 32: (8, 7, 1)}, "strip": {8: (8, 8, 4), 16: (8, 8, 2), 32: (8, 8, 1)}},
}
SIZES = list(GEOMETRY)
STEPS = (8, 16, 32)
KERNELS = ("lane", "strip")
LANE_STRIP, LANE_CHUNK, LANE_GROUP, STRIP_TX = 480, 60, 8, 256      # svgf_atrous_geometry.h; strip_pick(): 256 columns everywhere

FRAME_SEED = 70
TARGETS = (3, 4, 5)
MIN_CHANGED, MIN_CHANGED_PER_LINE = 0.90, 0.80       # of all pixels by > 1e-3; of every row's and column's pixels by > 1e-4
MIN_SIGMA, SIGMA_UP = 0.50, 1.02                     # of all pixels by > 1e-4 for a sigma raised 2 % at the level alone
MIN_OUTER_RING = 0.50                                # of all pixels by > 1e-3 with the 16 outer taps dropped at the level alone
MIN_HISTORY, MIN_BLUR, MIN_NEXT_SIGMA_L = 0.50, 0.25, 0.25
# float32 oracle against the float64 model, one level from the same inputs.  Colour: a ratio of two float32 sums of 25 terms; the
# roundings of the weights are common to numerator and denominator and largely cancel, what is left is the accumulation of each sum
# (random walk of 25 roundings of 6e-8: 3e-7) and the division: 1e-6 bounds it.  Variance: the same with squared weights, whose
# relative error is twice a weight's, and no cancellation between var * w * w and w * w once the variance differs from tap to tap:
# 2e-6.  Measured (printed by the tests below): colour 5.4e-7 .. 7.6e-7, variance 3.9e-7 .. 1.4e-6.
MODEL_TOL, MODEL_TOL_VARIANCE = 1e-6, 2e-6

OUTER_RING = np.array([[abs(i) == 2 or abs(j) == 2 for j in range(-2, 3)] for i in range(-2, 3)])      # [i + 2, j + 2]


def size_id(size):
    return f"{size[0]}x{size[1]}"


def with_(params, **kw):
    """A copy of `params` with `kw` set (SvgfParams.set changes the structure in place)."""
    return type(params).from_buffer_copy(params).set(**kw)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------

def target_params(pkg, k, **kw):
    """The parameter set whose level k is looked at: sigma_x grows with the level's step, so that the position term of a tap one
    and two lattice steps away is O(1) at level k (random_frame's positions are 0.05 apart per pixel: 0.05 * 2^k / sigma_x = 0.5
    and 1.0), neither near 0 nor far below."""
    return pkg.reference_defaults().set(temporal_enable=0, spatial_enable=1, atrous_nlevel=k, history_level=k,
                                        sigma_l=0.45, sigma_n=0.2, sigma_x=0.1 * 2 ** k).set(**kw)


_frames = {}


def frame(pkg, W):
    """random_frame with the colours cubed: they spread about twice as wide around their mean (0 .. 8, mean 2, deviation 2.3),
    and what four levels leave of that keeps the luminance term O(1) against den_l = sqrt(10) 0.45.  Read-only, shared."""
    if W not in _frames:
        c, g = pkg.synth.random_frame(W, H, seed=FRAME_SEED)
        c = c ** 3
        c.setflags(write=False)
        g.setflags(write=False)
        _frames[W] = (c, g, pkg.synth.camera_for_frame(0, False))
    return _frames[W]


TEMPORAL_SIZE = (257, H)
TEMPORAL_TARGETS = (4, 5)
TEMPORAL_SIGMAS = dict(sigma_x=4.0, sigma_l=0.45, sigma_n=1.0)


def temporal_params(pkg, k, **kw):
    W, Ht = TEMPORAL_SIZE
    scale = (float(np.tan(np.radians(45.0)) * W / Ht), float(np.tan(np.radians(45.0))))
    return pkg.reference_defaults().set(temporal_enable=1, spatial_enable=1, atrous_nlevel=k, history_level=k, reproj_scale=scale,
                                        **TEMPORAL_SIGMAS).set(**kw)


_temporal = []


def temporal_frames(pkg):
    """Two frames under the static camera: the G-buffer of the ray-cast scene (render_frame(257, 193, seed=53): its positions
    reproject, random_frame's do not), with a background plane in place of the misses, and unstructured colours.

    The scene as it is misses the conditions.  At 257 x 193 with sigma_x = 2, sigma_l = 4, sigma_n = 1 (oracle): 38 % of the
    pixels are misses, which never get a history, and the reference's reprojection (no field of view, no aspect) finds a history
    for 37.8 % of the pixels (50 % asked); toggling blur_variance moves 18.9 % / 11.4 % of the pixels at levels 4 / 5 (25 % asked);
    sigma_l + 2 % moves 5.8 % at level 5 and 0.0 % at level 6 (25 % asked): the colours are smooth per surface, and the variance
    of a pixel without history is 100.  So
      * reproj_scale (temporal_params) makes the reprojection exact: every pixel finds its history;
      * misses: the texel of a miss is replaced by a plane behind the room (geomId 9, normal +z, z = -8 under the pixel's ray);
      * colours: frame 1 is random_frame's, cubed, 0.25 c^3 + 0.05; frame 2 is frame 1 times 1 +- (0.3 .. 0.7) per pixel.  The
        accumulated variance is then (l1 - l2)^2 / 4 with |l1 - l2| >= 0.3 l1: it differs from pixel to pixel over three decades
        (1e-4 .. 0.3) and stays away from 0, where den_l = sqrt(var) sigma_l + 1e-6 makes the luminance weight ill-conditioned in
        float32 (two independent draws: oracle vs float64 model up to 1.3e-5 in colour, 1.6e-4 in variance, with blur_variance 0).
    Read-only, shared."""
    if not _temporal:
        W, Ht = TEMPORAL_SIZE
        c1, _ = pkg.synth.random_frame(W, Ht, seed=FRAME_SEED + 10)
        c1 = (c1 ** 3 * np.float32(0.25) + np.float32(0.05)).astype(np.float32)
        rng = np.random.default_rng(FRAME_SEED + 11)
        sign = np.where(rng.random((Ht, W, 1)) < 0.5, -1.0, 1.0)
        c2 = (c1 * (1.0 + sign * (0.3 + 0.4 * rng.random((Ht, W, 1))))).astype(np.float32)
        for f, c in enumerate((c1, c2)):
            _, g, cam = pkg.synth.render_frame(W, Ht, f, seed=53, moving=False)
            g = g.copy()
            miss = g["geomId"] < 0
            eye = cam["position"].astype(np.float32)
            d = eye[None, :] - g["position"][miss]           # a miss stores eye - dir
            t = (np.float32(-8.0) - eye[2]) / d[:, 2]
            assert (t > 0).all()
            g["position"][miss] = eye[None, :] + t[:, None] * d
            g["normal"][miss] = np.array([0, 0, 1], np.float32)
            g["geomId"][miss] = 9
            assert np.isfinite(g["position"]).all()
            c.setflags(write=False)
            g.setflags(write=False)
            _temporal.append((c, g, cam))
    return _temporal


# ---- the oracle, one level at a time ------------------------------------------------------------------------------------------------

def oracle_level(pkg, orc, color, var, g, level, p, threads=16):
    """One level of the reference's ATrousFilter (svgf_oracle_atrous, snapshot variance): (colour, variance) out.  `level` is the
    1-based level of the reference's cascade (step 2^level).  No re-modulation."""
    lib = orc.load(pkg.SvgfCamera, pkg.SvgfParams)
    Hh, W = var.shape
    color = np.ascontiguousarray(color, dtype=np.float32)
    var = np.ascontiguousarray(var, dtype=np.float32)
    g = np.ascontiguousarray(g)
    assert color.shape == (Hh, W, 3) and g.nbytes == 52 * W * Hh and not p.paper_steps and not (p.sepcolor and p.addcolor)
    out, var_out = np.empty_like(color), np.empty_like(var)
    lib.svgf_oracle_atrous(color.ctypes.data, out.ctypes.data, var.ctypes.data, var_out.ctypes.data, g.ctypes.data, W, Hh, int(level), 0,
                           C.c_float(p.sigma_l), C.c_float(p.sigma_n), C.c_float(p.sigma_x), int(p.blur_variance), 0, 0, int(threads))
    return out, var_out


def cascade(pkg, orc, color, var, g, p, nlevel):
    """[(colour, variance) entering level 1, after level 1, ..., after level nlevel]: index k is the output of level k."""
    levels = [(np.ascontiguousarray(color, dtype=np.float32), np.ascontiguousarray(var, dtype=np.float32))]
    for k in range(1, nlevel + 1):
        levels.append(oracle_level(pkg, orc, *levels[-1], g, k, p))
    for c, v in levels:
        c.setflags(write=False)
        v.setflags(write=False)
    return levels


_cascades = {}


def frame_cascade(pkg, orc, W, k, nlevel=None, **kw):
    """The shared oracle cascade of the non-temporal frame of width W under target_params(k, **kw), levels 1 .. k + 1 (the GPU
    module compares level k + 1 as the reader of level k's variance).  Computed once per session, read-only."""
    key = (W, k, tuple(sorted(kw.items())))
    if key not in _cascades:
        c, g, _ = frame(pkg, W)
        _cascades[key] = cascade(pkg, orc, c, np.full((H, W), 10.0, np.float32), g, target_params(pkg, k, **kw), k + 1)
    return _cascades[key]


def temporal_state(pkg, orc, h, **kw):
    """(colour, variance) that enter level 1 of the second temporal frame (read_state(4), read_state(3)) and its history length,
    both frames run under temporal_params(h, **kw).  The state depends on h: the colour history the second frame blends with is
    the first frame's level h."""
    W, Ht = TEMPORAL_SIZE
    o = orc.Oracle(pkg, W, Ht, threads=16)
    for c, g, cam in temporal_frames(pkg):
        o.denoise(c, g, cam, temporal_params(pkg, h, **kw))
    state = o.read_state(4), o.read_state(3), o.read_state(0)
    o.free()
    return state


def temporal_cascade(pkg, orc, h, **kw):
    """Like frame_cascade for the temporal leg: levels 1 .. h + 1 of the second frame of a sequence run with history_level = h
    under temporal_params(h, **kw).  Level h is that run's colour history; level h + 1 is what atrous_nlevel = h + 1 returns."""
    key = ("temporal", h, tuple(sorted(kw.items())))
    if key not in _cascades:
        c, v, _ = temporal_state(pkg, orc, h, **kw)
        _cascades[key] = cascade(pkg, orc, c, v, temporal_frames(pkg)[1][1], temporal_params(pkg, h, **kw), h + 1)
    return _cascades[key]


# ---- one level in float64 -----------------------------------------------------------------------------------------------------------

def _shifted(a, dx, dy):
    """a[y + dy, x + dx] where that lies in the image (zeros elsewhere), and the mask of where it does."""
    Hh, W = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((Hh, W), dtype=bool)
    ys, yd = (slice(dy, Hh), slice(0, Hh - dy)) if dy >= 0 else (slice(0, Hh + dy), slice(-dy, Hh))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < Hh and abs(dx) < W:
        out[yd, xd] = a[ys, xs]
        ok[yd, xd] = True
    return out, ok


def model_level(color, var, g, step, sigma_l, sigma_n, sigma_x, blur_variance, taps=None):
    """One a-trous level of the reference in float64: (colour, variance) out.  taps[i + 2, j + 2] (i: x offset, j: y offset) says
    which of the 25 taps exist; None: all.  The parameters are taken as the float32 values the oracle gets."""
    f8 = np.float64
    color, var_in = np.asarray(color, f8), np.asarray(var, f8)
    nrm, pos = np.asarray(g["normal"], f8), np.asarray(g["position"], f8)
    taps = np.ones((5, 5), dtype=bool) if taps is None else np.asarray(taps, dtype=bool)
    if blur_variance:
        s, sw = np.zeros_like(var_in), np.zeros_like(var_in)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                v, ok = _shifted(var_in, dx, dy)
                gw = (2 - abs(dx)) * (2 - abs(dy)) / 16.0
                s += gw * v
                sw += gw * ok
        centre = np.maximum(s / sw, 0.0)
    else:
        centre = np.maximum(var_in, 0.0)
    lum = 0.2126 * color[..., 0] + 0.7152 * color[..., 1] + 0.0722 * color[..., 2]
    den_l = np.sqrt(centre) * f8(np.float32(sigma_l)) + 1e-6
    den_n, den_x = f8(np.float32(sigma_n)) + 1e-6, f8(np.float32(sigma_x)) + 1e-6
    binom = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    csum, vsum = np.zeros_like(color), np.zeros_like(var_in)
    wsum, w2sum = np.zeros_like(var_in), np.zeros_like(var_in)
    for i in range(-2, 3):
        for j in range(-2, 3):
            if not taps[i + 2, j + 2]:
                continue
            lq, ok = _shifted(lum, step * i, step * j)
            cq, _ = _shifted(color, step * i, step * j)
            vq, _ = _shifted(var_in, step * i, step * j)
            nq, _ = _shifted(nrm, step * i, step * j)
            pq, _ = _shifted(pos, step * i, step * j)
            wl = np.exp(-np.abs(lq - lum) / den_l)
            wn = np.minimum(1.0, np.exp(-np.sqrt(((nq - nrm) ** 2).sum(axis=2)) / den_n))
            wx = np.minimum(1.0, np.exp(-np.sqrt(((pq - pos) ** 2).sum(axis=2)) / den_x))
            w = np.where(ok, binom[i + 2] * binom[j + 2] * wl * wn * wx, 0.0)
            wsum += w
            w2sum += w * w
            csum += cq * w[..., None]
            vsum += vq * w * w
    keep = wsum > 10e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(keep[..., None], csum / wsum[..., None], color)
        var_out = np.where(keep, vsum / w2sum, var_in)
    return out, var_out


# ---- the conditions -----------------------------------------------------------------------------------------------------------------

def moved(cur, prev, bar):
    """Share of the pixels that differ by more than `bar` (relerr, maximum over the channels)."""
    return float((relerr(cur, prev).max(axis=2) > bar).mean())


def changed_fractions(cur, prev):
    """(share of all pixels that differ by more than 1e-3, smallest share over the image rows and over the image columns of pixels
    that differ by more than 1e-4)."""
    e = relerr(cur, prev).max(axis=2)
    return float((e > 1e-3).mean()), float((e > 1e-4).mean(axis=1).min()), float((e > 1e-4).mean(axis=0).min())


def assert_level_changes_the_frame(cur, prev, what):
    frac, row, col = changed_fractions(cur, prev)
    print(f"{what}: the level moves {100 * frac:.1f} % of the pixels by > 1e-3, at least {100 * row:.1f} % of every row and "
          f"{100 * col:.1f} % of every column by > 1e-4")
    assert frac >= MIN_CHANGED and row >= MIN_CHANGED_PER_LINE and col >= MIN_CHANGED_PER_LINE, \
        f"{what}: the level barely changes this frame ({frac:.3f} of the pixels, {row:.3f} / {col:.3f} of the weakest row / column): change the input"


def sigma_shares(pkg, orc, levels, g, p, k):
    """Share of the pixels that level k moves by more than 1e-4 when one sigma is raised 2 % at that level alone."""
    shares = {}
    for name in ("sigma_l", "sigma_n", "sigma_x"):
        out, _ = oracle_level(pkg, orc, *levels[k - 1], g, k, with_(p, **{name: getattr(p, name) * SIGMA_UP}))
        shares[name] = moved(out, levels[k][0], 1e-4)
    return shares


def outer_ring_share(levels, g, p, k):
    """(share of the pixels that level k moves by more than 1e-3 when its 16 outer taps are dropped; worst relerr of the oracle's
    level k against the model's with every tap, colour; the same for the variance)."""
    args = (*levels[k - 1], g, 1 << k, p.sigma_l, p.sigma_n, p.sigma_x, p.blur_variance)
    full, full_var = model_level(*args)
    inner, _ = model_level(*args, taps=~OUTER_RING)
    return moved(inner, full, 1e-3), float(relerr(levels[k][0], full).max()), float(relerr(levels[k][1][..., None], full_var[..., None]).max())


@pytest.mark.parametrize("k", TARGETS)
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_target_level_acts_on_the_frame(pkg, orc, size, k):
    """Level k of target_params(k) on frame(W): it moves the frame, every sigma acts, the outer ring acts."""
    W, _ = size
    _, g, _ = frame(pkg, W)
    p = target_params(pkg, k)
    levels = frame_cascade(pkg, orc, W, k)
    what = f"{W}x{H} level {k} (step {1 << k})"
    assert all(np.isfinite(c).all() and np.isfinite(v).all() for c, v in levels)
    assert_level_changes_the_frame(levels[k][0], levels[k - 1][0], what)
    shares = sigma_shares(pkg, orc, levels, g, p, k)
    print(f"{what}: +2 % at this level alone moves by > 1e-4: " + ", ".join(f"{n} {100 * s:.1f} %" for n, s in shares.items()))
    assert all(s >= MIN_SIGMA for s in shares.values()), f"{what}: a sigma does not act: {shares}: change the input"
    ring, model_err, model_err_var = outer_ring_share(levels, g, p, k)
    print(f"{what}: without the 16 outer taps {100 * ring:.1f} % of the pixels move by > 1e-3; oracle vs float64 model {model_err:.2e} "
          f"(variance {model_err_var:.2e})")
    assert ring >= MIN_OUTER_RING, f"{what}: the outer ring does not act ({ring:.3f}): change the input"
    assert model_err <= MODEL_TOL and model_err_var <= MODEL_TOL_VARIANCE, f"{what}: oracle vs model {model_err:.3e}, variance {model_err_var:.3e}"


@pytest.mark.parametrize("k", TEMPORAL_TARGETS)
def test_target_level_acts_on_the_temporal_frames(pkg, orc, k):
    """Level k of the second temporal frame: it moves the frame, the history is an accumulated one, the 3x3 variance blur acts at
    level k, and level k + 1's luminance weight reads the variance level k wrote."""
    W, Ht = TEMPORAL_SIZE
    g = temporal_frames(pkg)[1][1]
    what = f"{W}x{Ht} temporal, frame 2, level {k}"
    _, var0, hlen = temporal_state(pkg, orc, k)
    accumulated = float((hlen > 1).mean())
    print(f"{what}: {100 * accumulated:.1f} % of the pixels have a history longer than 1; variance entering level 1: "
          f"median {np.median(var0):.3g}, 10th / 90th percentile {np.percentile(var0, 10):.3g} / {np.percentile(var0, 90):.3g}")
    assert accumulated >= MIN_HISTORY
    for bv in (1, 0):
        p = temporal_params(pkg, k, blur_variance=bv)
        levels = temporal_cascade(pkg, orc, k, blur_variance=bv)
        assert all(np.isfinite(c).all() and np.isfinite(v).all() for c, v in levels)
        assert_level_changes_the_frame(levels[k][0], levels[k - 1][0], f"{what}, blur_variance {bv}")
        v = levels[k][1]
        print(f"{what}, blur_variance {bv}: variance the level writes: 10th / 50th / 90th percentile "
              f"{np.percentile(v, 10):.3g} / {np.median(v):.3g} / {np.percentile(v, 90):.3g}")
        toggled, _ = oracle_level(pkg, orc, *levels[k - 1], g, k, with_(p, blur_variance=1 - bv))
        blur = moved(toggled, levels[k][0], 1e-4)
        raised, _ = oracle_level(pkg, orc, *levels[k], g, k + 1, with_(p, sigma_l=p.sigma_l * SIGMA_UP))
        nxt = moved(raised, levels[k + 1][0], 1e-4)
        print(f"{what}, blur_variance {bv}: toggling blur_variance at this level alone moves {100 * blur:.1f} % of the pixels by > 1e-4; "
              f"sigma_l + 2 % at level {k + 1} alone {100 * nxt:.1f} %")
        assert blur >= MIN_BLUR, f"{what}: the variance blur does not act ({blur:.3f}): change the input"
        assert nxt >= MIN_NEXT_SIGMA_L, f"{what}: level {k + 1} does not read the variance ({nxt:.3f}): change the input"
        full, full_var = model_level(*levels[k - 1], g, 1 << k, p.sigma_l, p.sigma_n, p.sigma_x, bv)
        err, err_var = float(relerr(levels[k][0], full).max()), float(relerr(v[..., None], full_var[..., None]).max())
        print(f"{what}, blur_variance {bv}: oracle vs float64 model {err:.2e} (variance {err_var:.2e})")
        assert err <= MODEL_TOL and err_var <= MODEL_TOL_VARIANCE, f"{what}: oracle vs model {err:.3e}, variance {err_var:.3e}"


# ---- the helpers, pinned ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", TARGETS)
def test_cascade_is_the_oracles_cascade_bit_for_bit(pkg, orc, k):
    """Every level of cascade() equals Oracle.denoise's colour history with atrous_nlevel = history_level = that level."""
    W = SIZES[0][0]
    c, g, cam = frame(pkg, W)
    levels = frame_cascade(pkg, orc, W, k)
    o = orc.Oracle(pkg, W, H, threads=16)
    for n in range(1, k + 2):
        o.reset()
        out = o.denoise(c, g, cam, target_params(pkg, k, atrous_nlevel=n, history_level=n))
        assert np.array_equal(o.read_state(2), levels[n][0]) and np.array_equal(out, levels[n][0]), f"target {k}: level {n} differs"
    o.free()


@pytest.mark.parametrize("bv", [1, 0], ids=["blur", "noblur"])
def test_temporal_cascade_is_the_oracles_cascade_bit_for_bit(pkg, orc, bv):
    """For every history_level h: level h of temporal_cascade(h) is the colour history of the sequence, as the last level
    (atrous_nlevel = h) and as an inner one (atrous_nlevel = h + 1, which returns level h + 1), and its input is the state."""
    W, Ht = TEMPORAL_SIZE
    o = orc.Oracle(pkg, W, Ht, threads=16)
    for h in range(1, TEMPORAL_TARGETS[-1] + 1):
        levels = temporal_cascade(pkg, orc, h, blur_variance=bv)
        for n in (h, h + 1):
            o.reset()
            for c, g, cam in temporal_frames(pkg):
                out = o.denoise(c, g, cam, temporal_params(pkg, h, atrous_nlevel=n, blur_variance=bv))
            assert np.array_equal(o.read_state(2), levels[h][0]), f"blur_variance {bv}, history_level {h} of {n} levels"
            assert np.array_equal(out, levels[n][0]), f"blur_variance {bv}, history_level {h}: the image of {n} levels"
            assert np.array_equal(o.read_state(4), levels[0][0]) and np.array_equal(o.read_state(3), levels[0][1])
    o.free()


def test_model_matches_the_oracle_level_by_level(pkg, orc):
    """model_level with every tap against the oracle at every level of one cascade, colour and variance (the variance stays 10.0
    here: test_target_level_acts_on_the_temporal_frames holds the model to the oracle on a variance that differs from pixel to
    pixel, with and without the 3x3 blur); and the model's own edge cases: a mask of the centre alone, the fall-through of a pixel
    without weight."""
    W = SIZES[0][0]
    _, g, _ = frame(pkg, W)
    k = TARGETS[-1]
    p = target_params(pkg, k)
    levels = frame_cascade(pkg, orc, W, k)
    for n in range(1, k + 2):
        full, full_var = model_level(*levels[n - 1], g, 1 << n, p.sigma_l, p.sigma_n, p.sigma_x, p.blur_variance)
        e, ev = float(relerr(levels[n][0], full).max()), float(relerr(levels[n][1][..., None], full_var[..., None]).max())
        print(f"{W}x{H} level {n}: oracle vs float64 model {e:.2e}, variance {ev:.2e}")
        assert e <= MODEL_TOL and ev <= MODEL_TOL_VARIANCE
    # the centre tap alone: its weight is h(0, 0), the pixel and its variance come back
    centre = np.zeros((5, 5), dtype=bool)
    centre[2, 2] = True
    out, var = model_level(*levels[0], g, 32, p.sigma_l, p.sigma_n, p.sigma_x, 0, taps=centre)
    assert np.allclose(out, levels[0][0], rtol=1e-14, atol=0) and np.allclose(var, 10.0, rtol=1e-14)
    # no tap at all: wsum = 0 is not > 10e-6, the pixel and its variance fall through unchanged — as the oracle does for a pixel
    # whose every weight underflows (sigma_x tiny: the centre's own weight stays h(0, 0) = 0.14, so the oracle cannot show it)
    out, var = model_level(*levels[0], g, 32, p.sigma_l, p.sigma_n, p.sigma_x, 0, taps=np.zeros((5, 5), dtype=bool))
    assert np.array_equal(out, levels[0][0]) and np.array_equal(var, levels[0][1])


# ---- the sizes ----------------------------------------------------------------------------------------------------------------------

def lattice_rows(step):
    return (H + step - 1) // step


def lane_chunks(W, step):
    """Chunks of 60 lattice columns, groups of 8 x-phases (steps 16 and 32)."""
    return ((W + step - 1) // step + LANE_CHUNK - 1) // LANE_CHUNK, step // LANE_GROUP


@pytest.mark.experiments
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_table_is_the_geometry_the_library_launches(pkg, size):
    W, Ht = size
    for kernel in KERNELS:
        for step in STEPS:
            out, est = pkg.binding.atrous_geometry(kernel, W, Ht, step)
            supported, n_strips, seg_rows, n_segs, n_groups, grid, threads, lds = out
            assert supported and est is not None and est > 0, f"{W}x{Ht} {kernel} step {step}"
            assert (n_strips, seg_rows, n_segs) == GEOMETRY[size][kernel][step], f"{W}x{Ht} {kernel} step {step}: library {(n_strips, seg_rows, n_segs)}"
            # the segments cover the phase, none is empty; the strips are what this module's coordinates assume
            assert (n_segs - 1) * seg_rows < lattice_rows(step) <= n_segs * seg_rows and n_groups == step * n_segs
            if kernel == "strip":
                assert n_strips == (W + STRIP_TX - 1) // STRIP_TX
            elif step <= 8:
                assert n_strips == (W + LANE_STRIP - 1) // LANE_STRIP
            else:
                chunks, groups = lane_chunks(W, step)
                assert n_strips == chunks * groups


def test_table_covers_every_path_of_the_kernels():
    coarse = (16, 32)
    for kernel in KERNELS:
        rec = {(size, step): GEOMETRY[size][kernel][step] for size in SIZES for step in STEPS}
        assert any(n > 1 for (_, step), (n, _, _) in rec.items() if step <= 8), f"{kernel}: several strips at a step <= 8"
        for step in coarse:
            assert any(n > 1 for (_, s), (n, _, _) in rec.items() if s == step), f"{kernel}: several strips at step {step}"
    # strip kernel: strips of 256 pixel columns whatever the step; a last strip narrower than the others
    assert any(W % STRIP_TX for W, _ in SIZES) and any(W > STRIP_TX for W, _ in SIZES)
    # lane kernel, steps <= 8: 480-column strips, a last one narrower
    assert any(W > LANE_STRIP and W % LANE_STRIP for W, _ in SIZES)
    for step in coarse:
        chunks = {W: lane_chunks(W, step) for W, _ in SIZES}
        assert any(c > 1 for c, _ in chunks.values()), f"lane, step {step}: several chunks of {LANE_CHUNK} lattice columns"
        assert all(grp > 1 for _, grp in chunks.values()), f"lane, step {step}: several groups of {LANE_GROUP} x-phases"
        assert any(c > 1 and ((W + step - 1) // step) % LANE_CHUNK for W, (c, _) in chunks.items()), f"lane, step {step}: a narrower last chunk"
        # the last lattice column ends inside a group of x-phases: the group's later phases are one column narrower
        assert any(c > 1 and (W % step) % LANE_GROUP for W, (c, _) in chunks.items()), f"lane, step {step}: a group with narrower phases"
        # y-phases of unequal length
        assert H % step
    # segments of the library's own choosing at the coarse steps (a 256-CU device): the lane kernel cuts the 13 lattice rows of
    # step 16 into four segments of 4 or two of 7 and the 7 rows of step 32 into two of 4 at the three smaller sizes; the strip
    # kernel cuts step 16 into two of 8.  At step 32 the strip kernel's search does not go below 8 rows (2 rows x 4), and 7 rows
    # are one segment at any width; the lane kernel keeps one segment of 7 at 1921 columns.  The forced segment lengths of
    # test_coarse_levels_gpu.py cover those seams.
    for kernel, step in (("lane", 16), ("lane", 32), ("strip", 16)):
        assert any(GEOMETRY[size][kernel][step][2] > 1 for size in SIZES), f"{kernel}, step {step}: several segments"
    assert all(GEOMETRY[size]["strip"][32][2] == 1 for size in SIZES) and GEOMETRY[(1921, H)]["lane"][32][2] == 1
