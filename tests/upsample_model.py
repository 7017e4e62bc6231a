"""The float32 numpy model of guided upsampling (include/svgf.h: svgf_upsample; csrc/svgf_upsample.hip: k_upsample) - the yardstick
of tests/test_upsample.py.  Test infrastructure only; not part of the package.

numpy rounds every array operation to float32 and never contracts a multiply and an add; sums are written as the kernel's
sequences of additions, in its order (taps k = 0..3)."""
import numpy as np

F = np.float32
PASS_A, PASS_B, PASS_C, PASS_NONE = 0, 1, 2, 3


def coords(n_hi, n_lo):
    """Per hi index: (floor of the lo coordinate as int64, fraction float32): u = ((float)i + 0.5f) * r - 0.5f, r = (float)n_lo / (float)n_hi."""
    r = F(n_lo) / F(n_hi)
    u = (np.arange(n_hi).astype(F) + F(0.5)) * r - F(0.5)
    f = np.floor(u)
    return f.astype(np.int64), (u - f).astype(F)


def _sums(rgb_lo, lo, hi, sigma_n, sigma_x):
    """The three passes' (acc float32[H, W, 3], sumw float32[H, W])."""
    Hl, Wl = lo.shape
    Hh, Wh = hi.shape
    rgb_lo = np.asarray(rgb_lo, F).reshape(Hl, Wl, 3)
    sn, sx = F(sigma_n), F(sigma_x)
    fx, ax = coords(Wh, Wl)
    fy, ay = coords(Hh, Hl)
    fx, ax, fy, ay = fx[None, :], ax[None, :], fy[:, None], ay[:, None]
    one = F(1)
    wb = [(one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay]
    g, n, p = hi["geomId"], hi["normal"], hi["position"]
    S = [[np.zeros((Hh, Wh, 3), F), np.zeros((Hh, Wh), F)] for _ in range(3)]

    def add(s, counted, w, c):
        s[0] = np.where(counted[..., None], s[0] + w[..., None] * c, s[0])
        s[1] = np.where(counted, s[1] + w, s[1])

    for k in range(4):
        tx, ty = fx + (k & 1), fy + (k >> 1)
        inside = np.broadcast_to((tx >= 0) & (tx < Wl) & (ty >= 0) & (ty < Hl), (Hh, Wh))
        qx, qy = np.broadcast_to(np.clip(tx, 0, Wl - 1), (Hh, Wh)), np.broadcast_to(np.clip(ty, 0, Hl - 1), (Hh, Wh))
        t = lo[qy, qx]
        c = rgb_lo[qy, qx]
        w = np.broadcast_to(wb[k], (Hh, Wh)).astype(F)
        same = inside & (t["geomId"] == g)
        wa = w
        if sn > 0:
            d = t["normal"] - n
            s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            e = one - np.sqrt(s) / sn
            wa = wa * np.where(e > 0, e, F(0))
        if sx > 0:
            d = t["position"] - p
            s = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
            e = one - np.abs(s) / sx
            wa = wa * np.where(e > 0, e, F(0))
        wa = np.where(g != -1, wa, w).astype(F)
        add(S[0], same, wa, c)
        add(S[1], same, w, c)
        add(S[2], inside, w, c)
    return S


def upsample(rgb_lo, lo, hi, sigma_n, sigma_x, modulate):
    """rgb_lo float32[Hl, Wl, 3]; lo, hi: synth.GBUFFER_DTYPE[H, W] (a planar guide holds the same values; its albedo plane is
    albedo * ialbedo rounded to float32, which is what the AoS side multiplies by).  Returns (out float32[Hh, Wh, 3], the pass each
    pixel took int8[Hh, Wh]: PASS_A / PASS_B / PASS_C / PASS_NONE)."""
    with np.errstate(all="ignore"):
        S = _sums(rgb_lo, lo, hi, sigma_n, sigma_x)
        out = np.zeros(hi.shape + (3,), F)
        took = np.full(hi.shape, PASS_NONE, np.int8)
        for which in (PASS_C, PASS_B, PASS_A):      # the earliest accepting pass wins: written last
            acc, sumw = S[which]
            ok = sumw.astype(np.float64) >= 0.01      # NaN fails
            out = np.where(ok[..., None], acc / sumw[..., None], out)
            took = np.where(ok, np.int8(which), took)
        if modulate:
            out = out * (hi["albedo"] * hi["ialbedo"]).astype(F)
    return out.astype(F), took.astype(np.int8)


def bilinear(rgb_lo, lo_shape, hi_shape):
    """The plain bilinear stretch the feature is measured against: pass C alone."""
    lo = np.zeros(lo_shape, [("normal", "<f4", 3), ("position", "<f4", 3), ("geomId", "<i4")])
    hi = np.zeros(hi_shape, lo.dtype)
    with np.errstate(all="ignore"):
        acc, sumw = _sums(rgb_lo, lo, hi, 0.0, 0.0)[2]
        return (acc / sumw[..., None]).astype(F)


def nearest_lo(hi, Wl, Hl):
    """The lo G-buffer of the GPU tests: the hi texel nearest each lo pixel centre."""
    Hh, Wh = hi.shape
    xs = np.minimum(((np.arange(Wl) + 0.5) * Wh / Wl).astype(np.int64), Wh - 1)
    ys = np.minimum(((np.arange(Hl) + 0.5) * Hh / Hl).astype(np.int64), Hh - 1)
    return np.ascontiguousarray(hi[ys[:, None], xs[None, :]])
