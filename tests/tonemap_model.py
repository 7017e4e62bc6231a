"""Numpy model of row f12 (include/svgf.h: svgf_exposure_reset, svgf_exposure_meter, svgf_display_tonemap,
svgf_tonemap_srgb_table): the normative arithmetic restated operation by operation.  Floats are float32 (numpy rounds every
elementwise operation once and fuses nothing), the luminance is the library's double sum, everything else is integer arithmetic in
Python ints.  No transcendental is evaluated anywhere but in srgb_table(), which is the DEFINITION of the committed literals.
Test infrastructure only; not part of the package."""
import numpy as np

F = np.float32
STATE_WORDS = 520
N, M, LBITS, TARGET, EXPOSURE, COUNT = 512, 513, 514, 515, 516, 517
ONE_BITS = 0x3F800000


def as_float(word):
    return np.array([word], dtype=np.uint32).view(F)[0]


def as_bits(x):
    return int(np.array([x], dtype=F).view(np.uint32)[0])


def luminance(rgb):
    """svgf_lum_strict: (float)((0.2126 (double)r + 0.7152 (double)g) + 0.0722 (double)b)"""
    d = np.asarray(rgb, dtype=F).astype(np.float64)
    with np.errstate(all="ignore"):
        l = 0.2126 * d[..., 0] + 0.7152 * d[..., 1]
        l = l + 0.0722 * d[..., 2]
        return l.astype(F)


def counted(L):
    return (L == L) & (L > 0) & (L < np.inf)


def bins_of(L):
    """bin of every COUNTED luminance (callers filter with counted())"""
    bits = np.ascontiguousarray(L, dtype=F).view(np.uint32)
    return np.clip((bits >> 20).astype(np.int64) - 888, 0, 255)


def histogram(rgb):
    L = luminance(rgb).reshape(-1)
    return np.bincount(bins_of(L[counted(L)]), minlength=256).astype(np.int64)


def reset():
    s = np.zeros(STATE_WORDS, dtype=np.uint32)
    s[TARGET] = s[EXPOSURE] = ONE_BITS
    return s


def meter(state, rgb, key=0.18, trim_low_1024=51, trim_high_1024=51, min_exposure=1.0 / 64.0, max_exposure=64.0, adapt=1.0):
    """Both launches of svgf_exposure_meter; returns the new 520 words (the argument is not changed)."""
    key, lo_e, hi_e, adapt = F(key), F(min_exposure), F(max_exposure), F(adapt)
    h = state[:256].astype(np.int64) + histogram(rgb)
    n = int(h.sum())
    lo, hi = (n * int(trim_low_1024)) >> 10, (n * int(trim_high_1024)) >> 10
    P = np.concatenate([[0], np.cumsum(h)])
    c = np.maximum(0, np.minimum(P[1:], n - hi) - np.maximum(P[:-1], lo))
    m = int(c.sum())
    count, prev = int(state[COUNT]), as_float(state[EXPOSURE])
    if m > 0:
        S = sum(int(c[b]) * (2 * (888 + b) + 1) for b in range(256))
        lbits = (((S << 19) + (m >> 1)) // m) & 0xFFFFFFFF
        t = key / as_float(lbits)
        if t < lo_e:
            t = lo_e
        if t > hi_e:
            t = hi_e
    else:
        lbits = 0
        t = prev if count > 0 else F(1.0)
    with np.errstate(all="ignore"):
        e = t if count == 0 else prev + ((t - prev) * adapt)
    out = np.zeros(STATE_WORDS, dtype=np.uint32)
    out[256:512] = h
    out[N], out[M], out[LBITS] = n, m, lbits
    out[TARGET], out[EXPOSURE] = as_bits(t), as_bits(e)
    out[COUNT] = min(count + 1, 2 ** 31 - 1)
    return out


def srgb_table():
    """T[k]: the float32 nearest to the sRGB decode of k / 255, computed in double"""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(F)


def to_byte(y):
    """svgf_display_pack's conversion: clamp((int)((double)y * 255.0), 0, 255), saturating, NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = y.astype(np.float64) * 255.0
        i = np.where(np.isnan(d), 0.0, np.clip(d, -1e9, 1e9)).astype(np.int64)
    return np.clip(i, 0, 255).astype(np.uint8)


def tonemap_bytes(v, e, op, transfer, iw2, table):
    v, e, iw2 = np.asarray(v, dtype=F), F(e), F(iw2)
    with np.errstate(all="ignore"):
        x = v * e
        if op == 0:
            y = x
        else:
            x = np.where(x > F(0), x, F(0))
            x = np.where(x > F(65504.0), F(65504.0), x)
            if op == 1:
                y = (x * (F(1.0) + x * iw2)) / (F(1.0) + x)
            else:
                y = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
        assert y.dtype == F
        if transfer == 2:
            # #{k in 1..255 : y >= T[k]}: T is increasing, so a sorted search counts them; a NaN is >= nothing
            return np.where(np.isnan(y), 0, np.searchsorted(table[1:], y, side="right")).astype(np.uint8)
        if transfer == 1:
            y = np.sqrt(y)
        return to_byte(y)


def display_tonemap(left, right, op, transfer, exposure_bias=1.0, white=0.0, state=None, table=None):
    """svgf_display_tonemap: (H, 2W, 4) uint8, or (H, W, 4) when left is None"""
    table = srgb_table() if table is None else table
    bias, white = F(exposure_bias), F(white)
    with np.errstate(all="ignore"):
        e = bias * as_float(state[EXPOSURE]) if state is not None else bias
        iw2 = F(1.0) / (white * white) if white > 0 else F(0.0)
    h, w = right.shape[:2]
    out = np.zeros((h, (1 if left is None else 2) * w, 4), dtype=np.uint8)
    if left is not None:
        out[:, :w, :3] = tonemap_bytes(left, e, op, transfer, iw2, table)
    out[:, -w:, :3] = tonemap_bytes(right, e, op, transfer, iw2, table)
    return out
