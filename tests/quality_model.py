"""numpy model of svgf_quality_meter / svgf_quality_read (include/svgf.h row f13): the normative arithmetic statement by statement,
float32 where the header says float32 and float64 elsewhere, in the header's order of additions inside a row, a cell and a window.
The two totals sum_se and sum_ssim are the EXACT sums of the per-pixel / per-window doubles (math.fsum), which is what the header's
bound n 2^-52 sum |term| is stated against; counts, max_abs, min_ssim and both maps are exact."""
import math

import numpy as np

F = np.float32
D = np.float64
NAN_BITS = 0x7FC00000
EXPOSURE_WORD = 516


def windows(d):
    return (d - 8) // 4 + 1 if d >= 8 else 0


def luminance(rgb):
    """the library's luminance: (float)((0.2126 (double)r + 0.7152 (double)g) + 0.0722 (double)b)"""
    r, g, b = (rgb[..., c].astype(D) for c in range(3))
    return ((0.2126 * r + 0.7152 * g) + 0.0722 * b).astype(F)


def effective_scale(scale, exposure_words=None):
    """e = scale, or scale * as_float(word[516]) in float32"""
    if exposure_words is None:
        return F(scale)
    return F(F(scale) * np.asarray(exposure_words, dtype=np.uint32)[EXPOSURE_WORD:EXPOSURE_WORD + 1].view(F)[0])


def _nan_where(values, keep):
    out = values.astype(F).view(np.uint32).copy()
    out[~keep] = NAN_BITS
    return out.view(F)


def meter(a, b, peak=1.0, scale=1.0, clamp=0, exposure_words=None):
    """-> dict: n_pixels, n_windows, sum_se, sum_ssim (exact sums), abs_se, abs_ssim (sum of |term|, for the bound), max_abs, min_ssim,
    peak, scale (the effective one), mse, psnr_db, mean_ssim, se_map (H, W) float32, ssim_map (nwy, nwx) float32, ssim (nwy, nwx)
    float64 and counted_windows (nwy, nwx) bool."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    assert a.shape == b.shape and a.ndim == 3 and a.shape[2] == 3
    H, W = a.shape[:2]
    peak, e = F(peak), effective_scale(scale, exposure_words)
    with np.errstate(all="ignore"):
        ta, tb = (a * e).astype(F), (b * e).astype(F)
        counted = np.isfinite(ta).all(axis=2) & np.isfinite(tb).all(axis=2)
        if clamp:
            def clamped(t):
                t = t.copy()
                t[t < 0] = F(0)
                t[t > peak] = peak
                return t
            ta, tb = clamped(ta), clamped(tb)
        d = ta.astype(D) - tb.astype(D)
        se = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        La, Lb = luminance(ta).astype(D), luminance(tb).astype(D)
        se_map = _nan_where(se, counted)

        n_pixels = int(counted.sum())
        terms = se[counted]
        sum_se, abs_se = math.fsum(terms), math.fsum(np.abs(terms))
        max_abs = float(np.abs(d[counted]).max()) if n_pixels else 0.0

        nwx, nwy = windows(W), windows(H)
        ssim = np.zeros((nwy, nwx), D)
        win_counted = np.zeros((nwy, nwx), bool)
        if nwx and nwy:
            cx, cy = nwx + 1, nwy + 1      # the cells the windows use

            def cells(v):
                v = v[:4 * cy, :4 * cx].reshape(cy, 4, cx, 4)
                row = ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]             # (cy, 4, cx)
                return ((row[:, 0] + row[:, 1]) + row[:, 2]) + row[:, 3]            # (cy, cx)

            def window(c):                                                          # c[y, x]: ((c00 + c10) + c01) + c11, cells c[x][y]
                return ((c[:-1, :-1] + c[:-1, 1:]) + c[1:, :-1]) + c[1:, 1:]

            sa, sb, saa, sbb, sab = (window(cells(v)) for v in (La, Lb, La * La, Lb * Lb, La * Lb))
            cell_ok = counted[:4 * cy, :4 * cx].reshape(cy, 4, cx, 4).all(axis=(1, 3))
            win_counted = cell_ok[:-1, :-1] & cell_ok[:-1, 1:] & cell_ok[1:, :-1] & cell_ok[1:, 1:]
            k = 0.015625
            ma, mb = sa * k, sb * k
            va, vb, cv = saa * k - ma * ma, sbb * k - mb * mb, sab * k - ma * mb
            c1, c2 = 0.01 * D(peak), 0.03 * D(peak)
            C1, C2 = c1 * c1, c2 * c2
            ssim = ((2.0 * ma * mb + C1) * (2.0 * cv + C2)) / (((ma * ma + mb * mb) + C1) * ((va + vb) + C2))
        ssim_map = _nan_where(ssim, win_counted)
        n_windows = int(win_counted.sum())
        wterms = ssim[win_counted]
        sum_ssim, abs_ssim = math.fsum(wterms), math.fsum(np.abs(wterms))
        min_ssim = float(wterms.min()) if n_windows else math.inf

        mse = sum_se / (3.0 * n_pixels) if n_pixels else math.nan
        if not n_pixels:
            psnr = math.nan
        elif mse == 0.0:
            psnr = math.inf
        else:
            psnr = 10.0 * math.log10(float(D(peak) * D(peak)) / mse)
        mean_ssim = sum_ssim / n_windows if n_windows else math.nan
    return dict(n_pixels=n_pixels, n_windows=n_windows, sum_se=sum_se, sum_ssim=sum_ssim, abs_se=abs_se, abs_ssim=abs_ssim,
                max_abs=max_abs, min_ssim=min_ssim, peak=float(D(peak)), scale=float(D(e)), mse=mse, psnr_db=psnr, mean_ssim=mean_ssim,
                se_map=se_map, ssim_map=ssim_map, ssim=ssim, counted_windows=win_counted)
