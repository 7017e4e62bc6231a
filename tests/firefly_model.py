"""The float32 numpy model of the firefly filter (include/svgf.h: svgf_set_firefly_filter; csrc/svgf_temporal.h:
svgf_firefly_filter) — the yardstick of tests/test_firefly_filter.py.  Test infrastructure only; not part of the package.

The statement of the feature is that a frame runs exactly as if in_rgb had been F(in_rgb), so the model of a filtered frame
is tests/temporal_model.py fed firefly_filter(colour): nothing of that model is repeated here.

numpy rounds every array operation to float32 and never contracts; the luminance is temporal_model.luminance (double
promotion, rounded to float), the division is correctly rounded on both sides, and the list of the largest neighbour
luminances is built by the header's own swap sequence, so +-0 and ties select the same bits as the kernel's."""
import numpy as np

import temporal_model as tm

F = np.float32


def firefly_filter(color, rank, scale):
    """F(color): color float32[H, W, 3]; rank 0 returns the image as it is, 1..3 filter; scale finite and >= 0."""
    color = np.asarray(color, dtype=F)
    if rank == 0:
        return color.copy()
    assert 1 <= rank <= 3 and color.ndim == 3
    H, W = color.shape[:2]
    lum = tm.luminance(color)
    inside = np.ones((H, W), bool)
    t = [np.full((H, W), -np.inf, F) for _ in range(rank)]
    n = np.zeros((H, W), np.int32)
    with np.errstate(all="ignore"):
        for yy in (-1, 0, 1):
            for xx in (-1, 0, 1):
                if xx == 0 and yy == 0:
                    continue
                v = tm._shifted(lum, yy, xx)
                ok = tm._shifted(inside, yy, xx, False) & ~np.isnan(v)
                n = n + ok
                for j in range(rank):
                    sw = ok & (v > t[j])
                    t[j], v = np.where(sw, v, t[j]), np.where(sw, t[j], v)
        k = np.minimum(rank, n)
        B = t[0]
        for j in range(1, rank):
            B = np.where(k == j + 1, t[j], B)
        bound = (F(scale) * B).astype(F)
        act = (n > 0) & (lum > bound)
        s = (bound / lum).astype(F)
        return np.where(act[..., None], color * s[..., None], color).astype(F)
