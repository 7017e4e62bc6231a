"""The float32 numpy model of the output pass (include/svgf.h: svgf_set_output_taa; csrc/svgf_kernels.hip: k_output_taa) — the
yardstick of tests/test_output_taa.py.  Test infrastructure only; not part of the package.

One frame: the image C the frame would have written, this frame's geomId, the PREV_COORD_F32 plane the history is looked up at
(temporal_model.coord_plane of the call's motion plane, or temporal_model.motion_plane(..., COORD): the camera path's own
projection), the previous frame's (output, geomId) or None, alpha and sigma_scale.  numpy rounds every array operation to float32
and never contracts a multiply and an add; sums are written as the kernel's sequences of additions, in its order; the clip's
window statistics are temporal_model.clamp_box, the history clamp's."""
import numpy as np

import temporal_model as tm

F = np.float32


def output_taa(C, gid, coord, prev, alpha, k):
    """C float32[H, W, 3]; gid int32[H, W]; coord float32[H, W, 2]; prev: (colour float32[H, W, 3], gid int32[H, W]) or None.
    Returns (o, (o, gid)): the output and the history the next frame reads."""
    C, gid = np.asarray(C, F), np.asarray(gid, np.int32)
    if prev is None:
        o = C.copy()
        return o, (o, gid.copy())
    with np.errstate(all="ignore"):
        o, _ = _blend(C, gid, np.asarray(coord, F), np.asarray(prev[0], F), np.asarray(prev[1], np.int32), F(alpha), F(k))
    return o, (o, gid.copy())


def has_history(C, gid, coord, prev, alpha, k):
    """The pixels that blend (steps 1 to 3 found a history); for tests that say where "no history" must result."""
    if prev is None:
        return np.zeros(np.asarray(gid).shape, bool)
    with np.errstate(all="ignore"):
        return _blend(np.asarray(C, F), np.asarray(gid, np.int32), np.asarray(coord, F), np.asarray(prev[0], F),
                      np.asarray(prev[1], np.int32), F(alpha), F(k))[1]


def _blend(C, gid, coord, p_col, p_gid, alpha, k):
    H, W = gid.shape
    px, py = coord[..., 0], coord[..., 1]
    fx, fy = np.floor(px), np.floor(py)
    fracx, fracy = px - fx, py - fy
    on_screen = (fx >= 0) & (fy >= 0) & (fx < F(W)) & (fy < F(H))      # false for NaN
    p_col, p_gid = p_col.reshape(-1, 3), p_gid.reshape(-1)
    w = [(F(1) - fracx) * (F(1) - fracy), fracx * (F(1) - fracy), (F(1) - fracx) * fracy, fracx * fracy]
    h, sumw = np.zeros((H, W, 3), F), np.zeros((H, W), F)
    for wk, (dx, dy) in zip(w, [(0, 0), (1, 0), (0, 1), (1, 1)]):
        qx, qy = fx + F(dx), fy + F(dy)
        ok = ~np.isnan(qx) & ~np.isnan(qy) & (qx >= 0) & (qx < F(W)) & (qy >= 0) & (qy < F(H))      # svgf_tap_index
        idx = np.where(ok, np.where(ok, qx, 0).astype(np.int64) + np.where(ok, qy, 0).astype(np.int64) * W, 0)
        counted = ok & (p_gid[idx] == gid)
        h = np.where(counted[..., None], h + wk[..., None] * p_col[idx], h)
        sumw = np.where(counted, sumw + wk, sumw)
    have = (gid != -1) & on_screen & (sumw.astype(np.float64) >= 0.01)
    h = h / sumw[..., None]
    m, q, n = tm.clamp_box(C, 1)                                         # svgf_history_clamp<1>: comparisons, NaN leaves h as it is
    sd = np.sqrt(q / n[..., None])
    ksd = k * sd
    lo, hi = m - ksd, m + ksd
    h = np.where(h < lo, lo, h)
    h = np.where(h > hi, hi, h)
    o = (alpha * C) + ((F(1) - alpha) * h)
    return np.where(have[..., None], o, C).astype(F), have


def run_sequence(images, gids, coords, alpha, k):
    """Per frame the output; the first frame has no history.  images / gids / coords: per frame C, geomId, PREV_COORD_F32."""
    prev, out = None, []
    for C, g, co in zip(images, gids, coords):
        o, prev = output_taa(C, g, co, prev, alpha, k)
        out.append(o)
    return out
