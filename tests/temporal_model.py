"""The float32 numpy model of the temporal pass (csrc/svgf_temporal.h, svgf_temporal_pixel.inc.h) — the yardstick of
tests/test_motion_vectors.py, test_history_clamp.py, test_object_motion.py and (behind tests/firefly_model.py) test_firefly_filter.py
and test_temporal_matrix.py.  Test infrastructure only; not part of the package.

One model with four optional parts, each off at its default: the history clamp of svgf_set_history_clamp (`radius`, `k`), the
position test of SvgfParams::reproj_position_tol (`pos_tol`), the object motion table of svgf_set_object_motion (`tables`,
`compare_normal` / `compare_position`) and the spatial variance estimate of SvgfParams::spatial_variance_frames (`svf`;
spatial_variance below, the model of k_spatial_variance in csrc/svgf_kernels.hip), which rewrites the variance alone.

The model looks a pixel's history up at the coordinate a PREV_COORD_F32 plane gives (svgf_denoise_motion); the camera path is
the same model fed the plane svgf_motion_reproject would write (project_prev below: the camera path's own projection) — with a
table, of the MOVED position, which is what svgf_motion_reproject(X) writes.  The two tests that decide whether a tap's history
may be used compare the tap's previous normal / position with `compare_normal` / `compare_position`: the pixel's own without a
table, moved_normal() / apply_xf() with one.  The state kept for the next frame holds the true normal and position.

numpy rounds every array operation to float32 and never contracts a multiply and an add, which is the kernel's arithmetic
(`#pragma clang fp contract(off)`); sums are written as the kernel's sequences of additions, in its order.  Division and sqrt
are correctly rounded on both sides.

What pins the model, on the CPU (the oracle knows no plane, no clamp and no table, so each part is pinned where it can be):
- without clamp, position test and table, to the C oracle on the moving block of box_room:
  test_history_clamp.py::test_model_without_clamp_is_the_oracle_on_the_moving_block;
- the position test, to the oracle's: test_object_motion.py::test_model_position_test_is_the_oracle;
- the table, to the oracle on texels whose normal and position were replaced by the moved ones:
  test_object_motion.py::test_model_with_table_is_the_oracle_on_substituted_texels;
- the clamp (and everything else on the moving block, radius 0 to 3), to the results recorded in
  tests/golden/temporal_model/moving_block.json from the model the clamp's suite was first written against:
  test_object_motion.py::test_model_without_table_is_the_clamp_model_on_the_moving_block;
- the spatial variance estimate, in tests/test_spatial_variance.py:
  - to the oracle's on the bits of every pixel, every frame of noisy_sequence at seven sizes and five K:
    test_model_is_the_oracle_on_bits;
  - to a per-pixel float64 restatement written from the header's sentence, which shares no text with either, within the
    rounding of the float32 sums: test_model_is_the_float64_restatement_within_rounding;
  - by value, on hand-built 9x9 frames, case by case (the centre under a NaN normal, a NaN neighbour, distance 0.1f and the
    next float above, another geomId, ray misses, corner and edge windows, the boost at history lengths 1 to 5, NaN, 1e20
    and bright flat moments, hlen >= K, K <= 1): the test_case_* tests, each through the model and through the oracle;
  - and it leaves hlen, mom and color as a run without it: test_the_part_changes_the_variance_alone.
The GPU suites then hold the kernels to the model on the bits of every pixel."""
import numpy as np

F = np.float32
COORD, D32, D16 = 1, 2, 3      # SVGF_MOTION_PREV_COORD_F32, SVGF_MOTION_DELTA_F32, SVGF_MOTION_DELTA_F16
NORMAL_THRESHOLD = np.array([0x3c23d70b], dtype=np.uint32).view(F)[0]      # svgf_normals_close: squared distance


# ---- coordinates: replicas of svgf_to_prev_space, svgf_project_prev and svgf_motion_reproject -------------------------------------
def apply_xf(X, gid, pos):
    """pos float32[..., 3] mapped by X[gid] (float32[n, 12], 3x4 row-major) where 0 <= gid < n: ((m0 v0 + m1 v1) + m2 v2) + m3."""
    pos = np.asarray(pos, dtype=F)
    if X is None or len(X) == 0:
        return pos
    ok = (gid >= 0) & (gid < len(X))
    m = np.asarray(X, dtype=F).reshape(-1, 3, 4)[np.where(ok, gid, 0)]
    with np.errstate(all="ignore"):
        out = np.stack([((m[..., r, 0] * pos[..., 0] + m[..., r, 1] * pos[..., 1]) + m[..., r, 2] * pos[..., 2]) + m[..., r, 3]
                        for r in range(3)], axis=-1).astype(F)
    return np.where(ok[..., None], out, pos)


def moved_normal(X, gid, nrm):
    """nrm float32[..., 3] through the linear block of X[gid] where 0 <= gid < n, not renormalised: (m0 n0 + m1 n1) + m2 n2."""
    nrm = np.asarray(nrm, dtype=F)
    if X is None or len(X) == 0:
        return nrm
    ok = (gid >= 0) & (gid < len(X))
    m = np.asarray(X, dtype=F).reshape(-1, 3, 4)[np.where(ok, gid, 0)]
    with np.errstate(all="ignore"):
        out = np.stack([(m[..., r, 0] * nrm[..., 0] + m[..., r, 1] * nrm[..., 1]) + m[..., r, 2] * nrm[..., 2]
                        for r in range(3)], axis=-1).astype(F)
    return np.where(ok[..., None], out, nrm)


def project_prev(M, W, H, sx, sy, pos):
    """svgf_project_prev: world position through the previous view matrix M (float32[16], column-major) to (prevx, prevy)."""
    M = np.asarray(M, dtype=F)
    px, py, pz = pos[..., 0], pos[..., 1], pos[..., 2]
    with np.errstate(all="ignore"):
        vs = [(M[r] * px + M[4 + r] * py) + (M[8 + r] * pz + M[12 + r] * F(1)) for r in range(3)]
        clipx, clipy = vs[0] / vs[2], vs[1] / vs[2]
        if sx > 0:
            clipx = clipx / F(sx)
        if sy > 0:
            clipy = clipy / F(sy)
        ndcx, ndcy = -clipx * F(0.5) + F(0.5), -clipy * F(0.5) + F(0.5)
        return np.stack([ndcx * F(W) - F(0.5), ndcy * F(H) - F(0.5)], axis=-1).astype(F)


def motion_plane(M, W, H, gb, X, fmt, sx=0.0, sy=0.0):
    """What svgf_motion_reproject writes for the texels `gb` (GBUFFER_DTYPE[H, W]) with reproj_scale (sx, sy)."""
    gid = gb["geomId"]
    prev = project_prev(M, W, H, sx, sy, apply_xf(X, gid, gb["position"]))
    if fmt != COORD:
        prev = (prev - pixel_grid(W, H)).astype(F)
    prev = np.where((gid == -1)[..., None], F(np.nan), prev).astype(F)
    with np.errstate(over="ignore"):
        return prev.astype(np.float16) if fmt == D16 else prev


def pixel_grid(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs, ys], axis=-1).astype(F)


def coord_plane(plane, fmt, W, H):
    """A motion plane of any format as the PREV_COORD_F32 plane the kernel derives from it (include/svgf.h: a delta is converted
    to float first, then added to the float pixel coordinate)."""
    if fmt == COORD:
        return np.asarray(plane, dtype=F)
    with np.errstate(all="ignore"):
        return (pixel_grid(W, H) + np.asarray(plane).astype(F)).astype(F)


# ---- the pass -------------------------------------------------------------------------------------------------------------------------
def empty_state(W, H):
    """A fresh context: everything zero (history length 0: no pixel looks anything up)."""
    return dict(hlen=np.zeros((H, W), np.int32), mom=np.zeros((H, W, 2), F), color=np.zeros((H, W, 3), F),
                normal=np.zeros((H, W, 3), F), position=np.zeros((H, W, 3), F), gid=np.zeros((H, W), np.int32))


def luminance(c):
    l = 0.2126 * c[..., 0].astype(np.float64) + 0.7152 * c[..., 1].astype(np.float64)
    return (l + 0.0722 * c[..., 2].astype(np.float64)).astype(F)


def _shifted(a, dy, dx, fill=0):
    """a[y + dy, x + dx], `fill` outside (the caller masks those)."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return out


def clamp_box(color, radius):
    """Per pixel and channel (m, q, n) of the window of `color` (float32[H, W, 3]): taps yy outer, xx inner, inside the image."""
    H, W = color.shape[:2]
    inside = np.ones((H, W), bool)
    taps = []
    for yy in range(-radius, radius + 1):
        for xx in range(-radius, radius + 1):
            taps.append((_shifted(color, yy, xx), _shifted(inside, yy, xx, False)))
    n = np.zeros((H, W), F)
    s = np.zeros((H, W, 3), F)
    for v, ok in taps:
        s = np.where(ok[..., None], s + v, s)
        n = np.where(ok, n + F(1), n)
    m = s / n[..., None]
    q = np.zeros((H, W, 3), F)
    for v, ok in taps:
        d = v - m
        q = np.where(ok[..., None], q + d * d, q)
    return m, q, n


def temporal_pass(color, normal, position, gid, prev, coord, compare_normal=None, compare_position=None, pos_tol=0.0,
                  color_alpha=0.2, moment_alpha=0.2, radius=0, k=0.0):
    """One frame.  color float32[H, W, 3]; normal, position float32[H, W, 3] and gid int32[H, W] of this frame (the true ones: they
    become the next frame's state); prev: the state the previous frame left (empty_state() before the first); coord
    float32[H, W, 2]: PREV_COORD_F32; compare_normal (m) / compare_position (q): what the taps' previous normal / position are
    tested against, None: the pixel's own; pos_tol: SvgfParams::reproj_position_tol, the position test runs when it is > 0.
    Returns (state, variance): state as `prev` (color = accumulated colour = the colour history when the spatial filter is off)."""
    normal, position = np.asarray(normal, F), np.asarray(position, F)
    m = normal if compare_normal is None else np.asarray(compare_normal, F)
    q = position if compare_position is None else np.asarray(compare_position, F)
    with np.errstate(all="ignore"):
        return _temporal_pass(np.asarray(color, F), normal, position, np.asarray(gid, np.int32), prev, np.asarray(coord, F), m, q,
                              F(pos_tol), F(color_alpha), F(moment_alpha), int(radius), F(k))


def _temporal_pass(color, normal, position, gid, prev, coord, cmp_n, cmp_p, pos_tol, ca_min, ma_min, radius, k):
    H, W = gid.shape
    N = prev["hlen"]
    lum = luminance(color)
    active = (N > 0) & (gid != -1)
    px, py = coord[..., 0], coord[..., 1]
    fx, fy = np.floor(px), np.floor(py)
    fracx, fracy = px - fx, py - fy
    on_screen = (fx >= 0) & (fy >= 0) & (fx < F(W)) & (fy < F(H))

    p_gid, p_nrm, p_pos = prev["gid"].reshape(-1), prev["normal"].reshape(-1, 3), prev["position"].reshape(-1, 3)
    p_col, p_mom, p_len = prev["color"].reshape(-1, 3), prev["mom"].reshape(-1, 2), prev["hlen"].reshape(-1)

    def tap(dx, dy):
        """(usable, index) of the tap at (fx + dx, fy + dy): svgf_tap_index + svgf_tap_consistent + reproj_valid_pos."""
        qx, qy = fx + F(dx), fy + F(dy)
        ok = ~np.isnan(qx) & ~np.isnan(qy) & (qx >= 0) & (qx < F(W)) & (qy >= 0) & (qy < F(H))
        idx = np.where(ok, np.where(ok, qx, 0).astype(np.int64) + np.where(ok, qy, 0).astype(np.int64) * W, 0)
        gq = p_gid[idx]
        nq = p_nrm[idx]
        d = cmp_n - nq
        s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        s = s + d[..., 2] * d[..., 2]
        ok = ok & (gq != -1) & (gq == gid) & ~(s > NORMAL_THRESHOLD)
        if pos_tol > 0:      # svgf_dist3_strict(pos_prev_tap, q) <= tol; a NaN distance fails
            e = cmp_p - p_pos[idx]
            t = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
            t = t + e[..., 2] * e[..., 2]
            ok = ok & (np.sqrt(t) <= pos_tol)
        return ok, idx

    taps = {(dx, dy): tap(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    four = [(0, 0), (1, 0), (0, 1), (1, 1)]
    bilinear = active & on_screen
    for t in four:
        bilinear = bilinear & taps[t][0]

    # bilinear gather (svgf_hist_add_weighted; divided when (double)sumw >= 0.01)
    w = [(F(1) - fracx) * (F(1) - fracy), fracx * (F(1) - fracy), (F(1) - fracx) * fracy, fracx * fracy]
    b_col, b_mom, b_len, sumw = np.zeros((H, W, 3), F), np.zeros((H, W, 2), F), np.zeros((H, W), F), np.zeros((H, W), F)
    for wk, t in zip(w, four):
        idx = taps[t][1]
        b_col = b_col + wk[..., None] * p_col[idx]
        b_mom = b_mom + wk[..., None] * p_mom[idx]
        b_len = b_len + wk * p_len[idx].astype(F)
        sumw = sumw + wk
    div = sumw.astype(np.float64) >= 0.01
    b_col = np.where(div[..., None], b_col / sumw[..., None], b_col)
    b_mom = np.where(div[..., None], b_mom / sumw[..., None], b_mom)
    b_len = np.where(div, b_len / sumw, b_len)

    # 3x3 fallback in raster order (svgf_hist_add; divided by the count)
    f_col, f_mom, f_len, cnt = np.zeros((H, W, 3), F), np.zeros((H, W, 2), F), np.zeros((H, W), F), np.zeros((H, W), F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ok, idx = taps[(dx, dy)]
            f_col = np.where(ok[..., None], f_col + p_col[idx], f_col)
            f_mom = np.where(ok[..., None], f_mom + p_mom[idx], f_mom)
            f_len = np.where(ok, f_len + p_len[idx].astype(F), f_len)
            cnt = np.where(ok, cnt + F(1), cnt)
    fallback = active & ~bilinear & (cnt > 0)
    f_col, f_mom, f_len = f_col / cnt[..., None], f_mom / cnt[..., None], f_len / cnt

    valid = bilinear | fallback
    pc = np.where(bilinear[..., None], b_col, f_col)
    pm = np.where(bilinear[..., None], b_mom, f_mom)
    plen = np.where(bilinear, b_len, f_len)

    if radius > 0:      # the history clamp: comparisons, so that NaN leaves the value as it is
        m, q, n = clamp_box(color, radius)
        sd = np.sqrt(q / n[..., None])
        ksd = k * sd
        lo, hi = m - ksd, m + ksd
        pc = np.where(pc < lo, lo, pc)
        pc = np.where(pc > hi, hi, pc)

    # svgf_temporal_blend
    inv = F(1) / (N + 1).astype(F)
    ca, ma = np.maximum(inv, ca_min), np.maximum(inv, ma_min)
    m1 = ma * pm[..., 0] + (F(1) - ma) * lum
    m2 = ma * pm[..., 1] + ((F(1) - ma) * lum) * lum
    v = m2 - m1 * m1
    acc = color * ca[..., None] + pc * (F(1) - ca)[..., None]
    hl = np.where(valid, plen, 0).astype(np.int32) + 1
    state = dict(hlen=np.where(valid, hl, 1).astype(np.int32),
                 mom=np.where(valid[..., None], np.stack([m1, m2], axis=-1), np.stack([lum, lum * lum], axis=-1)).astype(F),
                 color=np.where(valid[..., None], acc, color).astype(F),
                 normal=normal.copy(), position=position.copy(), gid=gid.copy())
    variance = np.where(valid, np.where(v > 0, v, F(0)), F(100)).astype(F)
    return state, variance


SVF_REACH = 3                               # k_spatial_variance: the 7x7 window
SVF_NORMAL_DISTANCE = F(0.1)                # 1e-1f: a tap counts when its normal lies no further than this from the pixel's


def spatial_variance(variance, mom, hlen, normal, gid, K):
    """SvgfParams::spatial_variance_frames = K (k_spatial_variance, csrc/svgf_kernels.hip), behind the temporal pass of the same
    frame: variance float32[H, W] as that pass left it, mom float32[H, W, 2] and hlen int32[H, W] the UPDATED moments and history
    lengths, normal float32[H, W, 3] and gid int32[H, W] this frame's own (never the moved ones).  Returns the variance: the
    estimate where hlen < K, `variance` elsewhere.  Nothing else of the state changes.
    Taps in raster order (yy outer, xx inner); s1, s2 and cnt move only where a tap is accepted: inside the image, and — any tap
    but the centre — of the pixel's geomId with sqrt((dx dx + dy dy) + dz dz) <= 0.1f, which a NaN fails."""
    variance, mom, normal = np.asarray(variance, F), np.asarray(mom, F), np.asarray(normal, F)
    hlen, gid = np.asarray(hlen, np.int32), np.asarray(gid, np.int32)
    H, W = hlen.shape
    inside = np.ones((H, W), bool)
    s1, s2, cnt = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        for yy in range(-SVF_REACH, SVF_REACH + 1):
            for xx in range(-SVF_REACH, SVF_REACH + 1):
                if abs(yy) >= H or abs(xx) >= W:      # wholly outside an image smaller than the window
                    continue
                ok = _shifted(inside, yy, xx, False)
                if (yy, xx) != (0, 0):
                    d = normal - _shifted(normal, yy, xx)
                    s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
                    s = s + d[..., 2] * d[..., 2]
                    ok = ok & (_shifted(gid, yy, xx) == gid) & (np.sqrt(s) <= SVF_NORMAL_DISTANCE)
                m = _shifted(mom, yy, xx)
                s1 = np.where(ok, s1 + m[..., 0], s1)
                s2 = np.where(ok, s2 + m[..., 1], s2)
                cnt = np.where(ok, cnt + F(1), cnt)
        m1, m2 = s1 / cnt, s2 / cnt
        v = m2 - m1 * m1
        v = np.where(v > 0, v, F(0))
        boost = F(4) / np.maximum(hlen, 1).astype(F)
        est = v * np.where(boost > F(1), boost, F(1))
    return np.where(hlen < K, est, variance).astype(F)


def run_sequence(frames, coords=None, tables=None, views=None, scale=(0.0, 0.0), pos_tol=0.0, color_alpha=0.2, moment_alpha=0.2,
                 radius=0, k=0.0, svf=0, reset_before=()):
    """frames: per frame (color[H, W, 3], gb GBUFFER_DTYPE[H, W]); tables: per frame X float32[n, 12] or None (no table);
    coords: per frame the PREV_COORD_F32 plane the history is looked up at, or None: the camera path — the projection of the
    (moved) position through views[f], the PREVIOUS frame's view matrix, with reproj_scale `scale` (frame 0's is not looked at).
    svf: SvgfParams::spatial_variance_frames, one K or one per frame (a parameter of the call: nothing of it is kept).
    reset_before: the frames in front of which svgf_reset is called (the state is the fresh context's again).
    Per frame: dict(hlen, mom, color, variance)."""
    H, W = frames[0][1].shape
    st, out = empty_state(W, H), []
    Ks = [int(svf)] * len(frames) if np.isscalar(svf) else [int(K) for K in svf]
    assert len(Ks) == len(frames)
    for f, (col, gb) in enumerate(frames):
        if f in reset_before:
            st = empty_state(W, H)
        X = None if tables is None else tables[f]
        gid = gb["geomId"]
        q, m = apply_xf(X, gid, gb["position"]), moved_normal(X, gid, gb["normal"])
        co = coords[f] if coords is not None else project_prev(views[f], W, H, F(scale[0]), F(scale[1]), q)
        st, var = temporal_pass(np.asarray(col, F).reshape(H, W, 3), gb["normal"], gb["position"], gid, st, co, m, q, pos_tol,
                                color_alpha, moment_alpha, radius, k)
        if Ks[f] > 0:
            var = spatial_variance(var, st["mom"], st["hlen"], gb["normal"], gid, Ks[f])
        out.append(dict(hlen=st["hlen"], mom=st["mom"], color=st["color"], variance=var))
    return out
