// svgf_temporal_pixel.inc.h — one pixel of the temporal pass: the body shared by k_temporal and k_temporal_clamped (svgf_kernels.hip),
// included as text so that k_temporal compiles to exactly what it was before the history clamp existed (as a device function
// the same statements were allocated and scheduled differently).  Expects in scope:
//   a      TemporalArgs, the kernel's argument
//   p      int, the pixel (x + y * W, inside the image)
//   MOTION SVGF_MOTION_FMT_*: 0 projects the pixel's position through the previous camera; the others read the previous-frame
//          coordinate from the caller's plane in that format.  A template parameter: the camera path's kernel carries no trace of them.
//          SVGF_MOTION_FMT_RUNTIME (the filtered kernels): a.motion / a.motion_format decide, wave-uniformly, between the same four.
//   XF     bool, svgf_set_object_motion: the tests that decide whether a tap's history may be used compare it with the pixel's normal
//          and position moved into the previous frame's space by a.xf[geomId]; on the camera path (MOTION 0) the moved position
//          is also the one projected.  A template parameter like MOTION: false compiles to the kernels that knew no table.
//   R      constexpr int, radius of the history clamp; 0 = none: `tile` is not looked at
//   tile   ClampTile<R>
//   FILTERED constexpr bool, svgf_set_firefly_filter: the tile holds the FILTERED colour and the pixel's own is read from it at R = 0 too
// No include guard: it is a function body.
    float nx, ny, nz, px, py, pz;
    int gid;
    if (a.gbuf) {             // the boundary's AoS texel (52 B): read once, split into the planes every later kernel reads
        const float *t = a.gbuf + 13 * (size_t)p;
        nx = t[0]; ny = t[1]; nz = t[2];
        px = t[3]; py = t[4]; pz = t[5];
        gid = __float_as_int(t[12]);
        if (!a.skip_split) {
            a.nrm_cur[3 * (size_t)p] = nx; a.nrm_cur[3 * (size_t)p + 1] = ny; a.nrm_cur[3 * (size_t)p + 2] = nz;
            a.pos_cur[3 * (size_t)p] = px; a.pos_cur[3 * (size_t)p + 1] = py; a.pos_cur[3 * (size_t)p + 2] = pz;
            a.gid_cur[p] = gid;
        }
    } else {                  // planar path: the producer wrote the planes in place (svgf_planar_gbuffer), 28 B read, nothing split
        nx = a.nrm_cur[3 * (size_t)p]; ny = a.nrm_cur[3 * (size_t)p + 1]; nz = a.nrm_cur[3 * (size_t)p + 2];
        px = a.pos_cur[3 * (size_t)p]; py = a.pos_cur[3 * (size_t)p + 1]; pz = a.pos_cur[3 * (size_t)p + 2];
        gid = a.gid_cur[p];
    }

    float cr, cg, cb;
    if constexpr (R > 0 || FILTERED) {    // staged already
        cr = *tile.c0; cg = *tile.c1; cb = *tile.c2;
    } else {
        cr = a.in_rgb[3 * (size_t)p]; cg = a.in_rgb[3 * (size_t)p + 1]; cb = a.in_rgb[3 * (size_t)p + 2];
    }
    const float lum = lum_strict(cr, cg, cb);
    const int N = a.hlen[p];

    bool valid = false;
    SvgfHistSum hs = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (N > 0 && gid != -1) {
        float tnx = nx, tny = ny, tnz = nz, tpx = px, tpy = py, tpz = pz;   // what the taps are tested against (the planes above keep the true values)
        if constexpr (XF) {
            if (gid >= 0 && gid < a.n_geoms) svgf_to_prev_space(a.xf, gid, tpx, tpy, tpz, tnx, tny, tnz);
        }
        SvgfReproj rp;                                                // previous-frame pixel coordinate (:198-209)
        if constexpr (MOTION == SVGF_MOTION_FMT_NONE) {
            rp = svgf_reproject(a, tpx, tpy, tpz);
        } else if constexpr (MOTION == SVGF_MOTION_FMT_RUNTIME) {
            if (!a.motion) {
                rp = svgf_reproject(a, tpx, tpy, tpz);
            } else {
                SvgfPrevCoord c;
                switch (a.motion_format) {
                case SVGF_MOTION_FMT_COORD: c = svgf_motion_prev_coord<SVGF_MOTION_FMT_COORD>(a, p); break;
                case SVGF_MOTION_FMT_D32:   c = svgf_motion_prev_coord<SVGF_MOTION_FMT_D32>(a, p); break;
                default:                    c = svgf_motion_prev_coord<SVGF_MOTION_FMT_D16>(a, p); break;
                }
                rp = svgf_reproj_from_coord(c.x, c.y);
            }
        } else {
            const SvgfPrevCoord c = svgf_motion_prev_coord<MOTION>(a, p);
            rp = svgf_reproj_from_coord(c.x, c.y);
        }
        const float fx = rp.fx, fy = rp.fy;

        valid = svgf_reproj_on_screen(a, rp);
        int q4[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            q4[k] = reproj_valid_pos(a, reproj_valid(a, fx + (float)(k & 1), fy + (float)(k >> 1), gid, tnx, tny, tnz), tpx, tpy, tpz);
            valid = valid && (q4[k] >= 0);
        }

        if (valid) {                                                  // bilinear (:234-259)
            float w[4];
            svgf_bilinear_weights(rp.fracx, rp.fracy, w);
            float sumw = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = q4[k];
                const float4 ch = a.cv_hist[q];
                const float2 mh = a.mom_hist[q];
                svgf_hist_add_weighted(hs, w[k], ch.x, ch.y, ch.z, mh.x, mh.y, a.hlen[q]);
                sumw += w[k];
            }
            if ((double)sumw >= 0.01) svgf_hist_div(hs, sumw);
        } else {                                                      // 3x3 box around floor (:262-286)
            float cnt = 0.0f;
            for (int yy = -1; yy <= 1; yy++)
                for (int xx = -1; xx <= 1; xx++) {
                    // the four taps with xx, yy in {0, 1} are the bilinear taps tested above: same arguments, same answer
                    const int q = (xx >= 0 && yy >= 0) ? q4[xx + 2 * yy]
                                                       : reproj_valid_pos(a, reproj_valid(a, fx + (float)xx, fy + (float)yy, gid, tnx, tny, tnz), tpx, tpy, tpz);
                    if (q >= 0) {
                        const float4 ch = a.cv_hist[q];
                        const float2 mh = a.mom_hist[q];
                        svgf_hist_add(hs, ch.x, ch.y, ch.z, mh.x, mh.y, a.hlen[q]);
                        cnt += 1.0f;
                    }
                }
            if (cnt > 0.0f) {
                svgf_hist_div(hs, cnt);
                valid = true;
            }
        }
        if constexpr (R > 0) {                                        // usable history: clamp its colour to the current neighbourhood
            if (valid) svgf_history_clamp<R, ClampTile<R>::PITCH>(hs, tile.c0, tile.c1, tile.c2, tile.x, tile.y, a.W, a.H, a.clamp_k);
        }
    }
    const SvgfTemporalOut o = svgf_temporal_blend(a, cr, cg, cb, lum, N, valid, hs);
    a.hlen_upd[p] = o.hlen;
    a.mom_acc[p] = o.mom;
    a.cv_acc[p] = o.cv;
