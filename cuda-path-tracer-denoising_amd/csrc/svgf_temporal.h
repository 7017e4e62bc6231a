// svgf_temporal.h — the per-pixel arithmetic of the temporal pass (reference BackProjection src/denoise.cu:185-317 and
// isReprjValid :172-182), factored into device functions so that it lives in ONE place: k_temporal (svgf_kernels.hip, one
// thread per pixel) and the loader waves of the fused temporal + first-level kernel (svgf_atrous_fused.hip) both call them.
//
// Everything here keeps the reference's operation order with FMA contraction off (the temporal goldens are bit-exact):
// glm mat4 * vec4 association (m0 v0 + m1 v1) + (m2 v2 + m3 v3), luminance in double, alpha on the current side for colour
// (:297) and on the history side for the moments (:300-301), (int) truncation of the interpolated history length (:294).
#pragma once
#include <hip/hip_fp16.h>
#include "svgf_kernels.h"

// luminance with the reference's double promotion (src/denoise.cu:121,138,196)
__device__ __forceinline__ float svgf_lum_strict(float r, float g, float b)
{
#pragma clang fp contract(off)
    double l = 0.2126 * (double)r + 0.7152 * (double)g;
    l = l + 0.0722 * (double)b;
    return (float)l;
}

// glm::distance(vec3,vec3): sqrt((dx*dx + dy*dy) + dz*dz)
__device__ __forceinline__ float svgf_dist3_strict(float ax, float ay, float az, float bx, float by, float bz)
{
#pragma clang fp contract(off)
    float dx = bx - ax, dy = by - ay, dz = bz - az;
    float s = dx * dx + dy * dy;
    s = s + dz * dz;
    return sqrtf(s);
}

// The projection half of the reprojection (:198-206): world position (px,py,pz) through the previous view matrix M (column-major)
// to the previous-frame pixel coordinate, pixel centres at integers.  The one place this arithmetic lives: the camera path of the
// temporal pass and the motion-plane writer (k_motion_reproject, svgf_kernels.hip) both call it, so a plane written by the latter
// holds exactly the coordinates the former would have computed.
struct SvgfPrevCoord { float x, y; };
__device__ __forceinline__ SvgfPrevCoord svgf_project_prev(const float *M, int W, int H, float reproj_sx, float reproj_sy,
                                                           float px, float py, float pz)
{
#pragma clang fp contract(off)
    float vs[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        float a0 = M[0 * 4 + r] * px + M[1 * 4 + r] * py;
        float a1 = M[2 * 4 + r] * pz + M[3 * 4 + r] * 1.0f;
        vs[r] = a0 + a1;
    }
    float clipx = vs[0] / vs[2], clipy = vs[1] / vs[2];          // no tan(fov), no aspect (:202-203)
    if (reproj_sx > 0.0f) clipx = clipx / reproj_sx;              // f4 extension: exact for any fov / aspect
    if (reproj_sy > 0.0f) clipy = clipy / reproj_sy;
    float ndcx = -clipx * 0.5f + 0.5f, ndcy = -clipy * 0.5f + 0.5f;
    SvgfPrevCoord c;
    c.x = ndcx * (float)W - 0.5f; c.y = ndcy * (float)H - 0.5f;
    return c;
}

// The other half (:207-209): floor and fraction of a previous-frame pixel coordinate, wherever it came from (the projection above
// or a caller's motion plane).  Any float is a defined input: NaN stays NaN, +-inf stays +-inf, and both fail svgf_reproj_on_screen
// and svgf_tap_index below before an address is formed.
struct SvgfReproj { float fx, fy, fracx, fracy; };
__device__ __forceinline__ SvgfReproj svgf_reproj_from_coord(float prevx, float prevy)
{
#pragma clang fp contract(off)
    SvgfReproj r;
    r.fx = floorf(prevx); r.fy = floorf(prevy);
    r.fracx = prevx - r.fx; r.fracy = prevy - r.fy;
    return r;
}
// the reference's bounds rule on the floor (:210-211); false for NaN
__device__ __forceinline__ bool svgf_reproj_on_screen(const TemporalArgs &a, const SvgfReproj &r)
{
    return r.fx >= 0.0f && r.fy >= 0.0f && r.fx < (float)a.W && r.fy < (float)a.H;
}

// previous-frame pixel coordinate of world position (px,py,pz) (:198-209): floor and fraction of the reprojected position
__device__ __forceinline__ SvgfReproj svgf_reproject(const TemporalArgs &a, float px, float py, float pz)
{
    const SvgfPrevCoord c = svgf_project_prev(a.M, a.W, a.H, a.reproj_sx, a.reproj_sy, px, py, pz);
    return svgf_reproj_from_coord(c.x, c.y);
}

// Motion input (include/svgf.h SVGF_MOTION_*): the previous-frame coordinate of pixel p = x + y*W read from the caller's plane
// instead of being projected.  FORMAT is a compile-time constant of the kernel instantiation.
template <int FORMAT>
__device__ __forceinline__ SvgfPrevCoord svgf_motion_prev_coord(const TemporalArgs &a, int p)
{
#pragma clang fp contract(off)
    SvgfPrevCoord c;
    if constexpr (FORMAT == SVGF_MOTION_FMT_COORD) {
        const float2 m = ((const float2 *)a.motion)[p];
        c.x = m.x; c.y = m.y;
    } else {
        const int y = p / a.W, x = p - y * a.W;
        float dx, dy;
        if constexpr (FORMAT == SVGF_MOTION_FMT_D32) {
            const float2 m = ((const float2 *)a.motion)[p];
            dx = m.x; dy = m.y;
        } else {
            const __half2 m = ((const __half2 *)a.motion)[p];
            dx = __low2float(m); dy = __high2float(m);
        }
        c.x = (float)x + dx; c.y = (float)y + dy;
    }
    return c;
}

// Object motion (include/svgf.h: svgf_set_object_motion): the pixel's position and normal moved into the previous frame's world space
// by its object's rigid map M = xf[gid] (3x4 row-major; the caller has checked 0 <= gid < n_geoms).  Normative arithmetic, the
// position's being k_motion_reproject's own sequence: q[r] = ((M[4r] px + M[4r+1] py) + M[4r+2] pz) + M[4r+3]; the normal takes the
// linear block only and is not renormalised: m[r] = (M[4r] nx + M[4r+1] ny) + M[4r+2] nz.  Every float is a defined input.
// A row is one 16-byte load (the table is 16-byte aligned, a map is 48 bytes); geomId is almost wave-uniform and the table a few
// cache lines, so the three loads of a wave touch one or two lines of L1 / L2.
__device__ __forceinline__ void svgf_to_prev_space(const float *xf, int gid, float &px, float &py, float &pz, float &nx, float &ny, float &nz)
{
#pragma clang fp contract(off)
    const float4 *m = (const float4 *)xf + 3 * (size_t)gid;
    float q[3], n[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float4 row = m[r];
        float t0 = row.x * px + row.y * py;
        t0 = t0 + row.z * pz;
        q[r] = t0 + row.w;
        float t1 = row.x * nx + row.y * ny;
        n[r] = t1 + row.z * nz;
    }
    px = q[0]; py = q[1]; pz = q[2];
    nx = n[0]; ny = n[1]; nz = n[2];
}

// bounds part of isReprjValid (:173-176): texel index of the tap at float coordinate (qx, qy), -1 when it is outside the
// screen (a NaN coordinate is DEFINED as outside; the reference would index texel (int)NaN)
__device__ __forceinline__ int svgf_tap_index(const TemporalArgs &a, float qx, float qy)
{
    if (!(qx == qx) || !(qy == qy)) return -1;
    if (qx < 0.0f || qx >= (float)a.W || qy < 0.0f || qy >= (float)a.H) return -1;
    return (int)qx + (int)qy * a.W;
}

// consistency part of isReprjValid (:177-180) on the tap's previous-frame geomId / normal.  `distance(n_prev, n_cur) > 1e-1f`
// is evaluated on the SQUARED distance: sqrtf is correctly rounded and monotonic, so sqrtf(s) > 0.1f  <=>  s > 0x3c23d70b (the
// largest float whose root still rounds to <= 0.1f; found by stepping through the floats around 0.01, tools/experiments/
// temporal_branch_free_validity_32bit_offsets.patch carried the same constant in round 1).  NaN compares false either way, i.e.
// a NaN distance PASSES, as in the reference.  Branch-free: the fused kernel evaluates it for nine taps per pixel.
__device__ __forceinline__ bool svgf_normals_close(float nqx, float nqy, float nqz, float nx, float ny, float nz)
{
#pragma clang fp contract(off)
    const float dx = nx - nqx, dy = ny - nqy, dz = nz - nqz;          // glm::distance(a, b) = length(b - a): b is the current normal
    float s = dx * dx + dy * dy;
    s = s + dz * dz;
    return !(s > __uint_as_float(0x3c23d70bu));
}
__device__ __forceinline__ bool svgf_tap_consistent(int gq, float nqx, float nqy, float nqz, int gid, float nx, float ny, float nz)
{
    return (gq != -1) & (gq == gid) & svgf_normals_close(nqx, nqy, nqz, nx, ny, nz);
}

// bilinear weights of the four taps (0,0) (1,0) (0,1) (1,1) (:237-240)
__device__ __forceinline__ void svgf_bilinear_weights(float fracx, float fracy, float (&w)[4])
{
#pragma clang fp contract(off)
    w[0] = (1 - fracx) * (1 - fracy); w[1] = fracx * (1 - fracy); w[2] = (1 - fracx) * fracy; w[3] = fracx * fracy;
}

// history value being gathered: colour, moments, (float) length
struct SvgfHistSum { float pc0, pc1, pc2, pm0, pm1, plen; };
// bilinear tap (:242-249): sum += w * tap
__device__ __forceinline__ void svgf_hist_add_weighted(SvgfHistSum &h, float w, float c0, float c1, float c2, float m0, float m1, int len)
{
#pragma clang fp contract(off)
    h.pc0 += w * c0; h.pc1 += w * c1; h.pc2 += w * c2;
    h.pm0 += w * m0; h.pm1 += w * m1;
    h.plen += w * (float)len;
}
// 3x3 fallback tap (:272-279): sum += tap
__device__ __forceinline__ void svgf_hist_add(SvgfHistSum &h, float c0, float c1, float c2, float m0, float m1, int len)
{
#pragma clang fp contract(off)
    h.pc0 += c0; h.pc1 += c1; h.pc2 += c2;
    h.pm0 += m0; h.pm1 += m1;
    h.plen += (float)len;
}
__device__ __forceinline__ void svgf_hist_div(SvgfHistSum &h, float d)
{
#pragma clang fp contract(off)
    h.pc0 /= d; h.pc1 /= d; h.pc2 /= d; h.pm0 /= d; h.pm1 /= d; h.plen /= d;
}

// History clamp (include/svgf.h: svgf_set_history_clamp; variance clipping): the gathered history colour is clamped, per channel,
// to mean +- k * sigma of the CURRENT frame's colour over the (2R+1)^2 window around the pixel, before the blend.  Normative
// arithmetic: taps (x+xx, y+yy) with yy outer and xx inner, only those inside the image (n = their count, centre included);
// s = sum v; m = s / n; q = sum (v - m)(v - m), the product rounded and then added; sd = sqrtf(q / n); lo = m - k sd, hi = m + k sd.
// Two passes on purpose: E[x^2] - E[x]^2 cancels on flat regions.  Comparisons, not fminf / fmaxf: a NaN history value or NaN
// bounds leave the value as it is.
// c0 / c1 / c2: the pixel's own entry in the three colour planes of a staged tile with row pitch PITCH (LDS; the entries of taps
// outside the image are never read).  Moments, length and validity are not touched.
__device__ __forceinline__ float svgf_clamp_to_box(float pc, float m, float q, float n, float k)
{
#pragma clang fp contract(off)
    const float sd = sqrtf(q / n);
    const float ksd = k * sd;
    const float lo = m - ksd, hi = m + ksd;
    if (pc < lo) pc = lo;
    if (pc > hi) pc = hi;
    return pc;
}
template <int R, int PITCH>
__device__ __forceinline__ void svgf_history_clamp(SvgfHistSum &h, const float *c0, const float *c1, const float *c2,
                                                   int x, int y, int W, int H, float k)
{
#pragma clang fp contract(off)
    bool in_y[2 * R + 1], in_x[2 * R + 1];
#pragma unroll
    for (int d = -R; d <= R; d++) {
        in_y[d + R] = (unsigned)(y + d) < (unsigned)H;
        in_x[d + R] = (unsigned)(x + d) < (unsigned)W;
    }
    float n = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int yy = -R; yy <= R; yy++)
#pragma unroll
        for (int xx = -R; xx <= R; xx++)
            if (in_y[yy + R] && in_x[xx + R]) {
                const int o = yy * PITCH + xx;
                s0 += c0[o]; s1 += c1[o]; s2 += c2[o];
                n += 1.0f;
            }
    const float m0 = s0 / n, m1 = s1 / n, m2 = s2 / n;
    float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;
#pragma unroll
    for (int yy = -R; yy <= R; yy++)
#pragma unroll
        for (int xx = -R; xx <= R; xx++)
            if (in_y[yy + R] && in_x[xx + R]) {
                const int o = yy * PITCH + xx;
                const float d0 = c0[o] - m0, d1 = c1[o] - m1, d2 = c2[o] - m2;
                q0 += d0 * d0; q1 += d1 * d1; q2 += d2 * d2;
            }
    h.pc0 = svgf_clamp_to_box(h.pc0, m0, q0, n, k);
    h.pc1 = svgf_clamp_to_box(h.pc1, m1, q1, n, k);
    h.pc2 = svgf_clamp_to_box(h.pc2, m2, q2, n, k);
}

// Firefly filter (include/svgf.h: svgf_set_firefly_filter; rank clamp of the INPUT colour): a pixel whose luminance exceeds scale
// times the rank-th largest luminance among its up to eight neighbours (centre excluded, inside the image, NaN not counted) is
// scaled down to that bound.  Normative arithmetic: neighbours yy outer, xx inner; each counted luminance is inserted into the
// descending list t[0..rank-1] by the swap sequence below (so that +-0 and ties select the same bits everywhere);
// B = t[min(rank, n) - 1]; bound = scale * B; if (Lp > bound) c *= bound / Lp, one rounded quotient and one product per channel.
// A NaN centre, a NaN bound and a pixel without a counted neighbour are left as they are.
// lum: the pixel's own entry in the luminance plane (svgf_lum_strict of every staged texel) of a tile with row pitch PITCH and a
// margin of at least 1 around the pixel; the entries of taps outside the image are never read.
template <int PITCH>
__device__ __forceinline__ void svgf_firefly_filter(const float *lum, int x, int y, int W, int H, int rank, float scale,
                                                    float &r, float &g, float &b)
{
#pragma clang fp contract(off)
    const float ninf = __uint_as_float(0xff800000u);
    float t0 = ninf, t1 = ninf, t2 = ninf;
    int n = 0;
#pragma unroll
    for (int yy = -1; yy <= 1; yy++)
#pragma unroll
        for (int xx = -1; xx <= 1; xx++) {
            if (xx == 0 && yy == 0) continue;
            if ((unsigned)(x + xx) < (unsigned)W && (unsigned)(y + yy) < (unsigned)H) {
                float v = lum[yy * PITCH + xx];
                if (v == v) {
                    n += 1;
                    if (v > t0) { const float u = t0; t0 = v; v = u; }
                    if (rank > 1 && v > t1) { const float u = t1; t1 = v; v = u; }
                    if (rank > 2 && v > t2) { const float u = t2; t2 = v; v = u; }
                }
            }
        }
    if (n == 0) return;
    const int k = rank < n ? rank : n;
    const float B = k <= 1 ? t0 : (k == 2 ? t1 : t2);
    const float bound = scale * B;
    const float Lp = lum[0];
    if (Lp > bound) {
        const float s = bound / Lp;
        r = r * s; g = g * s; b = b * s;
    }
}

// The accumulated pixel.  `valid`: a usable history value (pc*, pm*, plen: interpolated colour, moments, length) was found.
struct SvgfTemporalOut { float4 cv; float2 mom; int hlen; };
__device__ __forceinline__ SvgfTemporalOut svgf_temporal_blend(const TemporalArgs &a, float cr, float cg, float cb, float lum, int N,
                                                              bool valid, const SvgfHistSum &hs)
{
#pragma clang fp contract(off)
    const float pc0 = hs.pc0, pc1 = hs.pc1, pc2 = hs.pc2, pm0 = hs.pm0, pm1 = hs.pm1, plen = hs.plen;
    SvgfTemporalOut o;
    if (valid) {
        const float ca = fmaxf(1.0f / (float)(N + 1), a.color_alpha_min);   // alpha on the current side (:297)
        const float ma = fmaxf(1.0f / (float)(N + 1), a.moment_alpha_min);  // alpha on the history side (:300-301)
        o.hlen = (int)plen + 1;
        const float m1 = ma * pm0 + (1.0f - ma) * lum;
        const float m2 = ma * pm1 + ((1.0f - ma) * lum) * lum;
        o.mom = make_float2(m1, m2);
        const float v = m2 - m1 * m1;
        o.cv = make_float4(cr * ca + pc0 * (1.0f - ca), cg * ca + pc1 * (1.0f - ca), cb * ca + pc2 * (1.0f - ca), v > 0.0f ? v : 0.0f);
    } else {                                                               // no usable history (:311-315)
        o.hlen = 1;
        o.mom = make_float2(lum, lum * lum);
        o.cv = make_float4(cr, cg, cb, 100.0f);
    }
    return o;
}
