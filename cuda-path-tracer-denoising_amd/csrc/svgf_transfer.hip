// svgf_transfer.hip — history transfer (include/svgf.h: svgf_transfer_history, row f11): everything the next frame of one context
// reads as history, resampled from another context of a different (or the same) size.  One launch, one thread per dst pixel on the
// 64 x 4 tile of the clamp, TAA and upsample kernels.  include/svgf.h has the normative arithmetic; float32, no contraction.
//
// The planes of the previous G-buffer and the history length are the texels of the src pixel nearest the dst pixel's centre (the
// anchor): true texels, never blends.  Colour and moments are the bilinear mean of the four src taps around the centre that carry the
// anchor's geomId; the output history of svgf_set_output_taa is gathered the same way under the geomId stored with it.  Equal sizes
// take the identity branch (wave-uniform, a kernel argument): loads and stores only, so every bit survives.
//
// This runs when a renderer changes its resolution, not every frame: plain global loads and stores, at most ~60 B/px on each side.
// The packed-float3 planes (12 B/px) are read and written as three dwords per lane: consecutive lanes cover consecutive 12-byte
// texels, so a wave's three accesses together touch each of its 768 bytes once.  Pixel indices are 64-bit.
#include "svgf_kernels.h"
#include "svgf_temporal.h"      // svgf_bilinear_weights

#define TR_TILE_W 64
#define TR_TILE_H 4
#define TR_BLOCK (TR_TILE_W * TR_TILE_H)

// src coordinate of dst pixel centre i: u = ((float)i + 0.5f) * r - 0.5f (svgf_upsample's mapping)
__device__ __forceinline__ float tr_coord(int i, float r)
{
#pragma clang fp contract(off)
    const float c = (float)i + 0.5f;
    const float m = c * r;
    return m - 0.5f;
}

// the src texel nearest u, clamped into the image (u is finite and lies in [-0.5, n): the conversion is exact)
__device__ __forceinline__ int tr_anchor(float u, int n)
{
#pragma clang fp contract(off)
    const float h = u + 0.5f;
    return min(max((int)floorf(h), 0), n - 1);
}

__device__ __forceinline__ void tr_copy3(float *d, const float *s)
{
    const float a = s[0], b = s[1], c = s[2];
    d[0] = a; d[1] = b; d[2] = c;
}

__global__ __launch_bounds__(TR_BLOCK) void k_transfer_history(TransferArgs a)
{
#pragma clang fp contract(off)
    const int tiles_x = (a.Wd + TR_TILE_W - 1) / TR_TILE_W;
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x = bx * TR_TILE_W + (threadIdx.x % TR_TILE_W), y = by * TR_TILE_H + (threadIdx.x / TR_TILE_W);
    if (x >= a.Wd || y >= a.Hd) return;
    const size_t p = (size_t)x + (size_t)y * a.Wd;

    if (a.identity) {      // equal sizes: every plane bit for bit
        a.cv_d[p] = a.cv_s[p];
        a.mom_d[p] = a.mom_s[p];
        a.hlen_d[p] = a.hlen_s[p];
        a.gid_d[p] = a.gid_s[p];
        tr_copy3(a.nrm_d + 3 * p, a.nrm_s + 3 * p);
        tr_copy3(a.pos_d + 3 * p, a.pos_s + 3 * p);
        if (a.taa_s) a.taa_d[p] = a.taa_s[p];
        return;
    }

    const float u = tr_coord(x, a.rx), v = tr_coord(y, a.ry);
    const size_t A = (size_t)tr_anchor(u, a.Ws) + (size_t)tr_anchor(v, a.Hs) * a.Ws;
    const float ffx = floorf(u), ffy = floorf(v);
    const float ax = u - ffx, ay = v - ffy;
    const int fx = (int)ffx, fy = (int)ffy;
    float w[4];
    svgf_bilinear_weights(ax, ay, w);
    // the four taps: inside the src image or not (no address is formed for a tap outside)
    bool inside[4];
    size_t q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int tx = fx + (k & 1), ty = fy + (k >> 1);
        inside[k] = (unsigned)tx < (unsigned)a.Ws && (unsigned)ty < (unsigned)a.Hs;
        q[k] = inside[k] ? (size_t)tx + (size_t)ty * a.Ws : A;
    }

    // the state planes: G-buffer and history length of the anchor, colour and moments of the taps of the anchor's object
    const int g = a.gid_s[A];
    a.gid_d[p] = g;
    a.hlen_d[p] = a.hlen_s[A];
    tr_copy3(a.nrm_d + 3 * p, a.nrm_s + 3 * A);
    tr_copy3(a.pos_d + 3 * p, a.pos_s + 3 * A);
    {
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, m0 = 0.0f, m1 = 0.0f, sumw = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!inside[k] || a.gid_s[q[k]] != g) continue;
            const float4 c = a.cv_s[q[k]];
            const float2 m = a.mom_s[q[k]];
            c0 += w[k] * c.x; c1 += w[k] * c.y; c2 += w[k] * c.z;
            m0 += w[k] * m.x; m1 += w[k] * m.y;
            sumw += w[k];
        }
        float4 o = a.cv_s[A];      // the fourth component is the anchor's either way
        float2 om = a.mom_s[A];
        if ((double)sumw >= 0.01) {      // (a NaN sum fails the test: the anchor's values, bit copies)
            o.x = c0 / sumw; o.y = c1 / sumw; o.z = c2 / sumw;
            om.x = m0 / sumw; om.y = m1 / sumw;
        }
        a.cv_d[p] = o;
        a.mom_d[p] = om;
    }

    // svgf_set_output_taa's history: the same gather under the geomId stored with it
    if (a.taa_s) {
        float4 o = a.taa_s[A];
        const int gh = __float_as_int(o.w);
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, sumw = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!inside[k]) continue;
            const float4 c = a.taa_s[q[k]];
            if (__float_as_int(c.w) != gh) continue;
            c0 += w[k] * c.x; c1 += w[k] * c.y; c2 += w[k] * c.z;
            sumw += w[k];
        }
        if ((double)sumw >= 0.01) { o.x = c0 / sumw; o.y = c1 / sumw; o.z = c2 / sumw; }
        a.taa_d[p] = o;
    }
}

hipError_t launch_transfer_history(const TransferArgs &a, hipStream_t s)
{
    const long long tiles = (long long)((a.Wd + TR_TILE_W - 1) / TR_TILE_W) * ((a.Hd + TR_TILE_H - 1) / TR_TILE_H);
    if (tiles <= 0 || tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    SVGF_LAUNCH_KERNEL(k_transfer_history, dim3((unsigned)tiles), dim3(TR_BLOCK), 0, s, a);
    return hipGetLastError();
}
