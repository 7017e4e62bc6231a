// svgf_upsample.hip — guided upsampling (include/svgf.h: svgf_upsample, row f10): the full-size image rebuilt from a reduced-size
// denoise and the full-size G-buffer.  One thread per hi pixel on the 64 x 4 tile of the clamp and TAA kernels; the four lo taps
// around the pixel's centre are weighted bilinearly and by how well the lo texel's G-buffer agrees with the hi pixel's (pass A),
// with two fallbacks (B: the same object, C: every tap).  include/svgf.h has the normative arithmetic; float32, no contraction.
//
// The lo footprint of a tile is staged in LDS as ten float planes (rgb, normal, position, geomId).  The bound: rx, ry <= 1 and
// u(x) = ((float)x + 0.5f) * rx - 0.5f is non-decreasing in x under rounding (an exact sum, a product with a positive constant and
// a difference, each monotone), so the taps of a tile's 64 columns lie in floor(u(x0)) .. floor(u(x0 + 63)) + 1; u(x0 + 63) -
// u(x0) <= 63 (+ rounding, far below 1), so the two floors differ by at most 64 and the taps span at most 66 columns; likewise
// 3 ry <= 3, floors at most 4 apart, 6 rows.  66 x 6 texels x 10 planes x 4 B = 15840 bytes.  A tile whose footprint is larger
// (none should be) reads its taps from global memory, and so does any single tap that falls outside the staged window.
// AoS / planar on either side and `modulate` are wave-uniform branches on kernel arguments: one kernel.
#include "svgf_kernels.h"
#include "svgf_temporal.h"      // svgf_bilinear_weights

#define UP_TILE_W 64
#define UP_TILE_H 4
#define UP_BLOCK (UP_TILE_W * UP_TILE_H)
#define UP_FOOT_W (UP_TILE_W + 2)
#define UP_FOOT_H (UP_TILE_H + 2)
#define UP_PLANE (UP_FOOT_W * UP_FOOT_H)

// lo coordinate of hi pixel centre i: u = ((float)i + 0.5f) * r - 0.5f
__device__ __forceinline__ float up_coord(int i, float r)
{
#pragma clang fp contract(off)
    const float c = (float)i + 0.5f;
    const float m = c * r;
    return m - 0.5f;
}

struct UpTexel { float r, g, b, nx, ny, nz, px, py, pz; int gid; };

// one lo texel from global memory (q inside the lo image)
__device__ __forceinline__ UpTexel up_load_lo(const UpsampleArgs &a, int q)
{
    UpTexel t;
    const float *c = a.rgb_lo + 3 * (size_t)q;
    t.r = c[0]; t.g = c[1]; t.b = c[2];
    if (a.lo.gbuf) {
        const float *g = a.lo.gbuf + 13 * (size_t)q;
        t.nx = g[0]; t.ny = g[1]; t.nz = g[2];
        t.px = g[3]; t.py = g[4]; t.pz = g[5];
        t.gid = __float_as_int(g[12]);
    } else {
        const float *n = a.lo.nrm + 3 * (size_t)q, *p = a.lo.pos + 3 * (size_t)q;
        t.nx = n[0]; t.ny = n[1]; t.nz = n[2];
        t.px = p[0]; t.py = p[1]; t.pz = p[2];
        t.gid = a.lo.gid[q];
    }
    return t;
}

// running sum of one pass: acc += w * rgb, sumw += w, in order of k
struct UpSum { float c0, c1, c2, w; };
__device__ __forceinline__ void up_add(UpSum &s, float w, const UpTexel &t)
{
#pragma clang fp contract(off)
    s.c0 += w * t.r; s.c1 += w * t.g; s.c2 += w * t.b;
    s.w += w;
}

__global__ __launch_bounds__(UP_BLOCK) void k_upsample(UpsampleArgs a)
{
#pragma clang fp contract(off)
    __shared__ float lds[10 * UP_PLANE];
    const int tiles_x = (a.Wh + UP_TILE_W - 1) / UP_TILE_W;
    const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int x0 = bx * UP_TILE_W, y0 = by * UP_TILE_H;
    const int x1 = min(x0 + UP_TILE_W - 1, a.Wh - 1), y1 = min(y0 + UP_TILE_H - 1, a.Hh - 1);
    // the tile's lo footprint, clipped to the lo image (u >= -0.5 and u < W_lo: the conversions are exact)
    const int lx0 = min(max((int)floorf(up_coord(x0, a.rx)), 0), a.Wl - 1), lx1 = min((int)floorf(up_coord(x1, a.rx)) + 1, a.Wl - 1);
    const int ly0 = min(max((int)floorf(up_coord(y0, a.ry)), 0), a.Hl - 1), ly1 = min((int)floorf(up_coord(y1, a.ry)) + 1, a.Hl - 1);
    const int fw = lx1 - lx0 + 1, fh = ly1 - ly0 + 1;
    const bool staged = fw >= 1 && fh >= 1 && fw <= UP_FOOT_W && fh <= UP_FOOT_H;
    if (staged) {
        for (int j = threadIdx.x; j < fw * fh; j += UP_BLOCK) {
            const int row = j / fw, col = j - row * fw;
            const UpTexel t = up_load_lo(a, (lx0 + col) + (ly0 + row) * a.Wl);
            float *d = lds + row * UP_FOOT_W + col;
            d[0] = t.r; d[UP_PLANE] = t.g; d[2 * UP_PLANE] = t.b;
            d[3 * UP_PLANE] = t.nx; d[4 * UP_PLANE] = t.ny; d[5 * UP_PLANE] = t.nz;
            d[6 * UP_PLANE] = t.px; d[7 * UP_PLANE] = t.py; d[8 * UP_PLANE] = t.pz;
            d[9 * UP_PLANE] = __int_as_float(t.gid);
        }
    }
    __syncthreads();
    const int x = x0 + (threadIdx.x % UP_TILE_W), y = y0 + (threadIdx.x / UP_TILE_W);
    if (x >= a.Wh || y >= a.Hh) return;
    const int p = x + y * a.Wh;

    float nx, ny, nz, px, py, pz, m0 = 1.0f, m1 = 1.0f, m2 = 1.0f;
    int gid;
    if (a.hi.gbuf) {
        const float *t = a.hi.gbuf + 13 * (size_t)p;
        nx = t[0]; ny = t[1]; nz = t[2];
        px = t[3]; py = t[4]; pz = t[5];
        gid = __float_as_int(t[12]);
        if (a.modulate) { m0 = t[6] * t[9]; m1 = t[7] * t[10]; m2 = t[8] * t[11]; }
    } else {
        nx = a.hi.nrm[3 * (size_t)p]; ny = a.hi.nrm[3 * (size_t)p + 1]; nz = a.hi.nrm[3 * (size_t)p + 2];
        px = a.hi.pos[3 * (size_t)p]; py = a.hi.pos[3 * (size_t)p + 1]; pz = a.hi.pos[3 * (size_t)p + 2];
        gid = a.hi.gid[p];
        if (a.modulate) { m0 = a.hi.albedo[3 * (size_t)p]; m1 = a.hi.albedo[3 * (size_t)p + 1]; m2 = a.hi.albedo[3 * (size_t)p + 2]; }
    }

    const float u = up_coord(x, a.rx), v = up_coord(y, a.ry);
    const float ffx = floorf(u), ffy = floorf(v);
    const float ax = u - ffx, ay = v - ffy;
    const int fx = (int)ffx, fy = (int)ffy;
    float wb[4];
    svgf_bilinear_weights(ax, ay, wb);

    // the three passes are independent sums over the same taps in the same order: one sweep
    UpSum sa = { 0.0f, 0.0f, 0.0f, 0.0f }, sb = sa, sc = sa;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int tx = fx + (k & 1), ty = fy + (k >> 1);
        if ((unsigned)tx >= (unsigned)a.Wl || (unsigned)ty >= (unsigned)a.Hl) continue;      // not inside: no address is formed
        UpTexel t;
        const int cx = tx - lx0, cy = ty - ly0;
        if (staged && (unsigned)cx < (unsigned)fw && (unsigned)cy < (unsigned)fh) {
            const float *s = lds + cy * UP_FOOT_W + cx;
            t.r = s[0]; t.g = s[UP_PLANE]; t.b = s[2 * UP_PLANE];
            t.nx = s[3 * UP_PLANE]; t.ny = s[4 * UP_PLANE]; t.nz = s[5 * UP_PLANE];
            t.px = s[6 * UP_PLANE]; t.py = s[7 * UP_PLANE]; t.pz = s[8 * UP_PLANE];
            t.gid = __float_as_int(s[9 * UP_PLANE]);
        } else {
            t = up_load_lo(a, tx + ty * a.Wl);
        }
        up_add(sc, wb[k], t);
        if (t.gid != gid) continue;
        up_add(sb, wb[k], t);
        float w = wb[k];
        if (gid != -1) {
            if (a.sigma_n > 0.0f) {
                const float dx = t.nx - nx, dy = t.ny - ny, dz = t.nz - nz;
                float s = dx * dx + dy * dy;
                s = s + dz * dz;
                float e = 1.0f - sqrtf(s) / a.sigma_n;
                if (!(e > 0.0f)) e = 0.0f;
                w = w * e;
            }
            if (a.sigma_x > 0.0f) {
                const float dx = t.px - px, dy = t.py - py, dz = t.pz - pz;
                float s = nx * dx + ny * dy;
                s = s + nz * dz;
                float e = 1.0f - fabsf(s) / a.sigma_x;
                if (!(e > 0.0f)) e = 0.0f;
                w = w * e;
            }
        }
        up_add(sa, w, t);
    }
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    if ((double)sa.w >= 0.01)      { o0 = sa.c0 / sa.w; o1 = sa.c1 / sa.w; o2 = sa.c2 / sa.w; }      // NaN fails the test
    else if ((double)sb.w >= 0.01) { o0 = sb.c0 / sb.w; o1 = sb.c1 / sb.w; o2 = sb.c2 / sb.w; }
    else if ((double)sc.w >= 0.01) { o0 = sc.c0 / sc.w; o1 = sc.c1 / sc.w; o2 = sc.c2 / sc.w; }
    if (a.modulate) { o0 = o0 * m0; o1 = o1 * m1; o2 = o2 * m2; }
    a.out[3 * (size_t)p] = o0; a.out[3 * (size_t)p + 1] = o1; a.out[3 * (size_t)p + 2] = o2;
}

hipError_t launch_upsample(const UpsampleArgs &a, hipStream_t s)
{
    const long long tiles = (long long)((a.Wh + UP_TILE_W - 1) / UP_TILE_W) * ((a.Hh + UP_TILE_H - 1) / UP_TILE_H);
    if (tiles <= 0 || tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    SVGF_LAUNCH_KERNEL(k_upsample, dim3((unsigned)tiles), dim3(UP_BLOCK), 0, s, a);
    return hipGetLastError();
}
