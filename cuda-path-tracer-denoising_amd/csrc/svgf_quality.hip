// svgf_quality.hip — row f13, the image-quality meter: MSE / PSNR, the largest error and a windowed SSIM of two packed-rgb device
// images, left in device memory (include/svgf.h has the normative arithmetic: float32 for the exposure product and the luminance's
// last rounding, double everywhere else, nothing contracted; the kernels equal tests/quality_model.py on every bit but the two sums,
// which are within the derived bound of the exact ones).
//
//   svgf_quality_meter   k_quality_tile + k_quality_resolve.
//     k_quality_tile: one workgroup of 256 threads owns a tile of Q_TILE_W x Q_TILE_H = 64 x 32 pixels = 16 x 8 whole 4x4 cells, and
//       reads one cell column and one cell row of halo behind it (17 x 9 cells): the windows whose FIRST cell is the tile's are the
//       tile's.  A lane takes one row of one cell, four pixels of either image (three 16-byte loads each when both images are 16-byte
//       aligned and the width is a multiple of four, so that every cell row starts on 16 bytes; dword loads otherwise), transforms
//       them, forms the squared error of the tile's OWN pixels and the five row sums of the luminances, all in registers.  The four
//       lanes of a quad hold the four rows of one cell: DPP quad broadcasts give ((r0 + r1) + r2) + r3, and the quad's first lane
//       puts the cell's five sums and its "all sixteen pixels counted" flag into LDS - the tile's luminances themselves never go there,
//       only what is left of them (153 cells x 44 bytes).  Then 128 lanes take one window each: four cells, the formula, one division.
//       A fixed butterfly per wave and thread 0 over the four waves give the tile's six partials, written to the state: no atomic.
//     k_quality_resolve: one workgroup; thread t adds tiles [t c, (t + 1) c) in index order, a fixed LDS tree adds the 256 chunks.
//   svgf_quality_read    the 64-byte block, copied on the caller's stream, and the three quotients on the host.
#include "svgf_kernels.h"
#include "svgf_temporal.h"      // svgf_lum_strict
#include "../../include/svgf.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#pragma clang fp contract(off)

namespace {

#define Q_TILE_W 64
#define Q_TILE_H 32
#define Q_CELLS_X (Q_TILE_W / 4 + 1)                       // the tile's cells and one column of halo
#define Q_CELLS_Y (Q_TILE_H / 4 + 1)
#define Q_CELLS (Q_CELLS_X * Q_CELLS_Y)
#define Q_BLOCK 256
#define Q_TURNS ((4 * Q_CELLS + Q_BLOCK - 1) / Q_BLOCK)    // cell rows per lane
#define Q_PLANES 6                                         // scratch: six planes of one 8-byte word per tile, behind the result block
#define Q_EXPOSURE_WORD 516                                // f12's state: the exposure

struct QualityArgs {
    unsigned long long *state;
    const float *a, *b;
    const unsigned *exposure;       // null: e = scale
    float *se_map, *ssim_map;       // either may be null
    int W, H, nwx, nwy, tiles_x, n_tiles;
    float peak, scale;
    int clamp, vec, vec_map;
    double C1, C2;
};

__device__ __forceinline__ bool q_finite(float t) { return fabsf(t) <= 3.402823466e38f; }      // false for NaN and either infinity

// lane K of the caller's quad, by a DPP quad_perm broadcast: a VALU move per half, nothing through the LDS (ds_bpermute, which
// __shfl compiles to, made the three turns' 120 lane reads the busiest thing on the LDS port).  Every lane of the wave is active.
template <int K>
__device__ __forceinline__ double q_quad_lane(double v)
{
    constexpr int ctrl = K | (K << 2) | (K << 4) | (K << 6);
    const long long bits = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)bits, ctrl, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(bits >> 32), ctrl, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

__device__ __forceinline__ double q_quad_sum(double v)
{
#pragma clang fp contract(off)
    return ((q_quad_lane<0>(v) + q_quad_lane<1>(v)) + q_quad_lane<2>(v)) + q_quad_lane<3>(v);
}

__global__ __launch_bounds__(Q_BLOCK) void k_quality_tile(QualityArgs q)
{
#pragma clang fp contract(off)
    __shared__ double cell[5][Q_CELLS];
    __shared__ int cell_ok[Q_CELLS];
    __shared__ double w_se[Q_BLOCK / 64], w_ssim[Q_BLOCK / 64], w_max[Q_BLOCK / 64], w_min[Q_BLOCK / 64];
    __shared__ unsigned w_px[Q_BLOCK / 64], w_win[Q_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int tx = blockIdx.x % q.tiles_x, ty = blockIdx.x / q.tiles_x;
    const float e = q.exposure ? q.scale * __uint_as_float(q.exposure[Q_EXPOSURE_WORD]) : q.scale;
    const float qnan = __uint_as_float(0x7FC00000u);
    double sum_se = 0.0, max_abs = 0.0;
    unsigned n_px = 0;

    for (int turn = 0; turn < Q_TURNS; turn++) {
        const int s = turn * Q_BLOCK + tid, c = s >> 2, r = s & 3;
        const int cx = c % Q_CELLS_X, cy = c / Q_CELLS_X;
        const int x0 = tx * Q_TILE_W + 4 * cx, y = ty * Q_TILE_H + 4 * cy + r;
        const bool live = c < Q_CELLS && x0 < q.W && y < q.H;
        const bool own = cx < Q_CELLS_X - 1 && cy < Q_CELLS_Y - 1;
        const int n_valid = live ? min(4, q.W - x0) : 0;          // pixels of this cell row inside the image
        const size_t p = live ? (size_t)y * q.W + x0 : 0;
        float va[12], vb[12];                                     // a pixel outside the image is NaN: counted nowhere
        if (live && q.vec) {
            const float4 *pa = reinterpret_cast<const float4 *>(q.a + 3 * p), *pb = reinterpret_cast<const float4 *>(q.b + 3 * p);
            const float4 a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2];
            va[0] = a0.x; va[1] = a0.y; va[2] = a0.z; va[3] = a0.w; va[4] = a1.x; va[5] = a1.y; va[6] = a1.z; va[7] = a1.w;
            va[8] = a2.x; va[9] = a2.y; va[10] = a2.z; va[11] = a2.w;
            vb[0] = b0.x; vb[1] = b0.y; vb[2] = b0.z; vb[3] = b0.w; vb[4] = b1.x; vb[5] = b1.y; vb[6] = b1.z; vb[7] = b1.w;
            vb[8] = b2.x; vb[9] = b2.y; vb[10] = b2.z; vb[11] = b2.w;
        } else {
#pragma unroll
            for (int k = 0; k < 12; k++) {
                const bool in = k / 3 < n_valid;
                va[k] = in ? q.a[3 * p + k] : qnan;
                vb[k] = in ? q.b[3 * p + k] : qnan;
            }
        }
        double row[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
        float se_out[4];
        bool row_ok = true;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float ta[3], tb[3];
            bool counted = true;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                ta[ch] = va[3 * k + ch] * e;
                tb[ch] = vb[3 * k + ch] * e;
                counted = counted && q_finite(ta[ch]) && q_finite(tb[ch]);
            }
            if (q.clamp) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    if (ta[ch] < 0.0f) ta[ch] = 0.0f;
                    if (ta[ch] > q.peak) ta[ch] = q.peak;
                    if (tb[ch] < 0.0f) tb[ch] = 0.0f;
                    if (tb[ch] > q.peak) tb[ch] = q.peak;
                }
            }
            const double dr = (double)ta[0] - (double)tb[0], dg = (double)ta[1] - (double)tb[1], db = (double)ta[2] - (double)tb[2];
            const double se = (dr * dr + dg * dg) + db * db;
            se_out[k] = counted ? (float)se : qnan;
            if (counted && own) {
                sum_se += se;
                n_px++;
                const double m = fmax(fmax(fabs(dr), fabs(dg)), fabs(db));
                if (m > max_abs) max_abs = m;
            }
            row_ok = row_ok && counted;
            const double A = (double)svgf_lum_strict(ta[0], ta[1], ta[2]), B = (double)svgf_lum_strict(tb[0], tb[1], tb[2]);
            const double t[5] = { A, B, A * A, B * B, A * B };
#pragma unroll
            for (int i = 0; i < 5; i++) row[i] = k == 0 ? t[i] : row[i] + t[i];      // ((v0 + v1) + v2) + v3
        }
        if (own && q.se_map) {
            if (q.vec_map && n_valid == 4) {
                *reinterpret_cast<float4 *>(q.se_map + p) = make_float4(se_out[0], se_out[1], se_out[2], se_out[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (k < n_valid) q.se_map[p + k] = se_out[k];
            }
        }
        // the four rows of a cell sit in the four lanes of a quad; every lane of the wave is here (no lane left the loop)
        const int quad_base = lane & ~3;
        const bool ok = ((__ballot(row_ok) >> quad_base) & 0xFull) == 0xFull;
        double cs[5];
#pragma unroll
        for (int i = 0; i < 5; i++) cs[i] = q_quad_sum(row[i]);
        if (r == 0 && c < Q_CELLS) {
#pragma unroll
            for (int i = 0; i < 5; i++) cell[i][c] = cs[i];
            cell_ok[c] = ok ? 1 : 0;
        }
    }
    __syncthreads();

    // one window per lane of the first two waves: cells (wi, wj), (wi + 1, wj), (wi, wj + 1), (wi + 1, wj + 1)
    double sum_ssim = 0.0, min_ssim = __builtin_inf();
    unsigned n_win = 0;
    if (tid < (Q_CELLS_X - 1) * (Q_CELLS_Y - 1)) {
        const int wi = tid % (Q_CELLS_X - 1), wj = tid / (Q_CELLS_X - 1);
        const int gi = tx * (Q_CELLS_X - 1) + wi, gj = ty * (Q_CELLS_Y - 1) + wj;
        if (gi < q.nwx && gj < q.nwy) {
            const int c00 = wj * Q_CELLS_X + wi, c10 = c00 + 1, c01 = c00 + Q_CELLS_X, c11 = c01 + 1;
            const bool counted = cell_ok[c00] && cell_ok[c10] && cell_ok[c01] && cell_ok[c11];
            double sm[5];
#pragma unroll
            for (int i = 0; i < 5; i++) sm[i] = ((cell[i][c00] + cell[i][c10]) + cell[i][c01]) + cell[i][c11];
            const double k = 0.015625;
            const double ma = sm[0] * k, mb = sm[1] * k;
            const double va = sm[2] * k - ma * ma, vb = sm[3] * k - mb * mb, cv = sm[4] * k - ma * mb;
            const double ssim = ((2.0 * ma * mb + q.C1) * (2.0 * cv + q.C2)) / (((ma * ma + mb * mb) + q.C1) * ((va + vb) + q.C2));
            if (q.ssim_map) q.ssim_map[(size_t)gj * q.nwx + gi] = counted ? (float)ssim : qnan;
            if (counted) { sum_ssim = ssim; min_ssim = ssim; n_win = 1; }
        }
    }

    // the tile's partials: a fixed butterfly per wave (a + b == b + a: every lane ends with the same value), then the waves in order
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum_se = sum_se + __shfl_xor(sum_se, d, 64);
        sum_ssim = sum_ssim + __shfl_xor(sum_ssim, d, 64);
        const double om = __shfl_xor(max_abs, d, 64), on = __shfl_xor(min_ssim, d, 64);
        if (om > max_abs) max_abs = om;
        if (on < min_ssim) min_ssim = on;
        n_px += __shfl_xor(n_px, d, 64);
        n_win += __shfl_xor(n_win, d, 64);
    }
    if (lane == 0) {
        const int w = tid >> 6;
        w_se[w] = sum_se; w_ssim[w] = sum_ssim; w_max[w] = max_abs; w_min[w] = min_ssim; w_px[w] = n_px; w_win[w] = n_win;
    }
    __syncthreads();
    if (tid == 0) {
        double se = w_se[0], ss = w_ssim[0], mx = w_max[0], mn = w_min[0];
        unsigned long long px = w_px[0], win = w_win[0];
        for (int w = 1; w < Q_BLOCK / 64; w++) {
            se = se + w_se[w];
            ss = ss + w_ssim[w];
            if (w_max[w] > mx) mx = w_max[w];
            if (w_min[w] < mn) mn = w_min[w];
            px += w_px[w];
            win += w_win[w];
        }
        unsigned long long *part = q.state + 8 + blockIdx.x;
        const size_t n = (size_t)q.n_tiles;
        part[0] = px;
        part[n] = win;
        part[2 * n] = (unsigned long long)__double_as_longlong(se);
        part[3 * n] = (unsigned long long)__double_as_longlong(ss);
        part[4 * n] = (unsigned long long)__double_as_longlong(mx);
        part[5 * n] = (unsigned long long)__double_as_longlong(mn);
    }
}

__global__ __launch_bounds__(256) void k_quality_resolve(unsigned long long *state, int n_tiles, const unsigned *exposure, float peak,
                                                         float scale)
{
#pragma clang fp contract(off)
    __shared__ double r_se[256], r_ss[256], r_mx[256], r_mn[256];
    __shared__ unsigned long long r_px[256], r_win[256];
    const int t = threadIdx.x;
    const int chunk = (n_tiles + 255) / 256;
    const long long lo = (long long)t * chunk;
    const long long hi = lo + chunk < n_tiles ? lo + chunk : n_tiles;
    const unsigned long long *part = state + 8;
    const size_t n = (size_t)n_tiles;
    double se = 0.0, ss = 0.0, mx = 0.0, mn = __builtin_inf();
    unsigned long long px = 0, win = 0;
#pragma unroll 4
    for (long long i = lo; i < hi; i++) {      // unrolled: the loads of four tiles are in flight together, the additions stay in index order
        px += part[i];
        win += part[n + i];
        se = se + __longlong_as_double((long long)part[2 * n + i]);
        ss = ss + __longlong_as_double((long long)part[3 * n + i]);
        const double m = __longlong_as_double((long long)part[4 * n + i]), s = __longlong_as_double((long long)part[5 * n + i]);
        if (m > mx) mx = m;
        if (s < mn) mn = s;
    }
    r_se[t] = se; r_ss[t] = ss; r_mx[t] = mx; r_mn[t] = mn; r_px[t] = px; r_win[t] = win;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (t < d) {
            r_se[t] = r_se[t] + r_se[t + d];
            r_ss[t] = r_ss[t] + r_ss[t + d];
            if (r_mx[t + d] > r_mx[t]) r_mx[t] = r_mx[t + d];
            if (r_mn[t + d] < r_mn[t]) r_mn[t] = r_mn[t + d];
            r_px[t] += r_px[t + d];
            r_win[t] += r_win[t + d];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float e = exposure ? scale * __uint_as_float(exposure[Q_EXPOSURE_WORD]) : scale;
        state[0] = r_px[0];
        state[1] = r_win[0];
        state[2] = (unsigned long long)__double_as_longlong(r_se[0]);
        state[3] = (unsigned long long)__double_as_longlong(r_ss[0]);
        state[4] = (unsigned long long)__double_as_longlong(r_mx[0]);
        state[5] = (unsigned long long)__double_as_longlong(r_mn[0]);
        state[6] = (unsigned long long)__double_as_longlong((double)peak);
        state[7] = (unsigned long long)__double_as_longlong((double)e);
    }
}

bool q_finite_positive(float x) { return x > 0.0f && x <= 3.402823466e38f; }      // false for NaN, zero, negative, +inf

// 0: a size <= 0; -1: too many pixels; else the number of tiles
long long q_tiles(int width, int height, int *tiles_x)
{
    if (width <= 0 || height <= 0) return 0;
    if ((long long)width * height >= (1LL << 31) / 16) return -1;
    const long long gx = (width + Q_TILE_W - 1) / Q_TILE_W, gy = (height + Q_TILE_H - 1) / Q_TILE_H;
    if (tiles_x) *tiles_x = (int)gx;
    return gx * gy;
}

int q_windows(int d) { return d >= 8 ? (d - 8) / 4 + 1 : 0; }

}  // namespace

extern "C" {

unsigned long long svgf_quality_state_bytes(int width, int height)
{
    const long long n = q_tiles(width, height, nullptr);
    return n <= 0 ? 0ull : 64ull + 8ull * Q_PLANES * (unsigned long long)n;
}

int svgf_quality_windows(int width, int height, int *nwx, int *nwy)
{
    if (width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if (nwx) *nwx = q_windows(width);
    if (nwy) *nwy = q_windows(height);
    return SVGF_OK;
}

int svgf_quality_meter(int device, void *state_dev, const void *a_rgb_dev, const void *b_rgb_dev, int width, int height,
                       const SvgfQualityParams *qp, const void *exposure_state_dev, float *se_map_dev, float *ssim_map_dev, void *stream)
{
    if (!state_dev || !a_rgb_dev || !b_rgb_dev || !qp || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if (!q_finite_positive(qp->peak) || !q_finite_positive(qp->scale) || (qp->clamp != 0 && qp->clamp != 1)) return SVGF_ERR_INVALID_ARG;
    QualityArgs q;
    const long long n_tiles = q_tiles(width, height, &q.tiles_x);
    if (n_tiles < 0) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    q.state = static_cast<unsigned long long *>(state_dev);
    q.a = static_cast<const float *>(a_rgb_dev); q.b = static_cast<const float *>(b_rgb_dev);
    q.exposure = static_cast<const unsigned *>(exposure_state_dev);
    q.se_map = se_map_dev; q.ssim_map = ssim_map_dev;
    q.W = width; q.H = height; q.nwx = q_windows(width); q.nwy = q_windows(height);
    q.n_tiles = (int)n_tiles;
    q.peak = qp->peak; q.scale = qp->scale; q.clamp = qp->clamp;
    q.vec = ((reinterpret_cast<uintptr_t>(a_rgb_dev) | reinterpret_cast<uintptr_t>(b_rgb_dev)) & 15) == 0 && (width & 3) == 0;
    q.vec_map = q.vec && (reinterpret_cast<uintptr_t>(se_map_dev) & 15) == 0;
    const double c1 = 0.01 * (double)qp->peak, c2 = 0.03 * (double)qp->peak;
    q.C1 = c1 * c1; q.C2 = c2 * c2;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_quality_tile, dim3((unsigned)n_tiles), dim3(Q_BLOCK), 0, s, q);
    if (hipGetLastError() != hipSuccess) return SVGF_ERR_HIP;
    hipLaunchKernelGGL(k_quality_resolve, dim3(1), dim3(256), 0, s, q.state, q.n_tiles, q.exposure, q.peak, q.scale);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

int svgf_quality_read(int device, const void *state_dev, SvgfQualityResult *out_host, void *stream)
{
    if (!state_dev || !out_host) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long w[8];
    if (hipMemcpyAsync(w, state_dev, sizeof(w), hipMemcpyDeviceToHost, s) != hipSuccess) return SVGF_ERR_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) return SVGF_ERR_HIP;
    double d[8];
    memcpy(d, w, sizeof(w));
    SvgfQualityResult r;
    r.n_pixels = w[0]; r.n_windows = w[1];
    r.sum_se = d[2]; r.sum_ssim = d[3]; r.max_abs = d[4]; r.min_ssim = d[5]; r.peak = d[6]; r.scale = d[7];
    const double nan = std::nan("");
    r.mse = r.n_pixels ? r.sum_se / (3.0 * (double)r.n_pixels) : nan;
    r.psnr_db = r.n_pixels ? (r.mse == 0.0 ? (double)INFINITY : 10.0 * log10((r.peak * r.peak) / r.mse)) : nan;
    r.mean_ssim = r.n_windows ? r.sum_ssim / (double)r.n_windows : nan;
    *out_host = r;
    return SVGF_OK;
}

}  // extern "C"
