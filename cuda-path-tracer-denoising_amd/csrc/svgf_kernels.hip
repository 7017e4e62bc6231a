// svgf_kernels.hip — temporal accumulation (with and without the history clamp), G-buffer split, output TAA, strict a-trous gather, debug/copy kernels (gfx950).
//
// The temporal kernel and the strict gather kernel keep the reference's arithmetic order and double promotions
// (reference src/denoise.cu:121,138,143-145,159,196,252) with FMA contraction off, so that they agree with the CPU
// oracle to the last ulp except inside expf.  They are the correctness anchors; the bandwidth-shaped a-trous
// kernel lives in svgf_atrous_strip.hip.
#include "svgf_kernels.h"
#include "svgf_temporal.h"

#define SVGF_BLOCK 256

static inline int div_up(long long a, int b) { return (int)((a + b - 1) / b); }

// ----------------------------------------------------------------------------------------------------
// helpers
// ----------------------------------------------------------------------------------------------------

// luminance / distance in the reference's operation order: svgf_temporal.h (shared with the fused kernel)
__device__ __forceinline__ float lum_strict(float r, float g, float b) { return svgf_lum_strict(r, g, b); }
__device__ __forceinline__ float dist3_strict(float ax, float ay, float az, float bx, float by, float bz) { return svgf_dist3_strict(ax, ay, az, bx, by, bz); }

// ----------------------------------------------------------------------------------------------------
// temporal accumulation  (reference BackProjection src/denoise.cu:185-317, isReprjValid :172-182)
// One thread per pixel; the history taps are a data-dependent gather around the reprojected position, served
// by L1/L2 (neighbouring pixels reproject to neighbouring taps).  Also splits the 52-B texel into planes.
// ----------------------------------------------------------------------------------------------------

__device__ __forceinline__ int reproj_valid(const TemporalArgs &a, float qx, float qy, int gid, float nx, float ny, float nz)
{
    const int q = svgf_tap_index(a, qx, qy);                          // bounds (:173-176); NaN coordinate: defined as invalid
    if (q < 0) return -1;
    const int gq = a.gid_prev[q];
    if (gq == -1 || gq != gid) return -1;                             // (before the normal is fetched: most rejected taps end here)
    const float *n = a.nrm_prev + 3 * (size_t)q;
    return svgf_normals_close(n[0], n[1], n[2], nx, ny, nz) ? q : -1;
}

// SvgfParams::reproj_position_tol (f4 extension): the tap's previous-frame world position must lie within tol of the
// current pixel's
__device__ __forceinline__ int reproj_valid_pos(const TemporalArgs &a, int q, float px, float py, float pz)
{
    if (q < 0 || !(a.pos_tol > 0.0f)) return q;
    const float *pp = a.pos_prev + 3 * (size_t)q;
    return (dist3_strict(pp[0], pp[1], pp[2], px, py, pz) <= a.pos_tol) ? q : -1;
}

// History clamp (svgf_set_history_clamp): the tile of the current frame's colour a workgroup of the clamped kernels stages in LDS,
// TILE_W x TILE_H pixels and a margin of R on every side, as three float planes (packed 12-byte records would sit off the natural
// alignment of the wide LDS reads).
#define SVGF_CLAMP_TILE_W 64
#define SVGF_CLAMP_TILE_H (SVGF_BLOCK / SVGF_CLAMP_TILE_W)
template <int R> struct ClampTile {
    static constexpr int PITCH = SVGF_CLAMP_TILE_W + 2 * R, ROWS = SVGF_CLAMP_TILE_H + 2 * R, PLANE = PITCH * ROWS;
    const float *c0, *c1, *c2;      // the pixel's own entry in the three planes
    int x, y;                       // the pixel
};

// MOTION (SVGF_MOTION_FMT_*): 0 projects the pixel's position through the previous camera; the others read the previous-frame
// coordinate from the caller's plane in that format.  A template parameter: the camera path's kernel carries no trace of them.
// XF: the history tests (and the camera path's projection) use the pixel's normal and position moved by the caller's per-object maps
// (svgf_set_object_motion); false: no trace of the table either.
template <int BLOCK, int MOTION, bool XF>
__global__ __launch_bounds__(BLOCK) void k_temporal(TemporalArgs a)
{
#pragma clang fp contract(off)
    const int n = a.W * a.H;
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    constexpr int R = 0;                                              // no history clamp: the body below compiles to what it always was
    constexpr bool FILTERED = false;
    const ClampTile<R> tile = {};
#include "svgf_temporal_pixel.inc.h"
}

// The temporal pass with the history clamp of radius R = 1, 2, 3.  A workgroup owns a tile of 64 x 4 pixels — one wave per row
// piece, so every per-pixel stream is read and written in the same 64-pixel runs as by k_temporal — and stages the tile's colour
// with its margin (DESIGN.md 5.1 has the reasons for the 2-D tile).  A tile row is 3 * PITCH consecutive floats of in_rgb: they are
// loaded as such, one float per lane, and scattered into the three planes.  Nothing outside the image is read: those entries
// are zero and svgf_history_clamp never looks at them.
template <int BLOCK, int MOTION, bool XF, int R>
__global__ __launch_bounds__(BLOCK) void k_temporal_clamped(TemporalArgs a)
{
#pragma clang fp contract(off)
    typedef ClampTile<R> T;
    static_assert(BLOCK == SVGF_CLAMP_TILE_W * SVGF_CLAMP_TILE_H, "one thread per pixel of the tile");
    __shared__ float lds[3 * T::PLANE];
    const int x0 = blockIdx.x * SVGF_CLAMP_TILE_W, y0 = blockIdx.y * SVGF_CLAMP_TILE_H;
    for (int j = threadIdx.x; j < 3 * T::PLANE; j += BLOCK) {
        const int row = j / (3 * T::PITCH), k = j - row * (3 * T::PITCH), col = k / 3, ch = k - 3 * col;
        const int gx = x0 - R + col, gy = y0 - R + row;
        float v = 0.0f;
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) v = a.in_rgb[3 * ((size_t)gy * a.W + gx) + ch];
        lds[ch * T::PLANE + row * T::PITCH + col] = v;
    }
    __syncthreads();
    const int tx = threadIdx.x % SVGF_CLAMP_TILE_W, ty = threadIdx.x / SVGF_CLAMP_TILE_W;
    T tile;
    tile.x = x0 + tx; tile.y = y0 + ty;
    if (tile.x >= a.W || tile.y >= a.H) return;
    tile.c0 = lds + (ty + R) * T::PITCH + (tx + R); tile.c1 = tile.c0 + T::PLANE; tile.c2 = tile.c1 + T::PLANE;
    const int p = tile.x + tile.y * a.W;
    constexpr bool FILTERED = false;
#include "svgf_temporal_pixel.inc.h"
}

// Firefly filter (svgf_set_firefly_filter): the raw colour of a 64 x 4 tile with a margin of M, staged in LDS as three colour planes
// and one plane of svgf_lum_strict, which is so evaluated once per staged texel and not once per neighbourhood it belongs to.  One
// texel per lane: its three floats are 12 consecutive bytes, a wave's a run of 768.  Nothing outside the image is read: those entries
// are zero and svgf_firefly_filter never looks at them.
template <int M> struct FireflyRaw {
    static constexpr int PITCH = SVGF_CLAMP_TILE_W + 2 * M, ROWS = SVGF_CLAMP_TILE_H + 2 * M, PLANE = PITCH * ROWS;
};
template <int BLOCK, int M>
__device__ __forceinline__ void firefly_stage(float *raw, const float *__restrict__ in_rgb, int x0, int y0, int W, int H)
{
    typedef FireflyRaw<M> S;
    for (int j = threadIdx.x; j < S::PLANE; j += BLOCK) {
        const int row = j / S::PITCH, col = j - row * S::PITCH;
        const int gx = x0 - M + col, gy = y0 - M + row;
        float r = 0.0f, g = 0.0f, b = 0.0f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const float *c = in_rgb + 3 * ((size_t)gy * W + gx);
            r = c[0]; g = c[1]; b = c[2];
        }
        raw[j] = r; raw[S::PLANE + j] = g; raw[2 * S::PLANE + j] = b;
        raw[3 * S::PLANE + j] = lum_strict(r, g, b);
    }
}

// The temporal pass on the filtered colour, with the history clamp of radius R = 0 (none) .. 3: k_temporal_clamped's tile and pixel
// body, behind two more steps in LDS.  The raw tile is staged with margin R + 1; after a barrier the workgroup writes F of the tile
// with margin R into the planes the clamped kernel would have loaded from in_rgb; after a second barrier every pixel runs the shared
// body on those: its own colour, its luminance and the clamp's window statistics are the filtered image's.  in_rgb is only read.
// rank and scale are runtime arguments (TemporalArgs), and so are the motion input and the object motion table here: one
// instantiation per R.  (One per (MOTION, XF, R), as for the clamped kernels, is 32 more kernels and 0.6 MB more library than
// tests/test_abi.py allows the product; the choice between the four motion inputs is a wave-uniform branch on a kernel argument,
// and the XF body with n_geoms == 0 moves nothing: both compute what the specialised kernels compute, bit for bit.)
// Static LDS: 4 (PITCH + 2)(ROWS + 2) + 3 PITCH ROWS floats = 9408 / 13456 / 17728 / 22224 bytes for R = 0 / 1 / 2 / 3.
template <int BLOCK, int R>
__global__ __launch_bounds__(BLOCK) void k_temporal_filtered(TemporalArgs a)
{
#pragma clang fp contract(off)
    typedef ClampTile<R> T;
    typedef FireflyRaw<R + 1> S;
    static_assert(BLOCK == SVGF_CLAMP_TILE_W * SVGF_CLAMP_TILE_H, "one thread per pixel of the tile");
    __shared__ float raw[4 * S::PLANE];
    __shared__ float lds[3 * T::PLANE];
    const int x0 = blockIdx.x * SVGF_CLAMP_TILE_W, y0 = blockIdx.y * SVGF_CLAMP_TILE_H;
    firefly_stage<BLOCK, R + 1>(raw, a.in_rgb, x0, y0, a.W, a.H);
    __syncthreads();
    for (int j = threadIdx.x; j < T::PLANE; j += BLOCK) {
        const int row = j / T::PITCH, col = j - row * T::PITCH;
        const int gx = x0 - R + col, gy = y0 - R + row;
        float r = 0.0f, g = 0.0f, b = 0.0f;
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
            const int o = (row + 1) * S::PITCH + (col + 1);
            r = raw[o]; g = raw[S::PLANE + o]; b = raw[2 * S::PLANE + o];
            svgf_firefly_filter<S::PITCH>(raw + 3 * S::PLANE + o, gx, gy, a.W, a.H, a.firefly_rank, a.firefly_scale, r, g, b);
        }
        lds[j] = r; lds[T::PLANE + j] = g; lds[2 * T::PLANE + j] = b;
    }
    __syncthreads();
    const int tx = threadIdx.x % SVGF_CLAMP_TILE_W, ty = threadIdx.x / SVGF_CLAMP_TILE_W;
    T tile;
    tile.x = x0 + tx; tile.y = y0 + ty;
    if (tile.x >= a.W || tile.y >= a.H) return;
    tile.c0 = lds + (ty + R) * T::PITCH + (tx + R); tile.c1 = tile.c0 + T::PLANE; tile.c2 = tile.c1 + T::PLANE;
    const int p = tile.x + tile.y * a.W;
    constexpr bool FILTERED = true, XF = true;
    constexpr int MOTION = SVGF_MOTION_FMT_RUNTIME;
#include "svgf_temporal_pixel.inc.h"
}

static hipError_t launch_temporal_filtered(const TemporalArgs &a, hipStream_t s)
{
    if (a.firefly_rank < 1 || a.firefly_rank > 3 || !temporal_clamp_supported(a.W, a.H)) return hipErrorInvalidValue;
    if (a.motion && !temporal_motion_format_known(a.motion_format)) return hipErrorInvalidValue;
    const dim3 grid(div_up(a.W, SVGF_CLAMP_TILE_W), div_up(a.H, SVGF_CLAMP_TILE_H)), block(SVGF_BLOCK);
    switch (a.clamp_radius) {
    case 0: SVGF_LAUNCH_KERNEL((k_temporal_filtered<SVGF_BLOCK, 0>), grid, block, 0, s, a); break;
    case 1: SVGF_LAUNCH_KERNEL((k_temporal_filtered<SVGF_BLOCK, 1>), grid, block, 0, s, a); break;
    case 2: SVGF_LAUNCH_KERNEL((k_temporal_filtered<SVGF_BLOCK, 2>), grid, block, 0, s, a); break;
    case 3: SVGF_LAUNCH_KERNEL((k_temporal_filtered<SVGF_BLOCK, 3>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int MOTION, bool XF>
static hipError_t launch_temporal_clamped(const TemporalArgs &a, hipStream_t s)
{
    const dim3 grid(div_up(a.W, SVGF_CLAMP_TILE_W), div_up(a.H, SVGF_CLAMP_TILE_H)), block(SVGF_BLOCK);
    switch (a.clamp_radius) {
    case 1: SVGF_LAUNCH_KERNEL((k_temporal_clamped<SVGF_BLOCK, MOTION, XF, 1>), grid, block, 0, s, a); break;
    case 2: SVGF_LAUNCH_KERNEL((k_temporal_clamped<SVGF_BLOCK, MOTION, XF, 2>), grid, block, 0, s, a); break;
    case 3: SVGF_LAUNCH_KERNEL((k_temporal_clamped<SVGF_BLOCK, MOTION, XF, 3>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the clamped and the filtered kernels' grids have one row of workgroups per SVGF_CLAMP_TILE_H image rows (grid.y <= 65535)
bool temporal_clamp_supported(int W, int H) { (void)W; return H <= 65535 * SVGF_CLAMP_TILE_H; }

template <bool XF>
static hipError_t launch_temporal_xf(const TemporalArgs &a, hipStream_t s)
{
    if (a.clamp_radius != 0) {
        if (!temporal_clamp_supported(a.W, a.H)) return hipErrorInvalidValue;
        if (!a.motion) return launch_temporal_clamped<SVGF_MOTION_FMT_NONE, XF>(a, s);
        switch (a.motion_format) {
        case SVGF_MOTION_FMT_COORD: return launch_temporal_clamped<SVGF_MOTION_FMT_COORD, XF>(a, s);
        case SVGF_MOTION_FMT_D32:   return launch_temporal_clamped<SVGF_MOTION_FMT_D32, XF>(a, s);
        case SVGF_MOTION_FMT_D16:   return launch_temporal_clamped<SVGF_MOTION_FMT_D16, XF>(a, s);
        default: return hipErrorInvalidValue;
        }
    }
    const long long n = (long long)a.W * a.H;
    const dim3 grid(div_up(n, SVGF_BLOCK)), block(SVGF_BLOCK);
    if (!a.motion) {
        SVGF_LAUNCH_KERNEL((k_temporal<SVGF_BLOCK, SVGF_MOTION_FMT_NONE, XF>), grid, block, 0, s, a);
        return hipGetLastError();
    }
    switch (a.motion_format) {
    case SVGF_MOTION_FMT_COORD: SVGF_LAUNCH_KERNEL((k_temporal<SVGF_BLOCK, SVGF_MOTION_FMT_COORD, XF>), grid, block, 0, s, a); break;
    case SVGF_MOTION_FMT_D32:   SVGF_LAUNCH_KERNEL((k_temporal<SVGF_BLOCK, SVGF_MOTION_FMT_D32, XF>), grid, block, 0, s, a); break;
    case SVGF_MOTION_FMT_D16:   SVGF_LAUNCH_KERNEL((k_temporal<SVGF_BLOCK, SVGF_MOTION_FMT_D16, XF>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_temporal(const TemporalArgs &a, hipStream_t s)
{
    if (a.firefly_rank != 0) return launch_temporal_filtered(a, s);
    return (a.xf && a.n_geoms > 0) ? launch_temporal_xf<true>(a, s) : launch_temporal_xf<false>(a, s);
}

bool temporal_motion_format_known(int f) { return f == SVGF_MOTION_FMT_COORD || f == SVGF_MOTION_FMT_D32 || f == SVGF_MOTION_FMT_D16; }

// ----------------------------------------------------------------------------------------------------
// svgf_motion_reproject: writes the motion plane of a frame.  Per pixel: the texel's position, moved into the previous frame's
// world space by its object's 3x4 map where one is given, through svgf_project_prev — the camera path's own projection — and
// stored in the requested format (delta formats: prev - (float)pixel).  Ray misses (geomId == -1) get NaN: no usable tap.
// ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SVGF_BLOCK) void k_motion_reproject(MotionReprojArgs a)
{
#pragma clang fp contract(off)
    const int n = a.W * a.H;
    const int p = blockIdx.x * SVGF_BLOCK + threadIdx.x;
    if (p >= n) return;
    float px, py, pz;
    int gid;
    if (a.gbuf) {
        const float *t = a.gbuf + 13 * (size_t)p;
        px = t[3]; py = t[4]; pz = t[5];
        gid = __float_as_int(t[12]);
    } else {
        px = a.pos[3 * (size_t)p]; py = a.pos[3 * (size_t)p + 1]; pz = a.pos[3 * (size_t)p + 2];
        gid = a.gid[p];
    }
    float ox, oy;
    if (gid == -1) {
        ox = oy = __uint_as_float(0x7fc00000u);
    } else {
        if (a.xf && gid >= 0 && gid < a.n_geoms) {                   // ((m0 v0 + m1 v1) + m2 v2) + m3, as svgf_scene.hip's apply
            const float *m = a.xf + 12 * (size_t)gid;
            float q[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                float t0 = m[4 * r] * px + m[4 * r + 1] * py;
                t0 = t0 + m[4 * r + 2] * pz;
                q[r] = t0 + m[4 * r + 3];
            }
            px = q[0]; py = q[1]; pz = q[2];
        }
        const SvgfPrevCoord c = svgf_project_prev(a.M, a.W, a.H, a.reproj_sx, a.reproj_sy, px, py, pz);
        ox = c.x; oy = c.y;
        if (a.format != SVGF_MOTION_FMT_COORD) {
            const int y = p / a.W, x = p - y * a.W;
            ox = ox - (float)x; oy = oy - (float)y;
        }
    }
    if (a.format == SVGF_MOTION_FMT_D16) ((__half2 *)a.out)[p] = __halves2half2(__float2half(ox), __float2half(oy));
    else ((float2 *)a.out)[p] = make_float2(ox, oy);
}

hipError_t launch_motion_reproject(const MotionReprojArgs &a, hipStream_t s)
{
    const long long n = (long long)a.W * a.H;
    SVGF_LAUNCH_KERNEL(k_motion_reproject, dim3(div_up(n, SVGF_BLOCK)), dim3(SVGF_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------------
// Output TAA (svgf_set_output_taa; include/svgf.h has the normative arithmetic): the frame's image C, which the last level or the
// pass-through copy wrote to the context's `pre` plane, blended with the previous frame's OUTPUT.  k_temporal_clamped<.., 1>'s
// shape: a 64 x 4 tile of C with a margin of 1 staged in LDS as three float planes, one float per lane from consecutive addresses;
// one thread per pixel; the four history taps are 16-byte reads from global memory (neighbouring pixels reproject to
// neighbouring texels).  The coordinate is the temporal pass's own: the call's motion plane in its format, or the (moved)
// position through the previous camera — chosen at run time, wave-uniformly, as in k_temporal_filtered.  A tap counts when it
// lies inside the image and the geomId stored with it equals the pixel's; no address is formed from a coordinate that failed
// svgf_reproj_on_screen / svgf_tap_index.
// ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SVGF_BLOCK) void k_output_taa(OutputTaaArgs a)
{
#pragma clang fp contract(off)
    typedef ClampTile<1> T;
    static_assert(SVGF_BLOCK == SVGF_CLAMP_TILE_W * SVGF_CLAMP_TILE_H, "one thread per pixel of the tile");
    __shared__ float lds[3 * T::PLANE];
    const int x0 = blockIdx.x * SVGF_CLAMP_TILE_W, y0 = blockIdx.y * SVGF_CLAMP_TILE_H;
    for (int j = threadIdx.x; j < 3 * T::PLANE; j += SVGF_BLOCK) {
        const int row = j / (3 * T::PITCH), k = j - row * (3 * T::PITCH), col = k / 3, ch = k - 3 * col;
        const int gx = x0 - 1 + col, gy = y0 - 1 + row;
        float v = 0.0f;
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) v = a.pre[3 * ((size_t)gy * a.W + gx) + ch];
        lds[ch * T::PLANE + row * T::PITCH + col] = v;
    }
    __syncthreads();
    const int tx = threadIdx.x % SVGF_CLAMP_TILE_W, ty = threadIdx.x / SVGF_CLAMP_TILE_W;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= a.W || y >= a.H) return;
    const float *c0 = lds + (ty + 1) * T::PITCH + (tx + 1), *c1 = c0 + T::PLANE, *c2 = c1 + T::PLANE;
    const int p = x + y * a.W;
    const float cr = *c0, cg = *c1, cb = *c2;
    const int gid = a.gid[p];
    float o0 = cr, o1 = cg, o2 = cb;
    if (a.hist && gid != -1) {
        TemporalArgs t = {};                                          // what the shared coordinate functions look at: the image size, the plane
        t.W = a.W; t.H = a.H; t.motion = a.motion;
        SvgfPrevCoord pc;
        if (!a.motion) {
            float px = a.pos[3 * (size_t)p], py = a.pos[3 * (size_t)p + 1], pz = a.pos[3 * (size_t)p + 2];
            if (a.xf && gid >= 0 && gid < a.n_geoms) {
                float nx = 0.0f, ny = 0.0f, nz = 0.0f;                // (the normal's half of the map is not used here)
                svgf_to_prev_space(a.xf, gid, px, py, pz, nx, ny, nz);
            }
            pc = svgf_project_prev(a.M, a.W, a.H, a.reproj_sx, a.reproj_sy, px, py, pz);
        } else {
            switch (a.motion_format) {
            case SVGF_MOTION_FMT_COORD: pc = svgf_motion_prev_coord<SVGF_MOTION_FMT_COORD>(t, p); break;
            case SVGF_MOTION_FMT_D32:   pc = svgf_motion_prev_coord<SVGF_MOTION_FMT_D32>(t, p); break;
            default:                    pc = svgf_motion_prev_coord<SVGF_MOTION_FMT_D16>(t, p); break;
            }
        }
        const SvgfReproj rp = svgf_reproj_from_coord(pc.x, pc.y);
        if (svgf_reproj_on_screen(t, rp)) {
            float w[4];
            svgf_bilinear_weights(rp.fracx, rp.fracy, w);
            SvgfHistSum hs = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
            float sumw = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = svgf_tap_index(t, rp.fx + (float)(k & 1), rp.fy + (float)(k >> 1));
                if (q < 0) continue;
                const float4 h = a.hist[q];
                if (__float_as_int(h.w) != gid) continue;
                hs.pc0 += w[k] * h.x; hs.pc1 += w[k] * h.y; hs.pc2 += w[k] * h.z;
                sumw += w[k];
            }
            if ((double)sumw >= 0.01) {                               // NaN: no history
                hs.pc0 = hs.pc0 / sumw; hs.pc1 = hs.pc1 / sumw; hs.pc2 = hs.pc2 / sumw;
                svgf_history_clamp<1, T::PITCH>(hs, c0, c1, c2, x, y, a.W, a.H, a.k);
                const float b = 1.0f - a.alpha;
                o0 = (a.alpha * cr) + (b * hs.pc0);
                o1 = (a.alpha * cg) + (b * hs.pc1);
                o2 = (a.alpha * cb) + (b * hs.pc2);
            }
        }
    }
    a.out[3 * (size_t)p] = o0; a.out[3 * (size_t)p + 1] = o1; a.out[3 * (size_t)p + 2] = o2;
    a.hist_new[p] = make_float4(o0, o1, o2, __int_as_float(gid));
}

hipError_t launch_output_taa(const OutputTaaArgs &a, hipStream_t s)
{
    if (!temporal_clamp_supported(a.W, a.H)) return hipErrorInvalidValue;
    if (a.motion && !temporal_motion_format_known(a.motion_format)) return hipErrorInvalidValue;
    SVGF_LAUNCH_KERNEL(k_output_taa, dim3(div_up(a.W, SVGF_CLAMP_TILE_W), div_up(a.H, SVGF_CLAMP_TILE_H)), dim3(SVGF_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------------
// SvgfParams::spatial_variance_frames (f4 extension; the reference's EstimateVariance is a stub, src/denoise.cu:320-329):
// pixels whose updated history is shorter than K frames take their variance from the luminance moments of their 7x7
// neighbourhood (taps with the same geomId and |n_q - n_p| <= 0.1, the reference's own consistency predicate; sums in
// raster order), boosted by max(1, 4 / history length) (Schied et al. 2017, section 4.2).  Writes cv_acc.w only.
// ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SVGF_BLOCK) void k_spatial_variance(float4 *__restrict__ cv_acc, const float2 *__restrict__ mom_acc,
                                                                const int *__restrict__ hlen_upd, const float *__restrict__ nrm,
                                                                const int *__restrict__ gid, int W, int H, int K)
{
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * (SVGF_BLOCK / 64) + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int p = x + y * W;
    const int hl = hlen_upd[p];
    if (hl >= K) return;
    const int g0 = gid[p];
    const float nx = nrm[3 * (size_t)p], ny = nrm[3 * (size_t)p + 1], nz = nrm[3 * (size_t)p + 2];
    float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
    for (int yy = -3; yy <= 3; yy++)
        for (int xx = -3; xx <= 3; xx++) {
            const int qx = x + xx, qy = y + yy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const int q = qx + qy * W;
            if (q != p) {
                if (gid[q] != g0) continue;
                const float *n = nrm + 3 * (size_t)q;
                if (!(dist3_strict(n[0], n[1], n[2], nx, ny, nz) <= 1e-1f)) continue;
            }
            const float2 m = mom_acc[q];
            s1 += m.x; s2 += m.y; cnt += 1.0f;
        }
    const float m1 = s1 / cnt, m2 = s2 / cnt;
    float v = m2 - m1 * m1;
    v = v > 0.0f ? v : 0.0f;
    const float boost = 4.0f / (float)(hl > 0 ? hl : 1);
    cv_acc[p].w = v * (boost > 1.0f ? boost : 1.0f);
}

hipError_t launch_spatial_variance(float4 *cv_acc, const float2 *mom_acc, const int *hlen_upd, const float *nrm, const int *gid,
                                   int W, int H, int K, hipStream_t s)
{
    SVGF_LAUNCH_KERNEL(k_spatial_variance, dim3((W + 63) / 64, (H + SVGF_BLOCK / 64 - 1) / (SVGF_BLOCK / 64)), dim3(SVGF_BLOCK), 0, s,
                       cv_acc, mom_acc, hlen_upd, nrm, gid, W, H, K);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------------
// non-temporal prepare: variance = 10 (reference EstimateVariance :320-329), colour = input (:370), split texel
// ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SVGF_BLOCK) void k_prepare(const float *__restrict__ in_rgb, const float *__restrict__ gbuf,
                                                       float4 *__restrict__ cv, float *__restrict__ nrm,
                                                       int *__restrict__ gid, float *__restrict__ pos, int n)
{
    const int p = blockIdx.x * SVGF_BLOCK + threadIdx.x;
    if (p >= n) return;
    if (gbuf) {               // null on the planar path: the producer filled the planes itself
        const float *t = gbuf + 13 * (size_t)p;
        nrm[3 * (size_t)p] = t[0]; nrm[3 * (size_t)p + 1] = t[1]; nrm[3 * (size_t)p + 2] = t[2];
        pos[3 * (size_t)p] = t[3]; pos[3 * (size_t)p + 1] = t[4]; pos[3 * (size_t)p + 2] = t[5];
        gid[p] = __float_as_int(t[12]);
    }
    cv[p] = make_float4(in_rgb[3 * (size_t)p], in_rgb[3 * (size_t)p + 1], in_rgb[3 * (size_t)p + 2], 10.0f);
}

hipError_t launch_prepare(const float *in_rgb, const float *gbuf, float4 *cv, float *nrm, int *gid, float *pos,
                          int W, int H, hipStream_t s)
{
    const long long n = (long long)W * H;
    SVGF_LAUNCH_KERNEL(k_prepare, dim3(div_up(n, SVGF_BLOCK)), dim3(SVGF_BLOCK), 0, s, in_rgb, gbuf, cv, nrm, gid, pos, (int)n);
    return hipGetLastError();
}

// The same on the firefly-filtered colour (svgf_set_firefly_filter): cv = (F(input), 10).  A 64 x 4 tile per workgroup, the raw
// colour and its luminance staged with a margin of 1 (firefly_stage, 3.2 KB of LDS); every thread then filters its own pixel.
__global__ __launch_bounds__(SVGF_BLOCK) void k_prepare_filtered(const float *__restrict__ in_rgb, const float *__restrict__ gbuf,
                                                                float4 *__restrict__ cv, float *__restrict__ nrm,
                                                                int *__restrict__ gid, float *__restrict__ pos, int W, int H,
                                                                int rank, float scale)
{
#pragma clang fp contract(off)
    typedef FireflyRaw<1> S;
    __shared__ float raw[4 * S::PLANE];
    const int x0 = blockIdx.x * SVGF_CLAMP_TILE_W, y0 = blockIdx.y * SVGF_CLAMP_TILE_H;
    firefly_stage<SVGF_BLOCK, 1>(raw, in_rgb, x0, y0, W, H);
    __syncthreads();
    const int tx = threadIdx.x % SVGF_CLAMP_TILE_W, ty = threadIdx.x / SVGF_CLAMP_TILE_W;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    const int p = x + y * W;
    if (gbuf) {               // null on the planar path: the producer filled the planes itself
        const float *t = gbuf + 13 * (size_t)p;
        nrm[3 * (size_t)p] = t[0]; nrm[3 * (size_t)p + 1] = t[1]; nrm[3 * (size_t)p + 2] = t[2];
        pos[3 * (size_t)p] = t[3]; pos[3 * (size_t)p + 1] = t[4]; pos[3 * (size_t)p + 2] = t[5];
        gid[p] = __float_as_int(t[12]);
    }
    const int o = (ty + 1) * S::PITCH + (tx + 1);
    float r = raw[o], g = raw[S::PLANE + o], b = raw[2 * S::PLANE + o];
    svgf_firefly_filter<S::PITCH>(raw + 3 * S::PLANE + o, x, y, W, H, rank, scale, r, g, b);
    cv[p] = make_float4(r, g, b, 10.0f);
}

hipError_t launch_prepare_filtered(const float *in_rgb, const float *gbuf, float4 *cv, float *nrm, int *gid, float *pos,
                                   int W, int H, int rank, float scale, hipStream_t s)
{
    if (rank < 1 || rank > 3 || !temporal_clamp_supported(W, H)) return hipErrorInvalidValue;
    SVGF_LAUNCH_KERNEL(k_prepare_filtered, dim3(div_up(W, SVGF_CLAMP_TILE_W), div_up(H, SVGF_CLAMP_TILE_H)), dim3(SVGF_BLOCK), 0, s,
                       in_rgb, gbuf, cv, nrm, gid, pos, W, H, rank, scale);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------------
// strict a-trous gather  (reference ATrousFilter src/denoise.cu:77-170), snapshot variance semantics:
// variance is read from src.w and written to dst.w, never in place.
// ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SVGF_BLOCK) void k_atrous_gather(AtrousArgs a)
{
#pragma clang fp contract(off)
    const int n = a.W * a.H;
    const int p = blockIdx.x * SVGF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int x = p % a.W, y = p / a.W;

    const float4 cp = a.src[p];
    float var;
    if (a.blur_variance) {                                            // 3x3 gaussian, borders renormalised (:102-118)
        float sum = 0.0f, sumw = 0.0f;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int lx = x + dx, ly = y + dy;
                if (lx >= 0 && ly >= 0 && lx < a.W && ly < a.H) {
                    const float gw = (float)((2 - (dx & 1)) * (2 - (dy & 1))) * 0.0625f;   // [1 2 1]x[1 2 1]/16
                    sum += gw * a.src[lx + ly * a.W].w;
                    sumw += gw;
                }
            }
        var = fmaxf(sum / sumw, 0.0f);
    } else {
        var = fmaxf(cp.w, 0.0f);
    }

    const float lp = lum_strict(cp.x, cp.y, cp.z);
    const float npx = a.nrm[3 * (size_t)p], npy = a.nrm[3 * (size_t)p + 1], npz = a.nrm[3 * (size_t)p + 2];
    const float ppx = a.pos[3 * (size_t)p], ppy = a.pos[3 * (size_t)p + 1], ppz = a.pos[3 * (size_t)p + 2];

    const double den_l = (double)(sqrtf(var) * a.sigma_c) + 1e-6;
    const double den_n = (double)a.sigma_n + 1e-6;
    const double den_x = (double)a.sigma_x + 1e-6;

    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, vsum = 0.0f, wsum = 0.0f, w2sum = 0.0f;
    for (int i = -2; i <= 2; i++) {
        for (int j = -2; j <= 2; j++) {
            const int xq = x + a.step * i, yq = y + a.step * j;
            if (xq < 0 || xq >= a.W || yq < 0 || yq >= a.H) continue;
            const int q = xq + yq * a.W;
            const float4 cq = a.src[q];
            const float lq = lum_strict(cq.x, cq.y, cq.z);
            const float *nq = a.nrm + 3 * (size_t)q;
            const float *pq = a.pos + 3 * (size_t)q;
            const float wl = expf((float)(-(double)fabsf(lq - lp) / den_l));
            const float wn = fminf(1.0f, expf((float)(-(double)dist3_strict(npx, npy, npz, nq[0], nq[1], nq[2]) / den_n)));
            const float wx = fminf(1.0f, expf((float)(-(double)dist3_strict(ppx, ppy, ppz, pq[0], pq[1], pq[2]) / den_x)));
            const float hi = (i == 0) ? 6.0f : ((i == 1 || i == -1) ? 4.0f : 1.0f);
            const float hj = (j == 0) ? 6.0f : ((j == 1 || j == -1) ? 4.0f : 1.0f);
            float w = (hi * hj * (1.0f / 256.0f)) * wl;                 // h[k] exact in fp32
            w = w * wn;
            w = w * wx;
            wsum += w;
            w2sum += w * w;
            c0 += cq.x * w; c1 += cq.y * w; c2 += cq.z * w;
            vsum += (cq.w * w) * w;
        }
    }

    float o0, o1, o2, ov;
    if ((double)wsum > 10e-6) {                                       // NaN -> false -> pass-through (:159-164)
        o0 = c0 / wsum; o1 = c1 / wsum; o2 = c2 / wsum; ov = vsum / w2sum;
    } else {
        o0 = cp.x; o1 = cp.y; o2 = cp.z; ov = cp.w;
    }
    if (a.modulate) svgf_modulate(a, (unsigned)p, o0, o1, o2);        // last level: * albedo * ialbedo (:166-168)
    if (a.dst) a.dst[p] = make_float4(o0, o1, o2, ov);
    if (a.out_rgb) { a.out_rgb[3 * (size_t)p] = o0; a.out_rgb[3 * (size_t)p + 1] = o1; a.out_rgb[3 * (size_t)p + 2] = o2; }
}

hipError_t launch_atrous_gather(const AtrousArgs &a, hipStream_t s)
{
    const long long n = (long long)a.W * a.H;
    SVGF_LAUNCH_KERNEL(k_atrous_gather, dim3(div_up(n, SVGF_BLOCK)), dim3(SVGF_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------------
// debug views (reference DebugView :331-340) and pass-through copy (:382)
// ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SVGF_BLOCK) void k_debug_hlen(const int *__restrict__ hlen, float *__restrict__ out, int n, float scale)
{
    const int p = blockIdx.x * SVGF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const float v = (float)hlen[p] / scale;
    out[3 * (size_t)p] = v; out[3 * (size_t)p + 1] = v; out[3 * (size_t)p + 2] = v;
}
__global__ __launch_bounds__(SVGF_BLOCK) void k_debug_var(const float4 *__restrict__ cv, float *__restrict__ out, int n, float scale)
{
    const int p = blockIdx.x * SVGF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const float v = cv[p].w / scale;
    out[3 * (size_t)p] = v; out[3 * (size_t)p + 1] = v; out[3 * (size_t)p + 2] = v;
}
__global__ __launch_bounds__(SVGF_BLOCK) void k_copy_rgb(const float4 *__restrict__ cv, float *__restrict__ out, int n)
{
    const int p = blockIdx.x * SVGF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const float4 c = cv[p];
    out[3 * (size_t)p] = c.x; out[3 * (size_t)p + 1] = c.y; out[3 * (size_t)p + 2] = c.z;
}

hipError_t launch_debug_hlen(const int *hlen, float *out_rgb, int n, float scale, hipStream_t s)
{
    SVGF_LAUNCH_KERNEL(k_debug_hlen, dim3(div_up(n, SVGF_BLOCK)), dim3(SVGF_BLOCK), 0, s, hlen, out_rgb, n, scale);
    return hipGetLastError();
}
hipError_t launch_debug_var(const float4 *cv, float *out_rgb, int n, float scale, hipStream_t s)
{
    SVGF_LAUNCH_KERNEL(k_debug_var, dim3(div_up(n, SVGF_BLOCK)), dim3(SVGF_BLOCK), 0, s, cv, out_rgb, n, scale);
    return hipGetLastError();
}
hipError_t launch_copy_rgb(const float4 *cv, float *out_rgb, int n, hipStream_t s)
{
    SVGF_LAUNCH_KERNEL(k_copy_rgb, dim3(div_up(n, SVGF_BLOCK)), dim3(SVGF_BLOCK), 0, s, cv, out_rgb, n);
    return hipGetLastError();
}
