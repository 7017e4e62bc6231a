// svgf_display.hip — the step right after denoise(): pack for display, and save.
//
//   svgf_display_pack   reference sendTwoImagesToPBO (src/pathtrace.cu:45-77): two packed-rgb float images side by
//                       side into one (2W x H) RGBA8 buffer; channel = clamp((int)(v * 255.0), 0, 255) with the product
//                       in double, alpha = 0.  Float->int conversion saturates and maps NaN to 0 (what the CUDA
//                       original does); HBM-bound: 24 B read + 8 B written per pixel.
//   svgf_save_png       reference saveImage + image::savePNG (src/main.cpp:131-152, src/image.cpp:22-39): the image is
//                       mirrored in x (the renderer's rays run right-to-left), each channel is clamp(v,0,1) * 255.f
//                       truncated to a byte, written as an 8-bit RGB PNG.  The reference encodes with stb_image_write;
//                       this writer emits stored (uncompressed) deflate blocks — same pixels, larger file, no dependency.
//
// Row f12, the HDR display side (include/svgf.h has the normative arithmetic; float32 without contraction, integers otherwise, no
// transcendental: the kernels equal tests/tonemap_model.py on every bit):
//   svgf_exposure_reset   k_exposure_reset: the 520 state words, one launch.
//   svgf_exposure_meter   k_luma_histogram + k_exposure_resolve.  The histogram is a read-only stream of 12 B/px on a capped grid
//                         (HIST_MAX_BLOCKS workgroups, grid-stride): a thread takes four pixels as three 16-byte loads when the image
//                         is 16-byte aligned (one pixel at a time otherwise, and for the up to three pixels behind the last whole
//                         four), bins them into its WAVE's 256 LDS bins with integer LDS atomics, and at the end each thread adds one
//                         bin's workgroup total to the state with one global integer atomicAdd (zero bins skipped).  Flat regions put
//                         a whole wave on one LDS address, which the LDS serialises: the lanes that share the first counted lane's bin
//                         are peeled into one add of their popcount (SVGF_HIST_PEEL; DESIGN.md 5.4d has both measurements).
//                         The resolve is one workgroup, one bin per thread: prefix sum in LDS, trimmed counts, two 64-bit sums,
//                         thread 0 divides and does the float tail.  It leaves the accumulating bins zero.
//   svgf_display_tonemap  k_display_tonemap: k_display_pack's geometry and traffic; op, transfer, the NULL left image and the NULL
//                         state are wave-uniform branches on kernel arguments: one kernel.  The sRGB thresholds ride in the argument
//                         block (1 KB), are copied to LDS and searched in eight steps.
#include "svgf_kernels.h"
#include "svgf_temporal.h"      // svgf_lum_strict
#include "../../include/svgf.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

__device__ __forceinline__ int to_byte(float v)
{
    const int i = (int)((double)v * 255.0);        // v_cvt_i32_f64: saturating, NaN -> 0
    return min(max(i, 0), 255);
}

// ---- row f12: luminance histogram, exposure, tone-mapped pack ----
// Few, large workgroups: every workgroup ends with one add to each populated bin, and adds to ONE address run one after the other,
// about 10 ns apiece on the MI355X - the kernel took 27 / 16.7 / 11.5 us at 1080p with 2048 / 1024 / 512 workgroups of 256 threads,
// 8.7 us with 256 of 1024 (the same 16 waves per CU).  The #ifndef's are how those rows and the leader-bin peel's
// before / after were built (-DHIST_BLOCK=.. -DHIST_MAX_BLOCKS=.., -DSVGF_HIST_PEEL=0); the product defines none of them.
#ifndef HIST_BLOCK
#define HIST_BLOCK 1024
#define HIST_MAX_BLOCKS 256       // one workgroup per CU of a 256-CU part; at most 256 x 256 global adds per metering
#endif
#define HIST_WAVES (HIST_BLOCK / 64)
#ifndef SVGF_HIST_PEEL
#define SVGF_HIST_PEEL 1
#endif
#define EXP_N 512                 // state words: see include/svgf.h
#define EXP_M 513
#define EXP_LBITS 514
#define EXP_TARGET 515
#define EXP_EXPOSURE 516
#define EXP_COUNT 517

// one pixel into the wave's bins `h`
__device__ __forceinline__ void hist_count(unsigned *h, float r, float g, float b)
{
    const float L = svgf_lum_strict(r, g, b);
    if (L == L && L > 0.0f && L < __builtin_inff()) {
        const int bin = min(max((int)(__float_as_uint(L) >> 20) - 888, 0), 255);
#if SVGF_HIST_PEEL
        const int lead = __builtin_amdgcn_readfirstlane(bin);      // the first counted lane's bin
        if (bin == lead) {
            const unsigned long long same = __ballot(1);           // the counted lanes that share it
            if ((int)__lane_id() == __ffsll(same) - 1) atomicAdd(&h[lead], (unsigned)__popcll(same));
        } else {
            atomicAdd(&h[bin], 1u);
        }
#else
        atomicAdd(&h[bin], 1u);
#endif
    }
}

__global__ __launch_bounds__(HIST_BLOCK) void k_luma_histogram(unsigned *state, const float *rgb, int n, int vec)
{
    __shared__ unsigned h[HIST_WAVES][256];
    for (int i = threadIdx.x; i < HIST_WAVES * 256; i += HIST_BLOCK) (&h[0][0])[i] = 0;
    __syncthreads();
    unsigned *mine = h[threadIdx.x >> 6];
    const int gid = blockIdx.x * HIST_BLOCK + threadIdx.x, stride = gridDim.x * HIST_BLOCK;
    const int nq = vec ? n >> 2 : 0;                               // whole fours: 48 bytes, three aligned 16-byte loads
    const float4 *v4 = reinterpret_cast<const float4 *>(rgb);
    for (int q = gid; q < nq; q += stride) {
        const float4 a = v4[3 * (size_t)q], b = v4[3 * (size_t)q + 1], c = v4[3 * (size_t)q + 2];
        hist_count(mine, a.x, a.y, a.z);
        hist_count(mine, a.w, b.x, b.y);
        hist_count(mine, b.z, b.w, c.x);
        hist_count(mine, c.y, c.z, c.w);
    }
    for (int p = 4 * nq + gid; p < n; p += stride) {
        const float *c = rgb + 3 * (size_t)p;
        hist_count(mine, c[0], c[1], c[2]);
    }
    __syncthreads();
    if (threadIdx.x < 256) {
        unsigned s = 0;
        for (int w = 0; w < HIST_WAVES; w++) s += h[w][threadIdx.x];
        if (s) atomicAdd(&state[threadIdx.x], s);
    }
}

struct ResolveArgs {
    unsigned *state;
    float key, min_exposure, max_exposure, adapt;
    int trim_low, trim_high;
};

__global__ __launch_bounds__(256) void k_exposure_resolve(ResolveArgs a)
{
#pragma clang fp contract(off)
    __shared__ unsigned scan[2][256];
    __shared__ unsigned long long red_m[256], red_s[256];
    const int b = threadIdx.x;
    const unsigned hb = a.state[b];
    unsigned count = 0, prev_bits = 0;                             // thread 0's words, fetched beside the bins
    if (b == 0) { count = a.state[EXP_COUNT]; prev_bits = a.state[EXP_EXPOSURE]; }
    int cur = 0;
    scan[0][b] = hb;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                            // inclusive prefix sum
        unsigned v = scan[cur][b];
        if (b >= d) v += scan[cur][b - d];
        scan[cur ^ 1][b] = v;
        cur ^= 1;
        __syncthreads();
    }
    const long long P1 = scan[cur][b], P0 = P1 - hb, n = scan[cur][255];
    const long long lo = (n * a.trim_low) >> 10, hi = (n * a.trim_high) >> 10;
    long long c = min(P1, n - hi) - max(P0, lo);
    if (c < 0) c = 0;
    red_m[b] = (unsigned long long)c;
    red_s[b] = (unsigned long long)c * (unsigned)(2 * (888 + b) + 1);
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (b < d) { red_m[b] += red_m[b + d]; red_s[b] += red_s[b + d]; }
        __syncthreads();
    }
    a.state[256 + b] = hb;
    a.state[b] = 0;
    if (b == 0) {
        const unsigned long long m = red_m[0], S = red_s[0];
        const float prev = __uint_as_float(prev_bits);
        unsigned Lbits = 0;
        float t;
        if (m > 0) {
            Lbits = (unsigned)(((S << 19) + (m >> 1)) / m);
            t = a.key / __uint_as_float(Lbits);
            if (t < a.min_exposure) t = a.min_exposure;
            if (t > a.max_exposure) t = a.max_exposure;
        } else {
            t = count > 0 ? prev : 1.0f;
        }
        const float e = count == 0 ? t : prev + ((t - prev) * a.adapt);
        a.state[EXP_N] = (unsigned)n;
        a.state[EXP_M] = (unsigned)m;
        a.state[EXP_LBITS] = Lbits;
        a.state[EXP_TARGET] = __float_as_uint(t);
        a.state[EXP_EXPOSURE] = __float_as_uint(e);
        a.state[EXP_COUNT] = count < 0x7fffffffu ? count + 1 : 0x7fffffffu;
        a.state[518] = 0;
        a.state[519] = 0;
    }
}

__global__ __launch_bounds__(256) void k_exposure_reset(unsigned *state)
{
    for (int i = threadIdx.x; i < SVGF_EXPOSURE_STATE_WORDS; i += 256)
        state[i] = (i == EXP_TARGET || i == EXP_EXPOSURE) ? 0x3f800000u : 0u;
}

struct TonemapArgs {
    uchar4 *pbo;
    const float *left, *right;      // left null: the buffer is W x H and holds right alone
    const unsigned *state;          // null: e = bias
    int W, H, op, transfer;
    float bias, iw2;                // iw2 = 1 / white^2, or 0
    float T[256];                   // transfer 2: the thresholds in tonemap_tree_order
};

// N channels of one pixel (3: right alone, 6: left and right), in place: v -> bytes.  The wave-uniform branches on op and transfer
// stand OUTSIDE the loops over the channels, so that every stage is N independent chains (the loads of all channels are issued
// before this is called; with the branches inside a per-channel function each channel's load was waited for on its own).
template <int N>
__device__ __forceinline__ void tonemap_channels(const TonemapArgs &a, const float *T, float e, const float (&v)[N], int (&out)[N])
{
#pragma clang fp contract(off)
    float y[N];
#pragma unroll
    for (int c = 0; c < N; c++) y[c] = v[c] * e;
    if (a.op != 0) {
#pragma unroll
        for (int c = 0; c < N; c++) {
            if (!(y[c] > 0.0f)) y[c] = 0.0f;
            if (y[c] > 65504.0f) y[c] = 65504.0f;
        }
        if (a.op == 1) {
#pragma unroll
            for (int c = 0; c < N; c++) y[c] = (y[c] * (1.0f + y[c] * a.iw2)) / (1.0f + y[c]);
        } else {
#pragma unroll
            for (int c = 0; c < N; c++) y[c] = (y[c] * (2.51f * y[c] + 0.03f)) / (y[c] * (2.43f * y[c] + 0.59f) + 0.14f);
        }
    }
    if (a.transfer == 2) {          // #{k in 1..255 : y >= T[k]}, T increasing: the rank of y, by binary search in eight steps.
        int i[N];                   // T is the search tree level by level (tonemap_tree_order): a step's reads are neighbours in LDS
#pragma unroll
        for (int c = 0; c < N; c++) i[c] = 1;
#pragma unroll
        for (int step = 0; step < 8; step++) {
#pragma unroll
            for (int c = 0; c < N; c++) i[c] = 2 * i[c] + (y[c] >= T[i[c]] ? 1 : 0);
        }
#pragma unroll
        for (int c = 0; c < N; c++) out[c] = i[c] - 256;
        return;
    }
    if (a.transfer == 1) {
#pragma unroll
        for (int c = 0; c < N; c++) y[c] = sqrtf(y[c]);
    }
#pragma unroll
    for (int c = 0; c < N; c++) out[c] = to_byte(y[c]);
}

__global__ __launch_bounds__(256) void k_display_tonemap(TonemapArgs a)
{
#pragma clang fp contract(off)
    __shared__ float T[256];
    if (a.transfer == 2) {
        T[threadIdx.x] = a.T[threadIdx.x];
        __syncthreads();
    }
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.W * a.H) return;
    const float e = a.state ? a.bias * __uint_as_float(a.state[EXP_EXPOSURE]) : a.bias;
    const int x = p % a.W, y = p / a.W;
    const float *r = a.right + 3 * (size_t)p;
    if (a.left) {
        const float *l = a.left + 3 * (size_t)p;
        const float v[6] = { l[0], l[1], l[2], r[0], r[1], r[2] };
        int b[6];
        tonemap_channels<6>(a, T, e, v, b);
        a.pbo[(size_t)y * 2 * a.W + x] = make_uchar4((unsigned char)b[0], (unsigned char)b[1], (unsigned char)b[2], 0);
        a.pbo[(size_t)y * 2 * a.W + a.W + x] = make_uchar4((unsigned char)b[3], (unsigned char)b[4], (unsigned char)b[5], 0);
    } else {
        const float v[3] = { r[0], r[1], r[2] };
        int b[3];
        tonemap_channels<3>(a, T, e, v, b);
        a.pbo[p] = make_uchar4((unsigned char)b[0], (unsigned char)b[1], (unsigned char)b[2], 0);
    }
}

// float32 nearest to the sRGB decode of k / 255 (c / 12.92 up to 0.04045, else ((c + 0.055) / 1.055)^2.4, in double)
const float srgb_thresholds[256] = {
    0.0f, 0.000303526991f, 0.000607053982f, 0.000910580973f, 0.00121410796f, 0.00151763496f, 0.00182116195f, 0.00212468882f,
    0.00242821593f, 0.0027317428f, 0.00303526991f, 0.00334653584f, 0.00367650739f, 0.00402471703f, 0.00439144205f, 0.00477695325f,
    0.00518151652f, 0.00560539169f, 0.00604883302f, 0.00651209056f, 0.00699541019f, 0.00749903219f, 0.00802319311f, 0.00856812578f,
    0.00913405884f, 0.00972121768f, 0.010329823f, 0.0109600937f, 0.0116122449f, 0.012286488f, 0.0129830325f, 0.0137020834f,
    0.0144438436f, 0.0152085144f, 0.0159962941f, 0.0168073755f, 0.0176419541f, 0.01850022f, 0.0193823613f, 0.0202885624f,
    0.0212190095f, 0.0221738853f, 0.0231533665f, 0.0241576321f, 0.0251868591f, 0.0262412224f, 0.0273208916f, 0.02842604f,
    0.0295568351f, 0.0307134446f, 0.0318960324f, 0.0331047662f, 0.0343398079f, 0.0356013142f, 0.0368894488f, 0.0382043719f,
    0.0395462364f, 0.0409151986f, 0.0423114114f, 0.043735031f, 0.045186203f, 0.0466650873f, 0.0481718257f, 0.0497065671f,
    0.0512694567f, 0.0528606474f, 0.054480277f, 0.0561284907f, 0.0578054301f, 0.0595112368f, 0.0612460524f, 0.0630100146f,
    0.064803265f, 0.0666259378f, 0.0684781671f, 0.0703600943f, 0.0722718537f, 0.0742135718f, 0.0761853829f, 0.078187421f,
    0.0802198201f, 0.0822827071f, 0.0843762085f, 0.0865004584f, 0.0886555836f, 0.0908417106f, 0.0930589661f, 0.0953074694f,
    0.097587347f, 0.0998987257f, 0.102241732f, 0.104616486f, 0.107023105f, 0.10946171f, 0.111932427f, 0.114435375f,
    0.116970666f, 0.119538426f, 0.122138776f, 0.124771819f, 0.127437681f, 0.130136475f, 0.13286832f, 0.135633335f,
    0.138431609f, 0.141263291f, 0.144128472f, 0.147027269f, 0.149959788f, 0.152926147f, 0.155926466f, 0.158960834f,
    0.162029371f, 0.165132195f, 0.168269396f, 0.171441108f, 0.174647406f, 0.177888423f, 0.18116425f, 0.18447499f,
    0.187820777f, 0.191201687f, 0.194617838f, 0.198069319f, 0.20155625f, 0.205078736f, 0.208636865f, 0.212230757f,
    0.215860501f, 0.219526201f, 0.223227963f, 0.226965874f, 0.230740055f, 0.23455058f, 0.238397568f, 0.242281124f,
    0.246201321f, 0.25015828f, 0.254152089f, 0.258182853f, 0.262250662f, 0.266355604f, 0.270497799f, 0.274677306f,
    0.278894275f, 0.283148736f, 0.287440836f, 0.291770637f, 0.296138257f, 0.300543785f, 0.304987311f, 0.309468925f,
    0.313988715f, 0.318546772f, 0.323143214f, 0.327778101f, 0.332451522f, 0.337163627f, 0.341914415f, 0.346704066f,
    0.351532608f, 0.356400132f, 0.361306787f, 0.366252601f, 0.371237695f, 0.376262128f, 0.38132602f, 0.386429429f,
    0.391572475f, 0.396755219f, 0.401977777f, 0.407240212f, 0.412542611f, 0.417885065f, 0.423267663f, 0.428690493f,
    0.434153646f, 0.439657182f, 0.445201188f, 0.450785786f, 0.456411034f, 0.462076992f, 0.467783809f, 0.473531485f,
    0.479320168f, 0.48514995f, 0.491020858f, 0.496932983f, 0.502886474f, 0.50888133f, 0.514917672f, 0.520995557f,
    0.527115107f, 0.533276379f, 0.539479494f, 0.545724452f, 0.55201143f, 0.558340371f, 0.564711511f, 0.571124852f,
    0.577580452f, 0.584078431f, 0.590618849f, 0.597201765f, 0.603827357f, 0.610495567f, 0.617206573f, 0.623960376f,
    0.630757153f, 0.637596846f, 0.644479692f, 0.651405632f, 0.658374846f, 0.665387273f, 0.672443151f, 0.679542482f,
    0.686685324f, 0.693871737f, 0.701101899f, 0.708375752f, 0.715693474f, 0.723055124f, 0.730460763f, 0.73791039f,
    0.745404184f, 0.752942204f, 0.760524511f, 0.768151164f, 0.775822222f, 0.783537805f, 0.791297913f, 0.799102724f,
    0.806952238f, 0.814846575f, 0.822785735f, 0.830769897f, 0.838799f, 0.846873224f, 0.854992628f, 0.863157213f,
    0.871367097f, 0.8796224f, 0.887923121f, 0.896269381f, 0.904661179f, 0.913098633f, 0.921581864f, 0.930110872f,
    0.938685715f, 0.947306514f, 0.955973327f, 0.964686275f, 0.973445296f, 0.982250571f, 0.991102099f, 1.0f,
};

// The thresholds T[1..255] as a perfect search tree stored level by level: node i of level j (i in [2^(j-1), 2^j), j = 1..8) holds
// T[(2 (i - 2^(j-1)) + 1) * 2^(8-j)]; from node i the search goes to 2 i + (y >= node), and leaves the tree at 256 + rank.  In the
// sorted order the lanes of a step read T[k + d] with k a multiple of 2 d: up to 64 addresses on one or two LDS banks.
void tonemap_tree_order(float tree[256])
{
    tree[0] = 0.0f;      // not a node
    for (int j = 1; j <= 8; j++)
        for (int i = 1 << (j - 1); i < (1 << j); i++) tree[i] = srgb_thresholds[(2 * (i - (1 << (j - 1))) + 1) << (8 - j)];
}

bool finite_positive(float x) { return x > 0.0f && x <= 3.402823466e38f; }      // false for NaN, zero, negative, +inf
bool finite_nonneg(float x) { return x >= 0.0f && x <= 3.402823466e38f; }

__global__ __launch_bounds__(256) void k_display_pack(uchar4 *pbo, const float *left, const float *right, int W, int H)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= W * H) return;
    const int x = p % W, y = p / W;
    const float *l = left + 3 * (size_t)p, *r = right + 3 * (size_t)p;
    uchar4 a, b;
    a.x = (unsigned char)to_byte(l[0]); a.y = (unsigned char)to_byte(l[1]); a.z = (unsigned char)to_byte(l[2]); a.w = 0;
    b.x = (unsigned char)to_byte(r[0]); b.y = (unsigned char)to_byte(r[1]); b.z = (unsigned char)to_byte(r[2]); b.w = 0;
    pbo[(size_t)y * 2 * W + x] = a;
    pbo[(size_t)y * 2 * W + W + x] = b;
}

// ---- minimal PNG encoder: IHDR + one IDAT of stored deflate blocks + IEND ----
uint32_t crc_table[256];
bool crc_ready = false;
uint32_t crc32_update(uint32_t c, const unsigned char *buf, size_t n)
{
    if (!crc_ready) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t k = i;
            for (int j = 0; j < 8; j++) k = (k & 1) ? 0xEDB88320u ^ (k >> 1) : k >> 1;
            crc_table[i] = k;
        }
        crc_ready = true;
    }
    for (size_t i = 0; i < n; i++) c = crc_table[(c ^ buf[i]) & 0xFF] ^ (c >> 8);
    return c;
}
void put_be32(std::vector<unsigned char> &v, uint32_t x)
{
    v.push_back((unsigned char)(x >> 24)); v.push_back((unsigned char)(x >> 16));
    v.push_back((unsigned char)(x >> 8)); v.push_back((unsigned char)x);
}
bool write_chunk(FILE *f, const char tag[4], const std::vector<unsigned char> &data)
{
    std::vector<unsigned char> head;
    put_be32(head, (uint32_t)data.size());
    head.insert(head.end(), tag, tag + 4);
    uint32_t c = crc32_update(0xFFFFFFFFu, reinterpret_cast<const unsigned char *>(tag), 4);
    c = crc32_update(c, data.data(), data.size()) ^ 0xFFFFFFFFu;
    std::vector<unsigned char> tail;
    put_be32(tail, c);
    return fwrite(head.data(), 1, head.size(), f) == head.size() &&
           (data.empty() || fwrite(data.data(), 1, data.size(), f) == data.size()) &&
           fwrite(tail.data(), 1, 4, f) == 4;
}

}  // namespace

extern "C" {

int svgf_display_pack(int device, void *pbo_rgba8_dev, const void *left_rgb_dev, const void *right_rgb_dev, int width,
                      int height, void *stream)
{
    if (!pbo_rgba8_dev || !left_rgb_dev || !right_rgb_dev || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    const int n = width * height;
    hipLaunchKernelGGL(k_display_pack, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<uchar4 *>(pbo_rgba8_dev), static_cast<const float *>(left_rgb_dev),
                       static_cast<const float *>(right_rgb_dev), width, height);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

int svgf_exposure_reset(int device, void *state_dev, void *stream)
{
    if (!state_dev) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    hipLaunchKernelGGL(k_exposure_reset, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<unsigned *>(state_dev));
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

int svgf_exposure_meter(int device, void *state_dev, const void *rgb_dev, int width, int height, const SvgfExposureParams *ep,
                        void *stream)
{
    if (!state_dev || !rgb_dev || !ep || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if (!finite_positive(ep->key) || !finite_positive(ep->min_exposure) || !finite_positive(ep->max_exposure) ||
        ep->min_exposure > ep->max_exposure || !(ep->adapt > 0.0f && ep->adapt <= 1.0f))
        return SVGF_ERR_INVALID_ARG;
    if (ep->trim_low_1024 < 0 || ep->trim_low_1024 > 1023 || ep->trim_high_1024 < 0 || ep->trim_high_1024 > 1023 ||
        ep->trim_low_1024 + ep->trim_high_1024 > 1023)
        return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    const int n = width * height;
    const int vec = (reinterpret_cast<uintptr_t>(rgb_dev) & 15) == 0;
    const int items = vec ? (n + 3) / 4 : n;
    int blocks = (items + HIST_BLOCK - 1) / HIST_BLOCK;
    if (blocks > HIST_MAX_BLOCKS) blocks = HIST_MAX_BLOCKS;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_luma_histogram, dim3(blocks), dim3(HIST_BLOCK), 0, s, static_cast<unsigned *>(state_dev),
                       static_cast<const float *>(rgb_dev), n, vec);
    if (hipGetLastError() != hipSuccess) return SVGF_ERR_HIP;
    ResolveArgs a;
    a.state = static_cast<unsigned *>(state_dev);
    a.key = ep->key; a.min_exposure = ep->min_exposure; a.max_exposure = ep->max_exposure; a.adapt = ep->adapt;
    a.trim_low = ep->trim_low_1024; a.trim_high = ep->trim_high_1024;
    hipLaunchKernelGGL(k_exposure_resolve, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

int svgf_display_tonemap(int device, void *pbo_rgba8_dev, const void *left_rgb_dev, const void *right_rgb_dev, int width,
                         int height, const SvgfTonemapParams *tp, const void *state_dev, void *stream)
{
    if (!pbo_rgba8_dev || !right_rgb_dev || !tp || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if (tp->op < 0 || tp->op > 2 || tp->transfer < 0 || tp->transfer > 2 || !finite_nonneg(tp->exposure_bias) ||
        !finite_nonneg(tp->white))
        return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    TonemapArgs a;
    a.pbo = static_cast<uchar4 *>(pbo_rgba8_dev);
    a.left = static_cast<const float *>(left_rgb_dev); a.right = static_cast<const float *>(right_rgb_dev);
    a.state = static_cast<const unsigned *>(state_dev);
    a.W = width; a.H = height; a.op = tp->op; a.transfer = tp->transfer;
    a.bias = tp->exposure_bias;
    a.iw2 = tp->white > 0.0f ? 1.0f / (tp->white * tp->white) : 0.0f;
    tonemap_tree_order(a.T);
    const int n = width * height;
    hipLaunchKernelGGL(k_display_tonemap, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

int svgf_tonemap_srgb_table(float thresholds[256])
{
    if (!thresholds) return SVGF_ERR_INVALID_ARG;
    memcpy(thresholds, srgb_thresholds, sizeof(srgb_thresholds));
    return SVGF_OK;
}

int svgf_save_png(const char *path, const float *rgb_host, int width, int height, int mirror_x)
{
    if (!path || !rgb_host || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    // scanlines: filter byte 0 + 3*W bytes
    const size_t row = 1 + 3 * (size_t)width;
    std::vector<unsigned char> raw(row * height);
    for (int y = 0; y < height; y++) {
        unsigned char *d = raw.data() + row * y;
        *d++ = 0;
        for (int x = 0; x < width; x++) {
            const int sx = mirror_x ? (width - 1 - x) : x;            // saveImage: img.setPixel(width - 1 - x, y, pix)
            const float *p = rgb_host + 3 * ((size_t)y * width + sx);
            for (int c = 0; c < 3; c++) {
                float v = p[c];
                v = (v < 0.0f) ? 0.0f : ((v > 1.0f) ? 1.0f : v);      // glm::clamp(pix, 0, 1); NaN fails both tests
                if (!(v == v)) v = 0.0f;                              // (unsigned char)NaN is undefined in C++: define 0
                *d++ = (unsigned char)(v * 255.0f);
            }
        }
    }
    // zlib stream of stored blocks
    std::vector<unsigned char> z;
    z.push_back(0x78); z.push_back(0x01);
    uint32_t s1 = 1, s2 = 0;
    for (size_t off = 0; off < raw.size();) {
        const size_t n = (raw.size() - off < 65535) ? raw.size() - off : 65535;
        z.push_back(off + n == raw.size() ? 1 : 0);
        z.push_back((unsigned char)(n & 0xFF)); z.push_back((unsigned char)(n >> 8));
        z.push_back((unsigned char)(~n & 0xFF)); z.push_back((unsigned char)((~n >> 8) & 0xFF));
        z.insert(z.end(), raw.begin() + off, raw.begin() + off + n);
        for (size_t i = 0; i < n; i++) { s1 = (s1 + raw[off + i]) % 65521u; s2 = (s2 + s1) % 65521u; }
        off += n;
    }
    put_be32(z, (s2 << 16) | s1);

    FILE *f = fopen(path, "wb");
    if (!f) return SVGF_ERR_INVALID_ARG;
    static const unsigned char sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
    bool ok = fwrite(sig, 1, 8, f) == 8;
    std::vector<unsigned char> ihdr;
    put_be32(ihdr, (uint32_t)width); put_be32(ihdr, (uint32_t)height);
    ihdr.push_back(8); ihdr.push_back(2); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);   // 8-bit RGB
    ok = ok && write_chunk(f, "IHDR", ihdr) && write_chunk(f, "IDAT", z) && write_chunk(f, "IEND", {});
    ok = (fclose(f) == 0) && ok;
    return ok ? SVGF_OK : SVGF_ERR_INVALID_ARG;
}

}  // extern "C"
