// svgf_lbvh.hip — row f24, libsvgf_lbvh.so: a linear BVH over the resident scene's padded triangle boxes as drawn, built on the device
// in 5 + 3 * passes launches (include/svgf_lbvh.h states the result; svgf_lbvh_host.cpp computes it on the host; the arithmetic both
// compile is svgf_lbvh_core.h).  The library reaches the scene through svgf_scene_view and svgf_scene_adopt_tree alone.
//
// Kernel boundaries are the only synchronisation between workgroups: nothing here spins, hands a flag over inside a
// launch or climbs the tree with atomics.  The one atomic between workgroups (the top list's counter) is consumed by a later launch.
//   k_lbvh_bounds      per-block fminf / fmaxf of the centroids -> partial[]; block 0 clears the top list's counter
//   k_lbvh_keys        every block folds partial[] again (<= 256 entries), then one key per thread
//   per 8-bit digit:   k_lbvh_count (LDS histogram per 2048 keys, digit-major), k_lbvh_scan (ONE workgroup, exclusive prefix),
//                      k_lbvh_scatter (ranks by wave ballots, four waves joined through LDS: stable)
//   k_lbvh_hierarchy   one thread per internal node: both child records, a leaf child's box, the node's range; the child's slot;
//                      a node whose range spans two tiles of 512 leaves joins the top list
//   k_lbvh_tiles       one workgroup per tile: the boxes of the nodes inside it, in LDS, one barrier per sweep
//   k_lbvh_top         ONE workgroup: the nodes that span tiles, the same way through global memory (as k_scene_refit_top does)
// No runtime-indexed private array (0 B of scratch); the 32-byte node records move as two float4.
#include "svgf_kernels.h"
#include "../../include/svgf_lbvh.h"
#include "svgf_lbvh_core.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

namespace {

constexpr int kTile = SVGF_LBVH_TILE;
constexpr int kSortBlock = 2048;        // keys per workgroup of count / scatter: 8 rounds of 256
constexpr int kMaxSweeps = 64;          // > key_bits + 1: a bound on every box loop, whatever the arrays hold

struct LbvhArgs {
    const float4 *tri_boxes;
    int n_tris, n_leaves, L, nb, n_partial, top_cap;
    LbvhBits bits;
    lbvh_key *keys_a, *keys_b;
    const lbvh_key *sorted;
    unsigned *hist;
    float4 *partial;
    int2 *range;
    int *slot, *stamp, *top, *top_count;
    float4 *nodes;
    int *order;
};

struct DevKeys {
    const lbvh_key *sorted;
    int L;
    __device__ __forceinline__ lbvh_key operator()(int k) const { return sorted[(size_t)k * L]; }
};

// fminf / fmaxf of 256 threads' values; the result in every thread.  s: 6 x 256 floats of LDS.
__device__ __forceinline__ void block_minmax(float mn[3], float mx[3], float *s)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; c++) { s[256 * c + t] = mn[c]; s[256 * (3 + c) + t] = mx[c]; }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                s[256 * c + t] = fminf(s[256 * c + t], s[256 * c + t + w]);
                s[256 * (3 + c) + t] = fmaxf(s[256 * (3 + c) + t], s[256 * (3 + c) + t + w]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { mn[c] = s[256 * c]; mx[c] = s[256 * (3 + c)]; }
}

__global__ __launch_bounds__(256) void k_lbvh_bounds(LbvhArgs a)
{
#pragma clang fp contract(off)
    __shared__ float s[6 * 256];
    float mn[3] = { __builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf() };
    float mx[3] = { -__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf() };
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n_tris; i += a.n_partial * 256) {
        const float4 lo = a.tri_boxes[2 * (size_t)i], hi = a.tri_boxes[2 * (size_t)i + 1];
        const float c[3] = { lbvh_centroid(lo.x, hi.x), lbvh_centroid(lo.y, hi.y), lbvh_centroid(lo.z, hi.z) };
#pragma unroll
        for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], c[k]); mx[k] = fmaxf(mx[k], c[k]); }
    }
    block_minmax(mn, mx, s);
    if (threadIdx.x == 0) {
        a.partial[2 * blockIdx.x] = make_float4(mn[0], mn[1], mn[2], 0.0f);
        a.partial[2 * blockIdx.x + 1] = make_float4(mx[0], mx[1], mx[2], 0.0f);
        if (blockIdx.x == 0) *a.top_count = 0;
    }
}

__global__ __launch_bounds__(256) void k_lbvh_keys(LbvhArgs a)
{
#pragma clang fp contract(off)
    __shared__ float s[6 * 256];
    float mn[3] = { __builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf() };
    float mx[3] = { -__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf() };
    if ((int)threadIdx.x < a.n_partial) {
        const float4 lo = a.partial[2 * threadIdx.x], hi = a.partial[2 * threadIdx.x + 1];
        mn[0] = lo.x; mn[1] = lo.y; mn[2] = lo.z; mx[0] = hi.x; mx[1] = hi.y; mx[2] = hi.z;
    }
    block_minmax(mn, mx, s);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_tris) {
        const float4 lo4 = a.tri_boxes[2 * (size_t)i], hi4 = a.tri_boxes[2 * (size_t)i + 1];
        const float lo[3] = { lo4.x, lo4.y, lo4.z }, hi[3] = { hi4.x, hi4.y, hi4.z };
        a.keys_a[i] = lbvh_make_key(lo, hi, mn, mx, a.bits, i);
    }
}

// ---- the sort: LSD radix, 8-bit digits, hist[digit * nb + block] ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lbvh_count(LbvhArgs a, const lbvh_key *src, int shift)
{
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * kSortBlock;
    for (int r = 0; r < kSortBlock / 256; r++) {
        const int i = base + r * 256 + threadIdx.x;
        if (i < a.n_tris) atomicAdd(&h[(unsigned)(src[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    a.hist[threadIdx.x * a.nb + blockIdx.x] = h[threadIdx.x];
}

// ONE workgroup: hist[] becomes its own exclusive prefix sum
__global__ __launch_bounds__(1024) void k_lbvh_scan(LbvhArgs a)
{
    __shared__ unsigned s[1024];
    const int total = 256 * a.nb, per = (total + 1023) / 1024, t = threadIdx.x;
    const int b = t * per, e = (b + per < total) ? b + per : total;
    unsigned sum = 0;
    for (int k = b; k < e; k++) sum += a.hist[k];
    s[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned v = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    unsigned run = s[t] - sum;
    for (int k = b; k < e; k++) { const unsigned v = a.hist[k]; a.hist[k] = run; run += v; }
}

// Stable: a key's place is its digit's offset for this block, plus the keys of that digit in the rounds before, in the waves before and
// in the lanes before.  The lanes of a wave that hold the same digit are found with eight ballots.
__global__ __launch_bounds__(256) void k_lbvh_scatter(LbvhArgs a, const lbvh_key *src, lbvh_key *dst, int shift)
{
    __shared__ unsigned run[256];
    __shared__ unsigned wcnt[4 * 256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    run[t] = a.hist[t * a.nb + blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; k++) wcnt[256 * k + t] = 0;
    const int base = blockIdx.x * kSortBlock;
    for (int r = 0; r < kSortBlock / 256; r++) {
        __syncthreads();                                    // run[] and the cleared wcnt[] of the round before
        const int i = base + r * 256 + t;
        const bool valid = i < a.n_tris;
        const lbvh_key key = valid ? src[i] : 0;
        const unsigned d = (unsigned)(key >> shift) & 255u;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const unsigned rank = __popcll(same & ((1ull << lane) - 1ull)), cnt = __popcll(same);
        if (valid && rank == 0) wcnt[256 * w + d] = cnt;
        __syncthreads();
        if (valid) {
            unsigned pos = run[d] + rank;
            for (int k = 0; k < w; k++) pos += wcnt[256 * k + d];
            if (pos < (unsigned)a.n_tris) dst[pos] = key;
        }
        __syncthreads();
        unsigned add = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { add += wcnt[256 * k + t]; wcnt[256 * k + t] = 0; }
        run[t] += add;
    }
}

// ---- hierarchy ------------------------------------------------------------------------------------------------------------------------------
// leaf k's record: the union of its triangles' stored boxes
__device__ __forceinline__ void lbvh_leaf(const LbvhArgs &a, lbvh_key idx_mask, int k, float4 &lo, float4 &hi)
{
    const int first = k * a.L, count = (a.n_tris - first < a.L) ? a.n_tris - first : a.L;
    for (int t = first; t < first + count; t++) {
        int i = (int)(a.sorted[t] & idx_mask);
        i = i < a.n_tris ? i : a.n_tris - 1;
        const float4 b0 = a.tri_boxes[2 * (size_t)i], b1 = a.tri_boxes[2 * (size_t)i + 1];
        if (t == first) { lo = b0; hi = b1; }
        else {
            lo.x = fminf(lo.x, b0.x); lo.y = fminf(lo.y, b0.y); lo.z = fminf(lo.z, b0.z);
            hi.x = fmaxf(hi.x, b1.x); hi.y = fmaxf(hi.y, b1.y); hi.z = fmaxf(hi.z, b1.z);
        }
    }
    lo.w = __int_as_float(first); hi.w = __int_as_float(count);
}

__global__ __launch_bounds__(256) void k_lbvh_hierarchy(LbvhArgs a)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    const lbvh_key idx_mask = ((lbvh_key)1 << a.bits.idx_bits) - 1;
    if (g < a.n_tris) {
        const int i = (int)(a.sorted[g] & idx_mask);
        a.order[g] = i < a.n_tris ? i : a.n_tris - 1;
    }
    if (a.n_leaves == 1) {
        if (g == 0) {
            float4 lo, hi;
            lbvh_leaf(a, idx_mask, 0, lo, hi);
            a.nodes[0] = lo; a.nodes[1] = hi;
        }
        return;
    }
    if (g >= a.n_leaves - 1) return;
    int lo, hi, gamma;
    lbvh_node(DevKeys{ a.sorted, a.L }, a.n_leaves, a.bits.key_bits, g, lo, hi, gamma);
#pragma unroll
    for (int side = 0; side < 2; side++) {
        const int child = gamma + side, at = 1 + 2 * g + side;
        float4 clo = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(1 + 2 * child)), chi = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0));
        if (side == 0 ? lo == gamma : hi == gamma + 1) lbvh_leaf(a, idx_mask, child, clo, chi);
        else a.slot[child] = at;
        a.nodes[2 * (size_t)at] = clo; a.nodes[2 * (size_t)at + 1] = chi;
    }
    if (g == 0) a.slot[0] = 0;
    a.range[g] = make_int2(lo, hi);
    a.stamp[g] = 0;
    if (lo / kTile != hi / kTile) {
        const int pos = atomicAdd(a.top_count, 1);
        if (pos < a.top_cap) a.top[pos] = g;
    }
}

// ---- boxes ----------------------------------------------------------------------------------------------------------------------------------
// A subtree's leaves and its internal indices are one contiguous range, so a node whose range lies inside tile b has every descendant
// in tile b too.  Thread t of workgroup b owns internal node b * 512 + t.  stamp 0 = pending, s = finished in sweep s; a sweep only
// trusts stamps below its own number, which were written in front of the barrier that ended the sweep before.
__global__ __launch_bounds__(kTile) void k_lbvh_tiles(LbvhArgs a)
{
    __shared__ float4 sbox[2 * kTile];
    __shared__ int sstamp[kTile];
    const int t = threadIdx.x, base = blockIdx.x * kTile, i = base + t, n_nodes = 2 * a.n_leaves - 1;
    sstamp[t] = 0;
    bool pending = false, leaf0 = false, leaf1 = false;
    int c0 = -1, c1 = -1, sl = -1;
    float4 alo, ahi, blo, bhi;
    alo = ahi = blo = bhi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < a.n_leaves - 1) {
        const int2 rg = a.range[i];
        if (rg.x / kTile == rg.y / kTile) {
            pending = true;
            sl = a.slot[i];
            const size_t at = 1 + 2 * (size_t)i;
            alo = a.nodes[2 * at]; ahi = a.nodes[2 * at + 1]; blo = a.nodes[2 * at + 2]; bhi = a.nodes[2 * at + 3];
            leaf0 = __float_as_int(ahi.w) > 0; leaf1 = __float_as_int(bhi.w) > 0;
            c0 = ((__float_as_int(alo.w) - 1) >> 1) - base; c1 = ((__float_as_int(blo.w) - 1) >> 1) - base;
            if (!leaf0 && (c0 < 0 || c0 >= kTile)) c0 = -1;          // never ready: the node stays pending and the sweep bound ends the loop
            if (!leaf1 && (c1 < 0 || c1 >= kTile)) c1 = -1;
            if (sl < 0 || sl >= n_nodes) pending = false;
        }
    }
    __syncthreads();
    for (int s = 1; s <= kMaxSweeps; s++) {
        if (pending) {
            const int st0 = (leaf0 || c0 < 0) ? 0 : sstamp[c0], st1 = (leaf1 || c1 < 0) ? 0 : sstamp[c1];
            const bool r0 = leaf0 || (st0 != 0 && st0 < s), r1 = leaf1 || (st1 != 0 && st1 < s);
            if (r0 && r1) {
                if (!leaf0) { alo = sbox[2 * c0]; ahi = sbox[2 * c0 + 1]; }
                if (!leaf1) { blo = sbox[2 * c1]; bhi = sbox[2 * c1 + 1]; }
                const float4 lo = make_float4(fminf(alo.x, blo.x), fminf(alo.y, blo.y), fminf(alo.z, blo.z), __int_as_float(1 + 2 * i));
                const float4 hi = make_float4(fmaxf(ahi.x, bhi.x), fmaxf(ahi.y, bhi.y), fmaxf(ahi.z, bhi.z), __int_as_float(0));
                sbox[2 * t] = lo; sbox[2 * t + 1] = hi;
                sstamp[t] = s;
                a.nodes[2 * (size_t)sl] = lo; a.nodes[2 * (size_t)sl + 1] = hi;
                a.stamp[i] = 1;
                pending = false;
            }
        }
        if (!__syncthreads_or(pending ? 1 : 0)) break;
    }
}

// ONE workgroup: the nodes that span tiles.  A child is a leaf, a node the launch before finished (stamp 1) or a top node of an
// earlier sweep; sweeps count from 2.
__global__ __launch_bounds__(1024) void k_lbvh_top(LbvhArgs a)
{
    const int n_nodes = 2 * a.n_leaves - 1;
    int n_top = *a.top_count;
    n_top = n_top < a.top_cap ? n_top : a.top_cap;
    for (int s = 2; s < 2 + kMaxSweeps; s++) {
        int pending = 0;
        for (int e = threadIdx.x; e < n_top; e += 1024) {
            const int i = a.top[e];
            if (i < 0 || i >= a.n_leaves - 1 || a.stamp[i] != 0) continue;
            const size_t at = 1 + 2 * (size_t)i;
            const float4 alo = a.nodes[2 * at], ahi = a.nodes[2 * at + 1], blo = a.nodes[2 * at + 2], bhi = a.nodes[2 * at + 3];
            const int c0 = (__float_as_int(alo.w) - 1) >> 1, c1 = (__float_as_int(blo.w) - 1) >> 1;
            bool r0 = __float_as_int(ahi.w) > 0, r1 = __float_as_int(bhi.w) > 0;
            if (!r0 && c0 >= 0 && c0 < a.n_leaves - 1) { const int st = a.stamp[c0]; r0 = st != 0 && st < s; }
            if (!r1 && c1 >= 0 && c1 < a.n_leaves - 1) { const int st = a.stamp[c1]; r1 = st != 0 && st < s; }
            const int sl = a.slot[i];
            if (r0 && r1 && sl >= 0 && sl < n_nodes) {
                a.nodes[2 * (size_t)sl] = make_float4(fminf(alo.x, blo.x), fminf(alo.y, blo.y), fminf(alo.z, blo.z), __int_as_float(1 + 2 * i));
                a.nodes[2 * (size_t)sl + 1] = make_float4(fmaxf(ahi.x, bhi.x), fmaxf(ahi.y, bhi.y), fmaxf(ahi.z, bhi.z), __int_as_float(0));
                a.stamp[i] = s;
            } else {
                pending = 1;
            }
        }
        if (!__syncthreads_or(pending)) break;
    }
}

constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

struct svgf_lbvh {
    const svgf_scene *scene;
    int device, passes;
    char *dev;
    LbvhArgs args;
    SvgfLbvhInfo info;
};

extern "C" int svgf_lbvh_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_lbvh_create(const svgf_scene *scene, const SvgfLbvhParams *p, svgf_lbvh **out)
{
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    if (!scene || (p && (p->leaf_tris < 0 || p->leaf_tris > 8))) return SVGF_ERR_INVALID_ARG;
    SvgfSceneView v;
    if (svgf_scene_view(scene, &v) != SVGF_OK || v.n_tris < 1 || v.n_tris > SVGF_SCENE_MAX_TRIS) return SVGF_ERR_INVALID_ARG;
    const int n = v.n_tris, L = (p && p->leaf_tris) ? p->leaf_tris : 4, n_leaves = (n + L - 1) / L;
    const LbvhBits bits = lbvh_bits(n);
    const int passes = lbvh_passes(bits.key_bits), nb = (n + kSortBlock - 1) / kSortBlock;
    const int n_partial = (n + 255) / 256 < 256 ? (n + 255) / 256 : 256, n_tiles = (n_leaves + kTile - 1) / kTile;
    // a node that spans tiles contains one of the n_tiles - 1 seams, and the nodes that contain one seam are a path of <= key_bits nodes
    const long long cap = (long long)bits.key_bits * (n_tiles - 1);
    const int top_cap = (int)(cap < n_leaves ? (cap > 0 ? cap : 1) : n_leaves);
    // one allocation: [keys a | keys b | hist | partial | range | slot | stamp | top | top_count | nodes | order], 16-byte aligned parts
    const size_t o_ka = 0, o_kb = o_ka + align16(8 * (size_t)n), o_h = o_kb + align16(8 * (size_t)n), o_p = o_h + align16(4 * 256 * (size_t)nb);
    const size_t o_r = o_p + 32 * (size_t)n_partial, o_s = o_r + align16(8 * (size_t)n_leaves), o_st = o_s + align16(4 * (size_t)n_leaves);
    const size_t o_t = o_st + align16(4 * (size_t)n_leaves), o_tc = o_t + align16(4 * (size_t)top_cap), o_n = o_tc + 16;
    const size_t o_o = o_n + 32 * 2 * (size_t)n_leaves, bytes = o_o + align16(4 * (size_t)n);
    svgf_lbvh *t = new (std::nothrow) svgf_lbvh();
    if (!t) return SVGF_ERR_OOM;
    SvgfDeviceGuard dev_guard(v.device);
    if (!dev_guard.ok) { (void)hipGetLastError(); delete t; return SVGF_ERR_NO_DEVICE; }
    char *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) { (void)hipGetLastError(); delete t; return SVGF_ERR_OOM; }
    if (hipMemset(d, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); (void)hipFree(d); delete t; return SVGF_ERR_HIP; }
    t->scene = scene; t->device = v.device; t->passes = passes; t->dev = d;
    LbvhArgs &a = t->args;
    a.tri_boxes = nullptr;
    a.n_tris = n; a.n_leaves = n_leaves; a.L = L; a.nb = nb; a.n_partial = n_partial; a.top_cap = top_cap; a.bits = bits;
    a.keys_a = reinterpret_cast<lbvh_key *>(d + o_ka); a.keys_b = reinterpret_cast<lbvh_key *>(d + o_kb);
    a.sorted = (passes & 1) ? a.keys_b : a.keys_a;
    a.hist = reinterpret_cast<unsigned *>(d + o_h); a.partial = reinterpret_cast<float4 *>(d + o_p);
    a.range = reinterpret_cast<int2 *>(d + o_r); a.slot = reinterpret_cast<int *>(d + o_s); a.stamp = reinterpret_cast<int *>(d + o_st);
    a.top = reinterpret_cast<int *>(d + o_t); a.top_count = reinterpret_cast<int *>(d + o_tc);
    a.nodes = reinterpret_cast<float4 *>(d + o_n); a.order = reinterpret_cast<int *>(d + o_o);
    const int depth_bound = bits.key_bits < n_leaves - 1 ? bits.key_bits : n_leaves - 1;
    t->info = SvgfLbvhInfo{ n, n_leaves, 2 * n_leaves - 1, L, bits.idx_bits, bits.axis_bits, bits.key_bits, depth_bound, 5 + 3 * passes,
                            (unsigned long long)bytes };
    *out = t;
    return SVGF_OK;
}

extern "C" int svgf_lbvh_build(svgf_lbvh *t, void *stream)
{
    if (!t) return SVGF_ERR_INVALID_ARG;
    SvgfSceneView v;
    if (svgf_scene_view(t->scene, &v) != SVGF_OK || v.n_tris != t->args.n_tris || !v.tri_boxes || v.device != t->device) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(t->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    LbvhArgs a = t->args;
    a.tri_boxes = reinterpret_cast<const float4 *>(v.tri_boxes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = a.n_tris;
    hipLaunchKernelGGL(k_lbvh_bounds, dim3(a.n_partial), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_lbvh_keys, dim3((n + 255) / 256), dim3(256), 0, st, a);
    for (int p = 0; p < t->passes; p++) {
        const lbvh_key *src = (p & 1) ? a.keys_b : a.keys_a;
        lbvh_key *dst = (p & 1) ? a.keys_a : a.keys_b;
        hipLaunchKernelGGL(k_lbvh_count, dim3(a.nb), dim3(256), 0, st, a, src, 8 * p);
        hipLaunchKernelGGL(k_lbvh_scan, dim3(1), dim3(1024), 0, st, a);
        hipLaunchKernelGGL(k_lbvh_scatter, dim3(a.nb), dim3(256), 0, st, a, src, dst, 8 * p);
    }
    hipLaunchKernelGGL(k_lbvh_hierarchy, dim3((n + 255) / 256), dim3(256), 0, st, a);
    const int inner = a.n_leaves > 1 ? a.n_leaves - 1 : 1;
    hipLaunchKernelGGL(k_lbvh_tiles, dim3((inner + kTile - 1) / kTile), dim3(kTile), 0, st, a);
    hipLaunchKernelGGL(k_lbvh_top, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_lbvh_attach(svgf_lbvh *t, svgf_scene *scene)
{
    if (!t || !scene || scene != t->scene) return SVGF_ERR_INVALID_ARG;
    return svgf_scene_adopt_tree(scene, reinterpret_cast<const SvgfBvhNode *>(t->args.nodes), t->args.order, t->info.n_nodes, t->info.n_leaves,
                                 t->info.depth_bound);
}

extern "C" int svgf_lbvh_info(const svgf_lbvh *t, SvgfLbvhInfo *out)
{
    if (!t || !out) return SVGF_ERR_INVALID_ARG;
    *out = t->info;
    return SVGF_OK;
}

extern "C" int svgf_lbvh_read(const svgf_lbvh *t, int which, void *host_dst, unsigned long long host_bytes)
{
    if (!t || which < 0 || which > 2 || !host_dst) return SVGF_ERR_INVALID_ARG;
    const void *src[3] = { t->args.nodes, t->args.order, t->args.sorted };
    const unsigned long long size[3] = { 32ull * t->info.n_nodes, 4ull * t->info.n_tris, 8ull * t->info.n_tris };
    if (host_bytes != size[which]) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(t->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_dst, src[which], (size_t)host_bytes, hipMemcpyDeviceToHost) != hipSuccess) return SVGF_ERR_HIP;
    return SVGF_OK;
}

extern "C" void svgf_lbvh_destroy(svgf_lbvh *t)
{
    if (!t) return;
    {
        SvgfDeviceGuard dev_guard(t->device);
        if (dev_guard.ok) { (void)hipDeviceSynchronize(); (void)hipFree(t->dev); }
    }
    delete t;
}
