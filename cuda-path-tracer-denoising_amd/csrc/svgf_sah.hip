// svgf_sah.hip — row f25, libsvgf_sah.so: svgf_bvh_build_host's binned-SAH tree over the resident scene's triangles as drawn, built on
// the device in 2 + 5 * rounds launches (include/svgf_sah.h states the result and the layout).  The library reaches the scene through
// svgf_scene_view and svgf_scene_adopt_tree alone.
//
// Kernel boundaries are the only synchronisation between workgroups.  What workgroups share is integer counts and
// min / max of floats through the monotone integer view of their bits (sah_key); no thread adds a float to another thread's, so the
// bytes do not depend on who came first.  The slot a node gets in a round's table does (an atomic counter hands them out), and no
// output byte depends on the slot.
//   k_sah_init       zero records, order = identity, centroids, the counters, the root's slot (or its entry in the small list)
//   per round r, over the nodes of more than 256 triangles at depth r (one slot each; node_of[p] names the slot of position p):
//     k_sah_bounds   centroid bounds and box per node: LDS per workgroup (a block of 256 positions meets at most two such nodes), one flush
//     k_sah_hist     3 x 16 counts and bin boxes per node, the same way (336 words per node in LDS)
//     k_sah_decide   one wave per node: lane (axis, plane) prices its plane in double, the first strict minimum wins; the record, the
//                    children's slots (or small-list entries)
//     k_sah_count    flags (bin_of <= best bin) per block and node part
//     k_sah_scatter  stable: a flag's rank = the blocks before (summed from k_sah_count's words) + the waves before + the lanes before
//   k_sah_small      one wave per subtree of <= 256 triangles: box, centroid and two order buffers in LDS, the same rules over its own
//                    node stack; a node a round left larger runs the same code through global memory
// A round with no slot exits on the device counter.  No runtime-indexed private array.
#include "svgf_kernels.h"
#include "../../include/svgf_sah.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

namespace {

constexpr int kSmall = SVGF_SAH_SMALL;
constexpr int kBlock = 256;             // positions per workgroup of the round kernels; <= kSmall + 1, so a block meets <= 2 large nodes
constexpr int kBins = 16;
constexpr int kHist = 3 * kBins * 7;    // 48 counts, then 48 boxes of 6 keys
constexpr unsigned kKeyPosInf = 0xFF800000u, kKeyNegInf = 0x007FFFFFu;
static_assert(kBlock <= kSmall + 1, "a block of positions must not hold a whole large node");

struct SahSlot {
    int b, e, level, rec;
    unsigned cb[6], bx[6];              // keys: centroid min xyz, max xyz; box lo xyz, hi xyz
    int pred, axis, bin, pl, nl, child[2];
    float lo, ext;
    int pad;
    unsigned hist[kHist];
};

struct SahArgs {
    const float *tris;
    const float4 *tri_boxes;
    int n, L, rounds, max_slots, small_cap, n_blocks;
    float *cen;
    int *ord[2], *node_of[2], *order;
    SahSlot *slots[2];
    int4 *small;
    int *ctr;                           // [0 .. rounds] slots of round r, [rounds + 1] entries of the small list
    unsigned *blk;
    int *counts;
    float4 *rec;
};

__device__ __forceinline__ unsigned sah_key(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float sah_unkey(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// total: the comparisons come before the cast
__device__ __forceinline__ int sah_bin(float v, float lo, float ext)
{
#pragma clang fp contract(off)
    const float q = ((v - lo) / ext) * (float)kBins;
    return !(q >= 0.0f) ? 0 : (q >= (float)kBins ? kBins - 1 : (int)q);
}

__device__ __forceinline__ bool sah_axis_ok(float ext) { return ext > 0.0f && ext <= 3.402823466e+38f; }

__device__ __forceinline__ long long sah_room(int L, int below) { return below >= 40 ? (1LL << 62) : (below < 0 ? 0 : (long long)L << below); }

__device__ __forceinline__ float wave_min(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ double sah_area(const unsigned k[6])
{
#pragma clang fp contract(off)
    const double x = (double)sah_unkey(k[3]) - sah_unkey(k[0]), y = (double)sah_unkey(k[4]) - sah_unkey(k[1]), z = (double)sah_unkey(k[5]) - sah_unkey(k[2]);
    return x * y + y * z + z * x;
}

// One wave prices the 45 planes of a node of n triangles: lane = 16 * axis + plane.  hist: 48 counts, then 48 x 6 keys.  Returns
// whether a plane is usable; the winner's lane (the first strict minimum in lane order) and its left count in every lane.
__device__ __forceinline__ bool sah_choose(const unsigned *hist, int n, unsigned axis_mask, int lane, int &best_lane, int &best_left)
{
#pragma clang fp contract(off)
    const int axis = lane >> 4, plane = lane & 15;
    double cost = __builtin_huge_val();
    int left = 0;
    if (lane < 48 && plane < kBins - 1 && ((axis_mask >> axis) & 1u)) {
        unsigned l[6] = { kKeyPosInf, kKeyPosInf, kKeyPosInf, kKeyNegInf, kKeyNegInf, kKeyNegInf };
        unsigned r[6] = { kKeyPosInf, kKeyPosInf, kKeyPosInf, kKeyNegInf, kKeyNegInf, kKeyNegInf };
        for (int k = 0; k < kBins; k++) {
            const unsigned *bb = hist + 48 + 6 * (16 * axis + k);
            const bool on_left = k <= plane;
            if (on_left) left += (int)hist[16 * axis + k];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const unsigned lo = bb[c], hi = bb[3 + c];
                if (on_left) { l[c] = lo < l[c] ? lo : l[c]; l[3 + c] = hi > l[3 + c] ? hi : l[3 + c]; }
                else { r[c] = lo < r[c] ? lo : r[c]; r[3 + c] = hi > r[3 + c] ? hi : r[3 + c]; }
            }
        }
        if (left > 0 && left < n) {
            const double c = sah_area(l) * left + sah_area(r) * (n - left);
            if (c < __builtin_huge_val()) cost = c;
        }
    }
    double m = cost;
    for (int o = 32; o > 0; o >>= 1) { const double v = __shfl_xor(m, o); m = v < m ? v : m; }
    const bool found = m < __builtin_huge_val();
    const unsigned long long who = __ballot(found && cost == m);
    best_lane = who ? __ffsll((long long)who) - 1 : 0;
    best_left = __shfl(left, best_lane);
    return found && who != 0;
}

__device__ __forceinline__ void sah_write_record(const SahArgs &a, int rec, const float lo[3], const float hi[3], int first, int count)
{
    if (rec < 0 || rec >= 2 * a.n - 1) return;
    a.rec[2 * (size_t)rec] = make_float4(lo[0], lo[1], lo[2], __int_as_float(first));
    a.rec[2 * (size_t)rec + 1] = make_float4(hi[0], hi[1], hi[2], __int_as_float(count));
}

__device__ __forceinline__ void sah_clear_slot(SahSlot &s, int lane)
{
    if (lane < 6) { s.cb[lane] = lane < 3 ? kKeyPosInf : kKeyNegInf; s.bx[lane] = lane < 3 ? kKeyPosInf : kKeyNegInf; }
    for (int j = lane; j < kHist; j += 64) s.hist[j] = j < 48 ? 0u : ((j - 48) % 6 < 3 ? kKeyPosInf : kKeyNegInf);
}

__device__ __forceinline__ int sah_slots_of_round(const SahArgs &a, int r)
{
    const int v = a.ctr[r];
    return v < 0 ? 0 : (v < a.max_slots ? v : a.max_slots);
}

// the slot whose node holds position p in round r, or -1
__device__ __forceinline__ int sah_slot_of(const SahArgs &a, int r, int p, int n_slots, int &b, int &e)
{
    if (p >= a.n) return -1;
    const int s = a.node_of[r & 1][p];
    if (s < 0 || s >= n_slots) return -1;
    b = a.slots[r & 1][s].b; e = a.slots[r & 1][s].e;
    return (p >= b && p < e && e <= a.n) ? s : -1;
}

__global__ __launch_bounds__(256) void k_sah_init(SahArgs a)
{
#pragma clang fp contract(off)
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < 2 * a.n - 1) { a.rec[2 * (size_t)g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); a.rec[2 * (size_t)g + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    if (g < a.n) {
        const float *T = a.tris + 24 * (size_t)g;
        for (int c = 0; c < 3; c++)
            a.cen[3 * (size_t)g + c] = 0.5f * fminf(fminf(T[c], T[8 + c]), T[16 + c]) + 0.5f * fmaxf(fmaxf(T[c], T[8 + c]), T[16 + c]);
        a.ord[0][g] = g;
        a.node_of[0][g] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const bool large = a.n > kSmall;
        if (lane < a.rounds + 2) a.ctr[lane] = (lane == 0 && large) || (lane == a.rounds + 1 && !large) ? 1 : 0;
        if (lane < 4) a.counts[lane] = 0;
        if (large) {
            SahSlot &s = a.slots[0][0];
            if (lane == 0) { s.b = 0; s.e = a.n; s.level = 0; s.rec = 0; }
            sah_clear_slot(s, lane);
        } else if (lane == 0) {
            a.small[0] = make_int4(0, a.n, 0, 0);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_sah_bounds(SahArgs a, int r)
{
    __shared__ unsigned acc[2][12];
    __shared__ int owner[2];
    const int n_slots = sah_slots_of_round(a, r);
    if (n_slots == 0) return;
    const int t = threadIdx.x, start = blockIdx.x * kBlock, p = start + t;
    if (t < 24) acc[t / 12][t % 12] = (t % 6) < 3 ? kKeyPosInf : kKeyNegInf;
    if (t < 2) owner[t] = -1;
    __syncthreads();
    int b = 0, e = 0;
    const int s = sah_slot_of(a, r, p, n_slots, b, e);
    if (s >= 0) {
        const int w = b > start ? 1 : 0;
        owner[w] = s;
        const unsigned i = (unsigned)a.ord[r & 1][p] < (unsigned)a.n ? (unsigned)a.ord[r & 1][p] : 0u;
        const float4 lo = a.tri_boxes[2 * (size_t)i], hi = a.tri_boxes[2 * (size_t)i + 1];
        const float v[12] = { a.cen[3 * (size_t)i], a.cen[3 * (size_t)i + 1], a.cen[3 * (size_t)i + 2], 0.0f, 0.0f, 0.0f, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z };
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (v[c] == v[c]) { atomicMin(&acc[w][c], sah_key(v[c])); atomicMax(&acc[w][3 + c], sah_key(v[c])); }
            if (v[6 + c] == v[6 + c]) atomicMin(&acc[w][6 + c], sah_key(v[6 + c]));
            if (v[9 + c] == v[9 + c]) atomicMax(&acc[w][9 + c], sah_key(v[9 + c]));
        }
    }
    __syncthreads();
    if (t < 24 && owner[t / 12] >= 0) {
        SahSlot &S = a.slots[r & 1][owner[t / 12]];
        const int k = t % 12;
        unsigned *dst = k < 6 ? &S.cb[k] : &S.bx[k - 6];
        if ((k % 6) < 3) atomicMin(dst, acc[t / 12][k]); else atomicMax(dst, acc[t / 12][k]);
    }
}

__global__ __launch_bounds__(kBlock) void k_sah_hist(SahArgs a, int r)
{
#pragma clang fp contract(off)
    __shared__ unsigned h[2][kHist];
    __shared__ int owner[2];
    const int n_slots = sah_slots_of_round(a, r);
    if (n_slots == 0) return;
    const int t = threadIdx.x, start = blockIdx.x * kBlock, p = start + t;
    for (int j = t; j < 2 * kHist; j += kBlock) { const int k = j % kHist; h[j / kHist][k] = k < 48 ? 0u : ((k - 48) % 6 < 3 ? kKeyPosInf : kKeyNegInf); }
    if (t < 2) owner[t] = -1;
    __syncthreads();
    int b = 0, e = 0;
    const int s = sah_slot_of(a, r, p, n_slots, b, e);
    if (s >= 0) {
        const int w = b > start ? 1 : 0;
        owner[w] = s;
        const SahSlot &S = a.slots[r & 1][s];
        const unsigned i = (unsigned)a.ord[r & 1][p] < (unsigned)a.n ? (unsigned)a.ord[r & 1][p] : 0u;
        const float4 lo = a.tri_boxes[2 * (size_t)i], hi = a.tri_boxes[2 * (size_t)i + 1];
        const float bx[6] = { lo.x, lo.y, lo.z, hi.x, hi.y, hi.z };
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float clo = sah_unkey(S.cb[c]), ext = sah_unkey(S.cb[3 + c]) - clo;
            if (!sah_axis_ok(ext)) continue;
            const int j = 16 * c + sah_bin(a.cen[3 * (size_t)i + c], clo, ext);
            atomicAdd(&h[w][j], 1u);
#pragma unroll
            for (int q = 0; q < 6; q++) {
                if (!(bx[q] == bx[q])) continue;
                if (q < 3) atomicMin(&h[w][48 + 6 * j + q], sah_key(bx[q])); else atomicMax(&h[w][48 + 6 * j + q], sah_key(bx[q]));
            }
        }
    }
    __syncthreads();
    for (int j = t; j < 2 * kHist; j += kBlock) {
        const int w = j / kHist, k = j % kHist;
        if (owner[w] < 0) continue;
        unsigned *dst = &a.slots[r & 1][owner[w]].hist[k];
        const unsigned v = h[w][k];
        if (k < 48) { if (v) atomicAdd(dst, v); }
        else if ((k - 48) % 6 < 3) { if (v != kKeyPosInf) atomicMin(dst, v); }
        else if (v != kKeyNegInf) atomicMax(dst, v);
    }
}

// one wave per slot
__global__ __launch_bounds__(64) void k_sah_decide(SahArgs a, int r)
{
#pragma clang fp contract(off)
    const int n_slots = sah_slots_of_round(a, r), s = blockIdx.x, lane = threadIdx.x;
    if (s >= n_slots) return;
    SahSlot &S = a.slots[r & 1][s];
    const int b = S.b, e = S.e, n = e - b, level = S.level;
    if (b < 0 || e > a.n || n < 2) return;
    float clo[3], ext[3];
    unsigned mask = 0;
    for (int c = 0; c < 3; c++) { clo[c] = sah_unkey(S.cb[c]); ext[c] = sah_unkey(S.cb[3 + c]) - clo[c]; if (sah_axis_ok(ext[c])) mask |= 1u << c; }
    int best_lane, pl;
    const bool found = sah_choose(S.hist, n, mask, lane, best_lane, pl);
    int nl = found ? pl : 0;
    const long long room = sah_room(a.L, SVGF_SCENE_MAX_DEPTH - level - 1);
    const bool forced = nl <= 0 || nl >= n || nl > room || n - nl > room;
    if (forced) nl = (n + 1) / 2;
    int child[2] = { -1, -1 };
    for (int side = 0; side < 2; side++) {
        const int cb = side ? b + nl : b, ce = side ? e : b + nl, crec = 2 * (b + nl) - 1 + side;
        int idx = 0;
        if (ce - cb > kSmall) {
            if (lane == 0) idx = atomicAdd(&a.ctr[r + 1], 1);
            idx = __shfl(idx, 0);
            if (idx >= a.max_slots) continue;
            SahSlot &C = a.slots[(r + 1) & 1][idx];
            if (lane == 0) { C.b = cb; C.e = ce; C.level = level + 1; C.rec = crec; }
            sah_clear_slot(C, lane);
            child[side] = idx;
        } else if (lane == 0) {
            idx = atomicAdd(&a.ctr[a.rounds + 1], 1);
            if (idx < a.small_cap) a.small[idx] = make_int4(cb, ce, (level + 1) | (((r + 1) & 1) << 8), crec);
        }
    }
    if (lane == 0) {
        const int axis = best_lane >> 4;
        S.pred = found ? 1 : 0; S.axis = axis; S.bin = best_lane & 15; S.pl = pl; S.nl = nl; S.child[0] = child[0]; S.child[1] = child[1];
        S.lo = axis == 0 ? clo[0] : (axis == 1 ? clo[1] : clo[2]);
        S.ext = axis == 0 ? ext[0] : (axis == 1 ? ext[1] : ext[2]);
        const float lo[3] = { sah_unkey(S.bx[0]), sah_unkey(S.bx[1]), sah_unkey(S.bx[2]) }, hi[3] = { sah_unkey(S.bx[3]), sah_unkey(S.bx[4]), sah_unkey(S.bx[5]) };
        sah_write_record(a, S.rec, lo, hi, 2 * (b + nl) - 1, 0);
        atomicAdd(&a.counts[0], 1);
        atomicMax(&a.counts[2], level);
        if (forced) atomicAdd(&a.counts[3], 1);
    }
}

__device__ __forceinline__ bool sah_flag(const SahArgs &a, const SahSlot &S, int r, int p)
{
    if (!S.pred) return false;
    const unsigned i = (unsigned)a.ord[r & 1][p] < (unsigned)a.n ? (unsigned)a.ord[r & 1][p] : 0u;
    const int axis = S.axis < 0 ? 0 : (S.axis > 2 ? 2 : S.axis);
    return sah_bin(a.cen[3 * (size_t)i + axis], S.lo, S.ext) <= S.bin;
}

__global__ __launch_bounds__(kBlock) void k_sah_count(SahArgs a, int r)
{
    __shared__ unsigned cnt[2];
    const int n_slots = sah_slots_of_round(a, r);
    if (n_slots == 0) return;
    const int t = threadIdx.x, start = blockIdx.x * kBlock, p = start + t;
    if (t < 2) cnt[t] = 0;
    __syncthreads();
    int b = 0, e = 0;
    const int s = sah_slot_of(a, r, p, n_slots, b, e);
    const bool flag = s >= 0 && sah_flag(a, a.slots[r & 1][s], r, p);
    const int w = (s >= 0 && b > start) ? 1 : 0;
    const unsigned long long m0 = __ballot(flag && w == 0), m1 = __ballot(flag && w == 1);
    if ((t & 63) == 0) { if (m0) atomicAdd(&cnt[0], (unsigned)__popcll(m0)); if (m1) atomicAdd(&cnt[1], (unsigned)__popcll(m1)); }
    __syncthreads();
    if (t < 2) a.blk[2 * blockIdx.x + t] = cnt[t];
}

__global__ __launch_bounds__(kBlock) void k_sah_scatter(SahArgs a, int r)
{
    __shared__ unsigned wtot[2][kBlock / 64];
    __shared__ unsigned carry;
    __shared__ int head_b, head_pred;
    const int n_slots = sah_slots_of_round(a, r);
    if (n_slots == 0) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, start = blockIdx.x * kBlock, p = start + t;
    int b = 0, e = 0;
    const int s = sah_slot_of(a, r, p, n_slots, b, e);
    if (t == 0) { carry = 0; head_b = s >= 0 ? b : -1; head_pred = s >= 0 ? a.slots[r & 1][s].pred : 0; }
    const bool flag = s >= 0 && sah_flag(a, a.slots[r & 1][s], r, p);
    const int w = (s >= 0 && b > start) ? 1 : 0;
    const unsigned long long m0 = __ballot(flag && w == 0), m1 = __ballot(flag && w == 1);
    if (lane == 0) { wtot[0][wave] = (unsigned)__popcll(m0); wtot[1][wave] = (unsigned)__popcll(m1); }
    __syncthreads();
    if (head_b >= 0 && head_b < start && head_pred) {       // the head node began in an earlier block: its flags in the blocks before
        const int first = head_b / kBlock;
        unsigned sum = 0;
        for (int j = first + t; j < (int)blockIdx.x; j += kBlock) sum += a.blk[2 * j + ((j == first && head_b % kBlock != 0) ? 1 : 0)];
        if (sum) atomicAdd(&carry, sum);
    }
    __syncthreads();
    if (s < 0) return;
    const SahSlot &S = a.slots[r & 1][s];
    int dest = p;
    if (S.pred) {
        unsigned before = (w == 0 ? carry : 0u) + (unsigned)__popcll((w == 0 ? m0 : m1) & ((1ull << lane) - 1ull));
        for (int k = 0; k < wave; k++) before += wtot[w][k];
        dest = flag ? b + (int)before : b + S.pl + ((p - b) - (int)before);
    }
    if (dest < b || dest >= e) return;
    a.ord[(r + 1) & 1][dest] = a.ord[r & 1][p];
    a.node_of[(r + 1) & 1][dest] = S.child[dest < b + S.nl ? 0 : 1];
}

// ---- small subtrees: one wave, its own node stack ------------------------------------------------------------------------------------------
struct SahShared {
    unsigned hist[kHist];
    int4 stack[SVGF_SCENE_MAX_DEPTH + 2];
    float cen[3 * kSmall], box[6 * kSmall];
    int gid[kSmall];
    unsigned short ord[2][kSmall];
};

template <bool LDS>
__device__ __forceinline__ void sah_subtree(const SahArgs &a, int b0, int e0, int level, int rec, int par, SahShared &sh)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x, base = LDS ? b0 : 0;
    const float inf = __builtin_huge_valf();
    auto get = [&](int pr, int k) -> int { if (LDS) return sh.ord[pr][k]; const unsigned i = (unsigned)a.ord[pr][k]; return i < (unsigned)a.n ? (int)i : 0; };
    auto cen = [&](int id, int c) -> float { return LDS ? sh.cen[3 * id + c] : a.cen[3 * (size_t)id + c]; };
    auto box = [&](int id, int q) -> float { return LDS ? sh.box[6 * id + q] : reinterpret_cast<const float *>(a.tri_boxes + 2 * (size_t)id)[q < 3 ? q : q + 1]; };
    if (LDS) {
        for (int k = lane; k < e0 - b0; k += 64) {
            const unsigned g0 = (unsigned)a.ord[par][b0 + k];
            const int g = g0 < (unsigned)a.n ? (int)g0 : 0;
            const float4 lo = a.tri_boxes[2 * (size_t)g], hi = a.tri_boxes[2 * (size_t)g + 1];
            sh.gid[k] = g; sh.ord[0][k] = (unsigned short)k;
            sh.cen[3 * k] = a.cen[3 * (size_t)g]; sh.cen[3 * k + 1] = a.cen[3 * (size_t)g + 1]; sh.cen[3 * k + 2] = a.cen[3 * (size_t)g + 2];
            sh.box[6 * k] = lo.x; sh.box[6 * k + 1] = lo.y; sh.box[6 * k + 2] = lo.z; sh.box[6 * k + 3] = hi.x; sh.box[6 * k + 4] = hi.y; sh.box[6 * k + 5] = hi.z;
        }
        par = 0;
        __syncthreads();
    }
    int b = b0 - base, e = e0 - base, sp = 0, n_nodes = 0, n_leaves = 0, n_forced = 0, depth = 0;
    for (;;) {
        const int n = e - b;
        float blo[3] = { inf, inf, inf }, bhi[3] = { -inf, -inf, -inf }, clo[3] = { inf, inf, inf }, chi[3] = { -inf, -inf, -inf };
        for (int k = b + lane; k < e; k += 64) {
            const int id = get(par, k);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                blo[c] = fminf(blo[c], box(id, c)); bhi[c] = fmaxf(bhi[c], box(id, 3 + c));
                const float v = cen(id, c);
                clo[c] = fminf(clo[c], v); chi[c] = fmaxf(chi[c], v);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) { blo[c] = wave_min(blo[c]); bhi[c] = wave_max(bhi[c]); clo[c] = wave_min(clo[c]); chi[c] = wave_max(chi[c]); }
        n_nodes++;
        depth = level > depth ? level : depth;
        bool leaf = n <= a.L;
        if (!leaf) {
            for (int j = lane; j < kHist; j += 64) sh.hist[j] = j < 48 ? 0u : ((j - 48) % 6 < 3 ? kKeyPosInf : kKeyNegInf);
            __syncthreads();
            float ext[3];
            unsigned mask = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) { ext[c] = chi[c] - clo[c]; if (sah_axis_ok(ext[c])) mask |= 1u << c; }
            for (int k = b + lane; k < e; k += 64) {
                const int id = get(par, k);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    if (!((mask >> c) & 1u)) continue;
                    const int j = 16 * c + sah_bin(cen(id, c), clo[c], ext[c]);
                    atomicAdd(&sh.hist[j], 1u);
#pragma unroll
                    for (int q = 0; q < 6; q++) {
                        const float v = box(id, q);
                        if (!(v == v)) continue;
                        if (q < 3) atomicMin(&sh.hist[48 + 6 * j + q], sah_key(v)); else atomicMax(&sh.hist[48 + 6 * j + q], sah_key(v));
                    }
                }
            }
            __syncthreads();
            int best_lane, pl;
            const bool found = sah_choose(sh.hist, n, mask, lane, best_lane, pl);
            __syncthreads();
            if (found) {
                const int axis = best_lane >> 4, bin = best_lane & 15;
                const float lo = axis == 0 ? clo[0] : (axis == 1 ? clo[1] : clo[2]), ex = axis == 0 ? ext[0] : (axis == 1 ? ext[1] : ext[2]);
                int lbase = 0, rbase = 0;
                for (int k0 = b; k0 < e; k0 += 64) {
                    const int k = k0 + lane;
                    const bool valid = k < e;
                    const int id = valid ? get(par, k) : 0;
                    const bool flag = valid && sah_bin(cen(id, axis), lo, ex) <= bin;
                    const unsigned long long mv = __ballot(valid), ml = __ballot(flag), mr = mv & ~ml, lt = (1ull << lane) - 1ull;
                    if (valid) {
                        const int dst = flag ? b + lbase + __popcll(ml & lt) : b + pl + rbase + __popcll(mr & lt);
                        if (dst >= b && dst < e) { if (LDS) sh.ord[par ^ 1][dst] = (unsigned short)id; else a.ord[par ^ 1][dst] = id; }
                    }
                    lbase += __popcll(ml); rbase += __popcll(mr);
                }
                par ^= 1;
                __syncthreads();
            }
            int nl = found ? pl : 0;
            const long long room = sah_room(a.L, SVGF_SCENE_MAX_DEPTH - level - 1);
            if (nl <= 0 || nl >= n || nl > room || n - nl > room) { nl = (n + 1) / 2; n_forced++; }
            const int at = b + base + nl;
            if (lane == 0) sah_write_record(a, rec, blo, bhi, 2 * at - 1, 0);
            if (sp < SVGF_SCENE_MAX_DEPTH + 2 && level < SVGF_SCENE_MAX_DEPTH) {
                sh.stack[sp++] = make_int4(b + nl, e, (level + 1) | (par << 8), 2 * at);
                e = b + nl; rec = 2 * at - 1; level++;
                continue;
            }
            leaf = true;                // unreachable by the room rule; never walk off the stack
        }
        if (lane == 0) sah_write_record(a, rec, blo, bhi, b + base, n);
        for (int k = b + lane; k < e; k += 64) { const int id = get(par, k); a.order[k + base] = LDS ? sh.gid[id] : id; }
        n_leaves++;
        if (sp == 0) break;
        const int4 top = sh.stack[--sp];
        b = top.x; e = top.y; level = top.z & 255; par = (top.z >> 8) & 1; rec = top.w;
    }
    if (lane == 0) {
        atomicAdd(&a.counts[0], n_nodes); atomicAdd(&a.counts[1], n_leaves); atomicMax(&a.counts[2], depth);
        if (n_forced) atomicAdd(&a.counts[3], n_forced);
    }
}

__global__ __launch_bounds__(64) void k_sah_small(SahArgs a)
{
    __shared__ SahShared sh;
    const int v = a.ctr[a.rounds + 1], n_small = v < 0 ? 0 : (v < a.small_cap ? v : a.small_cap);
    const int n_large = a.rounds > 0 ? sah_slots_of_round(a, a.rounds) : 0;
    for (int it = blockIdx.x; it < n_small + n_large; it += gridDim.x) {
        int b, e, level, rec, par;
        if (it < n_small) { const int4 m = a.small[it]; b = m.x; e = m.y; level = m.z & 255; par = (m.z >> 8) & 1; rec = m.w; }
        else { const SahSlot &S = a.slots[a.rounds & 1][it - n_small]; b = S.b; e = S.e; level = S.level; rec = S.rec; par = a.rounds & 1; }
        if (b < 0 || e > a.n || b >= e || level < 0 || level > SVGF_SCENE_MAX_DEPTH) continue;
        if (e - b <= kSmall) sah_subtree<true>(a, b, e, level, rec, par, sh);
        else sah_subtree<false>(a, b, e, level, rec, par, sh);
        __syncthreads();
    }
}

constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

struct svgf_sah {
    const svgf_scene *scene;
    int device, small_grid;
    char *dev;
    SahArgs args;
    SvgfSahInfo info;
};

extern "C" int svgf_sah_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_sah_create(const svgf_scene *scene, const SvgfSahParams *p, svgf_sah **out)
{
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    if (!scene || (p && (p->max_leaf_tris < 0 || p->max_leaf_tris > 8))) return SVGF_ERR_INVALID_ARG;
    SvgfSceneView v;
    if (svgf_scene_view(scene, &v) != SVGF_OK || v.n_tris < 1 || v.n_tris > SVGF_SCENE_MAX_TRIS) return SVGF_ERR_INVALID_ARG;
    const int n = v.n_tris, L = (p && p->max_leaf_tris) ? p->max_leaf_tris : 4;
    int rounds = 0;
    if (n > kSmall) { while (((long long)kSmall << rounds) < n) rounds++; rounds += 4; }
    const int max_slots = n / (kSmall + 1) + 1, n_blocks = (n + kBlock - 1) / kBlock;
    // one allocation: [records | order | ord a | ord b | node_of a | node_of b | centroids | slots a | slots b | small list | block counts |
    // counters | counts], 16-byte aligned parts
    const size_t o_rec = 0, o_order = o_rec + 32 * (2 * (size_t)n - 1), o_oa = o_order + align16(4 * (size_t)n), o_ob = o_oa + align16(4 * (size_t)n);
    const size_t o_na = o_ob + align16(4 * (size_t)n), o_nb = o_na + align16(4 * (size_t)n), o_cen = o_nb + align16(4 * (size_t)n);
    const size_t o_sa = o_cen + align16(12 * (size_t)n), o_sb = o_sa + align16(sizeof(SahSlot) * (size_t)max_slots), o_sm = o_sb + align16(sizeof(SahSlot) * (size_t)max_slots);
    const size_t o_blk = o_sm + 16 * (size_t)n, o_ctr = o_blk + align16(8 * (size_t)n_blocks), o_cnt = o_ctr + align16(4 * (size_t)(rounds + 2));
    const size_t bytes = o_cnt + 16;
    svgf_sah *t = new (std::nothrow) svgf_sah();
    if (!t) return SVGF_ERR_OOM;
    SvgfDeviceGuard dev_guard(v.device);
    if (!dev_guard.ok) { (void)hipGetLastError(); delete t; return SVGF_ERR_NO_DEVICE; }
    char *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) { (void)hipGetLastError(); delete t; return SVGF_ERR_OOM; }
    if (hipMemset(d, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); (void)hipFree(d); delete t; return SVGF_ERR_HIP; }
    t->scene = scene; t->device = v.device; t->dev = d;
    t->small_grid = n < 4096 ? n : 4096;
    SahArgs &a = t->args;
    a.tris = nullptr; a.tri_boxes = nullptr;
    a.n = n; a.L = L; a.rounds = rounds; a.max_slots = max_slots; a.small_cap = n; a.n_blocks = n_blocks;
    a.rec = reinterpret_cast<float4 *>(d + o_rec); a.order = reinterpret_cast<int *>(d + o_order);
    a.ord[0] = reinterpret_cast<int *>(d + o_oa); a.ord[1] = reinterpret_cast<int *>(d + o_ob);
    a.node_of[0] = reinterpret_cast<int *>(d + o_na); a.node_of[1] = reinterpret_cast<int *>(d + o_nb);
    a.cen = reinterpret_cast<float *>(d + o_cen);
    a.slots[0] = reinterpret_cast<SahSlot *>(d + o_sa); a.slots[1] = reinterpret_cast<SahSlot *>(d + o_sb);
    a.small = reinterpret_cast<int4 *>(d + o_sm); a.blk = reinterpret_cast<unsigned *>(d + o_blk);
    a.ctr = reinterpret_cast<int *>(d + o_ctr); a.counts = reinterpret_cast<int *>(d + o_cnt);
    const int depth_bound = SVGF_SCENE_MAX_DEPTH < n - 1 ? SVGF_SCENE_MAX_DEPTH : n - 1;
    t->info = SvgfSahInfo{ n, L, 2 * n - 1, depth_bound, 2 + 5 * rounds, (unsigned long long)bytes };
    *out = t;
    return SVGF_OK;
}

extern "C" int svgf_sah_build(svgf_sah *t, void *stream)
{
    if (!t) return SVGF_ERR_INVALID_ARG;
    SvgfSceneView v;
    if (svgf_scene_view(t->scene, &v) != SVGF_OK || v.n_tris != t->args.n || !v.tris || !v.tri_boxes || v.device != t->device) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(t->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    SahArgs a = t->args;
    a.tris = v.tris;
    a.tri_boxes = reinterpret_cast<const float4 *>(v.tri_boxes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = a.n;
    hipLaunchKernelGGL(k_sah_init, dim3((2 * n - 1 + 255) / 256), dim3(256), 0, st, a);
    for (int r = 0; r < a.rounds; r++) {
        hipLaunchKernelGGL(k_sah_bounds, dim3(a.n_blocks), dim3(kBlock), 0, st, a, r);
        hipLaunchKernelGGL(k_sah_hist, dim3(a.n_blocks), dim3(kBlock), 0, st, a, r);
        hipLaunchKernelGGL(k_sah_decide, dim3(a.max_slots), dim3(64), 0, st, a, r);
        hipLaunchKernelGGL(k_sah_count, dim3(a.n_blocks), dim3(kBlock), 0, st, a, r);
        hipLaunchKernelGGL(k_sah_scatter, dim3(a.n_blocks), dim3(kBlock), 0, st, a, r);
    }
    hipLaunchKernelGGL(k_sah_small, dim3(t->small_grid), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_sah_attach(svgf_sah *t, svgf_scene *scene)
{
    if (!t || !scene || scene != t->scene) return SVGF_ERR_INVALID_ARG;
    return svgf_scene_adopt_tree(scene, reinterpret_cast<const SvgfBvhNode *>(t->args.rec), t->args.order, t->info.n_records, t->info.n_tris, t->info.depth_bound);
}

extern "C" int svgf_sah_info(const svgf_sah *t, SvgfSahInfo *out)
{
    if (!t || !out) return SVGF_ERR_INVALID_ARG;
    *out = t->info;
    return SVGF_OK;
}

extern "C" int svgf_sah_read(const svgf_sah *t, int which, void *host_dst, unsigned long long host_bytes)
{
    if (!t || which < 0 || which > 2 || !host_dst) return SVGF_ERR_INVALID_ARG;
    const void *src[3] = { t->args.rec, t->args.order, t->args.counts };
    const unsigned long long size[3] = { 32ull * t->info.n_records, 4ull * t->info.n_tris, sizeof(SvgfSahCounts) };
    if (host_bytes != size[which]) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(t->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_dst, src[which], (size_t)host_bytes, hipMemcpyDeviceToHost) != hipSuccess) return SVGF_ERR_HIP;
    return SVGF_OK;
}

extern "C" void svgf_sah_destroy(svgf_sah *t)
{
    if (!t) return;
    {
        SvgfDeviceGuard dev_guard(t->device);
        if (dev_guard.ok) { (void)hipDeviceSynchronize(); (void)hipFree(t->dev); }
    }
    delete t;
}
