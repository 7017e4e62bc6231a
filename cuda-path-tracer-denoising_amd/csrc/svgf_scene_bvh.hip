// svgf_scene_bvh.hip — the resident scene (row f14): the scene producer's inputs kept on the device with a BVH over the triangles,
// and a draw that is one launch.  Row f15 (below the draw kernel) animates it: per-object poses applied to the rest state and a
// refit of the node boxes, three launches per frame.  Row f16 adds the shadowed form of the draw kernel (shadow rays as any-hit walks
// on the same stack).  include/svgf.h states the semantics (a gated brute force that every tree reproduces);
// svgf_bvh_build.cpp builds the tree on the host; the per-pixel body around the triangle search is svgf_scene_pixel.inc.h, the text
// k_scene_frame compiles too.
//
// k_scene_bvh: one thread per pixel, 256 per block.  The walk (svgf_scene_walk.inc.h) keeps the current node in registers, descends
// into the nearer child and parks the other one on a per-lane stack in LDS: stack[level][lane], 48 x 256 x 4 B = 48 KB per block, a lane's
// entries 1 KB apart so that the 64 lanes of a wave always touch 64 consecutive words (no bank conflict, no runtime-indexed private
// array, no scratch).  A parked node is tested again when it is popped - the nearest hit may have come closer since - which costs one
// 32-byte load of a node that was loaded as a child before.  SVGF_SCENE_MAX_DEPTH bounds the stack: a lane holds one entry per
// level above its current node.  Row f17's companion library (svgf_scene_trace.hip) compiles the same walks.
#include "svgf_kernels.h"
#include "../../include/svgf.h"
#include "../../include/svgf_scene_write.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

void svgf_bvh_tri_box(const float *T, float lo[3], float hi[3]);       // svgf_bvh_build.cpp

namespace {

#include "svgf_scene_pixel.inc.h"

#include "svgf_scene_walk.inc.h"     // SceneBvhArgs, SceneRay, scene_slab, scene_nearest, scene_occluded, scene_shadow_sample

// ---- row f16: shadow rays ---------------------------------------------------------------------------------------------------------------------
// svgf_scene_draw_shadowed (include/svgf.h states the rule): the primary walk as above, then per sample a point on the parallelogram
// light, the ray from the surface to it and an ANY-hit search inside (t_lo, t_hi): the primitives that do not emit, then a walk over
// the same nodes that leaves at the first counting triangle.  Occlusion is an OR, so neither the visiting order nor the early exit
// can change it.  The walk parks nodes on the same per-lane stack - the primary walk has emptied it by then - and the samples are a
// runtime loop (one copy of the walk in the code object, whatever `samples` is).
struct SceneShadowArgs {
    SceneBvhArgs b;
    float edge_u[3], edge_v[3];
    int samples;
};

__device__ __forceinline__ const SceneBvhArgs &scene_bvh_args(const SceneBvhArgs &b) { return b; }
__device__ __forceinline__ const SceneBvhArgs &scene_bvh_args(const SceneShadowArgs &sa) { return sa.b; }

// vis of pixel p: the share of its shadow rays that reach the light.  r holds the primary ray and is reused for the shadow rays.
__device__ __forceinline__ float scene_visibility(const SceneShadowArgs &sa, SceneRay &r, const SceneHit &h, const float pos[3], int *const stk, int p)
{
#pragma clang fp contract(off)
    int unoccluded = sa.samples;
    if (h.gid >= 0 && !(h.emit > 0.0f)) {       // a miss and an emitter cast no ray
        unoccluded = 0;
        for (int c = 0; c < 3; c++) r.o[c] = pos[c];
        for (int s = 0; s < sa.samples; s++)
            unoccluded += scene_shadow_sample(sa.b, sa.edge_u, sa.edge_v, r, pos, stk, p, 8 + 2 * s, 9 + 2 * s) ? 0 : 1;
    }
    return (float)unoccluded / (float)sa.samples;
}
__device__ __forceinline__ float scene_visibility(const SceneBvhArgs &, SceneRay &, const SceneHit &, const float *, int *, int) { return 1.0f; }

// SHADOWED = false is svgf_scene_draw's kernel, what it was before row f16 (the primary walk is scene_nearest of
// svgf_scene_walk.inc.h since row f17: the same statements, the same 64 VGPRs); true adds the part between the primary walk and the
// shared tail.
template <bool SHADOWED>
__global__ __launch_bounds__(256) void k_scene_bvh(typename std::conditional<SHADOWED, SceneShadowArgs, SceneBvhArgs>::type arg)
{
#pragma clang fp contract(off)
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneBvhArgs &b = scene_bvh_args(arg);
    const SceneArgs &a = b.s;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < a.W * a.H) {
        SceneRay r;
        scene_ray(a, p % a.W, p / a.W, r.o, r.d);
        SceneHit h;
        scene_primitives(a, r.o, r.d, h);
        for (int c = 0; c < 3; c++) { r.flat[c] = fabsf(r.d[c]) < 0x1p-100f; r.inv[c] = 1.0f / r.d[c]; }
        int best = -1;
        float bt = h.t_best, bbx = 0.0f, bby = 0.0f;
        scene_nearest(b, r, stack + threadIdx.x, 0.0f, bt, best, bbx, bby);
        if constexpr (SHADOWED) {
            float pos[3];
            scene_surface(a, r.o, r.d, h, best, bt, bbx, bby, pos);
            scene_shade<true>(a, p, h, pos, scene_visibility(arg, r, h, pos, stack + threadIdx.x, p));
        } else {
            scene_finish(a, p, r.o, r.d, h, best, bt, bbx, bby);
        }
    }
}

// ---- row f15: pose + refit ------------------------------------------------------------------------------------------------------------------
// Three launches, and no data passes between workgroups inside one of them (the per-XCD L2s are not coherent, and nothing here spins
// or climbs the tree with atomics): k_scene_pose writes posed triangles, their boxes, the primitives, the motion rows and the held
// table; k_scene_refit_treelets sweeps one treelet per workgroup in LDS; k_scene_refit_top, ONE workgroup, the nodes above them.
constexpr int kRefitCap = SVGF_SCENE_REFIT_CAP;

struct ScenePoseArgs {
    int n_tris, n_geoms, n_objects, tri_blocks;
    const float4 *rest_tris;    // 6 float4 per triangle: per vertex {px, py, pz, nx}, {ny, nz, u, v}
    float4 *tris;
    const int *tri_ids;
    float4 *tri_boxes;
    const SvgfSceneGeom *rest_geoms;
    SvgfSceneGeom *geoms;
    const int *geom_ids;
    const float4 *pose;         // 6 float4 per object: xf rows, inv rows
    float4 *held;
    float4 *motion;             // 3 float4 per object, or null
};

struct SceneRefitArgs {
    float4 *nodes;
    const int *order;
    const float4 *tri_boxes;
    const int4 *treelets;
    const unsigned char *level;
    const int *top, *top_seg;
    int n_top_depths;
};

// C = A o B (include/svgf.h, row f15); rows as float4 {m0, m1, m2, m3}
__device__ __forceinline__ void compose34(const float *A, const float *B, float *C)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) C[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
        C[4 * r + 3] = ((A[4 * r] * B[3] + A[4 * r + 1] * B[7]) + A[4 * r + 2] * B[11]) + A[4 * r + 3];
    }
}

__device__ __forceinline__ void load12(const float4 *src, float *m)
{
#pragma unroll
    for (int r = 0; r < 3; r++) { const float4 q = src[r]; m[4 * r] = q.x; m[4 * r + 1] = q.y; m[4 * r + 2] = q.z; m[4 * r + 3] = q.w; }
}

__global__ __launch_bounds__(256) void k_scene_pose(ScenePoseArgs a)
{
#pragma clang fp contract(off)
    if ((int)blockIdx.x < a.tri_blocks) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i >= a.n_tris) return;
        float4 q[6];
#pragma unroll
        for (int k = 0; k < 6; k++) q[k] = a.rest_tris[6 * (size_t)i + k];
        const int id = a.tri_ids[i];
        if (id >= 0 && id < a.n_objects) {
            float M[12];
            load12(a.pose + 6 * (size_t)id, M);
#pragma unroll
            for (int v = 0; v < 3; v++) {
                const float p[3] = { q[2 * v].x, q[2 * v].y, q[2 * v].z }, n[3] = { q[2 * v].w, q[2 * v + 1].x, q[2 * v + 1].y };
                float pp[3], nn[3];
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    pp[r] = ((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3];
                    nn[r] = (M[4 * r] * n[0] + M[4 * r + 1] * n[1]) + M[4 * r + 2] * n[2];
                }
                q[2 * v] = make_float4(pp[0], pp[1], pp[2], nn[0]);
                q[2 * v + 1].x = nn[1]; q[2 * v + 1].y = nn[2];
            }
        }
#pragma unroll
        for (int k = 0; k < 6; k++) a.tris[6 * (size_t)i + k] = q[k];
        // svgf_bvh_tri_box on the posed positions: the same literals, the same nesting
        const float P[3][3] = { { q[0].x, q[0].y, q[0].z }, { q[2].x, q[2].y, q[2].z }, { q[4].x, q[4].y, q[4].z } };
        float mn[3], mx[3], ext = 0.0f, lo[3], hi[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            mn[c] = fminf(fminf(P[0][c], P[1][c]), P[2][c]);
            mx[c] = fmaxf(fmaxf(P[0][c], P[1][c]), P[2][c]);
            const float e = mx[c] - mn[c];
            ext = e > ext ? e : ext;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float m = fmaxf(1.0f, fmaxf(fabsf(mn[c]), fabsf(mx[c])));
            const float pad = (ext * 0.00390625f) + (0.0000152587890625f * m);
            lo[c] = mn[c] - pad; hi[c] = mx[c] + pad;
        }
        a.tri_boxes[2 * (size_t)i] = make_float4(lo[0], lo[1], lo[2], __int_as_float(i));
        a.tri_boxes[2 * (size_t)i + 1] = make_float4(hi[0], hi[1], hi[2], __int_as_float(1));
        return;
    }
    // the tail blocks: thread j poses primitive j and writes table row j
    const int j = ((int)blockIdx.x - a.tri_blocks) * 256 + threadIdx.x;
    if (j < a.n_geoms) {
        const SvgfSceneGeom *g = a.rest_geoms + j;
        SvgfSceneGeom *o = a.geoms + j;
        o->type = g->type; o->material = g->material; o->emittance = g->emittance;
#pragma unroll
        for (int c = 0; c < 3; c++) o->albedo[c] = g->albedo[c];
        float Gx[12], Gi[12], Ox[12], Oi[12];
#pragma unroll
        for (int k = 0; k < 12; k++) { Gx[k] = g->xf[k]; Gi[k] = g->inv[k]; }
        const int id = a.geom_ids ? a.geom_ids[j] : j;
        if (id >= 0 && id < a.n_objects) {
            float X[12], I[12];
            load12(a.pose + 6 * (size_t)id, X);
            load12(a.pose + 6 * (size_t)id + 3, I);
            compose34(X, Gx, Ox);
            compose34(Gi, I, Oi);
#pragma unroll
            for (int k = 0; k < 12; k++) { o->xf[k] = Ox[k]; o->inv[k] = Oi[k]; }
#pragma unroll
            for (int r = 0; r < 3; r++) { o->invT[3 * r] = Oi[r]; o->invT[3 * r + 1] = Oi[4 + r]; o->invT[3 * r + 2] = Oi[8 + r]; }
        } else {
#pragma unroll
            for (int k = 0; k < 12; k++) { o->xf[k] = Gx[k]; o->inv[k] = Gi[k]; }
#pragma unroll
            for (int k = 0; k < 9; k++) o->invT[k] = g->invT[k];
        }
    }
    if (j < a.n_objects) {
        const float4 p0 = a.pose[6 * (size_t)j], p1 = a.pose[6 * (size_t)j + 1], p2 = a.pose[6 * (size_t)j + 2];
        const float4 p3 = a.pose[6 * (size_t)j + 3], p4 = a.pose[6 * (size_t)j + 4], p5 = a.pose[6 * (size_t)j + 5];
        if (a.motion) {
            float Hx[12], Mo[12];
            load12(a.held + 6 * (size_t)j, Hx);
            const float I[12] = { p3.x, p3.y, p3.z, p3.w, p4.x, p4.y, p4.z, p4.w, p5.x, p5.y, p5.z, p5.w };
            compose34(Hx, I, Mo);
#pragma unroll
            for (int r = 0; r < 3; r++) a.motion[3 * (size_t)j + r] = make_float4(Mo[4 * r], Mo[4 * r + 1], Mo[4 * r + 2], Mo[4 * r + 3]);
        }
        float4 *h = a.held + 6 * (size_t)j;
        h[0] = p0; h[1] = p1; h[2] = p2; h[3] = p3; h[4] = p4; h[5] = p5;
    }
}

__device__ __forceinline__ void box_union(float4 &lo, float4 &hi, const float4 &blo, const float4 &bhi)
{
    lo.x = fminf(lo.x, blo.x); lo.y = fminf(lo.y, blo.y); lo.z = fminf(lo.z, blo.z);
    hi.x = fmaxf(hi.x, bhi.x); hi.y = fmaxf(hi.y, bhi.y); hi.z = fmaxf(hi.z, bhi.z);
}

// One workgroup per treelet (svgf_bvh_refit_plan_host): local index 0 is the root, 1 + (g - begin) a descendant.  Leaves are filled
// from the posed triangle boxes, then the inner nodes level by level from the deepest, one barrier per level; every node box is
// stored once.  first / count travel through LDS unchanged in the .w lanes.
__global__ __launch_bounds__(256) void k_scene_refit_treelets(SceneRefitArgs r)
{
    __shared__ float4 box[2 * kRefitCap];
    __shared__ unsigned char lev[kRefitCap];
    const int4 t = r.treelets[blockIdx.x];      // root, begin, count, levels
    const int n = t.z + 1;
    for (int l = threadIdx.x; l < n; l += 256) {
        const int g = l == 0 ? t.x : t.y + l - 1;
        float4 lo = r.nodes[2 * (size_t)g], hi = r.nodes[2 * (size_t)g + 1];
        const int first = __float_as_int(lo.w), count = __float_as_int(hi.w);
        if (count > 0) {
            int i = r.order[first];
            const float4 b0 = r.tri_boxes[2 * (size_t)i], b1 = r.tri_boxes[2 * (size_t)i + 1];
            lo.x = b0.x; lo.y = b0.y; lo.z = b0.z; hi.x = b1.x; hi.y = b1.y; hi.z = b1.z;
            for (int k = first + 1; k < first + count; k++) {
                i = r.order[k];
                box_union(lo, hi, r.tri_boxes[2 * (size_t)i], r.tri_boxes[2 * (size_t)i + 1]);
            }
        }
        box[2 * l] = lo; box[2 * l + 1] = hi;
        lev[l] = r.level[g];
    }
    __syncthreads();
    for (int L = t.w - 1; L >= 0; L--) {
        for (int l = threadIdx.x; l < n; l += 256) {
            if (lev[l] != L) continue;
            float4 lo = box[2 * l], hi = box[2 * l + 1];
            if (__float_as_int(hi.w) > 0) continue;
            const int c = __float_as_int(lo.w) - t.y + 1;       // the first child's local index; children are descendants: >= 1
            const float4 alo = box[2 * c], ahi = box[2 * c + 1];
            lo.x = alo.x; lo.y = alo.y; lo.z = alo.z; hi.x = ahi.x; hi.y = ahi.y; hi.z = ahi.z;
            box_union(lo, hi, box[2 * c + 2], box[2 * c + 3]);
            box[2 * l] = lo; box[2 * l + 1] = hi;
        }
        __syncthreads();
    }
    for (int l = threadIdx.x; l < n; l += 256) {
        const int g = l == 0 ? t.x : t.y + l - 1;
        r.nodes[2 * (size_t)g] = box[2 * l]; r.nodes[2 * (size_t)g + 1] = box[2 * l + 1];
    }
}

// ONE workgroup: the nodes above the treelets, deepest depth first; the children of a node are treelet roots (the launch before) or
// nodes of an earlier segment (this workgroup, behind a barrier).
__global__ __launch_bounds__(256) void k_scene_refit_top(SceneRefitArgs r)
{
    for (int s = 0; s < r.n_top_depths; s++) {
        const int b = r.top_seg[s], e = r.top_seg[s + 1];
        for (int i = b + (int)threadIdx.x; i < e; i += 256) {
            const int g = r.top[i];
            float4 lo = r.nodes[2 * (size_t)g], hi = r.nodes[2 * (size_t)g + 1];
            const int c = __float_as_int(lo.w);
            const float4 alo = r.nodes[2 * (size_t)c], ahi = r.nodes[2 * (size_t)c + 1];
            lo.x = alo.x; lo.y = alo.y; lo.z = alo.z; hi.x = ahi.x; hi.y = ahi.y; hi.z = ahi.z;
            box_union(lo, hi, r.nodes[2 * (size_t)c + 2], r.nodes[2 * (size_t)c + 3]);
            r.nodes[2 * (size_t)g] = lo; r.nodes[2 * (size_t)g + 1] = hi;
        }
        __syncthreads();
    }
}

constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

const float kIdentityPose[24] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };

}  // namespace

struct svgf_scene {
    int device;
    char *dev;                  // the one allocation of svgf_scene_create: the REST state once a scene is posed
    SceneBvhArgs args;          // the scene's pointers (what the draws read); camera, outputs and frame are filled per draw
    SvgfSceneInfo info;
    // row f15, all zero on a static scene
    char *anim;                 // the one allocation of svgf_scene_enable_pose
    int n_objects, n_treelets, n_top;
    ScenePoseArgs pose;
    SceneRefitArgs refit;
    // row f24, all zero until svgf_scene_adopt_tree: the caller's tree, read by every draw in place of args.nodes / args.order
    const float4 *ad_nodes;
    const int *ad_order;
    int ad_n_nodes, ad_n_leaves, ad_depth;
};

// what the draws walk: the scene's own tree, or the adopted one
static inline const float4 *scene_nodes(const svgf_scene *sc) { return sc->ad_nodes ? sc->ad_nodes : sc->args.nodes; }
static inline const int *scene_order(const svgf_scene *sc) { return sc->ad_nodes ? sc->ad_order : sc->args.order; }
static inline SvgfSceneInfo scene_info(const svgf_scene *sc)
{
    SvgfSceneInfo in = sc->info;
    if (sc->ad_nodes) { in.n_nodes = sc->ad_n_nodes; in.n_leaves = sc->ad_n_leaves; in.depth = sc->ad_depth; }
    return in;
}

extern "C" int svgf_scene_create(int device, const SvgfSceneGeom *geoms, int n_geoms, const int *geom_ids, const float *tris, const int *tri_ids,
                                 const float *tri_albedo, int n_tris, const int *tri_tex, const int *tex_desc, const unsigned char *tex_data,
                                 int n_tex, const SvgfSceneBuildParams *bp, svgf_scene **out)
{
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    size_t n_texbytes = 0;
    if (scene_check_inputs(geoms, n_geoms, tris, tri_ids, tri_albedo, n_tris, tri_tex, tex_desc, tex_data, n_tex, &n_texbytes) != SVGF_OK) return SVGF_ERR_INVALID_ARG;
    if (device < 0 || device >= 64) return SVGF_ERR_UNSUPPORTED;
    // the builder refuses bp out of range and a vertex position that is not finite
    const size_t nt = (size_t)(n_tris > 0 ? n_tris : 1), ng = (size_t)(n_geoms > 0 ? n_geoms : 1);
    std::vector<SvgfBvhNode> nodes(2 * nt);
    std::vector<int> order(nt);
    int n_nodes = 0, depth = 0;
    const int rc = svgf_bvh_build_host(tris, n_tris, bp, nodes.data(), &n_nodes, order.data(), &depth);
    if (rc != SVGF_OK) return rc;
    if (depth > SVGF_SCENE_MAX_DEPTH) return SVGF_ERR_UNSUPPORTED;      // the kernel's stack; the builder never goes there
    // one allocation: [geoms | geom_ids | tris | tri_ids | tri_albedo | tri_tex | tex_desc | tex | nodes | order | tri_boxes], 16-byte aligned parts
    const size_t o_g = 0, o_gi = o_g + align16(sizeof(SvgfSceneGeom) * ng), o_t = o_gi + align16(sizeof(int) * ng);
    const size_t o_ti = o_t + align16(sizeof(float) * 24 * nt), o_ta = o_ti + align16(sizeof(int) * nt), o_tt = o_ta + align16(sizeof(float) * 3 * nt);
    const size_t o_td = o_tt + align16(sizeof(int) * nt), o_tex = o_td + align16(sizeof(int) * 3 * (size_t)(n_tex > 0 ? n_tex : 1));
    const size_t o_n = o_tex + align16(n_texbytes > 16 ? n_texbytes : 16), o_o = o_n + sizeof(SvgfBvhNode) * 2 * nt, o_b = o_o + align16(sizeof(int) * nt);
    const size_t bytes = o_b + sizeof(SvgfBvhNode) * nt;
    std::vector<char> host(bytes, 0);
    if (n_geoms > 0) std::memcpy(&host[o_g], geoms, sizeof(SvgfSceneGeom) * (size_t)n_geoms);
    if (n_geoms > 0 && geom_ids) std::memcpy(&host[o_gi], geom_ids, sizeof(int) * (size_t)n_geoms);
    int n_leaves = 0;
    if (n_tris > 0) {
        std::memcpy(&host[o_t], tris, sizeof(float) * 24 * (size_t)n_tris);
        std::memcpy(&host[o_ti], tri_ids, sizeof(int) * (size_t)n_tris);
        std::memcpy(&host[o_ta], tri_albedo, sizeof(float) * 3 * (size_t)n_tris);
        std::memcpy(&host[o_n], nodes.data(), sizeof(SvgfBvhNode) * (size_t)n_nodes);
        std::memcpy(&host[o_o], order.data(), sizeof(int) * (size_t)n_tris);
        SvgfBvhNode *boxes = reinterpret_cast<SvgfBvhNode *>(&host[o_b]);
        for (int i = 0; i < n_tris; i++) { svgf_bvh_tri_box(tris + 24 * (size_t)i, boxes[i].lo, boxes[i].hi); boxes[i].first = i; boxes[i].count = 1; }
        for (int k = 0; k < n_nodes; k++) n_leaves += nodes[k].count > 0;
    }
    if (n_tex > 0) {
        std::memcpy(&host[o_tt], tri_tex, sizeof(int) * (size_t)n_tris);
        std::memcpy(&host[o_td], tex_desc, sizeof(int) * 3 * (size_t)n_tex);
        std::memcpy(&host[o_tex], tex_data, n_texbytes);
    }
    svgf_scene *sc = new (std::nothrow) svgf_scene();
    if (!sc) return SVGF_ERR_OOM;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) { delete sc; return SVGF_ERR_NO_DEVICE; }
    char *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) { delete sc; return SVGF_ERR_OOM; }
    if (hipMemcpy(d, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); delete sc; return SVGF_ERR_HIP; }
    sc->device = device; sc->dev = d;
    SceneArgs &a = sc->args.s;
    a.n_geoms = n_geoms;
    a.geoms = reinterpret_cast<const SvgfSceneGeom *>(d + o_g);
    a.geom_ids = (n_geoms > 0 && geom_ids) ? reinterpret_cast<const int *>(d + o_gi) : nullptr;
    a.n_tris = n_tris;
    a.tris = reinterpret_cast<const float *>(d + o_t);
    a.tri_ids = reinterpret_cast<const int *>(d + o_ti);
    a.tri_albedo = reinterpret_cast<const float *>(d + o_ta);
    a.tri_tex = n_tex > 0 ? reinterpret_cast<const int *>(d + o_tt) : nullptr;
    a.tex_desc = reinterpret_cast<const int *>(d + o_td);
    a.tex = reinterpret_cast<const unsigned char *>(d + o_tex);
    sc->args.nodes = reinterpret_cast<const float4 *>(d + o_n);
    sc->args.order = reinterpret_cast<const int *>(d + o_o);
    sc->args.tri_boxes = reinterpret_cast<const float4 *>(d + o_b);
    const int max_leaf = bp && bp->max_leaf_tris != 0 ? bp->max_leaf_tris : 4;
    sc->info = SvgfSceneInfo{ n_geoms, n_tris, n_tex, n_nodes, n_leaves, depth, max_leaf, (unsigned long long)bytes };
    *out = sc;
    return SVGF_OK;
}

extern "C" int svgf_scene_destroy(svgf_scene *scene)
{
    if (!scene) return SVGF_OK;
    SvgfDeviceGuard dev_guard(scene->device);
    int rc = SVGF_OK;
    if (!dev_guard.ok || hipDeviceSynchronize() != hipSuccess || hipFree(scene->dev) != hipSuccess) rc = SVGF_ERR_HIP;
    if (scene->anim && (!dev_guard.ok || hipFree(scene->anim) != hipSuccess)) rc = SVGF_ERR_HIP;
    delete scene;
    return rc;
}

extern "C" int svgf_scene_info(const svgf_scene *scene, SvgfSceneInfo *out)
{
    if (!scene || !out) return SVGF_ERR_INVALID_ARG;
    *out = scene_info(scene);
    return SVGF_OK;
}

// row f17: what the draws read, for a renderer-side library that traces its own rays (svgf_scene_trace.hip); host only
extern "C" int svgf_scene_view(const svgf_scene *scene, SvgfSceneView *out)
{
    if (!scene || !out) return SVGF_ERR_INVALID_ARG;
    const SceneArgs &a = scene->args.s;
    const SvgfSceneInfo in = scene_info(scene);
    *out = SvgfSceneView{ scene->device, in.n_geoms, in.n_tris, in.n_tex, in.n_nodes, in.depth, a.geoms, a.geom_ids, a.tris, a.tri_ids, a.tri_albedo,
                          a.tri_tex, a.tex_desc, a.tex, reinterpret_cast<const SvgfBvhNode *>(scene_nodes(scene)), scene_order(scene),
                          reinterpret_cast<const SvgfBvhNode *>(scene->args.tri_boxes) };
    return SVGF_OK;
}

// `area` NULL: svgf_scene_draw*, k_scene_bvh; otherwise svgf_scene_draw_shadowed (light == area->centre), k_scene_bvh<true>
static int scene_draw_impl(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                           const SvgfCamera *cam, const SvgfSynthParams *sp, const float light[3], const SvgfSceneLight *area, void *stream)
{
    if (!scene || !out_rgb_dev || (!out_gbuffer_dev && !planes) || !cam || !sp || !light || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if (!out_gbuffer_dev && (!planes->normal || !planes->position || !planes->geom_id)) return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(scene->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    SceneBvhArgs b = scene->args;
    b.nodes = scene_nodes(scene); b.order = scene_order(scene);
    scene_frame_args(b.s, width, height, cam, sp, light);
    b.s.out_rgb = static_cast<float *>(out_rgb_dev);
    b.s.out_gbuf = static_cast<float *>(out_gbuffer_dev);
    b.s.pl_nrm = planes ? planes->normal : nullptr; b.s.pl_pos = planes ? planes->position : nullptr;
    b.s.pl_alb = planes ? planes->albedo : nullptr; b.s.pl_gid = planes ? planes->geom_id : nullptr;
    const int n = width * height;
    if (area) {
        SceneShadowArgs sa;
        sa.b = b;
        for (int c = 0; c < 3; c++) { sa.edge_u[c] = area->edge_u[c]; sa.edge_v[c] = area->edge_v[c]; }
        sa.samples = area->samples;
        hipLaunchKernelGGL(k_scene_bvh<true>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), sa);
    } else {
        hipLaunchKernelGGL(k_scene_bvh<false>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), b);
    }
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_scene_draw(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev, int width, int height, const SvgfCamera *cam,
                               const SvgfSynthParams *sp, const float light[3], void *stream)
{
    if (!out_gbuffer_dev) return SVGF_ERR_INVALID_ARG;
    return scene_draw_impl(scene, out_rgb_dev, out_gbuffer_dev, nullptr, width, height, cam, sp, light, nullptr, stream);
}

// the same frame written into the planes of svgf_planar_gbuffer
extern "C" int svgf_scene_draw_planar(const svgf_scene *scene, void *out_rgb_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                                      const SvgfCamera *cam, const SvgfSynthParams *sp, const float light[3], void *stream)
{
    if (!planes) return SVGF_ERR_INVALID_ARG;
    return scene_draw_impl(scene, out_rgb_dev, nullptr, planes, width, height, cam, sp, light, nullptr, stream);
}

// row f16: the same frame with stochastic shadow rays towards a parallelogram light; AoS or planar target, exactly one of them
extern "C" int svgf_scene_draw_shadowed(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes,
                                        int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light,
                                        void *stream)
{
    if (!light || light->samples < 1 || light->samples > SVGF_SCENE_MAX_SHADOW_SAMPLES) return SVGF_ERR_INVALID_ARG;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(light->centre[c]) || !std::isfinite(light->edge_u[c]) || !std::isfinite(light->edge_v[c])) return SVGF_ERR_INVALID_ARG;
    if ((out_gbuffer_dev != nullptr) == (planes != nullptr)) return SVGF_ERR_INVALID_ARG;
    return scene_draw_impl(scene, out_rgb_dev, out_gbuffer_dev, planes, width, height, cam, sp, light->centre, light, stream);
}

// ---- row f15: the animated resident scene ---------------------------------------------------------------------------------------------------
extern "C" int svgf_scene_enable_pose(svgf_scene *scene, int n_objects)
{
    if (!scene || n_objects < 1 || n_objects > SVGF_SCENE_MAX_POSED) return SVGF_ERR_INVALID_ARG;
    if (scene->anim) return n_objects == scene->n_objects ? SVGF_OK : SVGF_ERR_INVALID_ARG;
    const SvgfSceneInfo &in = scene->info;
    const size_t nt = (size_t)(in.n_tris > 0 ? in.n_tris : 1), ng = (size_t)(in.n_geoms > 0 ? in.n_geoms : 1), nn = (size_t)(in.n_nodes > 0 ? in.n_nodes : 1);
    // the plan, from the nodes as created (a blocking read; this call is not for use under capture)
    SvgfDeviceGuard dev_guard(scene->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    std::vector<SvgfBvhNode> nodes(nn);
    if (in.n_nodes > 0 && hipMemcpy(nodes.data(), scene->args.nodes, sizeof(SvgfBvhNode) * (size_t)in.n_nodes, hipMemcpyDeviceToHost) != hipSuccess) return SVGF_ERR_HIP;
    std::vector<SvgfRefitTreelet> treelets(nn);
    std::vector<unsigned char> level(nn);
    std::vector<int> top(nn), top_seg(SVGF_SCENE_MAX_DEPTH + 2, 0);
    SvgfRefitPlanInfo plan;
    const int rc = svgf_bvh_refit_plan_host(nodes.data(), in.n_nodes, kRefitCap, treelets.data(), level.data(), top.data(), top_seg.data(), &plan);
    if (rc != SVGF_OK) return rc;
    for (int k = 0; k < plan.n_treelets; k++)
        if (treelets[k].count + 1 > kRefitCap) return SVGF_ERR_UNSUPPORTED;      // the treelet kernel's LDS; the plan never goes there
    // one allocation: [tris | tri_boxes | nodes | geoms | held | treelets | level | top | top_seg], 16-byte aligned parts
    const size_t o_t = 0, o_b = o_t + align16(sizeof(float) * 24 * nt), o_n = o_b + sizeof(SvgfBvhNode) * nt, o_g = o_n + sizeof(SvgfBvhNode) * nn;
    const size_t o_h = o_g + align16(sizeof(SvgfSceneGeom) * ng), o_tl = o_h + sizeof(SvgfScenePose) * (size_t)n_objects;
    const size_t o_lv = o_tl + sizeof(SvgfRefitTreelet) * nn, o_tp = o_lv + align16(nn), o_ts = o_tp + align16(sizeof(int) * nn);
    const size_t bytes = o_ts + align16(sizeof(int) * top_seg.size());
    char *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), bytes) != hipSuccess) return SVGF_ERR_OOM;
    const SceneArgs &a = scene->args.s;
    std::vector<float> held(24 * (size_t)n_objects);
    for (int k = 0; k < n_objects; k++) std::memcpy(&held[24 * (size_t)k], kIdentityPose, sizeof(kIdentityPose));
    bool ok = hipMemset(d, 0, bytes) == hipSuccess;
    if (in.n_tris > 0) {
        ok = ok && hipMemcpy(d + o_t, a.tris, sizeof(float) * 24 * (size_t)in.n_tris, hipMemcpyDeviceToDevice) == hipSuccess;
        ok = ok && hipMemcpy(d + o_b, scene->args.tri_boxes, sizeof(SvgfBvhNode) * (size_t)in.n_tris, hipMemcpyDeviceToDevice) == hipSuccess;
        ok = ok && hipMemcpy(d + o_n, scene->args.nodes, sizeof(SvgfBvhNode) * (size_t)in.n_nodes, hipMemcpyDeviceToDevice) == hipSuccess;
        ok = ok && hipMemcpy(d + o_tl, treelets.data(), sizeof(SvgfRefitTreelet) * (size_t)plan.n_treelets, hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && hipMemcpy(d + o_lv, level.data(), (size_t)in.n_nodes, hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && (plan.n_top == 0 || hipMemcpy(d + o_tp, top.data(), sizeof(int) * (size_t)plan.n_top, hipMemcpyHostToDevice) == hipSuccess);
        ok = ok && hipMemcpy(d + o_ts, top_seg.data(), sizeof(int) * top_seg.size(), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (in.n_geoms > 0) ok = ok && hipMemcpy(d + o_g, a.geoms, sizeof(SvgfSceneGeom) * (size_t)in.n_geoms, hipMemcpyDeviceToDevice) == hipSuccess;
    ok = ok && hipMemcpy(d + o_h, held.data(), sizeof(float) * held.size(), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) { (void)hipFree(d); return SVGF_ERR_HIP; }
    ScenePoseArgs &p = scene->pose;
    p.n_tris = in.n_tris; p.n_geoms = in.n_geoms; p.n_objects = n_objects; p.tri_blocks = (in.n_tris + 255) / 256;
    p.rest_tris = reinterpret_cast<const float4 *>(a.tris); p.tris = reinterpret_cast<float4 *>(d + o_t);
    p.tri_ids = a.tri_ids; p.tri_boxes = reinterpret_cast<float4 *>(d + o_b);
    p.rest_geoms = a.geoms; p.geoms = reinterpret_cast<SvgfSceneGeom *>(d + o_g); p.geom_ids = a.geom_ids;
    p.pose = nullptr; p.held = reinterpret_cast<float4 *>(d + o_h); p.motion = nullptr;
    SceneRefitArgs &r = scene->refit;
    r.nodes = reinterpret_cast<float4 *>(d + o_n); r.order = scene->args.order; r.tri_boxes = p.tri_boxes;
    r.treelets = reinterpret_cast<const int4 *>(d + o_tl); r.level = reinterpret_cast<const unsigned char *>(d + o_lv);
    r.top = reinterpret_cast<const int *>(d + o_tp); r.top_seg = reinterpret_cast<const int *>(d + o_ts); r.n_top_depths = plan.n_top_depths;
    // from here on the draws read the posed copies
    scene->args.s.tris = reinterpret_cast<const float *>(p.tris);
    scene->args.s.geoms = p.geoms;
    scene->args.tri_boxes = p.tri_boxes;
    scene->args.nodes = r.nodes;
    scene->anim = d; scene->n_objects = n_objects; scene->n_treelets = plan.n_treelets; scene->n_top = plan.n_top;
    scene->info.device_bytes += (unsigned long long)bytes;
    return SVGF_OK;
}

extern "C" int svgf_scene_pose(svgf_scene *scene, const SvgfScenePose *pose_dev, int n_objects, float *motion_out_dev, void *stream)
{
    if (!scene || !pose_dev || !scene->anim || n_objects != scene->n_objects) return SVGF_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(pose_dev) & 15) || (reinterpret_cast<uintptr_t>(motion_out_dev) & 15)) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(scene->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    ScenePoseArgs p = scene->pose;
    p.pose = reinterpret_cast<const float4 *>(pose_dev);
    p.motion = reinterpret_cast<float4 *>(motion_out_dev);
    const int tail = (p.n_geoms > p.n_objects ? p.n_geoms : p.n_objects);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_scene_pose, dim3(p.tri_blocks + (tail + 255) / 256), dim3(256), 0, st, p);
    if (scene->ad_nodes) return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;      // row f24: the caller rebuilds its tree
    if (scene->n_treelets > 0) hipLaunchKernelGGL(k_scene_refit_treelets, dim3(scene->n_treelets), dim3(256), 0, st, scene->refit);
    if (scene->n_top > 0) hipLaunchKernelGGL(k_scene_refit_top, dim3(1), dim3(256), 0, st, scene->refit);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_scene_read(const svgf_scene *scene, int which, void *host_dst, unsigned long long host_bytes)
{
    if (!scene || which < 0 || which > 5 || (which == 5 && !scene->anim)) return SVGF_ERR_INVALID_ARG;
    const SvgfSceneInfo in = scene_info(scene);
    const void *src[6] = { scene->args.s.tris, scene->args.tri_boxes, scene_nodes(scene), scene->args.s.geoms, scene_order(scene), scene->pose.held };
    const unsigned long long size[6] = { 96ull * in.n_tris, 32ull * in.n_tris, 32ull * in.n_nodes, (unsigned long long)sizeof(SvgfSceneGeom) * in.n_geoms,
                                         4ull * in.n_tris, (unsigned long long)sizeof(SvgfScenePose) * scene->n_objects };
    if (host_bytes != size[which] || (host_bytes > 0 && !host_dst)) return SVGF_ERR_INVALID_ARG;
    if (host_bytes == 0) return SVGF_OK;
    SvgfDeviceGuard dev_guard(scene->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_dst, src[which], (size_t)host_bytes, hipMemcpyDeviceToHost) != hipSuccess) return SVGF_ERR_HIP;
    return SVGF_OK;
}

// row f24: draw with the caller's tree (host only; include/svgf.h states the contract)
extern "C" int svgf_scene_adopt_tree(svgf_scene *scene, const SvgfBvhNode *nodes_dev, const int *order_dev, int n_nodes, int n_leaves, int depth_bound)
{
    if (!scene || scene->info.n_tris == 0) return SVGF_ERR_INVALID_ARG;
    if (!nodes_dev) { scene->ad_nodes = nullptr; scene->ad_order = nullptr; scene->ad_n_nodes = scene->ad_n_leaves = scene->ad_depth = 0; return SVGF_OK; }
    if (!order_dev || n_leaves < 1 || n_leaves > scene->info.n_tris || n_nodes != 2 * n_leaves - 1 || depth_bound < 0 || depth_bound > SVGF_SCENE_MAX_DEPTH ||
        (reinterpret_cast<uintptr_t>(nodes_dev) & 15) || (reinterpret_cast<uintptr_t>(order_dev) & 15)) return SVGF_ERR_INVALID_ARG;
    scene->ad_nodes = reinterpret_cast<const float4 *>(nodes_dev); scene->ad_order = order_dev;
    scene->ad_n_nodes = n_nodes; scene->ad_n_leaves = n_leaves; scene->ad_depth = depth_bound;
    return SVGF_OK;
}

// row f26: the posed copies, writable, for renderer-side code that deforms them (libsvgf_deform.so); host only
extern "C" int svgf_scene_drawn_arrays(svgf_scene *scene, float **tris_dev, SvgfBvhNode **tri_boxes_dev)
{
    if (!scene || !tris_dev || !tri_boxes_dev || !scene->anim) return SVGF_ERR_INVALID_ARG;
    *tris_dev = reinterpret_cast<float *>(scene->pose.tris);
    *tri_boxes_dev = reinterpret_cast<SvgfBvhNode *>(scene->pose.tri_boxes);
    return SVGF_OK;
}

// row f26: svgf_scene_pose's two refit launches on the scene's own nodes, from the boxes as drawn, and nothing else
extern "C" int svgf_scene_refit(svgf_scene *scene, void *stream)
{
    if (!scene || !scene->anim) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(scene->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (scene->n_treelets > 0) hipLaunchKernelGGL(k_scene_refit_treelets, dim3(scene->n_treelets), dim3(256), 0, st, scene->refit);
    if (scene->n_top > 0) hipLaunchKernelGGL(k_scene_refit_top, dim3(1), dim3(256), 0, st, scene->refit);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
