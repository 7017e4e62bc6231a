// svgf_scene_bvh.hip — the resident scene (row f14): the scene producer's inputs kept on the device with a BVH over the triangles,
// and a draw that is one launch.  include/svgf.h states the semantics (a gated brute force that every tree reproduces);
// svgf_bvh_build.cpp builds the tree on the host; the per-pixel body around the triangle search is svgf_scene_pixel.inc.h, the text
// k_scene_frame compiles too.
//
// k_scene_bvh: one thread per pixel, 256 per block.  The walk keeps the current node in registers, descends into the nearer child
// and parks the other one on a per-lane stack in LDS: stack[level][lane], 48 levels x 256 lanes x 4 B = 48 KB per block, a lane's
// entries 1 KB apart so that the 64 lanes of a wave always touch 64 consecutive words (no bank conflict, no runtime-indexed private
// array, no scratch).  A parked node is tested again when it is popped - the nearest hit may have come closer since - which costs one
// 32-byte load of a node that was loaded as a child before.  SVGF_SCENE_MAX_DEPTH bounds the stack: a lane holds one entry per
// level above its current node.
#include "svgf_kernels.h"
#include "../../include/svgf.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

void svgf_bvh_tri_box(const float *T, float lo[3], float hi[3]);       // svgf_bvh_build.cpp

namespace {

#include "svgf_scene_pixel.inc.h"

struct SceneBvhArgs {
    SceneArgs s;
    const float4 *nodes;        // SvgfBvhNode as two float4: {lo, first}, {hi, count}
    const int *order;
    const float4 *tri_boxes;    // the padded box of triangle i, the same 32-byte layout: {lo, -}, {hi, -}
};

struct SceneRay { float o[3], d[3], inv[3]; bool flat[3]; };

// S(box, ray) of include/svgf.h
__device__ __forceinline__ bool scene_slab(const float4 &lo4, const float4 &hi4, const SceneRay &r, float &tn)
{
#pragma clang fp contract(off)
    const float lo[3] = { lo4.x, lo4.y, lo4.z }, hi[3] = { hi4.x, hi4.y, hi4.z };
    float tf = __builtin_huge_valf();
    bool pass = true;
    tn = 0.0f;
    for (int c = 0; c < 3; c++) {
        if (r.flat[c]) {
            pass = pass && (lo[c] <= r.o[c]) && (r.o[c] <= hi[c]);
        } else {
            const float t1 = (lo[c] - r.o[c]) * r.inv[c], t2 = (hi[c] - r.o[c]) * r.inv[c];
            tn = fmaxf(tn, fminf(t1, t2));
            tf = fminf(tf, fmaxf(t1, t2));
        }
    }
    return pass && (tn <= tf);
}

__global__ __launch_bounds__(256) void k_scene_bvh(SceneBvhArgs b)
{
#pragma clang fp contract(off)
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
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
        if (a.n_tris > 0) {
            int *const stk = stack + threadIdx.x;
            int sp = 0;
            float4 nlo = b.nodes[0], nhi = b.nodes[1];
            float tn;
            bool go = scene_slab(nlo, nhi, r, tn) && !(tn > bt);
            while (go) {
                const int first = __float_as_int(nlo.w), count = __float_as_int(nhi.w);
                bool down = false;
                if (count > 0) {
                    for (int k = first; k < first + count; k++) {
                        const int i = b.order[k];
                        float bx, by, t;
                        if (!scene_tri_test(a.tris + 24 * (size_t)i, r.o, r.d, bx, by, t) || !(t > 0.0f)) continue;
                        float tni;
                        if (!scene_slab(b.tri_boxes[2 * (size_t)i], b.tri_boxes[2 * (size_t)i + 1], r, tni) || !(t >= tni)) continue;
                        if (t < bt || (t == bt && best >= 0 && i < best)) { bt = t; best = i; bbx = bx; bby = by; }
                    }
                } else {
                    const float4 alo = b.nodes[2 * (size_t)first], ahi = b.nodes[2 * (size_t)first + 1];
                    const float4 blo = b.nodes[2 * (size_t)first + 2], bhi = b.nodes[2 * (size_t)first + 3];
                    float ta, tb;
                    const bool pa = scene_slab(alo, ahi, r, ta) && !(ta > bt), pb = scene_slab(blo, bhi, r, tb) && !(tb > bt);
                    const bool a_first = pa && (!pb || ta <= tb);
                    if (pa && pb) { stk[256 * sp] = a_first ? first + 1 : first; sp++; }
                    if (pa || pb) { nlo = a_first ? alo : blo; nhi = a_first ? ahi : bhi; down = true; }
                }
                if (!down) {
                    go = false;
                    while (sp > 0 && !go) {
                        sp--;
                        const int cur = stk[256 * sp];
                        nlo = b.nodes[2 * (size_t)cur]; nhi = b.nodes[2 * (size_t)cur + 1];
                        go = scene_slab(nlo, nhi, r, tn) && !(tn > bt);
                    }
                }
            }
        }
        scene_finish(a, p, r.o, r.d, h, best, bt, bbx, bby);
    }
}

constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

struct svgf_scene {
    int device;
    char *dev;                  // the one allocation
    SceneBvhArgs args;          // the scene's pointers; camera, outputs and frame are filled per draw
    SvgfSceneInfo info;
};

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
    delete scene;
    return rc;
}

extern "C" int svgf_scene_info(const svgf_scene *scene, SvgfSceneInfo *out)
{
    if (!scene || !out) return SVGF_ERR_INVALID_ARG;
    *out = scene->info;
    return SVGF_OK;
}

static int scene_draw_impl(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                           const SvgfCamera *cam, const SvgfSynthParams *sp, const float light[3], void *stream)
{
    if (!scene || !out_rgb_dev || (!out_gbuffer_dev && !planes) || !cam || !sp || !light || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if (!out_gbuffer_dev && (!planes->normal || !planes->position || !planes->geom_id)) return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(scene->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    SceneBvhArgs b = scene->args;
    scene_frame_args(b.s, width, height, cam, sp, light);
    b.s.out_rgb = static_cast<float *>(out_rgb_dev);
    b.s.out_gbuf = static_cast<float *>(out_gbuffer_dev);
    b.s.pl_nrm = planes ? planes->normal : nullptr; b.s.pl_pos = planes ? planes->position : nullptr;
    b.s.pl_alb = planes ? planes->albedo : nullptr; b.s.pl_gid = planes ? planes->geom_id : nullptr;
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_bvh, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), b);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_scene_draw(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev, int width, int height, const SvgfCamera *cam,
                               const SvgfSynthParams *sp, const float light[3], void *stream)
{
    if (!out_gbuffer_dev) return SVGF_ERR_INVALID_ARG;
    return scene_draw_impl(scene, out_rgb_dev, out_gbuffer_dev, nullptr, width, height, cam, sp, light, stream);
}

// the same frame written into the planes of svgf_planar_gbuffer
extern "C" int svgf_scene_draw_planar(const svgf_scene *scene, void *out_rgb_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                                      const SvgfCamera *cam, const SvgfSynthParams *sp, const float light[3], void *stream)
{
    if (!planes) return SVGF_ERR_INVALID_ARG;
    return scene_draw_impl(scene, out_rgb_dev, nullptr, planes, width, height, cam, sp, light, stream);
}
