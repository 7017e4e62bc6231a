// svgf_deform.hip — row f26, libsvgf_deform.so: skinned triangles in a resident scene (include/svgf_deform.h states the rig, the
// arithmetic and the previous-position rule).  The library reaches the scene through svgf_scene_view and svgf_scene_drawn_arrays alone
// (struct svgf_scene is unknown here) and links against libsvgf_hip.so alone.
//   k_deform_init   at creation: slot s copies its triangle as drawn into rest[s], its positions into cur[s] and prev[s]
//   k_deform_apply  one thread per skinned triangle: prev := cur, skin from rest, cur, the drawn triangle, its padded box.  A thread
//                   owns its slot and its triangle (tri_index is strictly increasing), so no two threads write one address and nothing
//                   passes between workgroups.  The bone rows are read through the table's 16-byte rows; every index was checked on
//                   the host (svgf_deform_rig.cpp) against the n_bones an apply must be called with.
//   k_deform_prev   one thread per pixel: the primary ray and the closest hit of k_scene_bvh - the product's own text,
//                   svgf_scene_pixel.inc.h and svgf_scene_walk.inc.h, with its per-lane stack in LDS (48 KB per block) - then the
//                   corner-weighted displacement prev - cur of the winning triangle's slot.
// float32, contraction off (build.TREE_BUILDERS' row adds -ffp-contract=off; the pragmas say it again where the arithmetic is normative).
#include "svgf_kernels.h"
#include "../../include/svgf_deform.h"
#include "../../include/svgf_scene_write.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

namespace {

#include "svgf_scene_pixel.inc.h"

#include "svgf_scene_walk.inc.h"

struct DeformArgs {
    int n_skinned;
    const int *tri_index;
    const unsigned short *bone;     // 12 per slot
    const float4 *weight;           // 3 float4 per slot: one per corner
    float4 *rest;                   // 6 float4 per slot: written once, by k_deform_init
    float *cur, *prev;              // 9 floats per slot
    float4 *tris;                   // the scene's triangles as drawn
    float4 *tri_boxes;
    const float4 *bones;            // SvgfScenePose records: 6 float4 each, the first three are xf
};

struct DeformPrevArgs {
    SceneBvhArgs b;
    const int *slot;
    const float *cur, *prev;
    float *out_pos;
    int *out_gid;
};

__global__ __launch_bounds__(256) void k_deform_init(DeformArgs a)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_skinned) return;
    const int i = a.tri_index[s];
    float4 q[6];
#pragma unroll
    for (int k = 0; k < 6; k++) q[k] = a.tris[6 * (size_t)i + k];
#pragma unroll
    for (int k = 0; k < 6; k++) a.rest[6 * (size_t)s + k] = q[k];
#pragma unroll
    for (int v = 0; v < 3; v++) {
        const float p[3] = { q[2 * v].x, q[2 * v].y, q[2 * v].z };
#pragma unroll
        for (int c = 0; c < 3; c++) { a.cur[9 * (size_t)s + 3 * v + c] = p[c]; a.prev[9 * (size_t)s + 3 * v + c] = p[c]; }
    }
}

__global__ __launch_bounds__(256) void k_deform_apply(DeformArgs a)
{
#pragma clang fp contract(off)
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_skinned) return;
    const int i = a.tri_index[s];
    // 1. prev := cur
#pragma unroll
    for (int k = 0; k < 9; k++) a.prev[9 * (size_t)s + k] = a.cur[9 * (size_t)s + k];
    // 2. the three corners from the REST triangle
    float4 q[6];
#pragma unroll
    for (int k = 0; k < 6; k++) q[k] = a.rest[6 * (size_t)s + k];
#pragma unroll
    for (int v = 0; v < 3; v++) {
        const float p[3] = { q[2 * v].x, q[2 * v].y, q[2 * v].z }, n[3] = { q[2 * v].w, q[2 * v + 1].x, q[2 * v + 1].y };
        const float4 w4 = a.weight[3 * (size_t)s + v];
        const float w[4] = { w4.x, w4.y, w4.z, w4.w };
        float pp[3] = { 0.0f, 0.0f, 0.0f }, nn[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int bi = a.bone[12 * (size_t)s + 4 * v + k];
            const float4 r0 = a.bones[6 * (size_t)bi], r1 = a.bones[6 * (size_t)bi + 1], r2 = a.bones[6 * (size_t)bi + 2];
            const float M[12] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w };
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const float qk = ((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3];
                const float mk = (M[4 * r] * n[0] + M[4 * r + 1] * n[1]) + M[4 * r + 2] * n[2];
                // ((w0 q0 + w1 q1) + w2 q2) + w3 q3: the first product stands alone, every later one is added to the sum so far
                pp[r] = k == 0 ? w[k] * qk : pp[r] + w[k] * qk;
                nn[r] = k == 0 ? w[k] * mk : nn[r] + w[k] * mk;
            }
        }
        q[2 * v] = make_float4(pp[0], pp[1], pp[2], nn[0]);
        q[2 * v + 1].x = nn[1]; q[2 * v + 1].y = nn[2];
        // 3. cur
#pragma unroll
        for (int c = 0; c < 3; c++) a.cur[9 * (size_t)s + 3 * v + c] = pp[c];
    }
    // 4. the triangle as drawn (uv are the rest's)
#pragma unroll
    for (int k = 0; k < 6; k++) a.tris[6 * (size_t)i + k] = q[k];
    // 5. svgf_bvh_tri_box on the skinned positions: the literals and the nesting of k_scene_pose
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
}

__global__ __launch_bounds__(256) void k_deform_prev(DeformPrevArgs arg)
{
#pragma clang fp contract(off)
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneBvhArgs &b = arg.b;
    const SceneArgs &a = b.s;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.W * a.H) return;
    SceneRay r;
    scene_ray(a, p % a.W, p / a.W, r.o, r.d);
    SceneHit h;
    scene_primitives(a, r.o, r.d, h);
    for (int c = 0; c < 3; c++) { r.flat[c] = fabsf(r.d[c]) < 0x1p-100f; r.inv[c] = 1.0f / r.d[c]; }
    int best = -1;
    float bt = h.t_best, bbx = 0.0f, bby = 0.0f;
    scene_nearest(b, r, stack + threadIdx.x, 0.0f, bt, best, bbx, bby);
    float pos[3];
    scene_surface(a, r.o, r.d, h, best, bt, bbx, bby, pos);
    float out[3] = { pos[0], pos[1], pos[2] };
    if (h.gid < 0) {
        out[0] = out[1] = out[2] = __builtin_nanf("");
    } else if (best >= 0) {
        const int s = arg.slot[best];
        if (s >= 0) {
            const float b0 = 1.0f - bbx - bby;
            const float *pv = arg.prev + 9 * (size_t)s, *cu = arg.cur + 9 * (size_t)s;
            for (int c = 0; c < 3; c++) {
                const float d = (b0 * (pv[c] - cu[c]) + bbx * (pv[3 + c] - cu[3 + c])) + bby * (pv[6 + c] - cu[6 + c]);
                out[c] = d == 0.0f ? pos[c] : pos[c] + d;
            }
        }
    }
    arg.out_pos[3 * (size_t)p] = out[0]; arg.out_pos[3 * (size_t)p + 1] = out[1]; arg.out_pos[3 * (size_t)p + 2] = out[2];
    if (arg.out_gid) arg.out_gid[p] = h.gid < 0 ? -1 : h.gid;
}

constexpr size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

struct svgf_deform {
    svgf_scene *scene;
    int device, n_tris, n_skinned, n_bones;
    char *dev;                  // the one allocation
    unsigned long long bytes;
    DeformArgs args;
    const int *slot;
};

extern "C" int svgf_deform_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_deform_create(svgf_scene *scene, const int *tri_index, int n_skinned, const unsigned short *bone, const float *weight, int n_bones,
                                  svgf_deform **out)
{
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    if (!scene) return SVGF_ERR_INVALID_ARG;
    SvgfSceneView v;
    float *tris = nullptr;
    SvgfBvhNode *boxes = nullptr;
    if (svgf_scene_view(scene, &v) != SVGF_OK || svgf_scene_drawn_arrays(scene, &tris, &boxes) != SVGF_OK) return SVGF_ERR_INVALID_ARG;
    const int rc = svgf_deform_check_rig_host(v.n_tris, tri_index, n_skinned, bone, weight, n_bones);
    if (rc != SVGF_OK) return rc;
    const size_t ns = (size_t)n_skinned, nt = (size_t)v.n_tris;
    // one allocation: [tri_index | bone | weight | slot | rest | cur | prev], 16-byte aligned parts
    const size_t o_i = 0, o_b = o_i + align16(sizeof(int) * ns), o_w = o_b + align16(sizeof(unsigned short) * 12 * ns);
    const size_t o_s = o_w + sizeof(float) * 12 * ns, o_r = o_s + align16(sizeof(int) * nt), o_c = o_r + sizeof(float) * 24 * ns;
    const size_t o_p = o_c + align16(sizeof(float) * 9 * ns), bytes = o_p + align16(sizeof(float) * 9 * ns);
    std::vector<char> host(o_r, 0);         // the uploaded part: the rig and the slots
    std::memcpy(&host[o_i], tri_index, sizeof(int) * ns);
    std::memcpy(&host[o_b], bone, sizeof(unsigned short) * 12 * ns);
    std::memcpy(&host[o_w], weight, sizeof(float) * 12 * ns);
    int *slot = reinterpret_cast<int *>(&host[o_s]);
    for (size_t i = 0; i < nt; i++) slot[i] = -1;
    for (size_t s = 0; s < ns; s++) slot[tri_index[s]] = (int)s;
    svgf_deform *d = new (std::nothrow) svgf_deform();
    if (!d) return SVGF_ERR_OOM;
    SvgfDeviceGuard dev_guard(v.device);
    if (!dev_guard.ok) { delete d; return SVGF_ERR_NO_DEVICE; }
    char *m = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&m), bytes) != hipSuccess) { delete d; return SVGF_ERR_OOM; }
    DeformArgs &a = d->args;
    a.n_skinned = n_skinned;
    a.tri_index = reinterpret_cast<const int *>(m + o_i); a.bone = reinterpret_cast<const unsigned short *>(m + o_b);
    a.weight = reinterpret_cast<const float4 *>(m + o_w); a.rest = reinterpret_cast<float4 *>(m + o_r);
    a.cur = reinterpret_cast<float *>(m + o_c); a.prev = reinterpret_cast<float *>(m + o_p);
    a.tris = reinterpret_cast<float4 *>(tris); a.tri_boxes = reinterpret_cast<float4 *>(boxes); a.bones = nullptr;
    bool ok = hipMemset(m, 0, bytes) == hipSuccess && hipMemcpy(m, host.data(), o_r, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_deform_init, dim3((n_skinned + 255) / 256), dim3(256), 0, nullptr, a);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) { (void)hipFree(m); delete d; return SVGF_ERR_HIP; }
    d->scene = scene; d->device = v.device; d->n_tris = v.n_tris; d->n_skinned = n_skinned; d->n_bones = n_bones;
    d->dev = m; d->bytes = (unsigned long long)bytes; d->slot = reinterpret_cast<const int *>(m + o_s);
    *out = d;
    return SVGF_OK;
}

extern "C" int svgf_deform_apply(svgf_deform *d, const SvgfScenePose *bones_dev, int n_bones, void *stream)
{
    if (!d || !bones_dev || n_bones != d->n_bones || (reinterpret_cast<uintptr_t>(bones_dev) & 15)) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(d->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    DeformArgs a = d->args;
    a.bones = reinterpret_cast<const float4 *>(bones_dev);
    hipLaunchKernelGGL(k_deform_apply, dim3((a.n_skinned + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_deform_prev_positions(const svgf_deform *d, float *out_prev_pos_dev, int *out_geom_id_dev, int width, int height,
                                          const SvgfCamera *cam, const float pixel_length[2], void *stream)
{
    if (!d || !out_prev_pos_dev || !cam || !pixel_length || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfSceneView v;
    if (svgf_scene_view(d->scene, &v) != SVGF_OK || v.n_tris != d->n_tris) return SVGF_ERR_INVALID_ARG;
    if (v.depth > SVGF_SCENE_MAX_DEPTH) return SVGF_ERR_UNSUPPORTED;        // the kernel's stack; svgf_scene_adopt_tree never lets it
    SvgfDeviceGuard dev_guard(d->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    DeformPrevArgs t;
    std::memset(&t, 0, sizeof(t));
    SceneArgs &a = t.b.s;
    a.n_geoms = v.n_geoms; a.geoms = v.geoms; a.geom_ids = v.geom_ids;
    a.n_tris = v.n_tris; a.tris = v.tris; a.tri_ids = v.tri_ids; a.tri_albedo = v.tri_albedo;
    a.tri_tex = v.tri_tex; a.tex_desc = v.tex_desc; a.tex = v.tex;
    t.b.nodes = reinterpret_cast<const float4 *>(v.nodes); t.b.order = v.order; t.b.tri_boxes = reinterpret_cast<const float4 *>(v.tri_boxes);
    const SvgfSynthParams sp = { 0, 0, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
    const float no_light[3] = { 0.0f, 0.0f, 0.0f };
    scene_frame_args(a, width, height, cam, &sp, no_light);
    t.slot = d->slot; t.cur = d->args.cur; t.prev = d->args.prev;
    t.out_pos = out_prev_pos_dev; t.out_gid = out_geom_id_dev;
    const int n = width * height;
    hipLaunchKernelGGL(k_deform_prev, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_deform_info(const svgf_deform *d, SvgfDeformInfo *out)
{
    if (!d || !out) return SVGF_ERR_INVALID_ARG;
    *out = SvgfDeformInfo{ d->n_tris, d->n_skinned, d->n_bones, 1, d->bytes };
    return SVGF_OK;
}

extern "C" int svgf_deform_read(const svgf_deform *d, int which, void *host_dst, unsigned long long host_bytes)
{
    if (!d || which < 0 || which > 2 || !host_dst) return SVGF_ERR_INVALID_ARG;
    const void *src[3] = { d->args.cur, d->args.prev, d->slot };
    const unsigned long long size[3] = { 36ull * d->n_skinned, 36ull * d->n_skinned, 4ull * d->n_tris };
    if (host_bytes != size[which]) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(d->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_dst, src[which], (size_t)host_bytes, hipMemcpyDeviceToHost) != hipSuccess) return SVGF_ERR_HIP;
    return SVGF_OK;
}

extern "C" void svgf_deform_destroy(svgf_deform *d)
{
    if (!d) return;
    SvgfDeviceGuard dev_guard(d->device);
    if (dev_guard.ok) { (void)hipDeviceSynchronize(); (void)hipFree(d->dev); }
    delete d;
}
