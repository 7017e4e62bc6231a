// svgf_scene_path.hip — libsvgf_path.so, the companion library of row f19: svgf_path_draw and svgf_path_draw_split, the resident scene
// traced along paths of up to SVGF_PATH_MAX_DEPTH diffuse bounces with next-event estimation at every vertex and Russian roulette.
// include/svgf_path.h states the semantics.  Like the other two companions this one links against libsvgf_hip.so and reaches a scene
// through svgf_scene_view alone.  Everything a ray, a sampled direction or a stored pixel consists of is svgf_scene_trace.inc.h's text
// (and through it svgf_scene_pixel.inc.h's and svgf_scene_walk.inc.h's): trace_prepare, trace_aim, trace_direction, trace_store_split,
// the two walks, scene_surface, scene_direct, scene_store.  What is new here is the loop that strings them into a path.
//
// k_scene_path: one thread per pixel, 256 per block, every ray of the pixel on the per-lane LDS stack stack[level][lane] (48 x 256 x 4 B;
// empty between rays).  Paths and bounces are runtime loops around ONE vertex body, so the code object holds one closest-hit walk and
// one any-hit walk behind the first hit whatever the counts.  A path's state is scalars in registers - thr, acc, the vertex and its
// normal; T and B are formed per bounce from the normal - no runtime-indexed private array, no scratch, no spinning, no traffic between
// workgroups.
#include "svgf_kernels.h"
#include "../../include/svgf_trace.h"
#include "../../include/svgf_path.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

namespace {

#include "svgf_scene_trace.inc.h"

// t (and for the split form s.t).bounce_samples carries `paths`
struct ScenePathArgs {
    SceneTraceArgs t;
    int max_depth, rr_depth;
};

struct ScenePathSplitArgs {
    SceneSplitArgs s;
    int max_depth, rr_depth;
};

__device__ __forceinline__ const SceneTraceArgs &trace_args(const ScenePathArgs &a) { return a.t; }
__device__ __forceinline__ const SceneTraceArgs &trace_args(const ScenePathSplitArgs &a) { return a.s.t; }

// Args = ScenePathArgs: svgf_path_draw.  Args = ScenePathSplitArgs: svgf_path_draw_split, the same rays with trace_store_split's tail.
template <class Args>
__global__ __launch_bounds__(256) void k_scene_path(Args args)
{
#pragma clang fp contract(off)
    constexpr bool SPLIT = std::is_same<Args, ScenePathSplitArgs>::value;
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneTraceArgs &arg = trace_args(args);
    const SceneBvhArgs &b = arg.b;
    const SceneArgs &a = b.s;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < a.W * a.H) {
        int *const stk = stack + threadIdx.x;
        // the first hit, its shadow rays and its term: k_scene_trace's statements
        SceneRay r;
        scene_ray(a, p % a.W, p / a.W, r.o, r.d);
        SceneHit h;
        scene_primitives(a, r.o, r.d, h);
        trace_aim(r);
        int best = -1;
        float bt = h.t_best, bbx = 0.0f, bby = 0.0f;
        scene_nearest(b, r, stk, 0.0f, bt, best, bbx, bby);
        float pos[3];
        scene_surface(a, r.o, r.d, h, best, bt, bbx, bby, pos);

        float shade[3] = { h.emit, h.emit, h.emit };
        float first_term = h.emit, ind_term[3] = { 0.0f, 0.0f, 0.0f };
        bool bounced = false;
        if (!(h.emit > 0.0f)) {
            const bool casts = h.gid >= 0;
            int unoccluded = arg.samples;
            if (casts) {
                unoccluded = 0;
                for (int c = 0; c < 3; c++) r.o[c] = pos[c];
                for (int s = 0; s < arg.samples; s++)
                    unoccluded += scene_shadow_sample(b, arg.edge_u, arg.edge_v, r, pos, stk, p, 8 + 2 * s, 9 + 2 * s) ? 0 : 1;
            }
            const float vis = (float)unoccluded / (float)arg.samples;
            const float first = arg.ambient + vis * scene_direct(a, h.n, pos);
            shade[0] = first; shade[1] = first; shade[2] = first;
            first_term = first;
            const int paths = arg.bounce_samples;
            if (casts && paths > 0) {
                float ind[3] = { 0.0f, 0.0f, 0.0f };
                for (int j = 0; j < paths; j++) {
                    float thr[3] = { 1.0f, 1.0f, 1.0f }, acc[3] = { 0.0f, 0.0f, 0.0f };
                    float x[3] = { pos[0], pos[1], pos[2] }, n[3] = { h.n[0], h.n[1], h.n[2] };
                    unsigned base = 256u + 16u * (unsigned)j;
                    for (int k = 1; ; k++, base += 128u) {
                        const float s = copysignf(1.0f, n[2]), q = -1.0f / (s + n[2]), w = (n[0] * n[1]) * q;
                        const float T[3] = { 1.0f + ((s * n[0]) * n[0]) * q, s * w, -(s * n[0]) };
                        const float B[3] = { w, s + (n[1] * n[1]) * q, -n[1] };
                        const float t_lo = 0x1p-10f * fmaxf(1.0f, fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fabsf(x[2])));
                        for (int c = 0; c < 3; c++) r.o[c] = x[c];
                        trace_direction(a, p, base, n, T, B, r.d);
                        trace_aim(r);
                        SceneHit h2;
                        scene_primitives_beyond(a, r.o, r.d, t_lo, h2);
                        int best2 = -1;
                        float bt2 = h2.t_best, bbx2 = 0.0f, bby2 = 0.0f;
                        scene_nearest(b, r, stk, t_lo, bt2, best2, bbx2, bby2);
                        scene_surface(a, r.o, r.d, h2, best2, bt2, bbx2, bby2, x);
                        if (h2.gid < 0) break;                  // a miss
                        float L = h2.emit;                      // per unit of albedo
                        const bool emitter = h2.emit > 0.0f;
                        if (!emitter) {
                            bool occluded = false;
                            if (arg.shadow_secondary) {
                                for (int c = 0; c < 3; c++) r.o[c] = x[c];
                                occluded = scene_shadow_sample(b, arg.edge_u, arg.edge_v, r, x, stk, p, base + 8, base + 9);
                            }
                            L = arg.ambient + (occluded ? 0.0f : 1.0f) * scene_direct(a, h2.n, x);
                        }
                        for (int c = 0; c < 3; c++) acc[c] = acc[c] + thr[c] * (h2.alb[c] * L);
                        if (emitter || k >= args.max_depth) break;
                        for (int c = 0; c < 3; c++) { thr[c] = thr[c] * h2.alb[c]; n[c] = h2.n[c]; }
                        if (args.rr_depth > 0 && k >= args.rr_depth) {
                            const float rq = fminf(fmaxf(fmaxf(thr[0], thr[1]), thr[2]), 1.0f);
                            if (!(rq > 0.0f && scene_hash(a.seed, a.frame, (unsigned)p, base + 10) < rq)) break;
                            for (int c = 0; c < 3; c++) thr[c] = thr[c] / rq;
                        }
                    }
                    for (int c = 0; c < 3; c++) ind[c] = ind[c] + acc[c];
                }
                for (int c = 0; c < 3; c++) { ind_term[c] = ind[c] / (float)paths; shade[c] = first + ind_term[c]; }
                bounced = true;
            }
        }
        if constexpr (SPLIT) trace_store_split(args.s, p, h, pos, first_term, ind_term, bounced, shade);
        else scene_store(a, p, h, pos, shade[0], shade[1], shade[2]);
    }
}

}  // namespace

extern "C" int svgf_path_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_path_draw(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                              const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp, void *stream)
{
    ScenePathArgs t;
    int device = 0;
    const int rc = path_prepare(t.t, device, scene, out_rgb_dev, true, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc != SVGF_OK) return rc;
    if (!path_params_ok(pp)) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    t.t.bounce_samples = pp->paths; t.max_depth = pp->max_depth; t.rr_depth = pp->rr_depth;
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_path<ScenePathArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_path_draw_split(const svgf_scene *scene, void *out_direct_dev, void *out_indirect_dev, void *out_rgb_dev, void *out_gbuffer_dev,
                                    const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                                    const SvgfSceneLight *light, const SvgfPathParams *pp, void *stream)
{
    ScenePathSplitArgs s;
    int device = 0;
    const int rc = path_prepare(s.s.t, device, scene, out_rgb_dev, false, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc != SVGF_OK) return rc;
    if (!out_direct_dev || !out_indirect_dev || out_direct_dev == out_indirect_dev) return SVGF_ERR_INVALID_ARG;
    if (!path_params_ok(pp)) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    s.s.out_direct = static_cast<float *>(out_direct_dev); s.s.out_indirect = static_cast<float *>(out_indirect_dev);
    s.s.t.bounce_samples = pp->paths; s.max_depth = pp->max_depth; s.rr_depth = pp->rr_depth;
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_path<ScenePathSplitArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), s);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
