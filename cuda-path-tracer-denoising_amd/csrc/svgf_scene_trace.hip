// svgf_scene_trace.hip — libsvgf_trace.so, the companion library of row f17: svgf_trace_draw, the resident scene path-traced with one
// diffuse bounce.  include/svgf_trace.h states the semantics.  Renderer-side code: it is NOT part of libsvgf_hip.so, links against
// it, and reaches a scene through svgf_scene_view alone (struct svgf_scene is unknown here).  The arithmetic is the product's own
// text: svgf_scene_pixel.inc.h (ray, primitive and triangle tests, surface, the light's term, noise and stores) and
// svgf_scene_walk.inc.h (the closest-hit and the any-hit walk), so a ray here and a ray of k_scene_bvh are the same operations.
//
// k_scene_trace: one thread per pixel, 256 per block, the walks on the per-lane LDS stack stack[level][lane] (48 x 256 x 4 B; empty
// between rays, so the four kinds of ray of a pixel - primary, shadow, bounce, the bounce's shadow - take turns on it).  The shadow
// samples and the bounce samples are runtime loops: one copy of each inlined walk in the code object whatever the counts.  No
// runtime-indexed private array, no scratch, no spinning, no traffic between workgroups.  The rays behind the first hit of a wave
// diverge - neighbouring pixels draw independent directions - and nothing here hides that: tools/traced_scene_time.py measures it.
#include "svgf_kernels.h"
#include "../../include/svgf_trace.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace {

#include "svgf_scene_pixel.inc.h"

#include "svgf_scene_walk.inc.h"

struct SceneTraceArgs {
    SceneBvhArgs b;
    float edge_u[3], edge_v[3];
    int samples;                // shadow rays of the first hit
    int bounce_samples;
    float ambient;
    int shadow_secondary;
};

__device__ __forceinline__ void trace_aim(SceneRay &r)
{
#pragma clang fp contract(off)
    for (int c = 0; c < 3; c++) { r.flat[c] = fabsf(r.d[c]) < 0x1p-100f; r.inv[c] = 1.0f / r.d[c]; }
}

// the direction of bounce sample j of pixel p around n: a disc point by bounded rejection, lifted onto the hemisphere in the
// branch-free frame (T, B, n)
__device__ __forceinline__ void trace_direction(const SceneArgs &a, int p, unsigned base, const float n[3], const float T[3], const float B[3], float d[3])
{
#pragma clang fp contract(off)
    float da = 0.0f, db = 0.0f;
    bool found = false;
#pragma unroll
    for (unsigned k = 0; k < 4; k++) {
        const float ak = 2.0f * scene_hash(a.seed, a.frame, (unsigned)p, base + 2 * k) - 1.0f;
        const float bk = 2.0f * scene_hash(a.seed, a.frame, (unsigned)p, base + 2 * k + 1) - 1.0f;
        const bool take = !found && (ak * ak + bk * bk < 1.0f);
        da = take ? ak : da; db = take ? bk : db;
        found = found || take;
    }
    const float cz = sqrtf(fmaxf(0.0f, 1.0f - (da * da + db * db)));
    for (int c = 0; c < 3; c++) d[c] = (da * T[c] + db * B[c]) + cz * n[c];
    normalise3(d);
}

__global__ __launch_bounds__(256) void k_scene_trace(SceneTraceArgs arg)
{
#pragma clang fp contract(off)
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneBvhArgs &b = arg.b;
    const SceneArgs &a = b.s;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < a.W * a.H) {
        int *const stk = stack + threadIdx.x;
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
        if (!(h.emit > 0.0f)) {
            const bool casts = h.gid >= 0;          // a miss casts no ray (and its colour is 0 whatever the shade)
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
            if (casts && arg.bounce_samples > 0) {
                const float *n = h.n;
                const float s = copysignf(1.0f, n[2]), q = -1.0f / (s + n[2]), w = (n[0] * n[1]) * q;
                const float T[3] = { 1.0f + ((s * n[0]) * n[0]) * q, s * w, -(s * n[0]) };
                const float B[3] = { w, s + (n[1] * n[1]) * q, -n[1] };
                const float t_lo = 0x1p-10f * fmaxf(1.0f, fmaxf(fmaxf(fabsf(pos[0]), fabsf(pos[1])), fabsf(pos[2])));
                float ind[3] = { 0.0f, 0.0f, 0.0f };
                for (int j = 0; j < arg.bounce_samples; j++) {
                    const unsigned base = 256u + 16u * (unsigned)j;
                    for (int c = 0; c < 3; c++) r.o[c] = pos[c];
                    trace_direction(a, p, base, n, T, B, r.d);
                    trace_aim(r);
                    SceneHit h2;
                    scene_primitives_beyond(a, r.o, r.d, t_lo, h2);
                    int best2 = -1;
                    float bt2 = h2.t_best, bbx2 = 0.0f, bby2 = 0.0f;
                    scene_nearest(b, r, stk, t_lo, bt2, best2, bbx2, bby2);
                    float pos2[3];
                    scene_surface(a, r.o, r.d, h2, best2, bt2, bbx2, bby2, pos2);
                    float L = 0.0f;             // per unit of albedo
                    if (h2.gid >= 0) {
                        if (h2.emit > 0.0f) {
                            L = h2.emit;
                        } else {
                            bool occluded = false;
                            if (arg.shadow_secondary) {
                                for (int c = 0; c < 3; c++) r.o[c] = pos2[c];
                                occluded = scene_shadow_sample(b, arg.edge_u, arg.edge_v, r, pos2, stk, p, base + 8, base + 9);
                            }
                            L = arg.ambient + (occluded ? 0.0f : 1.0f) * scene_direct(a, h2.n, pos2);
                        }
                    }
                    for (int c = 0; c < 3; c++) ind[c] = ind[c] + (h2.gid >= 0 ? h2.alb[c] * L : 0.0f);
                }
                for (int c = 0; c < 3; c++) shade[c] = first + ind[c] / (float)arg.bounce_samples;
            }
        }
        scene_store(a, p, h, pos, shade[0], shade[1], shade[2]);
    }
}

}  // namespace

extern "C" int svgf_trace_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_trace_draw(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                               const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfTraceParams *tp, void *stream)
{
    // svgf_scene_draw_shadowed's refusals, in its order, then this call's own
    if (!light || light->samples < 1 || light->samples > SVGF_SCENE_MAX_SHADOW_SAMPLES) return SVGF_ERR_INVALID_ARG;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(light->centre[c]) || !std::isfinite(light->edge_u[c]) || !std::isfinite(light->edge_v[c])) return SVGF_ERR_INVALID_ARG;
    if ((out_gbuffer_dev != nullptr) == (planes != nullptr)) return SVGF_ERR_INVALID_ARG;
    if (!scene || !out_rgb_dev || !cam || !sp || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if (!out_gbuffer_dev && (!planes->normal || !planes->position || !planes->geom_id)) return SVGF_ERR_INVALID_ARG;
    if (!tp || tp->bounce_samples < 0 || tp->bounce_samples > SVGF_TRACE_MAX_BOUNCE_SAMPLES) return SVGF_ERR_INVALID_ARG;
    if (!std::isfinite(tp->ambient) || tp->ambient < 0.0f || (tp->shadow_secondary != 0 && tp->shadow_secondary != 1)) return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfSceneView v;
    const int rc = svgf_scene_view(scene, &v);
    if (rc != SVGF_OK) return rc;
    if (v.depth > SVGF_SCENE_MAX_DEPTH) return SVGF_ERR_UNSUPPORTED;        // the kernel's stack; svgf_scene_create never goes there
    SvgfDeviceGuard dev_guard(v.device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    SceneTraceArgs t;
    SceneArgs &a = t.b.s;
    a.n_geoms = v.n_geoms; a.geoms = v.geoms; a.geom_ids = v.geom_ids;
    a.n_tris = v.n_tris; a.tris = v.tris; a.tri_ids = v.tri_ids; a.tri_albedo = v.tri_albedo;
    a.tri_tex = v.tri_tex; a.tex_desc = v.tex_desc; a.tex = v.tex;
    t.b.nodes = reinterpret_cast<const float4 *>(v.nodes); t.b.order = v.order; t.b.tri_boxes = reinterpret_cast<const float4 *>(v.tri_boxes);
    scene_frame_args(a, width, height, cam, sp, light->centre);
    a.out_rgb = static_cast<float *>(out_rgb_dev);
    a.out_gbuf = static_cast<float *>(out_gbuffer_dev);
    a.pl_nrm = planes ? planes->normal : nullptr; a.pl_pos = planes ? planes->position : nullptr;
    a.pl_alb = planes ? planes->albedo : nullptr; a.pl_gid = planes ? planes->geom_id : nullptr;
    for (int c = 0; c < 3; c++) { t.edge_u[c] = light->edge_u[c]; t.edge_v[c] = light->edge_v[c]; }
    t.samples = light->samples;
    t.bounce_samples = tp->bounce_samples; t.ambient = tp->ambient; t.shadow_secondary = tp->shadow_secondary;
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_trace, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
