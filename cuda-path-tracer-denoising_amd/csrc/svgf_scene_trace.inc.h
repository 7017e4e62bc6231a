// svgf_scene_trace.inc.h — the path-traced draw's kernel and its host-side preparation, shared as TEXT by the two companion libraries:
// libsvgf_trace.so (svgf_scene_trace.hip: svgf_trace_draw, row f17) instantiates k_scene_trace<SceneTraceArgs>, libsvgf_split.so
// (svgf_scene_split.hip: svgf_trace_draw_split, row f18) instantiates k_scene_trace<SceneSplitArgs> - every ray the same statements,
// and a tail that writes the direct and the indirect term apart and without the albedo (trace_store_split).
// Include inside an anonymous namespace, after svgf_kernels.h, svgf_trace.h, hip_runtime.h, <cmath>, <cstdint> and <type_traits>.
//
// k_scene_trace: one thread per pixel, 256 per block, the walks on the per-lane LDS stack stack[level][lane] (48 x 256 x 4 B; empty
// between rays, so the four kinds of ray of a pixel - primary, shadow, bounce, the bounce's shadow - take turns on it).  The shadow
// samples and the bounce samples are runtime loops: one copy of each inlined walk in the code object whatever the counts.  No
// runtime-indexed private array, no scratch, no spinning, no traffic between workgroups.  The rays behind the first hit of a wave
// diverge - neighbouring pixels draw independent directions - and nothing here hides that: tools/traced_scene_time.py measures it.

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

// svgf_trace_draw_split's: the two demodulated images beside the frame's own targets (b.s.out_rgb may be null there)
struct SceneSplitArgs {
    SceneTraceArgs t;
    float *out_direct, *out_indirect;
};

__device__ __forceinline__ const SceneTraceArgs &trace_args(const SceneTraceArgs &a) { return a; }
__device__ __forceinline__ const SceneTraceArgs &trace_args(const SceneSplitArgs &a) { return a.t; }

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

// The tail of the split draw (row f18), in scene_store's place: the pixel's noise multiplier and chroma are scene_store's statements,
// here applied to each term WITHOUT the albedo - D from `first` (the emittance on an emitter), I from ind where the pixel bounced -
// then scene_store's colour, where the caller asked for it, and scene_store's G-buffer stores.  svgf_scene_pixel.inc.h, which the
// product library compiles, stays as it is; a change to scene_store's tail has to be made here as well (tests/test_split_scene.py
// holds the colour and the G-buffer of this draw to svgf_trace_draw's on bits).
// `first` is per channel: one value three times in every draw but row f23's, whose first term carries a coloured highlight.
__device__ __forceinline__ void trace_store_split3(const SceneSplitArgs &s, int p, const SceneHit &h, const float pos[3], const float first[3],
                                                   const float ind[3], bool bounced, const float shade[3])
{
#pragma clang fp contract(off)
    const SceneArgs &a = s.t.b.s;
    const float *n = h.n, *alb = h.alb;
    const int gid = h.gid;
    const bool miss = gid < 0;

    const unsigned up = (unsigned)p;
    const float u = scene_hash(a.seed, a.frame, up, 0), v = scene_hash(a.seed, a.frame, up, 1);
    float mult = 1.0f + a.noise * (2.0f * u - 1.0f);
    if (v < a.fireflies) mult = mult * 6.0f;
    float *o_d = s.out_direct + 3 * (size_t)p, *o_i = s.out_indirect + 3 * (size_t)p;
    float col[3];
    for (int c = 0; c < 3; c++) {
        const float chroma = 1.0f + a.chroma_amp * (scene_hash(a.seed, a.frame, up, 2 + c) - 0.5f);
        col[c] = miss ? 0.0f : ((alb[c] * shade[c]) * mult) * chroma;
        o_d[c] = miss ? 0.0f : (first[c] * mult) * chroma;
        o_i[c] = bounced ? (ind[c] * mult) * chroma : 0.0f;
    }
    if (a.out_rgb) {
        float *o_rgb = a.out_rgb + 3 * (size_t)p;
        o_rgb[0] = col[0]; o_rgb[1] = col[1]; o_rgb[2] = col[2];
    }
    if (!a.out_gbuf) {
        a.pl_nrm[3 * (size_t)p] = n[0]; a.pl_nrm[3 * (size_t)p + 1] = n[1]; a.pl_nrm[3 * (size_t)p + 2] = n[2];
        a.pl_pos[3 * (size_t)p] = pos[0]; a.pl_pos[3 * (size_t)p + 1] = pos[1]; a.pl_pos[3 * (size_t)p + 2] = pos[2];
        if (a.pl_alb) { a.pl_alb[3 * (size_t)p] = alb[0]; a.pl_alb[3 * (size_t)p + 1] = alb[1]; a.pl_alb[3 * (size_t)p + 2] = alb[2]; }
        a.pl_gid[p] = gid;
        return;
    }
    float *g = a.out_gbuf + 13 * (size_t)p;
    g[0] = n[0]; g[1] = n[1]; g[2] = n[2];
    g[3] = pos[0]; g[4] = pos[1]; g[5] = pos[2];
    g[6] = alb[0]; g[7] = alb[1]; g[8] = alb[2];
    g[9] = 1.0f; g[10] = 1.0f; g[11] = 1.0f;
    reinterpret_cast<int *>(g)[12] = gid;
}

__device__ __forceinline__ void trace_store_split(const SceneSplitArgs &s, int p, const SceneHit &h, const float pos[3], float first, const float ind[3],
                                                  bool bounced, const float shade[3])
{
    const float first3[3] = { first, first, first };
    trace_store_split3(s, p, h, pos, first3, ind, bounced, shade);
}

// Args = SceneTraceArgs: svgf_trace_draw.  Args = SceneSplitArgs: svgf_trace_draw_split, the same rays with the tail above.
template <class Args>
__global__ __launch_bounds__(256) void k_scene_trace(Args args)
{
#pragma clang fp contract(off)
    constexpr bool SPLIT = std::is_same<Args, SceneSplitArgs>::value;
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneTraceArgs &arg = trace_args(args);
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
        float first_term = h.emit, ind_term[3] = { 0.0f, 0.0f, 0.0f };        // the split draw's two terms (unused otherwise)
        bool bounced = false;
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
            first_term = first;
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
                for (int c = 0; c < 3; c++) { ind_term[c] = ind[c] / (float)arg.bounce_samples; shade[c] = first + ind_term[c]; }
                bounced = true;
            }
        }
        if constexpr (SPLIT) trace_store_split(args, p, h, pos, first_term, ind_term, bounced, shade);
        else scene_store(a, p, h, pos, shade[0], shade[1], shade[2]);
    }
}

// svgf_trace_draw's refusals and its kernel arguments, for both draws (out_rgb_dev may be null where `rgb_required` is not set)
static inline int trace_prepare(SceneTraceArgs &t, int &device, const svgf_scene *scene, void *out_rgb_dev, bool rgb_required, void *out_gbuffer_dev,
                         const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                         const SvgfSceneLight *light, const SvgfTraceParams *tp)
{
    // svgf_scene_draw_shadowed's refusals, in its order, then this call's own
    if (!light || light->samples < 1 || light->samples > SVGF_SCENE_MAX_SHADOW_SAMPLES) return SVGF_ERR_INVALID_ARG;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(light->centre[c]) || !std::isfinite(light->edge_u[c]) || !std::isfinite(light->edge_v[c])) return SVGF_ERR_INVALID_ARG;
    if ((out_gbuffer_dev != nullptr) == (planes != nullptr)) return SVGF_ERR_INVALID_ARG;
    if (!scene || (rgb_required && !out_rgb_dev) || !cam || !sp || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if (!out_gbuffer_dev && (!planes->normal || !planes->position || !planes->geom_id)) return SVGF_ERR_INVALID_ARG;
    if (!tp || tp->bounce_samples < 0 || tp->bounce_samples > SVGF_TRACE_MAX_BOUNCE_SAMPLES) return SVGF_ERR_INVALID_ARG;
    if (!std::isfinite(tp->ambient) || tp->ambient < 0.0f || (tp->shadow_secondary != 0 && tp->shadow_secondary != 1)) return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfSceneView v;
    const int rc = svgf_scene_view(scene, &v);
    if (rc != SVGF_OK) return rc;
    if (v.depth > SVGF_SCENE_MAX_DEPTH) return SVGF_ERR_UNSUPPORTED;        // the kernel's stack; svgf_scene_create never goes there
    device = v.device;
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
    return SVGF_OK;
}

// The path family's (svgf_path_draw and the draws of svgf_scene_gloss.inc.h): trace_prepare's refusals with pp in tp's place (paths is
// checked behind them, so a bounce count it would accept goes in), then the path parameters'.  Compiled where the includer knows svgf_path.h.
#ifdef SVGF_PATH_H_
static inline int path_prepare(SceneTraceArgs &t, int &device, const svgf_scene *scene, void *out_rgb_dev, bool rgb_required, void *out_gbuffer_dev,
                               const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                               const SvgfSceneLight *light, const SvgfPathParams *pp)
{
    SvgfTraceParams tp = { 0, 0.0f, 0 };
    if (pp) { tp.ambient = pp->ambient; tp.shadow_secondary = pp->shadow_secondary; }
    return trace_prepare(t, device, scene, out_rgb_dev, rgb_required, out_gbuffer_dev, planes, width, height, cam, sp, light, pp ? &tp : nullptr);
}

static inline bool path_params_ok(const SvgfPathParams *pp)
{
    return pp->paths >= 0 && pp->paths <= SVGF_PATH_MAX_PATHS && pp->max_depth >= 1 && pp->max_depth <= SVGF_PATH_MAX_DEPTH &&
           pp->rr_depth >= 0 && pp->rr_depth <= SVGF_PATH_MAX_DEPTH;
}
#endif
