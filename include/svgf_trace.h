/* svgf_trace.h — C ABI of libsvgf_trace.so, the companion library of row f17: a path-traced draw of the resident scene.
 *
 * libsvgf_hip.so is the denoiser drop-in and stays small; what a renderer does BEHIND the first hit is renderer-side code and lives
 * here, beside it.  The library is built from the same tree, links against libsvgf_hip.so, and reaches a scene through
 * svgf_scene_view (svgf.h) and nothing else: it compiles the product's own per-pixel text (svgf_scene_pixel.inc.h) and BVH walks
 * (svgf_scene_walk.inc.h), so a ray means here what it means there.  It reads no environment variable.
 *
 * svgf_trace_draw draws svgf_scene_draw_shadowed's frame and, per pixel, gathers indirect light over `bounce_samples` cosine-weighted
 * directions: ONE diffuse bounce, each with the nearest hit through the BVH and, optionally, one shadow ray from there.  This is the
 * input SVGF, the f6 history clamp, the f8 firefly filter and the f9 output pass were written for: heavy-tailed, correlated with the
 * geometry, coloured by the surfaces the bounce meets, with fireflies where a bounce finds a small emitter.
 * One launch on `stream`, no allocation, no upload, no host wait, legal under stream capture (one kernel node); on a static scene
 * and on a posed one (row f15), where it reads the posed arrays exactly as svgf_scene_draw does.
 * Exactly one of out_gbuffer_dev (AoS texels) and planes (svgf_planar_gbuffer's layout) is non-NULL.
 * Errors, all before any device work: everything svgf_scene_draw_shadowed refuses (SVGF_ERR_INVALID_ARG for a NULL scene, output,
 *   camera, synth parameters or light, a size <= 0, samples outside 1..SVGF_SCENE_MAX_SHADOW_SAMPLES, a light field that is not
 *   finite, both targets or neither, planes without normal / position / geom_id; SVGF_ERR_UNSUPPORTED for width * height >= 2^31 / 16),
 *   and SVGF_ERR_INVALID_ARG for a NULL tp, bounce_samples outside 0..SVGF_TRACE_MAX_BOUNCE_SAMPLES, an ambient that is not finite
 *   or is negative, a shadow_secondary other than 0 or 1.
 *
 * Normative semantics - float32, one rounding per operation, no contraction, sqrtf and division only (no transcendental);
 * hash(k) = svgf_synth_render's hash(seed, frame, p, k) of pixel p = y * width + x:
 *   G-buffer: every field (AoS or planes) is what svgf_scene_draw writes with light = centre, bit for bit.
 *   vis and the direct term are svgf_scene_draw_shadowed's, unchanged: streams 8 + 2s and 9 + 2s, its occluder rule;
 *     direct = (30.0f * lam) / (4.0f + dist2), lam and dist2 from `centre` exactly as svgf_scene_draw forms them.
 *   A miss (geomId < 0) and an emissive hit (emittance > 0) cast no bounce and keep svgf_scene_draw_shadowed's colour.
 *   Every other pixel, n and pos its G-buffer normal and position, bounce sample j = 0 .. bounce_samples - 1, base = 256 + 16 j:
 *     Disc point by bounded rejection: for k = 0..3, a_k = 2 hash(base + 2k) - 1, b_k = 2 hash(base + 2k + 1) - 1; (a, b) is the
 *       first pair with a_k a_k + b_k b_k < 1, and (0, 0) if none of the four passes (probability (1 - pi/4)^4 = 0.0021: the normal
 *       itself, a bias of that size towards it).
 *     Frame without branches (Duff et al. 2017): s = copysignf(1, n.z), q = -1 / (s + n.z), w = (n.x n.y) q,
 *       T = (1 + ((s n.x) n.x) q,  s w,  -(s n.x)),   B = (w,  s + (n.y n.y) q,  -n.y).
 *     Direction: c = sqrtf(fmaxf(0, 1 - (a a + b b))), d_i = (a T_i + b B_i) + c n_i, then d = d / sqrtf((d0 d0 + d1 d1) + d2 d2)
 *       (Malley's method: cosine-weighted, so the pdf and the Lambert factor cancel and a sample's weight is 1).
 *     Nearest hit on the ray (pos, d) with t > t_lo, t_lo = 2^-10 * fmaxf(1, fmaxf(fmaxf(|pos.x|, |pos.y|), |pos.z|)): the primary
 *       ray's rule with t_lo in place of its lower bounds (1e-4 for a primitive's tw, 0 for a triangle's t) - primitives in order
 *       with tw < t_best; a triangle that counts (row f14's gate: S(padded box i) passes and t >= tn_i) replaces the hit when
 *       t < t_best, the lower index at equal t.  A node is skipped iff S(node) fails or tn_node > t_best, so every tree gives the same
 *       hit.  Position pos2, normal n2, albedo alb2 (texture included) and emittance emit2 at the hit are formed as for a primary hit.
 *     Radiance L_j: a miss gives 0; an emitter alb2_c * emit2; any other surface
 *       L_j,c = alb2_c * (ambient + vis2 * ((30.0f * lam2) / (4.0f + dist2_2)))     lam2, dist2_2 from pos2, n2 towards `centre`,
 *       where vis2 = 1 with shadow_secondary == 0, and otherwise 0 or 1 from ONE shadow ray of svgf_scene_draw_shadowed's rule cast
 *       from pos2, its light point from streams base + 8 and base + 9.
 *   Sum: ind_c = ((((0 + L_0,c) + L_1,c) + ...) + L_(bounce_samples-1),c) / (float)bounce_samples.
 *   Colour: shade_c = (ambient + vis * direct) + ind_c   (with bounce_samples == 0 the last addition is absent), then
 *     col_c = ((alb_c * shade_c) * mult) * chroma_c; the noise multiplier, fireflies, chroma and the stores are svgf_scene_draw's.
 *   With bounce_samples = 0 and ambient = 0.15f the frame is svgf_scene_draw_shadowed's on every bit.
 *   A NaN normal (a mesh without normals) has no special case: the direction is NaN, every comparison on the ray fails, the bounce
 *     misses and L_j = 0.
 * INTEGRATION.md 5k has the frame loop and the two-library link line, examples/traced_scene.cpp runs it. */
#ifndef SVGF_TRACE_H_
#define SVGF_TRACE_H_

#include "svgf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SvgfTraceParams {
    int   bounce_samples;      /* directions gathered per pixel and frame, 0..SVGF_TRACE_MAX_BOUNCE_SAMPLES */
    float ambient;             /* the constant term, at the first hit and at the bounce's; svgf_scene_draw's is 0.15f */
    int   shadow_secondary;    /* 1: one shadow ray from the bounce's hit; 0: the light reaches it unoccluded */
} SvgfTraceParams;
#define SVGF_TRACE_MAX_BOUNCE_SAMPLES 8

int svgf_trace_draw(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev /* or NULL */,
                    const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height, const SvgfCamera *cam,
                    const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfTraceParams *tp, void *stream);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against: a loader compares it with
 * svgf_version() of the libsvgf_hip.so it found and refuses a mismatch. */
int svgf_trace_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_TRACE_H_ */
