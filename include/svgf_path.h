/* svgf_path.h — C ABI of libsvgf_path.so, the companion library of row f19: the resident scene traced along PATHS of up to
 * SVGF_PATH_MAX_DEPTH diffuse bounces, with next-event estimation at every vertex and Russian roulette.
 *
 * A third companion beside libsvgf_trace.so (svgf_trace.h: one bounce) and libsvgf_split.so (svgf_split.h: that bounce as two
 * images), whose functions and whose ABI stay what they were: built from the same tree, linked against libsvgf_hip.so, reaching a
 * scene through svgf_scene_view alone, reading no environment variable.  Its kernel compiles the shared texts
 * csrc/svgf_scene_pixel.inc.h, svgf_scene_walk.inc.h and svgf_scene_trace.inc.h, so a ray, a sampled direction and a stored pixel
 * mean here what they mean there.
 *
 * svgf_path_draw is svgf_trace_draw with the constant behind the second hit replaced by what a path finds there;
 * svgf_path_draw_split is svgf_trace_draw_split in the same sense (arguments in that call's order: out_direct_dev and
 * out_indirect_dev both required and distinct, out_rgb_dev optional).  Either is ONE launch on `stream`, no allocation, no upload,
 * no host wait, legal under stream capture (one kernel node); on a static scene and on a posed one.  Exactly one of out_gbuffer_dev
 * and planes is non-NULL.
 * Errors, all before any device work: everything svgf_trace_draw (for the split form: svgf_trace_draw_split) refuses, in its order,
 *   with pp in tp's place - a NULL pp, an ambient that is not finite or is negative, a shadow_secondary other than 0 or 1 - then
 *   SVGF_ERR_INVALID_ARG for paths outside 0..SVGF_PATH_MAX_PATHS, max_depth outside 1..SVGF_PATH_MAX_DEPTH, rr_depth outside
 *   0..SVGF_PATH_MAX_DEPTH.
 *
 * Normative semantics - float32, one rounding per operation, no contraction, sqrtf and division only (no transcendental);
 * hash(k) = svgf_synth_render's hash(seed, frame, p, k) of pixel p = y * width + x:
 *   The G-buffer, vis, the first hit's term first = ambient + vis * direct, which pixels cast (neither a miss nor an emitter), the
 *     noise multiplier, fireflies, chroma and the stores are svgf_trace_draw's; for the split form D (from first), I (from ind), the
 *     colour and the G-buffer are svgf_trace_draw_split's, with paths in bounce_samples' place.
 *   A casting pixel, pos and n its G-buffer position and normal, path j = 0 .. paths - 1:
 *     thr = (1, 1, 1), acc = (0, 0, 0), x_0 = pos, n_0 = n.
 *     Bounce k = 1 .. max_depth, base = 256 + 128 (k - 1) + 16 j (bounce 1 reads svgf_trace_draw's streams; the highest stream any
 *     path reads is 256 + 128 * 7 + 16 * 7 + 10 = 1274):
 *       Direction: svgf_trace_draw's sampler - disc point by bounded rejection from streams base + 0..7, Duff's frame of n_(k-1)
 *         formed anew from n_(k-1), lifted and normalised.
 *       Nearest hit: svgf_trace_draw's rule on the ray (x_(k-1), d) with t > t_lo, t_lo = 2^-10 * fmaxf(1, max |x_(k-1)|); its
 *         position x_k, normal n_k, albedo alb_k (texture included) and emittance emit_k formed as for a primary hit.
 *       A miss ends the path.
 *       An emitter (emit_k > 0):  acc_c = acc_c + thr_c * (alb_k,c * emit_k), and the path ends.
 *       Any other surface:        acc_c = acc_c + thr_c * (alb_k,c * L_k),  L_k = ambient + vis_k * ((30.0f * lam_k) / (4.0f + dist2_k)),
 *         lam_k and dist2_k from x_k and n_k towards `centre`; vis_k = 1 with shadow_secondary == 0, otherwise 0 or 1 from ONE
 *         shadow ray of svgf_scene_draw_shadowed's rule cast from x_k, its light point from streams base + 8 and base + 9.
 *       The path ends after bounce max_depth.  Otherwise thr_c = thr_c * alb_k,c, and then, if rr_depth > 0 and k >= rr_depth:
 *         q = fminf(fmaxf(fmaxf(thr_0, thr_1), thr_2), 1.0f); the path ends unless q > 0 and hash(base + 10) < q; a path that
 *         survives continues with thr_c = thr_c / q.
 *     A NaN normal has no special case: the direction is NaN, every comparison on the ray fails, nothing is hit, the path ends.
 *   Sum: ind_c = ((((0 + acc_0,c) + acc_1,c) + ...) + acc_(paths-1),c) / (float)paths; shade_c = first + ind_c (with paths == 0 the
 *     last addition is absent, and I = +0).
 *   Two identities follow by construction (0 + 1 * v = v on every float32 v that an albedo times a radiance can be):
 *     with max_depth = 1 (any rr_depth) and paths = bounce_samples the frame is svgf_trace_draw's, and the split form's four outputs
 *     are svgf_trace_draw_split's, on every bit; and the streams do not depend on max_depth, so with rr_depth = 0 a path of depth K is
 *     a prefix of the same path at depth K + 1.
 *   The estimator: a cosine-weighted direction makes a bounce's weight the albedo alone (thr), the roulette continues with
 *     probability q and divides by it, so the expectation does not depend on rr_depth; everything behind bounce max_depth is dropped
 *     (not replaced by `ambient`), which is the bias a finite depth has.
 * INTEGRATION.md 5m has the frame loop and the link line, examples/path_scene.cpp runs it. */
#ifndef SVGF_PATH_H_
#define SVGF_PATH_H_

#include "svgf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SvgfPathParams {
    int   paths;             /* paths per pixel and frame, 0..SVGF_PATH_MAX_PATHS */
    int   max_depth;         /* bounces per path, 1..SVGF_PATH_MAX_DEPTH */
    int   rr_depth;          /* 0: no roulette; k >= 1: roulette after the hit of bounce k and every later one */
    float ambient;           /* the constant term at every vertex, as SvgfTraceParams' */
    int   shadow_secondary;  /* 1: one shadow ray from every vertex behind the first; 0: the light reaches them unoccluded */
} SvgfPathParams;            /* 20 bytes */
#define SVGF_PATH_MAX_PATHS 8
#define SVGF_PATH_MAX_DEPTH 8

int svgf_path_draw(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev /* or NULL */,
                   const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height, const SvgfCamera *cam,
                   const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp, void *stream);
int svgf_path_draw_split(const svgf_scene *scene, void *out_direct_dev, void *out_indirect_dev, void *out_rgb_dev /* or NULL */,
                         void *out_gbuffer_dev /* or NULL */, const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height,
                         const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                         void *stream);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_trace_version. */
int svgf_path_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_PATH_H_ */
