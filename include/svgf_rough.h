/* svgf_rough.h — C ABI of libsvgf_rough.so, the companion library of row f22: svgf_virtual_draw and svgf_virtual_draw_split
 * (svgf_virtual.h, row f21) with a ROUGH mirror lobe.  Every reflective surface of rows f20 and f21 is a perfect mirror or perfect
 * glass, whose lobe adds no noise of its own.  These draws give an object a GGX roughness alpha: a mirror vertex on it reflects about a
 * normal drawn from the distribution of visible normals, so its one-sample reflection is noisy and is neither the first hit's geometry
 * nor a sharp virtual image - the case the firefly filter, the history clamp and the guide have to be measured on.
 *
 * A sixth companion beside libsvgf_trace.so, libsvgf_split.so, libsvgf_path.so, libsvgf_gloss.so and libsvgf_virtual.so, whose
 * functions and whose ABI stay what they were: built from the same tree, linked against libsvgf_hip.so only, reaching a scene through
 * svgf_scene_view alone, reading no environment variable.  Its kernel is the text libsvgf_gloss.so and libsvgf_virtual.so compile
 * (csrc/svgf_scene_gloss.inc.h).  The surface table is the svgf_gloss_table that svgf_gloss_table_create of libsvgf_gloss.so makes.
 *
 * svgf_rough_table_create uploads n float32 values once: entry g is the GGX roughness alpha of object id g, 0 = smooth.  It belongs to
 *   no scene.  Refusals, all on the host before any device work, in svgf_gloss_table_create's order and with its codes:
 *   SVGF_ERR_INVALID_ARG for out == NULL; for n outside 0..SVGF_SCENE_MAX_POSED, alpha_host == NULL with n > 0 or device < 0; for a
 *   value that is not finite or outside [0, 1]; then SVGF_ERR_NO_DEVICE, SVGF_ERR_OOM, SVGF_ERR_HIP.  *out is NULL after a refusal.
 * svgf_rough_draw is svgf_virtual_draw, svgf_rough_draw_split is svgf_virtual_draw_split: the same arguments in the same order, then
 *   `rough` (or NULL) and `rp`.  Either is ONE launch on `stream`, no allocation, no upload, no host wait, legal under stream capture
 *   (one kernel node); on a static scene and on a posed one; AoS texels or planes.
 * Errors, all before any device work: the corresponding virtual draw's, in its order; then SVGF_ERR_INVALID_ARG for rp == NULL, for a
 *   guide_alpha that is not finite or is negative, and for a roughness table created on another device than the scene's.
 *
 * Normative semantics - float32, one rounding per operation, no contraction, sqrtf and division only, as in svgf_gloss.h.  dot(a, b) is
 *   (a_0 b_0 + a_1 b_1) + a_2 b_2 and normalised(a) is a_c / sqrtf(dot(a, a)) throughout.
 *   Roughness of a hit with object id g: alpha_g = rough[g] where 0 <= g < n, otherwise 0 (and 0 everywhere with rough == NULL).
 *   A vertex is ROUGH when svgf_gloss.h's class draw makes it a MIRROR (u < S.reflect on a vertex that is not glass), alpha_g > 0 and
 *     v_n > 0 below.  Every other vertex is svgf_gloss.h's and svgf_virtual.h's on every bit: glass reflection and transmission stay
 *     smooth, a mirror with alpha_g == 0 or seen from behind stays f20's; the class stream, w_d, first', the roulette, the emitters and
 *     the stores are unchanged.
 *   Direction of a rough vertex with normal n, reached along d, alpha = alpha_g.  (T, B) is the branch-free frame of n that the diffuse
 *     sampler uses (svgf_trace.h); all of the following in this order:
 *       v = -d;  v_t = dot(v, T), v_b = dot(v, B), v_n = dot(v, n)
 *       (t1, t2) = the disc point of the diffuse sampler's bounded rejection on the streams that sampler would have read for the
 *         direction leaving THIS vertex: cb + 117 + 0..7 with cb = 139 + 16 j + 128 v the class stream of vertex v of path j
 *         (svgf_gloss.h), that is svgf_path.h's 256 + 16 j + 128 v + 0..7; (0, 0) if none of the four pairs is inside the disc.  A
 *         rough vertex never runs the diffuse sampler, so no stream is read twice
 *       Vh = normalised(alpha v_t, alpha v_b, v_n)
 *       q = Vh_x Vh_x + Vh_y Vh_y;  T1 = (-Vh_y / sqrtf(q), Vh_x / sqrtf(q), 0) if q > 0, else (1, 0, 0) (the degenerate tangent)
 *       T2 = (-(Vh_z T1_y), Vh_z T1_x, Vh_x T1_y - Vh_y T1_x)
 *       s = 0.5 (1 + Vh_z);  w = 1 - t1 t1;  t2' = (1 - s) sqrtf(w) + s t2;  cz = sqrtf(fmaxf(0, w - t2' t2'))
 *       Nh = ((t1 T1_x + t2' T2_x) + cz Vh_x, (t1 T1_y + t2' T2_y) + cz Vh_y, t2' T2_z + cz Vh_z)
 *       hl = normalised(alpha Nh_x, alpha Nh_y, fmaxf(0, Nh_z));  h_c = (hl_x T_c + hl_y B_c) + hl_z n_c
 *       f = 2 dot(d, h);  d' = normalised(d_c - f h_c)
 *     (Heitz 2018, sampling the GGX distribution of visible normals, isotropic.)
 *   Weight: l_n = dot(d', n).  If not l_n > 0 the path ends at this vertex and adds nothing more (absorbed).  Otherwise
 *     a2 = alpha alpha, G1 = (2 l_n) / (l_n + sqrtf(a2 + (1 - a2) (l_n l_n))) and weight_c = S.spec_c G1, never above spec.
 *   Gathering: a rough vertex is specular for the path: no ambient term, no shadow ray; it ends at max_depth; otherwise
 *     thr *= alb * weight (thr = weight at the first hit), the roulette runs, and the ray d' leaves from the vertex unmoved.
 *   Guide (svgf_virtual.h): a full mirror with 0 < alpha_g <= guide_alpha is followed as if smooth, reflected about n.  A surface with
 *     alpha_g > guide_alpha is not specular for the guide: at the first hit no guide runs (chain = 0, the texel is the first hit's),
 *     deeper in a chain it is the virtual hit.  Colour, D and I depend on neither guide_alpha, max_chain nor id_offset.
 *   Identities by construction: with rough == NULL, n == 0 or an all-zero table both draws are the virtual draws' on every bit of every
 *     output, chain included, for any guide_alpha; roughness on an object no ray reaches, on an object with reflect == 0 or on a glass
 *     object changes no bit.
 * Limits: a rough vertex has no next-event estimation and no multiple importance sampling: a small emitter seen in a rough surface is
 *   noisy and the analytic light leaves no highlight, the rule svgf_gloss.h set for mirrors (svgf_highlight.h, row f23, adds the
 *   light's term in draws of its own; these stay as they are).  Glass is always smooth.  alpha is
 *   isotropic.  The guide's virtual hit under a rough surface is the smooth mirror's: between alpha = 0 and guide_alpha that is an
 *   approximation.
 * INTEGRATION.md 5p has the frame loop and the link line. */
#ifndef SVGF_ROUGH_H_
#define SVGF_ROUGH_H_

#include "svgf.h"
#include "svgf_path.h"
#include "svgf_gloss.h"
#include "svgf_virtual.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svgf_rough_table svgf_rough_table;

typedef struct SvgfRoughParams {
    float guide_alpha;   /* >= 0: the guide follows a full mirror whose roughness is at most this (0: smooth mirrors only) */
} SvgfRoughParams;

int  svgf_rough_table_create(int device, const float *alpha_host, int n, svgf_rough_table **out);
void svgf_rough_table_destroy(svgf_rough_table *t);
/* n, or SVGF_ERR_INVALID_ARG for NULL */
int  svgf_rough_table_size(const svgf_rough_table *t);

int  svgf_rough_draw(const svgf_scene *scene, const svgf_gloss_table *table /* or NULL */, void *out_rgb_dev,
                     void *out_gbuffer_dev /* or NULL */, const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height,
                     const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                     const SvgfVirtualParams *vp, void *out_chain_dev /* int32 per pixel, or NULL */, void *stream,
                     const svgf_rough_table *rough /* or NULL */, const SvgfRoughParams *rp);
int  svgf_rough_draw_split(const svgf_scene *scene, const svgf_gloss_table *table /* or NULL */, void *out_direct_dev,
                           void *out_indirect_dev, void *out_rgb_dev /* or NULL */, void *out_gbuffer_dev /* or NULL */,
                           const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height, const SvgfCamera *cam,
                           const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                           const SvgfVirtualParams *vp, void *out_chain_dev /* int32 per pixel, or NULL */, void *stream,
                           const svgf_rough_table *rough /* or NULL */, const SvgfRoughParams *rp);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_virtual_version. */
int  svgf_rough_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_ROUGH_H_ */
