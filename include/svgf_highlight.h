/* svgf_highlight.h — C ABI of libsvgf_highlight.so, the companion library of row f23: svgf_rough_draw and svgf_rough_draw_split
 * (svgf_rough.h, row f22) with the LIGHT's term at rough vertices.  The draws' light is analytic (SvgfSceneLight: a.light +- edge_u,
 * edge_v), not geometry, so no lobe-sampled ray ever meets it, and row f22's rough vertex gathers nothing: a rough metal floor under
 * the lamp shows the walls and no highlight of the lamp.  These draws evaluate the GGX BRDF towards the light at every ROUGH vertex
 * (next-event estimation).  Emitter geometry is still found by the lobe's ray alone and the analytic light by this term alone: the two
 * sets of lights are disjoint, so the estimator is complete without multiple importance sampling and counts nothing twice.
 *
 * A seventh companion beside libsvgf_trace.so, libsvgf_split.so, libsvgf_path.so, libsvgf_gloss.so, libsvgf_virtual.so and
 * libsvgf_rough.so, whose functions and whose ABI stay what they were: built from the same tree, linked against libsvgf_hip.so only,
 * reaching a scene through svgf_scene_view alone, reading no environment variable.  Its kernel is the text the three before it compile
 * (csrc/svgf_scene_gloss.inc.h).  The surface table is libsvgf_gloss.so's svgf_gloss_table, the roughness table libsvgf_rough.so's
 * svgf_rough_table.
 *
 * svgf_highlight_draw is svgf_rough_draw, svgf_highlight_draw_split is svgf_rough_draw_split: the same arguments in the same order,
 *   then `hp`.  Either is ONE launch on `stream`, no allocation, no upload, no host wait, legal under stream capture (one kernel
 *   node); on a static scene and on a posed one; AoS texels or planes.
 * Errors, all before any device work: the corresponding rough draw's, in its order; then SVGF_ERR_INVALID_ARG for hp == NULL, for an
 *   `enable` outside 0..1 and for a `clamp` that is not finite or is negative.
 *
 * Normative semantics - float32, one rounding per operation, no contraction, sqrtf and division only, as in svgf_rough.h, whose dot(),
 *   normalised() and ROUGH vertex (MIRROR class, alpha_g > 0, v_n > 0, not glass) these are.  Everything about a rough vertex stays
 *   row f22's: its direction d', its lobe weight spec * G1, absorption, the roulette, every stream the path reads.  With enable == 1
 *   such a vertex additionally gathers the light:
 *   The factor H at a point x with normal n, reached along d, roughness alpha, towards the unit direction l - in this order:
 *       l_n = dot(l, n);  H = 0 unless l_n > 0
 *       v = -d;  v_n = dot(v, n);  h = normalised(v_c + l_c);  h_n = dot(h, n)
 *       a2 = alpha alpha;  t = (h_n h_n) (a2 - 1) + 1
 *       tl_c = light_c - x_c (the light's CENTRE, as in the diffuse term);  E = 30 / (4 + dot(tl, tl))
 *       G = (2 l_n) / (l_n + sqrtf(a2 + (1 - a2) (l_n l_n)))
 *       H = ((E (a2 / (t t))) G) / (2 (v_n + sqrtf(a2 + (1 - a2) (v_n v_n))))
 *       H = fminf(H, clamp) where clamp > 0
 *     That is E pi D G1(v) G1(l) / (4 v_n) with the GGX distribution D and the separable Smith term - the BRDF of which row f22's
 *     visible-normal sample with weight spec * G1(l) is the exact importance sampler - in the scene's convention that a Lambert surface
 *     contributes alb * E * lam.  pi cancels and nothing is divided by v_n.
 *   Light points and visibility.  A shadow sample is svgf_trace.h's: the light point from two streams, the unit direction l to it, at
 *     distance dl, occluded or not.  A sample with !(dl > 0) forms no ray and contributes 0.
 *     At a vertex v >= 1 of path j (cb = 139 + 16 j + 128 v) with shadow_secondary: ONE shadow sample on streams cb - 3, cb - 2 -
 *       the pair a diffuse vertex reads there and a specular one leaves unread, so no stream is read twice.  The contribution is
 *       c = H(l) when the sample is not occluded, else 0.
 *     Without shadow_secondary no ray is cast: l = normalised(light_c - x_c), c = H(l) (0 where that l is not a number).
 *     At the first hit: the `samples` shadow samples on streams 8 + 2 s, 9 + 2 s - the very samples the first term uses when
 *       w_d != 0, each cast once per pixel and shared by both terms, and cast for the highlight alone when w_d == 0.
 *       hsum = 0;  for s in order: hsum = hsum + c_s;  hm = hsum / (float)samples.
 *   Where it goes.  At a vertex v >= 1, ahead of the absorption test and the max_depth break:
 *       acc_c = acc_c + thr_c * (alb_c * (spec_c * c))
 *     so a rough vertex gathers the light whether or not its lobe sample is absorbed (the two are independent estimates), and the
 *     last vertex of a path gathers like a diffuse one does.
 *     The first hit is rough for the highlight when it is a hit that is no emitter, its surface is not glass, reflect > 0, alpha > 0
 *     and v_n > 0.  The term is deterministic there, like w_d's: first'_c = first' + (reflect spec_c) hm is svgf_gloss.h's first' in
 *     every place it is used (shade_c = first'_c + ind_c; D_c from first'_c).  In the split form it belongs to D, not to I.  The
 *     path's class draw at the first hit and its throughput are untouched, so the expected highlight of a partial mirror,
 *     reflect spec H, is the same at every depth.
 *   The guide, `chain` and every G-buffer field do not depend on hp.
 *   Identities by construction, on every bit of every output: enable == 0 is the rough draw; rough == NULL, n == 0 or an all-zero table
 *     is the virtual draw for any hp; roughness on glass, on objects with reflect == 0 or on objects no ray reaches changes nothing;
 *     clamp has no effect on a frame in which no H exceeds it.
 * Limits: for small alpha H peaks near E / a2 (and t can round to 0 for alpha below about 2^-12: H is then infinite unless clamped),
 *   and a one-sample highlight of an area light is noisy - `clamp` and the firefly filter of row f8 exist for that; the clamp biases
 *   (darkens) the highlight.  E is taken towards the light's centre also for a sampled light point, the diffuse term's convention.
 *   Glass stays smooth.  An emitter seen in a rough surface is still found by the lobe alone.  A smooth mirror (alpha == 0) has no
 *   highlight: its BRDF is a delta the analytic light's sample never meets.
 * INTEGRATION.md 5q has the frame loop and the link line. */
#ifndef SVGF_HIGHLIGHT_H_
#define SVGF_HIGHLIGHT_H_

#include "svgf.h"
#include "svgf_path.h"
#include "svgf_gloss.h"
#include "svgf_virtual.h"
#include "svgf_rough.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SvgfHighlightParams {
    int   enable;   /* 0: the rough draws on every bit; 1: the light's GGX term at ROUGH vertices */
    float clamp;    /* > 0: the scalar highlight factor H is min(H, clamp); 0: no clamp */
} SvgfHighlightParams;

int  svgf_highlight_draw(const svgf_scene *scene, const svgf_gloss_table *table /* or NULL */, void *out_rgb_dev,
                         void *out_gbuffer_dev /* or NULL */, const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height,
                         const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                         const SvgfVirtualParams *vp, void *out_chain_dev /* int32 per pixel, or NULL */, void *stream,
                         const svgf_rough_table *rough /* or NULL */, const SvgfRoughParams *rp, const SvgfHighlightParams *hp);
int  svgf_highlight_draw_split(const svgf_scene *scene, const svgf_gloss_table *table /* or NULL */, void *out_direct_dev,
                               void *out_indirect_dev, void *out_rgb_dev /* or NULL */, void *out_gbuffer_dev /* or NULL */,
                               const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height, const SvgfCamera *cam,
                               const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                               const SvgfVirtualParams *vp, void *out_chain_dev /* int32 per pixel, or NULL */, void *stream,
                               const svgf_rough_table *rough /* or NULL */, const SvgfRoughParams *rp, const SvgfHighlightParams *hp);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_rough_version. */
int  svgf_highlight_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_HIGHLIGHT_H_ */
