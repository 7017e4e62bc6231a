/* svgf_gloss.h — C ABI of libsvgf_gloss.so, the companion library of row f20: svgf_path_draw's paths (svgf_path.h, row f19) with a
 * MIRROR and a GLASS lobe at every vertex, chosen per object from a table of SvgfSurface records: what the scene format's REFL, REFR,
 * REFRIOR and SPECRGB mean in the reference's scatterRay (src/interactions.h:95-136) and its rt kernel (src/pathtrace.cu:340,358).
 *
 * A fourth companion beside libsvgf_trace.so, libsvgf_split.so and libsvgf_path.so, whose functions and whose ABI stay what they
 * were: built from the same tree, linked against libsvgf_hip.so only, reaching a scene through svgf_scene_view alone, reading no
 * environment variable.  Its kernel compiles the shared texts csrc/svgf_scene_pixel.inc.h, svgf_scene_walk.inc.h and
 * svgf_scene_trace.inc.h unchanged, so a ray, a sampled direction and a stored pixel mean here what they mean there.
 *
 * svgf_gloss_table_create validates on the host before any device work - n in 0..SVGF_SCENE_MAX_POSED, host non-NULL where n > 0,
 *   device >= 0, out non-NULL; every field finite, reflect in [0, 1], refract >= 0, ior > 0, spec >= 0: otherwise
 *   SVGF_ERR_INVALID_ARG and *out = NULL - then allocates and uploads once (SVGF_ERR_NO_DEVICE, SVGF_ERR_OOM, SVGF_ERR_HIP), so it
 *   is not legal under stream capture.  A table belongs to no scene: record g is the surface of object id g (what the G-buffer calls
 *   geomId) of whichever scene it is drawn with.  svgf_gloss_table_size is n (SVGF_ERR_INVALID_ARG for NULL); svgf_gloss_table_destroy
 *   takes NULL.
 * svgf_gloss_draw is svgf_path_draw, svgf_gloss_draw_split is svgf_path_draw_split, each with `table` (or NULL) behind the scene and
 *   SvgfPathParams unchanged.  Either is ONE launch on `stream`, no allocation, no upload, no host wait, legal under stream capture
 *   (one kernel node); on a static scene and on a posed one; AoS texels or planes.
 * Errors, all before any device work: svgf_path_draw's (for the split form svgf_path_draw_split's), in its order; then
 *   SVGF_ERR_INVALID_ARG for a table created on another device than the scene's.
 *
 * Normative semantics - float32, one rounding per operation, no contraction, sqrtf and division only (no powf, no transcendental);
 * hash(k) as in svgf_path.h; a.b = (a_0 * b_0 + a_1 * b_1) + a_2 * b_2; `normalised` = svgf_trace_draw's v / sqrtf(v.v) per channel.
 *   Everything not named here is svgf_path_draw's, bit for bit: the G-buffer, vis, first, which pixels cast, the sampler, the
 *     nearest-hit and shadow rules, t_lo, the roulette, the sum over paths, noise and stores.
 *   Surface: a hit with id g has S = table[g] when 0 <= g < n, otherwise the diffuse surface (all fields 0).  An emitter is handled
 *     before its surface is looked at, as in f19: it adds thr * (alb * emit) and ends the path, whatever sent the path there.
 *   Class of vertex k of path j (k = 0: the first hit), d the direction that arrived there, n the hit's normal as the nearest-hit rule
 *     reports it, u = hash(139 + 128 k + 16 j) (for k >= 1 f19's base + 11, unused there; for k = 0 above the shadow streams 8..135):
 *     GLASS when S.refract > 0 and the hit is a cube or a sphere.  A triangle hit is never glass: meshes are back-face culled, so a ray
 *       inside one has no exit face; a triangle uses its `reflect` only.  Each path carries one bit `inside`, false at the camera,
 *       toggled by every transmission (NOT derived from the sign of d.n: a cube's reported normal is already turned towards the ray,
 *       a sphere's always points outwards).
 *         nn = (d.n > 0) ? -n : n;  eta = inside ? ior : 1 / ior;  c = -(d.nn);  r = (1 - eta) / (1 + eta);  R0 = r * r;  m = 1 - c;
 *         R = R0 + (1 - R0) * (((m * m) * (m * m)) * m);  k2 = 1 - (eta * eta) * (1 - c * c).
 *         If !(k2 >= 0) (total internal reflection) or u < R: the mirror lobe about nn, d' = d - (2 * (d.nn)) * nn normalised, weight
 *         S.spec.  Otherwise a transmission: d' = eta * d + (eta * c - sqrtf(k2)) * nn normalised, weight 1, `inside` toggled.
 *     MIRROR otherwise, when u < S.reflect: d' = d - (2 * (d.n)) * n normalised, weight S.spec.
 *     DIFFUSE otherwise: f19's vertex (weight 1).
 *   A specular (glass or mirror) vertex k >= 1 gathers nothing - no ambient, no shadow ray, acc unchanged; the path ends there if
 *     k == max_depth; otherwise thr_c = thr_c * (alb_k,c * weight_c), then f19's roulette (stream base + 10), then the ray d'.  (A
 *     diffuse vertex is the same statement with weight 1, which is f19's thr_c * alb_k,c on every bit.)
 *   Vertex 0: w_d = glass ? 0 : 1 - S.reflect.  first' = w_d * first; with w_d == 0 no shadow ray is cast at vertex 0, vis is not
 *     formed and first' = +0.  Path j draws its own class: a diffuse draw continues as f19's path; a specular draw starts with
 *     thr = weight and the ray d' from pos (the first hit's albedo is applied by the store, as for every pixel).
 *     shade_c = first' + ind_c; in the split form D comes from first', I from ind; with paths == 0 the frame is first' alone.
 *   Origin of the next ray: a reflected and a diffuse ray start at x_k as in f19.  A TRANSMITTED ray starts at
 *     o_c = x_c + (-(4 * t_lo)) * nn_c, t_lo = 2^-10 * fmaxf(1, max |x_k|) as for every ray, and is then subject to t > t_lo as usual.
 *     Why: for an origin ON a sphere the near root of the primitive test is 0 up to rounding; where it comes out tiny and positive it
 *     is chosen, fails t > t_lo, and the far root - the exit - is never offered; the cube's entering-face test has the same
 *     coin-flip.  Measured in the model on `glass_pair` (a glass sphere and a glass cube of scale 3, ior 1.5, 67x41, 4 paths, depth
 *     4, rr_depth 2; tests/test_gloss_scene.py): with the factor 4 the share of transmissions INTO an object whose next hit is not
 *     that object is 0.00 % (0 of 1083; the cap is 1 %); with the origin left at x_k it is 31.06 % (333 of 1072).
 *   Two identities hold by construction: with table == NULL, n == 0 or a table of all-diffuse records both draws are svgf_path_draw /
 *     svgf_path_draw_split on every bit of every output (w_d = 1 - 0 = 1, 1 * v = v, alb * 1 = alb); and a surface on an object that
 *     no ray reaches changes no bit.
 * Limits: a camera inside glass starts with inside = false and so refracts the wrong way; overlapping glass objects share the one
 *   bit; glass meshes are mirrors at most (see above).  The G-buffer is the first hit's: what a mirror or a pane shows moves
 *   independently of it, which a temporal filter sees as ghosting (examples/gloss_scene.cpp; svgf_virtual.h, row f21, draws a virtual-hit one).
 * INTEGRATION.md 5n has the frame loop and the link line, examples/gloss_scene.cpp runs it. */
#ifndef SVGF_GLOSS_H_
#define SVGF_GLOSS_H_

#include "svgf.h"
#include "svgf_path.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SvgfSurface {      /* 24 bytes, one per object id (what the G-buffer calls geomId) */
    float reflect;                /* REFL: probability of the mirror lobe, 0..1 */
    float refract;                /* REFR: > 0 makes a cube / sphere glass (Fresnel by Schlick) */
    float ior;                    /* REFRIOR, finite, > 0 */
    float spec[3];                /* SPECRGB: weight of a mirror / Fresnel reflection */
} SvgfSurface;
typedef struct svgf_gloss_table svgf_gloss_table;

int  svgf_gloss_table_create(int device, const SvgfSurface *host, int n, svgf_gloss_table **out);
void svgf_gloss_table_destroy(svgf_gloss_table *t);
int  svgf_gloss_table_size(const svgf_gloss_table *t);
int  svgf_gloss_draw(const svgf_scene *scene, const svgf_gloss_table *table /* or NULL */, void *out_rgb_dev,
                     void *out_gbuffer_dev /* or NULL */, const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height,
                     const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                     void *stream);
int  svgf_gloss_draw_split(const svgf_scene *scene, const svgf_gloss_table *table /* or NULL */, void *out_direct_dev,
                           void *out_indirect_dev, void *out_rgb_dev /* or NULL */, void *out_gbuffer_dev /* or NULL */,
                           const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height, const SvgfCamera *cam,
                           const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp, void *stream);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_path_version. */
int  svgf_gloss_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_GLOSS_H_ */
