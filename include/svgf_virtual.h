/* svgf_virtual.h — C ABI of libsvgf_virtual.so, the companion library of row f21: svgf_gloss_draw and svgf_gloss_draw_split
 * (svgf_gloss.h, row f20) with a VIRTUAL-HIT G-buffer.  Where the first hit is a full mirror or glass, the colour of the pixel shows
 * something else than that surface, and it moves independently of it.  Everything downstream of the producer - svgf_project_prev, the
 * geomId and normal tests of the history taps, the a-trous edge-stopping terms - assumes that the G-buffer describes what the colour
 * shows.  These draws make it so for purely specular pixels: the texel's normal, position and geomId are those of the first
 * NON-specular surface a deterministic GUIDE chain reaches behind the first hit.
 *
 * A fifth companion beside libsvgf_trace.so, libsvgf_split.so, libsvgf_path.so and libsvgf_gloss.so, whose functions and whose ABI stay
 * what they were: built from the same tree, linked against libsvgf_hip.so only, reaching a scene through svgf_scene_view alone, reading
 * no environment variable.  Its kernel is the text libsvgf_gloss.so compiles (csrc/svgf_scene_gloss.inc.h).  The table is the
 * svgf_gloss_table that svgf_gloss_table_create of libsvgf_gloss.so makes.
 *
 * svgf_virtual_draw is svgf_gloss_draw, svgf_virtual_draw_split is svgf_gloss_draw_split: the same arguments in the same order, then
 *   `vp` and `out_chain_dev` ahead of the stream.  Either is ONE launch on `stream`, no allocation, no upload, no host wait, legal under
 *   stream capture (one kernel node); on a static scene and on a posed one; AoS texels or planes.
 * Errors, all before any device work: the corresponding gloss draw's, in its order; then SVGF_ERR_INVALID_ARG for vp == NULL, max_chain
 *   outside 1..SVGF_PATH_MAX_DEPTH or id_offset outside 0..(1 << 24).
 *
 * Normative semantics - float32, one rounding per operation, no contraction, as in svgf_gloss.h.
 *   Colour, D and I are svgf_gloss_draw's / svgf_gloss_draw_split's on every bit, for every table and every vp: the guide consumes no
 *     hash stream and changes no ray of any path.
 *   G-buffer: albedo and ialbedo (AoS) and the albedo plane (planar) are ALWAYS the first hit's, so svgf_trace_compose works on this
 *     G-buffer unchanged.  normal, position and geomId are the first hit's, on bits, unless the pixel has a virtual hit.
 *   The guide runs on a pixel whose first hit has geomId >= 0, is no emitter, and has the diffuse share w_d == 0 of svgf_gloss.h (glass
 *     on a cube or a sphere, or 1 - reflect == 0).  Every other pixel - partial mirrors, diffuse surfaces, misses, emitters - keeps the
 *     first hit's texel, chain = 0.
 *   The guide chain is deterministic and carries its own bit `inside`, false at the camera.
 *     1. Vertex 0 is the first hit; L = t_0, the distance the nearest-hit rule reports for the primary ray.
 *     2. Vertex v is classified by svgf_gloss.h's rule with u replaced: u = 1 on a glass vertex (it transmits unless total internal
 *        reflection occurs); otherwise u = (reflect >= 1) ? 0 : 1 (a mirror exactly where the surface is a full mirror).
 *     3. A vertex that is not specular is the VIRTUAL HIT; the chain ends.
 *     4. If v == max_chain the guide gives up.
 *     5. Otherwise the ray that leaves vertex v is traced exactly as the path's is: the same t_lo, the same origin moved 4 t_lo behind
 *        a transmitting surface, the same nearest-hit rule beyond t_lo.  A miss: the guide gives up.  Otherwise L = L + t_(v+1); an
 *        emitter is the virtual hit, before its surface is looked at; otherwise go on with vertex v + 1.
 *   A virtual hit writes normal = the hit's normal as the nearest-hit rule reports it; geomId = the hit's id + id_offset;
 *     position_c = o_c + L * d0_c, o the camera's position and d0 the primary direction: the path UNFOLDED along the primary ray.
 *     Why unfolded: for a planar mirror the unfolded position is the mirror image of the seen point, a fixed point of the world while
 *     the camera moves, so svgf_project_prev sends it to the pixel of the previous frame in which the same reflection was seen.  The
 *     seen point's own world position would reproject to the pixel where that point is visible directly - another surface's history.
 *   out_chain_dev, if given, receives one int32 per pixel: +k a virtual hit after k guide rays; -k the guide gave up after k rays (a
 *     miss or the cap), the texel is the first hit's; 0 no guide ran.
 *   Identities by construction: with table == NULL, an empty or an all-diffuse table, or any table none of whose fully specular objects
 *     is a first hit, every output is svgf_gloss_draw(_split)'s on bits and chain is 0 everywhere; vp never changes a colour bit.
 * Limits: the reprojection is exact only for static planar mirrors; for curved mirrors, refraction and moving reflectors the unfolded
 *   position is an approximation (examples/virtual_scene.cpp measures it).  With svgf_set_object_motion a virtual texel that carries a
 *   moving object's id would be moved by that object's map in unmirrored space: id_offset lets the caller point virtual ids at rows
 *   of the motion table that hold the identity.  The seen surface's albedo is not demodulated, so reflected texture stays in the
 *   indirect term.
 * INTEGRATION.md 5o has the frame loop and the link line, examples/virtual_scene.cpp runs it. */
#ifndef SVGF_VIRTUAL_H_
#define SVGF_VIRTUAL_H_

#include "svgf.h"
#include "svgf_path.h"
#include "svgf_gloss.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SvgfVirtualParams {
    int max_chain;   /* 1..SVGF_PATH_MAX_DEPTH: the most rays the guide chain may trace */
    int id_offset;   /* 0..(1 << 24): added to the geomId of a virtual hit (0 keeps the seen object's id) */
} SvgfVirtualParams;

int  svgf_virtual_draw(const svgf_scene *scene, const svgf_gloss_table *table /* or NULL */, void *out_rgb_dev,
                       void *out_gbuffer_dev /* or NULL */, const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height,
                       const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                       const SvgfVirtualParams *vp, void *out_chain_dev /* int32 per pixel, or NULL */, void *stream);
int  svgf_virtual_draw_split(const svgf_scene *scene, const svgf_gloss_table *table /* or NULL */, void *out_direct_dev,
                             void *out_indirect_dev, void *out_rgb_dev /* or NULL */, void *out_gbuffer_dev /* or NULL */,
                             const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height, const SvgfCamera *cam,
                             const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                             const SvgfVirtualParams *vp, void *out_chain_dev /* int32 per pixel, or NULL */, void *stream);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_gloss_version. */
int  svgf_virtual_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_VIRTUAL_H_ */
