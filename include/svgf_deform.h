/* svgf_deform.h — row f26: a resident scene whose vertices move independently of each other (libsvgf_deform.so).
 *
 * svgf_scene_pose (row f15) moves whole objects rigidly.  This library skins triangles: per frame it blends up to four bone maps per
 * triangle corner, writes the result into the scene's triangles AS DRAWN with row f14's padded boxes, keeps the previous frame's
 * positions, and turns them into the per-pixel previous position that svgf_motion_reproject (row f5) takes.  It links against
 * libsvgf_hip.so alone and reaches the scene through svgf_scene_view, svgf_scene_drawn_arrays and nothing else.
 * The frame loop: svgf_scene_pose, svgf_deform_apply, a tree (svgf_scene_refit | svgf_lbvh_build | svgf_sah_build), the draw,
 * svgf_deform_prev_positions, svgf_motion_reproject, svgf_denoise_motion.  INTEGRATION.md 5t has it in full.
 *
 * THE RIG is given per triangle corner, because the scene's triangles are unindexed (3 vertices x {pos, normal, uv}):
 *   tri_index[n_skinned]       the skinned triangles: strictly increasing, each in [0, n_tris)
 *   bone[n_skinned * 3 * 4]    unsigned short, four influences per corner, each in [0, n_bones)
 *   weight[n_skinned * 3 * 4]  float, finite and >= 0; expected to sum to 1 per corner (NOT checked)
 *   n_bones                    1..SVGF_DEFORM_MAX_BONES; n_skinned >= 1
 * svgf_deform_check_rig_host: host only, no device needed.  SVGF_OK, or SVGF_ERR_INVALID_ARG for a NULL array, n_tris < 1, n_skinned
 *   outside 1..n_tris, n_bones outside 1..SVGF_DEFORM_MAX_BONES, a tri_index that is out of range or not above the one before it, a
 *   bone index >= n_bones, a weight that is negative or not finite.
 * svgf_deform_create(scene, rig..., out): needs a scene with svgf_scene_enable_pose (its drawn arrays are writable copies; a scene
 *   without has only its REST state: SVGF_ERR_INVALID_ARG).  Runs the check above before any device work (*out cleared on every
 *   refusal), then makes ONE device allocation: the rig, slot[n_tris] (the skinned slot of a triangle, or -1), the REST triangles of
 *   the rig and cur[n_skinned * 9], prev[n_skinned * 9] (three corners x xyz), both initialised to the REST positions.  THE REST
 *   TRIANGLE of a skinned triangle is a bit copy of the triangle as drawn when this call runs: create the rig before anything deforms
 *   the scene.  (svgf_scene_pose keeps the rest bytes of every triangle whose id stands outside its table, so a rig may be created
 *   after poses as long as the skinned objects' ids do.)  Allocates, launches one kernel and synchronises: not under capture.
 * svgf_deform_apply(d, bones_dev, n_bones, stream): ONE launch, one thread per skinned triangle; no allocation, no copy, no host wait;
 *   legal under stream capture.  bones_dev: n_bones SvgfScenePose records in device memory, 16-byte aligned; only xf is read, and the
 *   CONTENTS are read when the kernel runs (row f7's rule: a captured apply replays with whatever the table holds then).  n_bones must
 *   be the rig's.  The thread of slot s, triangle i = tri_index[s], in this order:
 *     1. prev[s] := cur[s]
 *     2. skins the three corners from the REST triangle (never from the previous result: the same table twice leaves the same bytes)
 *     3. writes cur[s]
 *     4. writes triangle i of the scene's drawn array: positions and normals; uv are the rest's
 *     5. writes padded box i by row f14's formula (the literals and nesting of svgf_scene_pose's kernel), first = i, count = 1
 *   Triangles outside the rig are never touched.  In a mixed scene svgf_scene_pose runs FIRST (it rewrites every triangle, the skinned
 *   ones with their rest bytes) and the skinned objects' ids stand outside its table.
 *   AFTER AN APPLY THE SCENE'S TREE IS STALE - its boxes no longer bound the triangles - until svgf_scene_refit or a rebuild
 *   (svgf_lbvh_build, svgf_sah_build on an attached tree).  The topology is fixed, so a draw in between cannot loop or read out of
 *   bounds; it may miss triangles.
 * svgf_deform_prev_positions(d, out_prev_pos_dev, out_geom_id_dev, width, height, cam, pixel_length, stream): ONE launch, one thread per
 *   pixel, behind the frame's apply and tree.  Per pixel the primary ray and the closest hit of svgf_scene_draw with that camera and
 *   pixel_length (SvgfSynthParams.pixel_length) - the product's own text (csrc/svgf_scene_pixel.inc.h, csrc/svgf_scene_walk.inc.h) over
 *   whatever tree svgf_scene_view hands out.  out_prev_pos_dev: width * height packed float3, the layout of svgf_motion_reproject's
 *   position_dev; out_geom_id_dev (or NULL): width * height ints, the hit's id.  The caller turns the pair into a motion plane with
 *   svgf_motion_reproject(position_dev = that plane, geom_id_dev, prev_cam, ...): the projection stays the product's own.
 *   No allocation, no host wait; legal under capture.
 * svgf_deform_read(d, which, host_dst, host_bytes): blocking (tests, debugging).  0 cur, 1 prev (36 B * n_skinned), 2 slot
 *   (4 B * n_tris).  host_bytes must be the array's size exactly; otherwise, or for another kind or a NULL argument,
 *   SVGF_ERR_INVALID_ARG.
 * svgf_deform_destroy waits for the device first; NULL is accepted.  Destroy the rig before its scene.
 * Every other error (a NULL handle or pointer, an n_bones that is not the rig's, a table that is not 16-byte aligned, width or height
 *   < 1: SVGF_ERR_INVALID_ARG; width * height >= 2^31 / 16: SVGF_ERR_UNSUPPORTED) is answered before any device work.
 *
 * Normative arithmetic - float32, one rounding per operation, no contraction.  Corner v of slot s has rest position p, rest normal n,
 * influences k = 0..3 with M_k = bones[bone[(3 s + v) 4 + k]].xf and w_k = weight[(3 s + v) 4 + k].  ALL FOUR are always evaluated
 * (a weight of 0 does not skip its bone: 0 * inf is NaN):
 *   q_k[r] = ((M_k[4r] px + M_k[4r+1] py) + M_k[4r+2] pz) + M_k[4r+3]              (row f15's formula)
 *   p'[r]  = ((w0 q_0[r] + w1 q_1[r]) + w2 q_2[r]) + w3 q_3[r]
 *   m_k[r] = (M_k[4r] nx + M_k[4r+1] ny) + M_k[4r+2] nz;   n'[r] = ((w0 m_0[r] + w1 m_1[r]) + w2 m_2[r]) + w3 m_3[r]
 *            (the linear block only, not renormalised: row f7's rule)
 *   Padded box: row f14's formula on the three p'.
 * Previous position of a pixel.  pos is the position the G-buffer gets; i the winning triangle with barycentrics (bx, by) as
 *   svgf_scene_draw forms them; the corner weights are b0 = (1.0f - bx) - by, b1 = bx, b2 = by; s = slot[i]:
 *     d_c   = (b0 (prev[s][0][c] - cur[s][0][c]) + b1 (prev[s][1][c] - cur[s][1][c])) + b2 (prev[s][2][c] - cur[s][2][c])
 *     out_c = pos_c where d_c == 0, pos_c + d_c otherwise
 *   A hit on a primitive or on a triangle outside the rig (s < 0): out = pos.  A miss: NaN, NaN, NaN and id -1.
 *   So a rig that does not move reproduces the camera path bit for bit through svgf_motion_reproject with n_geoms = 0.
 * What stays as it is: the set of triangles, textures and uv; primitives move only through svgf_scene_pose; the temporal pass's
 *   normal test is unchanged, so STRONG BENDING MAY REJECT HISTORY THERE (the previous normal is the previous frame's, not a
 *   re-skinned one).
 * Every float is a defined input to the above; the bone indices were checked at creation and the topology is fixed, so a NaN or inf
 *   bone row cannot make anything read out of bounds. */
#ifndef SVGF_DEFORM_H_
#define SVGF_DEFORM_H_

#include "svgf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svgf_deform svgf_deform;
#define SVGF_DEFORM_MAX_BONES 1024
typedef struct SvgfDeformInfo {
    int n_tris, n_skinned, n_bones, launches /* of an apply: 1 */;
    unsigned long long device_bytes;
} SvgfDeformInfo;

int  svgf_deform_check_rig_host(int n_tris, const int *tri_index, int n_skinned, const unsigned short *bone, const float *weight, int n_bones);
int  svgf_deform_create(svgf_scene *scene, const int *tri_index, int n_skinned, const unsigned short *bone, const float *weight, int n_bones,
                        svgf_deform **out);
int  svgf_deform_apply(svgf_deform *d, const SvgfScenePose *bones_dev, int n_bones, void *stream);
int  svgf_deform_prev_positions(const svgf_deform *d, float *out_prev_pos_dev, int *out_geom_id_dev /* or NULL */, int width, int height,
                                const SvgfCamera *cam, const float pixel_length[2], void *stream);
int  svgf_deform_info(const svgf_deform *d, SvgfDeformInfo *out);
int  svgf_deform_read(const svgf_deform *d, int which, void *host_dst, unsigned long long host_bytes);   /* blocking: 0 cur, 1 prev, 2 slot */
void svgf_deform_destroy(svgf_deform *d);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_trace_version. */
int  svgf_deform_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_DEFORM_H_ */
