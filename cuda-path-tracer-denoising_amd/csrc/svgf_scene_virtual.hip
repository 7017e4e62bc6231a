// svgf_scene_virtual.hip — libsvgf_virtual.so, the companion library of row f21: svgf_virtual_draw and svgf_virtual_draw_split, the
// glossy draws of row f20 with a VIRTUAL-HIT G-buffer: where the first hit is purely specular the texel's normal, position and id
// describe what the mirror or the pane shows, found by a deterministic guide chain.  include/svgf_virtual.h states the semantics.  Like
// the other four companions this one links against libsvgf_hip.so only and reaches a scene through svgf_scene_view alone; the table is
// the svgf_gloss_table libsvgf_gloss.so creates, read through the private csrc/svgf_gloss_table.h.
//
// The kernel is svgf_scene_gloss.inc.h's k_scene_gloss, the text libsvgf_gloss.so compiles, instantiated with the guide's arguments
// beside the glossy draw's: every ray of every path is the same statement, so colour, D and I are that library's on every bit, and the
// guide is one more turn of its vertex loop.  Nothing of the kernel is written here.
#include "svgf_kernels.h"
#include "../../include/svgf_trace.h"
#include "../../include/svgf_path.h"
#include "../../include/svgf_virtual.h"
#include "svgf_gloss_table.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

namespace {

#include "svgf_scene_trace.inc.h"

#include "svgf_scene_gloss.inc.h"

}  // namespace

extern "C" int svgf_virtual_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_virtual_draw(const svgf_scene *scene, const svgf_gloss_table *table, void *out_rgb_dev, void *out_gbuffer_dev,
                                 const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                                 const SvgfSceneLight *light, const SvgfPathParams *pp, const SvgfVirtualParams *vp, void *out_chain_dev,
                                 void *stream)
{
    SceneVirtualArgs t;
    int device = 0;
    int rc = gloss_draw_args(t.g, device, scene, table, out_rgb_dev, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc == SVGF_OK) rc = guide_args(t.v, vp, out_chain_dev);
    return gloss_launch(rc, t, device, width, height, stream);
}

extern "C" int svgf_virtual_draw_split(const svgf_scene *scene, const svgf_gloss_table *table, void *out_direct_dev, void *out_indirect_dev,
                                       void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                                       const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                                       const SvgfVirtualParams *vp, void *out_chain_dev, void *stream)
{
    SceneVirtualSplitArgs s;
    int device = 0;
    int rc = gloss_draw_split_args(s.g, device, scene, table, out_direct_dev, out_indirect_dev, out_rgb_dev, out_gbuffer_dev, planes,
                                   width, height, cam, sp, light, pp);
    if (rc == SVGF_OK) rc = guide_args(s.v, vp, out_chain_dev);
    return gloss_launch(rc, s, device, width, height, stream);
}
