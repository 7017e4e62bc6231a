// svgf_scene_highlight.hip — libsvgf_highlight.so, the companion library of row f23: svgf_highlight_draw and svgf_highlight_draw_split,
// the rough draws of row f22 with the analytic light's GGX term at the rough vertices.  include/svgf_highlight.h states the semantics.
// Like the other six companions this one links against libsvgf_hip.so only and reaches a scene through svgf_scene_view alone; the
// surface table is libsvgf_gloss.so's and the roughness table libsvgf_rough.so's, read through the private csrc/svgf_gloss_table.h and
// csrc/svgf_rough_table.h.
//
// The kernel is svgf_scene_gloss.inc.h's k_scene_gloss, the text the three libraries before this one compile, instantiated with the
// highlight's two parameters beside the rough draw's arguments (SHINE): the vertex body, the walks, the guide, the lobe and the
// light's factor (shine_factor) are that text's.  This file keeps the two draws.
#include "svgf_kernels.h"
#include "../../include/svgf_trace.h"
#include "../../include/svgf_path.h"
#include "../../include/svgf_virtual.h"
#include "../../include/svgf_rough.h"
#include "../../include/svgf_highlight.h"
#include "svgf_gloss_table.h"
#include "svgf_rough_table.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

namespace {

#include "svgf_scene_trace.inc.h"

#include "svgf_scene_gloss.inc.h"

}  // namespace

extern "C" int svgf_highlight_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_highlight_draw(const svgf_scene *scene, const svgf_gloss_table *table, void *out_rgb_dev, void *out_gbuffer_dev,
                                   const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                                   const SvgfSceneLight *light, const SvgfPathParams *pp, const SvgfVirtualParams *vp, void *out_chain_dev,
                                   void *stream, const svgf_rough_table *rough, const SvgfRoughParams *rp, const SvgfHighlightParams *hp)
{
    SceneHighlightArgs t;
    int device = 0;
    int rc = gloss_draw_args(t.r.v.g, device, scene, table, out_rgb_dev, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc == SVGF_OK) rc = guide_args(t.r.v.v, vp, out_chain_dev);
    if (rc == SVGF_OK) rc = rough_args(t.r.r, rp, rough, device);
    if (rc == SVGF_OK) rc = shine_args(t.h, hp);
    return gloss_launch(rc, t, device, width, height, stream);
}

extern "C" int svgf_highlight_draw_split(const svgf_scene *scene, const svgf_gloss_table *table, void *out_direct_dev, void *out_indirect_dev,
                                         void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                                         const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                                         const SvgfVirtualParams *vp, void *out_chain_dev, void *stream, const svgf_rough_table *rough,
                                         const SvgfRoughParams *rp, const SvgfHighlightParams *hp)
{
    SceneHighlightSplitArgs s;
    int device = 0;
    int rc = gloss_draw_split_args(s.r.v.g, device, scene, table, out_direct_dev, out_indirect_dev, out_rgb_dev, out_gbuffer_dev, planes,
                                   width, height, cam, sp, light, pp);
    if (rc == SVGF_OK) rc = guide_args(s.r.v.v, vp, out_chain_dev);
    if (rc == SVGF_OK) rc = rough_args(s.r.r, rp, rough, device);
    if (rc == SVGF_OK) rc = shine_args(s.h, hp);
    return gloss_launch(rc, s, device, width, height, stream);
}
