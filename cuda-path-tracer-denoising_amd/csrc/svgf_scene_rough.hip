// svgf_scene_rough.hip — libsvgf_rough.so, the companion library of row f22: svgf_rough_draw and svgf_rough_draw_split, the virtual-hit
// draws of row f21 with a GGX lobe on the mirror vertices of the objects a roughness table (svgf_rough_table_*) names.
// include/svgf_rough.h states the semantics.  Like the other five companions this one links against libsvgf_hip.so only and reaches a
// scene through svgf_scene_view alone; the surface table is the svgf_gloss_table libsvgf_gloss.so creates, read through the private
// csrc/svgf_gloss_table.h.
//
// The kernel is svgf_scene_gloss.inc.h's k_scene_gloss, the text libsvgf_gloss.so and libsvgf_virtual.so compile, instantiated with the
// roughness table beside the virtual draw's arguments (ROUGH): the vertex body, the walks and the guide are that text's, and so is
// rough_vertex, the lobe.  This file keeps the roughness table and the two draws.
#include "svgf_kernels.h"
#include "../../include/svgf_trace.h"
#include "../../include/svgf_path.h"
#include "../../include/svgf_virtual.h"
#include "../../include/svgf_rough.h"
#include "svgf_gloss_table.h"
#include "svgf_rough_table.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

namespace {

#include "svgf_scene_trace.inc.h"

#include "svgf_scene_gloss.inc.h"

bool alpha_ok(const float &alpha) { return std::isfinite(alpha) && alpha >= 0.0f && alpha <= 1.0f; }

}  // namespace

extern "C" int svgf_rough_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_rough_table_create(int device, const float *alpha_host, int n, svgf_rough_table **out)
{
    return svgf_device_table_create(device, alpha_host, n, out, alpha_ok);
}

extern "C" void svgf_rough_table_destroy(svgf_rough_table *t) { svgf_device_table_destroy(t); }

extern "C" int svgf_rough_table_size(const svgf_rough_table *t) { return svgf_device_table_size(t); }

extern "C" int svgf_rough_draw(const svgf_scene *scene, const svgf_gloss_table *table, void *out_rgb_dev, void *out_gbuffer_dev,
                               const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                               const SvgfSceneLight *light, const SvgfPathParams *pp, const SvgfVirtualParams *vp, void *out_chain_dev,
                               void *stream, const svgf_rough_table *rough, const SvgfRoughParams *rp)
{
    SceneRoughArgs t;
    int device = 0;
    int rc = gloss_draw_args(t.v.g, device, scene, table, out_rgb_dev, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc == SVGF_OK) rc = guide_args(t.v.v, vp, out_chain_dev);
    if (rc == SVGF_OK) rc = rough_args(t.r, rp, rough, device);
    return gloss_launch(rc, t, device, width, height, stream);
}

extern "C" int svgf_rough_draw_split(const svgf_scene *scene, const svgf_gloss_table *table, void *out_direct_dev, void *out_indirect_dev,
                                     void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                                     const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                                     const SvgfVirtualParams *vp, void *out_chain_dev, void *stream, const svgf_rough_table *rough,
                                     const SvgfRoughParams *rp)
{
    SceneRoughSplitArgs s;
    int device = 0;
    int rc = gloss_draw_split_args(s.v.g, device, scene, table, out_direct_dev, out_indirect_dev, out_rgb_dev, out_gbuffer_dev, planes,
                                   width, height, cam, sp, light, pp);
    if (rc == SVGF_OK) rc = guide_args(s.v.v, vp, out_chain_dev);
    if (rc == SVGF_OK) rc = rough_args(s.r, rp, rough, device);
    return gloss_launch(rc, s, device, width, height, stream);
}
