// svgf_scene_gloss.hip — libsvgf_gloss.so, the companion library of row f20: svgf_gloss_draw and svgf_gloss_draw_split, svgf_path_draw's
// paths with a mirror and a glass lobe at every vertex, chosen per object from a table of SvgfSurface records (svgf_gloss_table_*).
// include/svgf_gloss.h states the semantics.  Like the other three companions this one links against libsvgf_hip.so and reaches a scene
// through svgf_scene_view alone.  Every ray, sampled direction and stored pixel is svgf_scene_trace.inc.h's text (and through it
// svgf_scene_pixel.inc.h's and svgf_scene_walk.inc.h's).  What row f20 added - gloss_vertex (the class of a vertex and the direction a
// specular one sends the path on in) and the loop that strings vertices into a path - is svgf_scene_gloss.inc.h's text, which
// libsvgf_virtual.so (row f21) compiles too; this file keeps the table and the two draws.
//
// k_scene_gloss: one thread per pixel, 256 per block; svgf_scene_gloss.inc.h describes the pixel.
#include "svgf_kernels.h"
#include "../../include/svgf_trace.h"
#include "../../include/svgf_path.h"
#include "svgf_gloss_table.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

namespace {

#include "svgf_scene_trace.inc.h"

#include "svgf_scene_gloss.inc.h"

bool surface_ok(const SvgfSurface &s)
{
    if (!std::isfinite(s.reflect) || !std::isfinite(s.refract) || !std::isfinite(s.ior)) return false;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(s.spec[c]) || s.spec[c] < 0.0f) return false;
    return s.reflect >= 0.0f && s.reflect <= 1.0f && s.refract >= 0.0f && s.ior > 0.0f;
}

}  // namespace

extern "C" int svgf_gloss_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_gloss_table_create(int device, const SvgfSurface *host, int n, svgf_gloss_table **out)
{
    return svgf_device_table_create(device, host, n, out, surface_ok);
}

extern "C" void svgf_gloss_table_destroy(svgf_gloss_table *t) { svgf_device_table_destroy(t); }

extern "C" int svgf_gloss_table_size(const svgf_gloss_table *t) { return svgf_device_table_size(t); }

extern "C" int svgf_gloss_draw(const svgf_scene *scene, const svgf_gloss_table *table, void *out_rgb_dev, void *out_gbuffer_dev,
                               const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                               const SvgfSceneLight *light, const SvgfPathParams *pp, void *stream)
{
    SceneGlossArgs t;
    int device = 0;
    const int rc = gloss_draw_args(t, device, scene, table, out_rgb_dev, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    return gloss_launch(rc, t, device, width, height, stream);
}

extern "C" int svgf_gloss_draw_split(const svgf_scene *scene, const svgf_gloss_table *table, void *out_direct_dev, void *out_indirect_dev,
                                     void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                                     const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                                     void *stream)
{
    SceneGlossSplitArgs s;
    int device = 0;
    const int rc = gloss_draw_split_args(s, device, scene, table, out_direct_dev, out_indirect_dev, out_rgb_dev, out_gbuffer_dev, planes, width,
                                         height, cam, sp, light, pp);
    return gloss_launch(rc, s, device, width, height, stream);
}
