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
#include <new>
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
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    if (n < 0 || n > SVGF_SCENE_MAX_POSED || (n > 0 && !host) || device < 0) return SVGF_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (!surface_ok(host[i])) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) {
        (void)hipGetLastError();        // a device that does not exist must not fail the next launch's check
        return SVGF_ERR_NO_DEVICE;
    }
    svgf_gloss_table *t = new (std::nothrow) svgf_gloss_table{ device, n, nullptr };
    if (!t) return SVGF_ERR_OOM;
    if (n > 0) {
        if (hipMalloc(reinterpret_cast<void **>(&t->dev), (size_t)n * sizeof(SvgfSurface)) != hipSuccess) {
            (void)hipGetLastError();
            delete t;
            return SVGF_ERR_OOM;
        }
        if (hipMemcpy(t->dev, host, (size_t)n * sizeof(SvgfSurface), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(t->dev);
            delete t;
            return SVGF_ERR_HIP;
        }
    }
    *out = t;
    return SVGF_OK;
}

extern "C" void svgf_gloss_table_destroy(svgf_gloss_table *t)
{
    if (!t) return;
    if (t->dev) {
        SvgfDeviceGuard dev_guard(t->device);
        (void)hipFree(t->dev);
    }
    delete t;
}

extern "C" int svgf_gloss_table_size(const svgf_gloss_table *t) { return t ? t->n : SVGF_ERR_INVALID_ARG; }

extern "C" int svgf_gloss_draw(const svgf_scene *scene, const svgf_gloss_table *table, void *out_rgb_dev, void *out_gbuffer_dev,
                               const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                               const SvgfSceneLight *light, const SvgfPathParams *pp, void *stream)
{
    SceneGlossArgs t;
    int device = 0;
    const int rc = gloss_draw_args(t, device, scene, table, out_rgb_dev, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc != SVGF_OK) return rc;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_gloss<SceneGlossArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
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
    if (rc != SVGF_OK) return rc;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_gloss<SceneGlossSplitArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), s);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
