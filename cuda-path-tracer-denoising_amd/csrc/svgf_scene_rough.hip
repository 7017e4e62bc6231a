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
#include <new>
#include <type_traits>

namespace {

#include "svgf_scene_trace.inc.h"

#include "svgf_scene_gloss.inc.h"

bool virtual_params_ok(const SvgfVirtualParams *vp)
{
    return vp && vp->max_chain >= 1 && vp->max_chain <= SVGF_PATH_MAX_DEPTH && vp->id_offset >= 0 && vp->id_offset <= (1 << 24);
}

// what follows the virtual draw's refusals: rp's and the roughness table's
bool rough_params_ok(const SvgfRoughParams *rp, const svgf_rough_table *rough, int device)
{
    if (!rp || !std::isfinite(rp->guide_alpha) || rp->guide_alpha < 0.0f) return false;
    return !rough || rough->device == device;
}

SceneRough rough_of(const svgf_rough_table *rough, const SvgfRoughParams *rp)
{
    return SceneRough{ rough ? rough->dev : nullptr, rough ? rough->n : 0, rp->guide_alpha };
}

}  // namespace

extern "C" int svgf_rough_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_rough_table_create(int device, const float *alpha_host, int n, svgf_rough_table **out)
{
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    if (n < 0 || n > SVGF_SCENE_MAX_POSED || (n > 0 && !alpha_host) || device < 0) return SVGF_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (!std::isfinite(alpha_host[i]) || alpha_host[i] < 0.0f || alpha_host[i] > 1.0f) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) {
        (void)hipGetLastError();        // a device that does not exist must not fail the next launch's check
        return SVGF_ERR_NO_DEVICE;
    }
    svgf_rough_table *t = new (std::nothrow) svgf_rough_table{ device, n, nullptr };
    if (!t) return SVGF_ERR_OOM;
    if (n > 0) {
        if (hipMalloc(reinterpret_cast<void **>(&t->dev), (size_t)n * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            delete t;
            return SVGF_ERR_OOM;
        }
        if (hipMemcpy(t->dev, alpha_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(t->dev);
            delete t;
            return SVGF_ERR_HIP;
        }
    }
    *out = t;
    return SVGF_OK;
}

extern "C" void svgf_rough_table_destroy(svgf_rough_table *t)
{
    if (!t) return;
    if (t->dev) {
        SvgfDeviceGuard dev_guard(t->device);
        (void)hipFree(t->dev);
    }
    delete t;
}

extern "C" int svgf_rough_table_size(const svgf_rough_table *t) { return t ? t->n : SVGF_ERR_INVALID_ARG; }

extern "C" int svgf_rough_draw(const svgf_scene *scene, const svgf_gloss_table *table, void *out_rgb_dev, void *out_gbuffer_dev,
                               const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                               const SvgfSceneLight *light, const SvgfPathParams *pp, const SvgfVirtualParams *vp, void *out_chain_dev,
                               void *stream, const svgf_rough_table *rough, const SvgfRoughParams *rp)
{
    SceneRoughArgs t;
    int device = 0;
    const int rc = gloss_draw_args(t.v.g, device, scene, table, out_rgb_dev, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc != SVGF_OK) return rc;
    if (!virtual_params_ok(vp)) return SVGF_ERR_INVALID_ARG;
    if (!rough_params_ok(rp, rough, device)) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    t.v.v = SceneGuide{ vp->max_chain, vp->id_offset, static_cast<int *>(out_chain_dev) };
    t.r = rough_of(rough, rp);
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_gloss<SceneRoughArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_rough_draw_split(const svgf_scene *scene, const svgf_gloss_table *table, void *out_direct_dev, void *out_indirect_dev,
                                     void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                                     const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                                     const SvgfVirtualParams *vp, void *out_chain_dev, void *stream, const svgf_rough_table *rough,
                                     const SvgfRoughParams *rp)
{
    SceneRoughSplitArgs s;
    int device = 0;
    const int rc = gloss_draw_split_args(s.v.g, device, scene, table, out_direct_dev, out_indirect_dev, out_rgb_dev, out_gbuffer_dev, planes,
                                         width, height, cam, sp, light, pp);
    if (rc != SVGF_OK) return rc;
    if (!virtual_params_ok(vp)) return SVGF_ERR_INVALID_ARG;
    if (!rough_params_ok(rp, rough, device)) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    s.v.v = SceneGuide{ vp->max_chain, vp->id_offset, static_cast<int *>(out_chain_dev) };
    s.r = rough_of(rough, rp);
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_gloss<SceneRoughSplitArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), s);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
