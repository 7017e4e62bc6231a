// svgf_scene_trace.hip — libsvgf_trace.so, the companion library of row f17: svgf_trace_draw, the resident scene path-traced with one
// diffuse bounce.  include/svgf_trace.h states the semantics.  Renderer-side code: it is NOT part of libsvgf_hip.so, links against
// it, and reaches a scene through svgf_scene_view alone (struct svgf_scene is unknown here).  The arithmetic is the product's own
// text: svgf_scene_pixel.inc.h (ray, primitive and triangle tests, surface, the light's term, noise and stores) and
// svgf_scene_walk.inc.h (the closest-hit and the any-hit walk), so a ray here and a ray of k_scene_bvh are the same operations.
// The kernel itself is svgf_scene_trace.inc.h, which libsvgf_split.so (row f18) compiles too.
#include "svgf_kernels.h"
#include "../../include/svgf_trace.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

namespace {

#include "svgf_scene_trace.inc.h"

}  // namespace

extern "C" int svgf_trace_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_trace_draw(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                               const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfTraceParams *tp, void *stream)
{
    SceneTraceArgs t;
    int device = 0;
    const int rc = trace_prepare(t, device, scene, out_rgb_dev, true, out_gbuffer_dev, planes, width, height, cam, sp, light, tp);
    if (rc != SVGF_OK) return rc;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_trace<SceneTraceArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
