// svgf_scene_split.hip — libsvgf_split.so, the companion library of row f18: svgf_trace_draw_split, svgf_trace_draw's frame with direct
// and indirect light written apart and without the albedo.  include/svgf_split.h states the semantics.  The kernel is
// svgf_scene_trace.inc.h, the text libsvgf_trace.so compiles, instantiated over SceneSplitArgs: the rays are one text.  Like that
// library this one links against libsvgf_hip.so and reaches a scene through svgf_scene_view alone.  svgf_trace_compose, which puts two
// terms back together, is svgf_trace_compose.hip.
#include "svgf_kernels.h"
#include "../../include/svgf_split.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

namespace {

#include "svgf_scene_trace.inc.h"

}  // namespace

extern "C" int svgf_trace_draw_split(const svgf_scene *scene, void *out_direct_dev, void *out_indirect_dev, void *out_rgb_dev, void *out_gbuffer_dev,
                                     const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                                     const SvgfSceneLight *light, const SvgfTraceParams *tp, void *stream)
{
    SceneSplitArgs s;
    int device = 0;
    const int rc = trace_prepare(s.t, device, scene, out_rgb_dev, false, out_gbuffer_dev, planes, width, height, cam, sp, light, tp);
    if (rc != SVGF_OK) return rc;
    if (!out_direct_dev || !out_indirect_dev || out_direct_dev == out_indirect_dev) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    s.out_direct = static_cast<float *>(out_direct_dev); s.out_indirect = static_cast<float *>(out_indirect_dev);
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_trace<SceneSplitArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), s);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
