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

// what follows the gloss draw's refusals, in svgf_rough_draw's order: vp's, rp's and the roughness table's, then hp's
bool highlight_params_ok(const SvgfVirtualParams *vp, const SvgfRoughParams *rp, const svgf_rough_table *rough, int device, const SvgfHighlightParams *hp)
{
    if (!vp || vp->max_chain < 1 || vp->max_chain > SVGF_PATH_MAX_DEPTH || vp->id_offset < 0 || vp->id_offset > (1 << 24)) return false;
    if (!rp || !std::isfinite(rp->guide_alpha) || rp->guide_alpha < 0.0f) return false;
    if (rough && rough->device != device) return false;
    return hp && hp->enable >= 0 && hp->enable <= 1 && std::isfinite(hp->clamp) && hp->clamp >= 0.0f;
}

template <class Args>
void highlight_fill(Args &t, const SvgfVirtualParams *vp, void *out_chain_dev, const svgf_rough_table *rough, const SvgfRoughParams *rp,
                    const SvgfHighlightParams *hp)
{
    t.r.v.v = SceneGuide{ vp->max_chain, vp->id_offset, static_cast<int *>(out_chain_dev) };
    t.r.r = SceneRough{ rough ? rough->dev : nullptr, rough ? rough->n : 0, rp->guide_alpha };
    t.h = SceneHighlight{ hp->enable, hp->clamp };
}

}  // namespace

extern "C" int svgf_highlight_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_highlight_draw(const svgf_scene *scene, const svgf_gloss_table *table, void *out_rgb_dev, void *out_gbuffer_dev,
                                   const SvgfPlanarGBuffer *planes, int width, int height, const SvgfCamera *cam, const SvgfSynthParams *sp,
                                   const SvgfSceneLight *light, const SvgfPathParams *pp, const SvgfVirtualParams *vp, void *out_chain_dev,
                                   void *stream, const svgf_rough_table *rough, const SvgfRoughParams *rp, const SvgfHighlightParams *hp)
{
    SceneHighlightArgs t;
    int device = 0;
    const int rc = gloss_draw_args(t.r.v.g, device, scene, table, out_rgb_dev, out_gbuffer_dev, planes, width, height, cam, sp, light, pp);
    if (rc != SVGF_OK) return rc;
    if (!highlight_params_ok(vp, rp, rough, device, hp)) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    highlight_fill(t, vp, out_chain_dev, rough, rp, hp);
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_gloss<SceneHighlightArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_highlight_draw_split(const svgf_scene *scene, const svgf_gloss_table *table, void *out_direct_dev, void *out_indirect_dev,
                                         void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                                         const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfPathParams *pp,
                                         const SvgfVirtualParams *vp, void *out_chain_dev, void *stream, const svgf_rough_table *rough,
                                         const SvgfRoughParams *rp, const SvgfHighlightParams *hp)
{
    SceneHighlightSplitArgs s;
    int device = 0;
    const int rc = gloss_draw_split_args(s.r.v.g, device, scene, table, out_direct_dev, out_indirect_dev, out_rgb_dev, out_gbuffer_dev, planes,
                                         width, height, cam, sp, light, pp);
    if (rc != SVGF_OK) return rc;
    if (!highlight_params_ok(vp, rp, rough, device, hp)) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    highlight_fill(s, vp, out_chain_dev, rough, rp, hp);
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_gloss<SceneHighlightSplitArgs>, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), s);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
