/* svgf_split.h — C ABI of libsvgf_split.so, the companion library of row f18: direct and indirect light apart, and put back together.
 *
 * A second companion beside libsvgf_trace.so (svgf_trace.h, whose two functions and whose ABI stay what they were): built from the same
 * tree, linked against libsvgf_hip.so, reaching a scene through svgf_scene_view alone, reading no environment variable.  Its draw is
 * svgf_trace_draw's kernel text (csrc/svgf_scene_trace.inc.h) compiled a second time, so a ray means here what it means there.  A
 * program that uses both draws links -lsvgf_split -lsvgf_trace -lsvgf_hip.
 *
 * SVGF as published (Schied et al. 2017) does not filter svgf_trace_draw's frame as it is: it takes the albedo out, filters direct and indirect
 * illumination SEPARATELY - each with its own history, variance, clamp and firefly filter - and multiplies the albedo back at the
 * end.  svgf_trace_draw_split is svgf_trace_draw with that kind of output: the same rays from the same hash streams in the same
 * order, ONE launch, and two demodulated images, out_direct_dev and out_indirect_dev (packed rgb float32, width * height each, both
 * required, not the same pointer).  Each goes to a context of its own run with sepcolor = 1 and addcolor = 0 (both contexts may read
 * the same AoS G-buffer); svgf_trace_compose below puts the two denoised terms together.  INTEGRATION.md 5l has the frame loop.
 * out_rgb_dev may be NULL; otherwise it receives svgf_trace_draw's colour on every bit, so that the one-image and the two-image
 * pipeline can be compared on identical rays.  The G-buffer (AoS or planes, exactly one of the two) is svgf_trace_draw's on every bit.
 * No allocation, no upload, no host wait, one kernel node under capture; on a static scene and on a posed one.
 * Errors, all before any device work: svgf_trace_draw's, in its order (out_rgb_dev exempt), then SVGF_ERR_INVALID_ARG for a NULL
 *   out_direct_dev or out_indirect_dev or when the two are the same pointer.
 *
 * Normative semantics - float32, one rounding per operation, no contraction; first = ambient + vis * direct, ind_c, mult, chroma_c,
 * alb_c and emit (the hit's emittance) are exactly svgf_trace_draw's quantities of pixel p (the ambient term belongs to the direct
 * image):
 *   pixel                                   D_c (direct)                  I_c (indirect)
 *   a miss (geomId < 0)                     +0.0f                         +0.0f
 *   an emitter (emit > 0)                   (emit * mult) * chroma_c      +0.0f
 *   any other, bounce_samples > 0           (first * mult) * chroma_c     (ind_c * mult) * chroma_c
 *   any other, bounce_samples == 0          (first * mult) * chroma_c     +0.0f
 * With noise = 0 both factors are exactly 1: D = first and I = ind on bits.  alb_c * (D_c + I_c) is svgf_trace_draw's colour up to
 * rounding (four roundings of the same product either way), not on bits. */
#ifndef SVGF_SPLIT_H_
#define SVGF_SPLIT_H_

#include "svgf_trace.h"

#ifdef __cplusplus
extern "C" {
#endif

int svgf_trace_draw_split(const svgf_scene *scene, void *out_direct_dev, void *out_indirect_dev, void *out_rgb_dev /* or NULL */,
                          void *out_gbuffer_dev /* or NULL */, const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height,
                          const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneLight *light, const SvgfTraceParams *tp,
                          void *stream);

/* The modulation for two terms: out_c = a_c * (D_c + I_c) per pixel and channel - one addition, then one multiplication, float32, no
 * contraction; no special case for a miss (its albedo is 0), NaN or an infinity: plain IEEE.  a_c = albedo_c * ialbedo_c of the AoS
 * texel when guide->gbuffer != NULL, else guide->albedo[3 p + c] (svgf_upsample's `modulate` convention; the guide's other fields are
 * not read).  out_rgb_dev may be the same pointer as direct_dev or indirect_dev (every element is read before it is written, by
 * the thread that writes it); any other overlap is the caller's fault.  The images need 4-byte alignment only; 16-byte accesses are
 * used where every image (and the albedo plane) sits at the same offset from a 16-byte boundary, as fresh allocations do.
 * Stateless, asynchronous on `stream`, one launch, no allocation, legal under stream capture (one kernel node).
 * Errors, all before any device work: SVGF_ERR_INVALID_ARG for a NULL image or guide, a guide with neither gbuffer nor albedo, a
 * size <= 0; SVGF_ERR_UNSUPPORTED for width * height >= 2^31 / 16; SVGF_ERR_NO_DEVICE as elsewhere. */
int svgf_trace_compose(int device, void *out_rgb_dev, const void *direct_dev, const void *indirect_dev, const SvgfGuide *guide,
                       int width, int height, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_SPLIT_H_ */
