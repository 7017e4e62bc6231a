/* svgf_restir_gi.h — row f28: reservoir resampling of the one-bounce indirect term (libsvgf_restir_gi.so).
 *
 * svgf_trace_draw_split (rows f17 / f18) estimates the indirect term I of a pixel from independent cosine samples of that pixel and
 * frame alone.  This library estimates the same I from a G-buffer of a resident scene by spatiotemporal reservoir resampling of the
 * bounce samples (Ouyang et al. 2021, "ReSTIR GI"): a pixel's sample is the hit of one bounce ray with the radiance it sends back, and
 * a pixel may take the sample a neighbour or its own history found.  The combination is the paper's BIASED one: the target function
 * carries no visibility, a taken sample is tested with ONE ray at the end of launch 2 and only if it came from a neighbour there (a
 * history sample chosen in launch 1 is not retested), and the normalisation counts every accepted tap.  Samples are NOT re-validated:
 * a stored radiance L is what it was in the frame that drew it, so moving lights or objects leave stale radiance in the history until
 * m_cap ages it out (or svgf_restir_gi_reset drops it).  Both are out of scope here.
 * It writes the demodulated indirect term I in the layout svgf_trace_compose and svgf_denoise take (packed rgb float).  It links
 * against libsvgf_hip.so alone, reaches the scene through svgf_scene_view and nothing else, and reads no environment variable.
 * INTEGRATION.md 5v has the frame loop (svgf_restir_frame for D, this for I, one svgf_denoise context each, svgf_trace_compose).
 *
 * Notation - float32, one rounding per operation, no contraction, sqrtf and division only; a.b = (a_0 b_0 + a_1 b_1) + a_2 b_2;
 * hash(k) = svgf_synth_render's hash(seed, frame, p, k) of pixel p = y * width + x; pos, n, id = the G-buffer's position, normal and
 * geomId at p; lum = the denoiser's luminance, (float)((0.2126 * (double)r + 0.7152 * (double)g) + 0.0722 * (double)b).
 * The integrand is written in the pixel's own cosine measure (the density of row f17's sampler is 1 there), so that one candidate
 * without reuse is svgf_trace_draw_split's I on bits.
 *   t_lo(pos) = 2^-10 fmaxf(1, fmaxf(fmaxf(|pos_0|, |pos_1|), |pos_2|))                                    - row f17's
 *   A SAMPLE is { xs, ns, L, g }: the position and the normal of the bounce hit, the radiance L_c it sends back per channel, and
 *     the geometry term g of the pixel that holds it.
 *   bounce(p, c): row f17's bounce sample j = c of pixel p on bits (svgf_trace.h: streams base = 256 + 16c, the rejection sampler in
 *     the branch-free frame of n, the nearest hit beyond t_lo(pos)): xs, ns = the hit's position and normal (a miss: the miss
 *     position and 0); L_c = 0 on a miss, alb2_c * emit2 on an emitter, otherwise alb2_c * (ambient + vis2 * direct2) with vis2 = 0
 *     iff shadow_secondary == 1 and row f16's shadow sample from xs towards the light point of streams base + 8, base + 9 is occluded
 *     (direct2 = svgf_scene_draw's light term at xs, ns towards light.centre).
 *   g_p(xs, ns): v = xs - pos; dist2 = v.v; wd = v / sqrtf(dist2); c = fmaxf(n.wd, 0); cphi = fmaxf(-(ns.wd), 0); (c * cphi) / dist2.
 *     (fmaxf of a NaN and 0 is 0.)
 *   The TARGET is phat_p(s) = lum(L) where g_p(s) > 0, and 0 otherwise; the candidates of a pixel's own sampler are weighed lum(L)
 *     whatever g says (they were drawn in the hemisphere of n; g only decides whether another pixel may take them).
 *   A RESERVOIR r is { sample, M, W, phat, valid } and, while it is being filled, w_sum.  Stored it is 64 bytes, four 16-byte words:
 *     xs, M | ns, W | L, phat | g, valid, 0, 0.  EMPTY is all zero.  A reservoir with valid == 0 is stored with every field but M zero.
 *   update(r, sample, phat, w, M_s, xi): w = (w > 0) ? w : 0 (a NaN weighs nothing); before = r.w_sum; r.w_sum = r.w_sum + w;
 *     r.M = r.M + M_s; the sample is selected iff w > 0 && (before == 0 || xi * r.w_sum < w); on selection r.sample and r.phat are
 *     set and r.valid = 1.
 *   finish(r): r.W = (r.valid && r.phat > 0) ? r.w_sum / (r.M * r.phat) : 0.
 *   take(s, r, xi) for a stored reservoir r of THIS pixel: update(s, r.sample, r.phat, (r.phat * r.W) * r.M, r.M, xi); a reservoir
 *     with valid == 0 adds its M and nothing else.
 *   take'(s, r, M', xi) for a reservoir r of ANOTHER pixel or frame: g' = g_p(r.xs, r.ns) AT THIS PIXEL, J = g' / r.g.  The tap is
 *     REFUSED - it adds nothing, not even to M - when r.valid == 0, when !(r.g > 0) or !(g' > 0), or when
 *     !(J >= 1 / jacobian_max && J <= jacobian_max) (a NaN refuses; 1 / jacobian_max is one float32 division).  Otherwise
 *     phat' = lum(r.L); update(s, { r.xs, r.ns, r.L, g' }, phat', ((phat' * r.W) * J) * M', M', xi).  Whether the selected sample
 *     is FOREIGN (came in by take') is kept in a register of the launch and never stored.
 *   visible(pos, xs): q = xs - pos; dl = sqrtf(q.q); !(dl > 0) forms no ray and is visible; otherwise d = q / dl and the point is
 *     OCCLUDED iff an occluder of svgf_scene_draw_shadowed counts on (pos, d) inside (t_lo(pos), dl - 2^-10 fmaxf(1, dl)).
 *   emissive(id): the state's table from geomId to emittance says > 0 (ids outside the table: 0).
 *
 * HASH STREAMS (above row f27's 4096..4224; the bounce itself reads row f17's 256 + 16c .. 256 + 16c + 9):
 *   8192 + c             candidate c's selection draw,  c = 0..7
 *   8224                 the history sample's selection draw
 *   8256 + 4k, + 1, + 2  neighbour k's offset in x, in y, and its selection draw,   k = 0..7
 *
 * THE STATE.  svgf_restir_gi_create(scene, width, height, &state): one allocation for one frame size - a history reservoir plane H, a
 *   scratch plane T (64 bytes per pixel each), the previous frame's normal and geomId planes, and the table from geomId to emittance
 *   of svgf_restir_create (same rules, same refusals: SVGF_ERR_INVALID_ARG for NULL, a size <= 0, an id that is negative or above
 *   SVGF_RESTIR_GI_MAX_ID, or one id naming surfaces of differing emittance; SVGF_ERR_UNSUPPORTED for width * height >= 2^31 / 32).
 *   Allocates, copies, launches the reset and synchronises: not under capture.  The scene must outlive the state.
 *   svgf_restir_gi_reset(state, stream): ONE launch; H becomes EMPTY everywhere and the previous ids -1.
 *   svgf_restir_gi_read(state, which, host_dst, host_bytes): blocking (tests, debugging).  0 H, 1 T: SvgfReservoirGI[width * height];
 *     2 the previous normals (12 B per pixel), 3 the previous ids (4 B per pixel).  host_bytes must be the plane's size exactly.
 *   svgf_restir_gi_destroy waits for the device first; NULL is accepted.
 *   As in svgf_restir.h the history is decided on the device: H is read as history (launch 1) and written as the frame's result
 *   (launch 2), every frame is the same two launches and a captured frame replays with the history of the moment.
 *
 * ONE FRAME.  svgf_restir_gi_frame is exactly TWO launches on `stream`, one thread per pixel; no allocation, copy, memset, host wait
 *   or atomic; nothing passes between workgroups; legal under stream capture (two kernel nodes).  light: centre, edge_u and edge_v
 *   are read (for L; `samples` is not).  Exactly one of gbuffer_dev (AoS texels) and planes (normal, position, geom_id) is given, of
 *   the state's size.  motion_prev_coord_dev: SVGF_MOTION_PREV_COORD_F32, or NULL = no temporal reuse this frame.  sp: seed and frame.
 *   Errors, all before any device work: SVGF_ERR_INVALID_ARG for a NULL state, light, gp, sp or out_I_dev; a light field that is not
 *   finite; both targets or neither; planes without normal / position / geom_id; candidates outside 1..8; temporal other than 0 / 1;
 *   m_cap not finite or < 1; neighbours outside 0..8; radius not finite, < 1 or > 65536; normal_min_dot not finite; jacobian_max not
 *   finite or < 1; ambient not finite or negative; shadow_secondary other than 0 / 1; a state on another device than the scene's.
 *   SVGF_ERR_UNSUPPORTED for a tree deeper than SVGF_SCENE_MAX_DEPTH.
 *
 *   Launch 1, k_restir_gi_initial.  A miss (id < 0) or emissive(id): T[p] = EMPTY.  Otherwise
 *     r = EMPTY; for c = 0 .. candidates - 1: (xs, ns, L) = bounce(p, c);
 *       update(r, { xs, ns, L, g_p(xs, ns) }, lum(L), lum(L), 1, hash(8192 + c));
 *     finish(r); s = EMPTY; take(s, r, 0).
 *     If temporal == 1 and a plane is given: row f27's tap on bits - (mx, my) = the plane at p; fx = floorf(mx + 0.5f),
 *       fy = floorf(my + 0.5f); ON SCREEN iff fx >= 0 && fx < (float)width && fy >= 0 && fy < (float)height; q = (int)fy * width +
 *       (int)fx; ACCEPTED iff prev_id[q] == id && n.prev_n[q] >= normal_min_dot.  Then take'(s, H[q], fminf(H[q].M, m_cap * r.M), hash(8224)).
 *     finish(s); T[p] = s.
 *   Launch 2, k_restir_gi_spatial_shade.  A miss or an emitter (emitters carry no indirect light, row f18): I = 0, H[p] = EMPTY.  Otherwise
 *     s = EMPTY; take(s, T[p], 0); for k = 0 .. neighbours - 1:
 *       ox = (int)floorf(((2 hash(8256 + 4k) - 1) * radius) + 0.5f), oy the same from 8257 + 4k; the neighbour (x + ox, y + oy) must be
 *       on screen and not p, have THIS frame's geomId equal to id and THIS frame's normal n_q with n.n_q >= normal_min_dot; then
 *       take'(s, T[q], T[q].M, hash(8258 + 4k)).
 *     finish(s).  vis = 1; if the selected sample is foreign and s.W > 0 and !visible(pos, s.xs): vis = 0.
 *     I_c = vis * (s.L_c * s.W)  (0 where s.valid == 0).  H[p] = s.  Every pixel: prev_n[p] = n, prev_id[p] = id.
 *   With candidates = 1 and no reuse, W is 1.0f exactly wherever lum(L) > 0, and I is svgf_trace_draw_split's I at bounce_samples = 1,
 *   noise = 0 on bits.
 */
#ifndef SVGF_RESTIR_GI_H_
#define SVGF_RESTIR_GI_H_

#include "svgf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVGF_RESTIR_GI_MAX_CANDIDATES 8
#define SVGF_RESTIR_GI_MAX_NEIGHBOURS 8
#define SVGF_RESTIR_GI_MAX_ID         ((1 << 20) - 1)

typedef struct SvgfReservoirGI {
    float xs[3], M;
    float ns[3], W;
    float L[3], phat;
    float g;
    int   valid;          /* 0 / 1 */
    int   zero[2];
} SvgfReservoirGI;        /* 64 bytes, read and written as four 16-byte words */

typedef struct SvgfRestirGIParams {
    int   candidates;       /* 1..8 */
    int   temporal;         /* 0 / 1 */
    float m_cap;            /* >= 1; 20 */
    int   neighbours;       /* 0..8 */
    float radius;           /* >= 1 pixels; 30 */
    float normal_min_dot;   /* 0.9 */
    float jacobian_max;     /* >= 1; 10 */
    float ambient;          /* svgf_trace_draw's; 0.15 */
    int   shadow_secondary; /* svgf_trace_draw's; 0 / 1 */
} SvgfRestirGIParams;

typedef struct SvgfRestirGIInfo {
    int width, height, n_ids, launches;
    unsigned long long device_bytes;
} SvgfRestirGIInfo;

typedef struct svgf_restir_gi svgf_restir_gi;

int  svgf_restir_gi_create(const svgf_scene *scene, int width, int height, svgf_restir_gi **out);
int  svgf_restir_gi_reset(svgf_restir_gi *state, void *stream);
void svgf_restir_gi_destroy(svgf_restir_gi *state);
int  svgf_restir_gi_info(const svgf_restir_gi *state, SvgfRestirGIInfo *out);
int  svgf_restir_gi_read(const svgf_restir_gi *state, int which, void *host_dst, unsigned long long host_bytes);
int  svgf_restir_gi_frame(svgf_restir_gi *state, const SvgfSceneLight *light, const void *gbuffer_dev /* or NULL */,
                          const SvgfPlanarGBuffer *planes /* or NULL */, const void *motion_prev_coord_dev /* or NULL */,
                          const SvgfRestirGIParams *gp, const SvgfSynthParams *sp, void *out_I_dev, void *stream);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_trace_version. */
int  svgf_restir_gi_version(void);

#ifdef __cplusplus
}
#endif

#endif
