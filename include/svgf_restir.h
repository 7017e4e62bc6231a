/* svgf_restir.h — row f27: many-light direct lighting by reservoir resampling (libsvgf_restir.so).
 *
 * Every draw of rows f14 to f26 shades from ONE analytic light.  This library lights a G-buffer of a resident scene from a TABLE of
 * up to 65 536 parallelogram lights at one final shadow ray per pixel: spatiotemporal reservoir resampling (Bitterli et al. 2020,
 * "ReSTIR DI"), the BIASED combination of the paper (neighbours' and history samples are taken without retesting visibility at the
 * pixel that takes them: penumbrae come out slightly darker than the truth; the unbiased, visibility-retesting combination is not here).
 * It writes the demodulated direct term D in the layout svgf_trace_compose and svgf_denoise take (packed rgb float), and
 * svgf_lights_draw_all writes the truth it is scored against.  It links against libsvgf_hip.so alone, reaches the scene through
 * svgf_scene_view and nothing else, and reads no environment variable.  INTEGRATION.md 5u has the frame loop.
 *
 * THE LIGHT TABLE.  SvgfLight is 48 bytes: centre, the two half-edges of a parallelogram around it (both zero: a point light), and a
 *   power per channel.  svgf_lights_create(device, host_lights, n, &table): n in 1..SVGF_RESTIR_MAX_LIGHTS, every field finite,
 *   otherwise SVGF_ERR_INVALID_ARG before any device work (*out cleared on every refusal); then one allocation and one upload
 *   (SVGF_ERR_NO_DEVICE, SVGF_ERR_OOM, SVGF_ERR_HIP): not under capture.  svgf_lights_size is n (SVGF_ERR_INVALID_ARG for NULL),
 *   svgf_lights_destroy takes NULL.  A table belongs to no scene.
 *
 * Notation - float32, one rounding per operation, no contraction; a.b = (a_0 b_0 + a_1 b_1) + a_2 b_2; hash(k) = svgf_synth_render's
 * hash(seed, frame, p, k) of pixel p = y * width + x; pos, n, id = the G-buffer's position, normal and geomId at p.
 *   F_j,c(pos, n): tl = centre_j - pos; dist2 = tl.tl; dl = sqrtf(dist2); lam = fmaxf((tl / dl).n, 0);
 *     F_j,c = (power_j,c * lam) / (4 + dist2)          - svgf_scene_draw's light term with power_j,c in 30's place, on bits
 *   phat_j(pos, n) = lum(F_j,0, F_j,1, F_j,2), the denoiser's luminance: (float)((0.2126 * (double)r + 0.7152 * (double)g) + 0.0722 * (double)b)
 *   ray(pos, j, u, v): row f16's shadow sample towards L = (centre_j + (2u - 1) edge_u_j) + (2v - 1) edge_v_j: q = L - pos, dl = sqrtf(q.q);
 *     !(dl > 0) forms no ray and is unoccluded; otherwise d = q / dl, t_lo = 2^-10 fmaxf(1, dl), t_hi = dl - t_lo, OCCLUDED iff an
 *     occluder of svgf_scene_draw_shadowed counts on (pos, d) inside (t_lo, t_hi).
 *   A reservoir r is { j, u, v, M, W, phat } and, while it is being filled, w_sum; EMPTY is j = -1, everything else 0.
 *   update(r, j, u, v, phat, w, M_s, xi): w = (w > 0) ? w : 0 (a NaN weighs nothing); before = r.w_sum; r.w_sum = r.w_sum + w;
 *     r.M = r.M + M_s; the sample is selected iff w > 0 && (before == 0 || xi * r.w_sum < w); on selection r.j, r.u, r.v, r.phat are set.
 *   finish(r): r.W = (r.j >= 0 && r.phat > 0) ? r.w_sum / (r.M * r.phat) : 0.
 *   take(s, r, xi) for a stored reservoir r of THIS pixel: update(s, r.j, r.u, r.v, r.phat, (r.phat * r.W) * r.M, r.M, xi).
 *   take'(s, r, M', xi) for a reservoir r of ANOTHER pixel or frame: phat' = phat_{r.j}(pos, n) AT THIS PIXEL where 0 <= r.j < N, else 0;
 *     update(s, r.j, r.u, r.v, phat', (phat' * r.W) * M', M', xi).
 *   emissive(id): the state's table from geomId to emittance says > 0 (ids outside the table: 0).
 *
 * HASH STREAMS (none collides with a draw's: those use 0..4 for the noise, 8..135 for row f16's shadow samples and 139..1274 plus a
 * few above for the bounces of rows f17 to f23 (svgf_path.h), all far below 4096):
 *   8, 9                 u, v of the light point of every candidate of the pixel (row f16's sample 0)
 *   4096 + c             candidate c's light index,            c = 0..31
 *   4128 + c             candidate c's selection draw
 *   4160                 the history sample's selection draw
 *   4192 + 4k, + 1, + 2  neighbour k's offset in x, in y, and its selection draw,   k = 0..7
 *   svgf_lights_draw_all: 8 + 2s, 9 + 2s for sample s, for every light.
 *
 * THE STATE.  svgf_restir_create(scene, width, height, &state): one allocation for one frame size - a history reservoir plane H, a
 *   scratch plane T (32 bytes per pixel each), the previous frame's normal and geomId planes, and a table from geomId to emittance
 *   built from the view (a primitive's id is geom_ids[k] or k, its emittance the primitive's; a triangle's id is tri_ids[i], its
 *   emittance 0).  SVGF_ERR_INVALID_ARG for NULL, a size <= 0, an id that is negative or above SVGF_RESTIR_MAX_ID, or one id naming
 *   surfaces of differing emittance; SVGF_ERR_UNSUPPORTED for width * height >= 2^31 / 16.  Allocates, copies, launches the reset and
 *   synchronises: not under capture.  The scene must outlive the state.
 *   svgf_restir_reset(state, stream): ONE launch; H becomes EMPTY everywhere and the previous ids -1, so the next frame finds no history.
 *   svgf_restir_read(state, which, host_dst, host_bytes): blocking (tests, debugging).  0 H, 1 T: SvgfReservoir[width * height];
 *     2 the previous normals (12 B per pixel), 3 the previous ids (4 B per pixel).  host_bytes must be the plane's size exactly.
 *   svgf_restir_destroy waits for the device first; NULL is accepted.
 *   The history is decided on the device, never by a host flag: the same plane H is read as history (launch 1) and written as the
 *   frame's result (launch 2), so every frame is the same two launches, no parity lives on the host and a captured frame replays
 *   with the history of the moment.
 *
 * ONE FRAME.  svgf_restir_frame is exactly TWO launches on `stream`, one thread per pixel; no allocation, copy, memset or host wait;
 *   legal under stream capture (two kernel nodes).  Exactly one of gbuffer_dev (AoS texels) and planes (normal, position, geom_id) is
 *   given, of the state's size.  motion_prev_coord_dev: SVGF_MOTION_PREV_COORD_F32 (what svgf_motion_reproject writes, from the
 *   G-buffer or from svgf_deform_prev_positions), or NULL = no temporal reuse this frame.  sp: seed and frame are read.  N = the table's size.
 *   Errors, all before any device work: SVGF_ERR_INVALID_ARG for a NULL state, table, rp, sp or out_D_dev; both targets or neither;
 *   planes without normal / position / geom_id; candidates outside 1..32; temporal other than 0 / 1; m_cap not finite or < 1; neighbours
 *   outside 0..8; radius not finite, < 1 or > 65536; normal_min_dot not finite; ambient not finite or negative; a table on another
 *   device than the scene's.  SVGF_ERR_UNSUPPORTED for a tree deeper than SVGF_SCENE_MAX_DEPTH.
 *
 *   Launch 1, k_restir_initial.  A miss (id < 0) or emissive(id): T[p] = EMPTY.  Otherwise
 *     u = hash(8), v = hash(9); r = EMPTY; for c = 0 .. candidates - 1:
 *       j = min((int)(hash(4096 + c) * (float)N), N - 1); update(r, j, u, v, phat_j, phat_j * (float)N, 1, hash(4128 + c));
 *     finish(r); if r.j >= 0 && r.W > 0 and ray(pos, r.j, r.u, r.v) is occluded: r.W = 0.
 *     s = EMPTY; take(s, r, 0).
 *     If temporal == 1 and a plane is given: (mx, my) = the plane at p; fx = floorf(mx + 0.5f), fy = floorf(my + 0.5f); the tap is ON
 *       SCREEN iff fx >= 0 && fx < (float)width && fy >= 0 && fy < (float)height (NaN and +-inf are not); q = (int)fy * width + (int)fx;
 *       it is ACCEPTED iff prev_id[q] == id && n.prev_n[q] >= normal_min_dot (a NaN normal refuses).  Then
 *       take'(s, H[q], fminf(H[q].M, m_cap * r.M), hash(4160)).
 *     finish(s); T[p] = s.
 *   Launch 2, k_restir_spatial_shade.  A miss: D = 0.  An emitter: D_c = its emittance.  Either: H[p] = EMPTY.  Otherwise
 *     s = EMPTY; take(s, T[p], 0); for k = 0 .. neighbours - 1:
 *       ox = (int)floorf(((2 hash(4192 + 4k) - 1) * radius) + 0.5f), oy the same from 4193 + 4k; the neighbour (x + ox, y + oy) must be on
 *       screen and not p, have THIS frame's geomId equal to id and THIS frame's normal n_q with n.n_q >= normal_min_dot; then
 *       take'(s, T[q], T[q].M, hash(4194 + 4k)).      (biased: no visibility retest)
 *     finish(s).  s.j < 0: D_c = ambient.  Otherwise vis = 1, and if s.W > 0 and ray(pos, s.j, s.u, s.v) is occluded vis = 0;
 *       D_c = ambient + vis * (F_{s.j},c * s.W).
 *     H[p] = s.  Every pixel: prev_n[p] = n, prev_id[p] = id.
 *   With N = 1, power = 30, candidates = 1 and no reuse, W is 1.0f exactly and D is svgf_trace_draw_split's D at noise = 0 on bits.
 *
 * THE TRUTH.  svgf_lights_draw_all(scene, table, gbuffer | planes, width, height, samples 1..64, sp, ambient, out_D, stream): ONE launch.
 *   A miss: D = 0.  A pixel whose id is a primitive's with emittance > 0 (the first primitive of that id): D_c = that emittance.
 *   Otherwise acc = 0; for j = 0 .. N - 1 in order: vis_j = (float)(the samples s with ray(pos, j, hash(8 + 2s), hash(9 + 2s)) unoccluded)
 *   / (float)samples; acc_c = acc_c + F_j,c * vis_j (a light with lam == 0 casts no ray: its term is 0 whatever vis); D_c = ambient + acc_c.
 *   Errors: as svgf_restir_frame's that apply, a size <= 0, samples outside 1..64.
 */
#ifndef SVGF_RESTIR_H_
#define SVGF_RESTIR_H_

#include "svgf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVGF_RESTIR_MAX_LIGHTS     65536
#define SVGF_RESTIR_MAX_CANDIDATES 32
#define SVGF_RESTIR_MAX_NEIGHBOURS 8
#define SVGF_RESTIR_MAX_ID         ((1 << 20) - 1)

typedef struct SvgfLight {
    float centre[3];
    float edge_u[3];
    float edge_v[3];
    float power[3];       /* 30, 30, 30 is svgf_scene_draw's light */
} SvgfLight;              /* 48 bytes */

typedef struct SvgfReservoir {
    int   j;              /* the light, or -1: empty */
    float u, v;           /* the point on it */
    float M, W, phat;
    int   zero[2];
} SvgfReservoir;          /* 32 bytes, read and written as two 16-byte words */

typedef struct SvgfRestirParams {
    int   candidates;     /* 1..32 */
    int   temporal;       /* 0 / 1 */
    float m_cap;          /* >= 1; 20 */
    int   neighbours;     /* 0..8 */
    float radius;         /* >= 1 pixels; 30 */
    float normal_min_dot; /* 0.9 */
} SvgfRestirParams;

typedef struct SvgfRestirInfo {
    int width, height, n_ids, launches;
    unsigned long long device_bytes;
} SvgfRestirInfo;

typedef struct svgf_lights svgf_lights;
typedef struct svgf_restir svgf_restir;

int  svgf_lights_create(int device, const SvgfLight *host_lights, int n, svgf_lights **out);
void svgf_lights_destroy(svgf_lights *table);
int  svgf_lights_size(const svgf_lights *table);

int  svgf_restir_create(const svgf_scene *scene, int width, int height, svgf_restir **out);
int  svgf_restir_reset(svgf_restir *state, void *stream);
void svgf_restir_destroy(svgf_restir *state);
int  svgf_restir_info(const svgf_restir *state, SvgfRestirInfo *out);
int  svgf_restir_read(const svgf_restir *state, int which, void *host_dst, unsigned long long host_bytes);
int  svgf_restir_frame(svgf_restir *state, const svgf_lights *table, const void *gbuffer_dev /* or NULL */,
                       const SvgfPlanarGBuffer *planes /* or NULL */, const void *motion_prev_coord_dev /* or NULL */,
                       const SvgfRestirParams *rp, const SvgfSynthParams *sp, float ambient, void *out_D_dev, void *stream);
int  svgf_lights_draw_all(const svgf_scene *scene, const svgf_lights *table, const void *gbuffer_dev /* or NULL */,
                          const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height, int samples, const SvgfSynthParams *sp,
                          float ambient, void *out_D_dev, void *stream);
/* (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR of the svgf.h this library was compiled against, as svgf_trace_version. */
int  svgf_restir_version(void);

#ifdef __cplusplus
}
#endif

#endif
