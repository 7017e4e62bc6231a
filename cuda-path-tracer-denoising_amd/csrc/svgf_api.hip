// svgf_api.hip — host side of libsvgf_hip.so: context, history rotation, per-frame kernel sequence, C ABI.
//
// Mirrors the host sequence of reference denoise() (src/denoise.cu:349-402) with two structural changes that
// do not alter results:
//   * no device-to-device copies: the five per-frame cudaMemcpy's (src/denoise.cu:366,391,396-398) become
//     index rotation over ping-pong planes;
//   * variance is never updated in place: each a-trous level reads {colour,variance} plane A and writes plane B,
//     which is the "snapshot" semantics the parity contract fixes (SURVEY.md §7 hard parts, §8c).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "../../include/svgf.h"
#include "svgf_atrous_geometry.h"

#define SVGF_MAX_KERNELS_PER_FRAME (SVGF_MAX_LEVELS + 4)
static_assert(SVGF_MOTION_PREV_COORD_F32 == SVGF_MOTION_FMT_COORD && SVGF_MOTION_DELTA_F32 == SVGF_MOTION_FMT_D32 &&
              SVGF_MOTION_DELTA_F16 == SVGF_MOTION_FMT_D16, "include/svgf.h and svgf_kernels.h name the same motion formats");
// the prepare pass of the non-temporal mode fused into the first level (svgf_atrous_prepare_fused.hip, FUSED = 3): on by default
// where the first level runs the lane kernel anyway (measured: profiles/r04_exp_prepare_fused.log)
static const bool kPrepareFusedByDefault = true;
#ifdef SVGF_BUILD_EXPERIMENTS
// a row of the fused temporal + first-level kernel against a row of the plain lane kernel, as measured at 1920x1080 (DESIGN.md
// 5.8, profiles/r04_exp_fused_*.log: 176 us in its last version against 42.7 for the plain level, i.e. the fused kernel LOSES to
// temporal pass + level, 55 + 46 us): with this factor the automatic choice never fuses; kernel_variant 6 forces it
static const double kFusedRowFactor = 4.1;
// temporal frames: only the G-buffer split fused into the first level (FUSED = 4); a measured loss, off unless svgf_exp_set("split_fused", 1)
static const bool kSplitFusedByDefault = false;
#endif

struct svgf_ctx {
    int device, W, H;
    size_t n;
    float4 *cv[6];         // colour + variance planes: history, source, destination of a level (roles rotate).  [3..5]: the second
                           // set of a PIPELINED context (see `pipelined`), allocated when the first frame asks for it
    float *vp[6];          // zero-margined (W+2) x (H+2) copies of cv[k].w: what the step-16/32 levels take their 3x3 variance pre-blur from
    unsigned vp_valid;     // bit k: vp[k] holds the variance of cv[k]
    // Frame pipeline (SvgfParams::inputs_ready, round 5).  A frame's temporal pass needs of the previous frame only what exists
    // once the level feeding the colour history has run (level 1 with the reference's defaults); levels 2-5 of frame n and the
    // temporal pass + level 1 of frame n+1 are independent.  A pipelined context runs even frames on pipe[0] with planes 0-2 and
    // odd frames on pipe[1] with planes 3-5; ev_hist[q] (recorded behind the level that writes the history of a frame of parity q)
    // is all that the other stream's next temporal pass waits for, and the caller's stream waits for ev_done[q] at the end of the
    // call.  The kernels of two consecutive frames then share the chip: one frame's level tails, launch gaps and opening bursts
    // lie under the other's tap rows (two INDEPENDENT sequences on two streams: +9-10 % in aggregate,
    // profiles/r05_exp_two_sequences.log — the ceiling of this).
    int pipelined;         // the second plane set, the internal streams and the events exist (svgf_create_ex / svgf_enable_pipeline)
    int piped_mode;        // frames alternate between the two plane sets (every frame of the context, once on)
    int pipe_serial;       // the probe at enable time found the two internal streams on ONE hardware queue: the promise is refused
    int ever_captured;     // a frame of this context has been recorded into a graph: promised frames order themselves behind `stream`
    hipStream_t pipe[2];
    // an event of the pipeline: recorded at least once since the last reset (`valid`), and the stream-capture id it was last recorded
    // under (0: eagerly).  Only pipe_record / pipe_wait / pipe_reset touch these (the per-frame disarm of ev_tdone aside).
    struct PipeEvent { hipEvent_t ev; int valid; unsigned long long cap; };
    PipeEvent ev_hist[2], ev_done[2];
    PipeEvent ev_tdone[2];    // planar frames: behind the temporal pass (the last reader of the PREVIOUS frame's G-buffer planes, which the next producer overwrites)
    hipEvent_t ev_in;
    int last_modulated;       // the last frame's last level read the (single) albedo plane
    long long pipe_frames;     // frames since the context became pipelined (parity = stream and plane set)
    int use_vplane;        // 0 only for A/B measurements (experiments build: svgf_exp_set("no_variance_plane", 1) before svgf_create)
    void *dump;            // 4 KB of scrap for the fused kernel (TemporalArgs::dump)
    char *arena;           // the one allocation cv[], nrm[], gid[], mom[], hlen[], pos[] and dump are carved from
    size_t arena_bytes;
    float4 *tp[2];         // cross-level reuse of the geometric terms: four terms per pixel, written by level L for level L+1 (lane kernels
                           // only, svgf_atrous_lane_reuse.hip; experiments build); allocated by svgf_create when use_reuse is set
    int use_split_fused;   // experiments build, svgf_exp_set("split_fused", 1): the G-buffer split of temporal frames in the first level's loaders
    int use_reuse;         // experiments build, svgf_exp_set("reuse", 1) before svgf_create: measured a loss, profiles/r04_ab_reuse_*.log
    int n_cu;              // compute units of the context's device (launch-geometry cost model of the kernel choice)
    signed char lane_cheaper[8];   // per log2(step): -1 not evaluated yet, 1 the lane kernel's estimate is the lower one
    signed char fuse_pays;         // -1 not evaluated yet, 1: the fused temporal + first-level kernel is the cheaper way through both
#ifdef SVGF_BUILD_EXPERIMENTS
    double est_lane_us[8], est_strip_us[8];   // per log2(step): the two estimates lane_cheaper[] was decided from
    // the a-trous levels of the last frame (svgf_exp_level_kernels), a copy of its plan: kernel (K_FUSED ..), step, and whether the
    // automatic choice compared the estimates of that step
    int lk_n;
    int lk_kind[SVGF_MAX_LEVELS], lk_step[SVGF_MAX_LEVELS], lk_asked[SVGF_MAX_LEVELS];
#endif
    float *nrm[2];
    int *gid[2];
    float *pos[2];
    float *albedo;         // planar path only (svgf_planar_gbuffer): packed float3 albedo * ialbedo, allocated on first use
    float2 *mom[2];
    int *hlen[2];
    int hist;      // cv index holding the colour history
    int acc;       // cv index the last temporal pass wrote
    int cur;       // mom/hlen index holding the history the next frame reads
    int gcur;      // nrm/gid/pos index holding the previous frame's planes
    float view_prev[16];   // column-major; identity until the first frame (reference src/denoise.cu:15)
    // svgf_set_history_clamp: configuration, not history (svgf_reset keeps it); read by plan_frame when a frame is enqueued
    int clamp_radius;      // 0 = off
    float clamp_k;
    // svgf_set_firefly_filter: configuration like the clamp; temporal and non-temporal frames alike run on F(in_rgb)
    int firefly_rank;      // 0 = off
    float firefly_scale;
    // svgf_set_object_motion: configuration like the clamp; the pointer and count are read by plan_frame, the table by the temporal kernel
    const float *xf_dev;   // null or xf_n == 0: off
    int xf_n;
    // svgf_set_output_taa: configuration like the clamp (svgf_reset keeps it); the planes exist from the first call that turns it on
    float taa_alpha;       // 0 = off
    float taa_k;
    float *taa_pre;        // packed rgb: the frame's image, written by the last level / the pass-through copy in place of `out`
    float4 *taa_hist[2];   // {output, geomId bits}: the previous frame's and the one being written
    int taa_cur;           // taa_hist index the next frame reads
    int taa_valid;         // taa_hist[taa_cur] holds the last frame's output (history, not configuration: svgf_reset clears it)
    // state capture for tests
    int capture;
    float4 *cv_capture;
    // staging for svgf_denoise_host
    float *st_in, *st_out; void *st_g;
    // profiling
    int prof_frames;       // 0 = off
    int prof_stride;       // bracket every prof_stride-th frame
    long long frame_no;    // frames denoised since profile_enable
    long long prof_count;  // frames recorded since enable
    hipEvent_t *ev;        // prof_frames * SVGF_MAX_KERNELS_PER_FRAME * 2
    int *ev_kind;          // prof_frames * SVGF_MAX_KERNELS_PER_FRAME
    int *ev_n;             // prof_frames
    char err[512];
};

static char g_create_err[512] = "";
static int step_log2(int step) { const int l = atrous_step_log2(step); return l < 7 ? l : 7; }      // index of lane_cheaper[] / est_*_us[]

#define HIPC(ctx, call)                                                                              \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) {                                                                     \
            snprintf((ctx)->err, sizeof((ctx)->err), "%s failed: %s (%s:%d)", #call,                 \
                     hipGetErrorString(e__), __FILE__, __LINE__);                                    \
            return SVGF_ERR_HIP;                                                                     \
        }                                                                                            \
    } while (0)

// Entry preamble: a null context is an invalid argument; the call runs on the context's device (SvgfDeviceGuard) or fails.
#define SVGF_ENTER(ctx)                                                                              \
    if (!(ctx)) return SVGF_ERR_INVALID_ARG;                                                         \
    SvgfDeviceGuard dev_guard((ctx)->device);                                                        \
    if (!dev_guard.ok) { snprintf((ctx)->err, sizeof((ctx)->err), "hipSetDevice(%d) failed", (ctx)->device); return SVGF_ERR_HIP; }

// ---- host copy of the view-matrix construction (reference GetViewMatrix src/denoise.cu:342-347) -------------
// inverse of the column-major matrix [right|0, up|0, view|0, position|1] by 2x2-minor (cofactor) expansion in the
// operation order of glm 0.9.6.3 (external/include/glm/detail/type_mat4x4.inl:37-92), so fp32 rounding matches.
static void view_matrix_from_camera(const SvgfCamera *cam, float *out)
{
    float m[16];
    for (int r = 0; r < 3; r++) {
        m[0 + r] = cam->right[r]; m[4 + r] = cam->up[r]; m[8 + r] = cam->view[r]; m[12 + r] = cam->position[r];
    }
    m[3] = m[7] = m[11] = 0.0f; m[15] = 1.0f;
    auto M = [&](int c, int r) { return m[c * 4 + r]; };
    float fac[6][4];
    const int rows[6][2] = { {2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1} };
    for (int k = 0; k < 6; k++) {
        const int ra = rows[k][0], rb = rows[k][1];
        const float a = M(2, ra) * M(3, rb) - M(3, ra) * M(2, rb);
        const float b = M(1, ra) * M(3, rb) - M(3, ra) * M(1, rb);
        const float c = M(1, ra) * M(2, rb) - M(2, ra) * M(1, rb);
        fac[k][0] = a; fac[k][1] = a; fac[k][2] = b; fac[k][3] = c;
    }
    float vec[4][4];
    for (int r = 0; r < 4; r++) { vec[r][0] = M(1, r); vec[r][1] = vec[r][2] = vec[r][3] = M(0, r); }
    const int comb[4][6] = { {1, 0, 2, 1, 3, 2}, {0, 0, 2, 3, 3, 4}, {0, 1, 1, 3, 3, 5}, {0, 2, 1, 4, 2, 5} };
    float inv[16];
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) {
            float t = vec[comb[c][0]][r] * fac[comb[c][1]][r] - vec[comb[c][2]][r] * fac[comb[c][3]][r];
            t = t + vec[comb[c][4]][r] * fac[comb[c][5]][r];
            inv[c * 4 + r] = ((c + r) & 1) ? t * -1.0f : t * 1.0f;
        }
    const float d0 = m[0] * inv[0], d1 = m[1] * inv[4], d2 = m[2] * inv[8], d3 = m[3] * inv[12];
    const float det = (d0 + d1) + (d2 + d3);
    const float rdet = 1.0f / det;
    for (int k = 0; k < 16; k++) out[k] = inv[k] * rdet;
}

#ifdef SVGF_BUILD_EXPERIMENTS
// ---- tuning table of the experiments build (libsvgf_hip_exp.so): name -> int, process-wide.  The product build has neither the
// table nor the entry point: SVGF_TUNE() is its default there and no environment variable is read anywhere in the library. ----
namespace {
struct ExpEntry { char name[32]; int value; };
ExpEntry g_exp[64];
int g_exp_n = 0;
std::mutex g_exp_mu;
}  // namespace
int svgf_exp_get(const char *name, int dflt)
{
    std::lock_guard<std::mutex> lk(g_exp_mu);
    for (int k = 0; k < g_exp_n; k++) if (!strcmp(g_exp[k].name, name)) return g_exp[k].value;
    return dflt;
}
extern "C" int svgf_exp_set(const char *name, int value)
{
    if (!name || strlen(name) >= sizeof(g_exp[0].name)) return SVGF_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_exp_mu);
    for (int k = 0; k < g_exp_n; k++) if (!strcmp(g_exp[k].name, name)) { g_exp[k].value = value; return SVGF_OK; }
    if (g_exp_n >= 64) return SVGF_ERR_OOM;
    strcpy(g_exp[g_exp_n].name, name);
    g_exp[g_exp_n++].value = value;
    return SVGF_OK;
}
extern "C" int svgf_exp_clear(void) { std::lock_guard<std::mutex> lk(g_exp_mu); g_exp_n = 0; return SVGF_OK; }
#endif

extern "C" int svgf_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }
// 1: this library was built with -DSVGF_BUILD_EXPERIMENTS (parked kernel variants 5 / 6, tuning table); the product build says 0
extern "C" int svgf_build_has_experiments(void)
{
#ifdef SVGF_BUILD_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}
extern "C" int svgf_params_sizeof(void) { return (int)sizeof(SvgfParams); }

extern "C" int svgf_params_default(SvgfParams *p)
{
    if (!p) return SVGF_ERR_INVALID_ARG;
    memset(p, 0, sizeof(*p));
    p->temporal_enable = 0; p->spatial_enable = 0;            // reference src/main.cpp:50-52
    p->color_alpha = 0.2f; p->moment_alpha = 0.2f;            // :53-54
    p->blur_variance = 1;                                     // :55
    p->sigma_l = 0.45f; p->sigma_x = 0.35f; p->sigma_n = 0.2f; // :56-58
    p->atrous_nlevel = 5; p->history_level = 1;               // :59-60
    p->sepcolor = 0; p->addcolor = 0; p->right_view_option = 0;
    return SVGF_OK;
}

// The context's planes live in ONE allocation (the arena), each with kPlanePad bytes in front of and behind its W*H elements:
//   * the fused temporal + first-level kernel reads the 3x3 window around a reprojected position as three 3-element row
//     pieces, and a piece that starts one element left of an image row's first pixel (or ends one right of its last) must stay
//     inside memory the context owns at the plane's two ends;
//   * it addresses every plane as arena + 32-bit byte offset (svgf_atrous_lane_impl.h: LaneFused), which needs them within
//     4 GiB of one base — true by construction up to the sizes atrous_fused_supported() admits.
static const size_t kPlanePad = 128, kPlaneAlign = 4096;
static size_t plane_span(size_t bytes) { return (bytes + 2 * kPlanePad + kPlaneAlign - 1) / kPlaneAlign * kPlaneAlign; }
static void *plane_carve(svgf_ctx *c, size_t *cursor, size_t bytes)
{
    char *p = c->arena + *cursor + kPlanePad;
    *cursor += plane_span(bytes);
    return p;
}

// the profiler's arrays and the first n_events of its events
static void profile_free(svgf_ctx *c, long long n_events)
{
    for (long long k = 0; c->ev && k < n_events; k++) (void)hipEventDestroy(c->ev[k]);
    free(c->ev); free(c->ev_kind); free(c->ev_n);
    c->ev = nullptr; c->ev_kind = nullptr; c->ev_n = nullptr;
}

static void free_all(svgf_ctx *c)
{
    if (c->arena) (void)hipFree(c->arena);          // cv[], nrm[], gid[], mom[], hlen[], pos[], dump
    for (int k = 0; k < 6; k++) if (c->vp[k]) (void)hipFree(c->vp[k]);
    for (int k = 3; k < 6; k++) if (c->cv[k]) (void)hipFree(reinterpret_cast<char *>(c->cv[k]) - kPlanePad);
    for (int q = 0; q < 2; q++) {
        if (c->pipe[q]) (void)hipStreamDestroy(c->pipe[q]);
        for (svgf_ctx::PipeEvent *e : { &c->ev_hist[q], &c->ev_done[q], &c->ev_tdone[q] }) if (e->ev) (void)hipEventDestroy(e->ev);
    }
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    for (int k = 0; k < 2; k++) if (c->tp[k]) (void)hipFree(c->tp[k]);
    if (c->albedo) (void)hipFree(c->albedo);
    if (c->taa_pre) (void)hipFree(c->taa_pre);
    for (int k = 0; k < 2; k++) if (c->taa_hist[k]) (void)hipFree(c->taa_hist[k]);
    if (c->cv_capture) (void)hipFree(c->cv_capture);
    if (c->st_in) (void)hipFree(c->st_in);
    if (c->st_out) (void)hipFree(c->st_out);
    if (c->st_g) (void)hipFree(c->st_g);
    profile_free(c, (long long)c->prof_frames * SVGF_MAX_KERNELS_PER_FRAME * 2);
}

// ---- the pipeline's events: record under a capture id, wait if recorded under the same one, forget everything ----
static hipError_t pipe_record(svgf_ctx::PipeEvent &e, hipStream_t s, unsigned long long cap_id)
{
    const hipError_t rc = hipEventRecord(e.ev, s);
    if (rc == hipSuccess) { e.valid = 1; e.cap = cap_id; }
    return rc;
}
// (an event recorded under another capture, or eagerly while the waiting frame is captured, or vice versa, is not waited for: such
// frames are ordered through the caller's stream)
static bool pipe_live(const svgf_ctx::PipeEvent &e, unsigned long long cap_id) { return e.valid && e.cap == cap_id; }
static hipError_t pipe_wait(hipStream_t s, const svgf_ctx::PipeEvent &e, unsigned long long cap_id) { return pipe_live(e, cap_id) ? hipStreamWaitEvent(s, e.ev, 0) : hipSuccess; }
static void pipe_reset(svgf_ctx *c)
{
    c->pipe_frames = 0;
    for (svgf_ctx::PipeEvent *e : { &c->ev_hist[0], &c->ev_hist[1], &c->ev_done[0], &c->ev_done[1], &c->ev_tdone[0], &c->ev_tdone[1] }) { e->valid = 0; e->cap = 0; }
}

static int zero_state(svgf_ctx *c)
{
    for (int k = 0; k < 6; k++) if (c->cv[k]) HIPC(c, hipMemset(c->cv[k], 0, c->n * sizeof(float4)));
    for (int k = 0; k < 6; k++) if (c->vp[k]) HIPC(c, hipMemset(c->vp[k], 0, (size_t)(c->W + 2) * (c->H + 2) * sizeof(float) + 64));
    c->vp_valid = 0;
    pipe_reset(c);      // (a pipelined context stays pipelined)
    for (int k = 0; k < 2; k++) {
        HIPC(c, hipMemset(c->nrm[k], 0, c->n * 3 * sizeof(float)));
        HIPC(c, hipMemset(c->gid[k], 0, c->n * sizeof(int)));
        HIPC(c, hipMemset(c->mom[k], 0, c->n * sizeof(float2)));
        HIPC(c, hipMemset(c->hlen[k], 0, c->n * sizeof(int)));
        HIPC(c, hipMemset(c->pos[k], 0, c->n * 3 * sizeof(float)));
    }
    // gcur is deliberately NOT reset: the pointers svgf_planar_gbuffer handed out (planes 1 - gcur) stay the ones the next
    // frame reads, so planar_gbuffer() -> reset() -> producer -> denoise_planar() works (both plane sets are zero again)
    c->hist = 0; c->acc = 0; c->cur = 0;
    c->taa_valid = 0;      // (the output history is dropped; svgf_set_output_taa's setting stays)
    // The clears above run on the legacy stream; a caller may enqueue the next svgf_denoise on a non-blocking stream that does not
    // order itself behind them: they are complete before svgf_create / svgf_reset return.
    HIPC(c, hipStreamSynchronize(nullptr));
    return SVGF_OK;
}

static int enable_pipeline(svgf_ctx *c);

extern "C" int svgf_create_ex(int device, int width, int height, unsigned flags, svgf_ctx **out)
{
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    if (flags & ~(unsigned)SVGF_CREATE_PIPELINED) {
        snprintf(g_create_err, sizeof(g_create_err), "svgf_create_ex: unknown flags 0x%x", flags);
        return SVGF_ERR_INVALID_ARG;
    }
    if (width <= 0 || height <= 0 || (long long)width * height > (1LL << 30)) {
        snprintf(g_create_err, sizeof(g_create_err), "svgf_create: bad size %dx%d", width, height);
        return SVGF_ERR_INVALID_ARG;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        snprintf(g_create_err, sizeof(g_create_err), "svgf_create: no usable HIP device %d (count %d, %s)", device,
                 ndev, hipGetErrorString(e));
        return SVGF_ERR_NO_DEVICE;
    }
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) {
        snprintf(g_create_err, sizeof(g_create_err), "hipSetDevice(%d) failed", device);
        return SVGF_ERR_NO_DEVICE;
    }
    svgf_ctx *c = new (std::nothrow) svgf_ctx();
    if (!c) return SVGF_ERR_OOM;
    memset(c, 0, sizeof(*c));
    c->device = device; c->W = width; c->H = height; c->n = (size_t)width * height;
    for (int k = 0; k < 16; k++) c->view_prev[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    c->use_vplane = SVGF_TUNE("no_variance_plane", 0) ? 0 : 1;
#ifdef SVGF_BUILD_EXPERIMENTS
    c->use_reuse = SVGF_TUNE("reuse", 0) ? 1 : 0;
    c->use_split_fused = SVGF_TUNE("split_fused", kSplitFusedByDefault ? 1 : 0) ? 1 : 0;
#endif
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu < 8) c->n_cu = 256;
    memset(c->lane_cheaper, -1, sizeof(c->lane_cheaper));
    c->fuse_pays = -1;
    bool ok = true;
    {
        const size_t n = c->n;
        c->arena_bytes = 3 * plane_span(n * sizeof(float4)) + 2 * (2 * plane_span(n * 3 * sizeof(float)) + 2 * plane_span(n * sizeof(int)) + plane_span(n * sizeof(float2)))
                         + plane_span(4096);
        ok = hipMalloc((void **)&c->arena, c->arena_bytes) == hipSuccess && hipMemset(c->arena, 0, c->arena_bytes) == hipSuccess;
        if (ok) {
            size_t cur = 0;
            for (int k = 0; k < 3; k++) c->cv[k] = (float4 *)plane_carve(c, &cur, n * sizeof(float4));
            for (int k = 0; k < 2; k++) {
                c->nrm[k] = (float *)plane_carve(c, &cur, n * 3 * sizeof(float));
                c->gid[k] = (int *)plane_carve(c, &cur, n * sizeof(int));
                c->mom[k] = (float2 *)plane_carve(c, &cur, n * sizeof(float2));
                c->hlen[k] = (int *)plane_carve(c, &cur, n * sizeof(int));
                c->pos[k] = (float *)plane_carve(c, &cur, n * 3 * sizeof(float));
            }
            c->dump = plane_carve(c, &cur, 4096);
            if (cur != c->arena_bytes) ok = false;         // (the size formula above and the carving below it disagree)
        }
    }
    // (+64 bytes: the step-16/32 lane kernel reads the variance plane in 16-byte pieces that may end 8 bytes behind the last margin)
    for (int k = 0; k < 3 && ok; k++) ok = hipMalloc((void **)&c->vp[k], (size_t)(width + 2) * (height + 2) * sizeof(float) + 64) == hipSuccess;
    // (the terms planes of the parked cross-level reuse: allocated here, never in the middle of a frame)
    for (int k = 0; k < 2 && ok && c->use_reuse; k++) ok = hipMalloc((void **)&c->tp[k], (size_t)(width + 64) * height * sizeof(float4)) == hipSuccess;
    int rc = ok ? zero_state(c) : SVGF_ERR_OOM;
    if (rc == SVGF_OK && (flags & SVGF_CREATE_PIPELINED)) rc = enable_pipeline(c);
    if (rc != SVGF_OK) {
        if (!ok) snprintf(g_create_err, sizeof(g_create_err), "svgf_create: hipMalloc failed for %dx%d", width, height);
        else snprintf(g_create_err, sizeof(g_create_err), "%s", c->err);
        free_all(c); delete c;
        return rc;
    }
    *out = c;
    return SVGF_OK;
}

extern "C" int svgf_create(int device, int width, int height, svgf_ctx **out) { return svgf_create_ex(device, width, height, 0u, out); }

extern "C" int svgf_destroy(svgf_ctx *c)
{
    if (!c) return SVGF_OK;
    SvgfDeviceGuard dev_guard(c->device);
    (void)hipDeviceSynchronize();
    free_all(c);
    delete c;
    return SVGF_OK;
}

extern "C" int svgf_reset(svgf_ctx *c)
{
    SVGF_ENTER(c);
    HIPC(c, hipDeviceSynchronize());
    return zero_state(c);
}

// History clamp of the temporal pass (include/svgf.h).  Host state only: no device work, nothing to order.
extern "C" int svgf_set_history_clamp(svgf_ctx *c, int radius, float sigma_scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (radius < 0 || radius > 3) {
        snprintf(c->err, sizeof(c->err), "svgf_set_history_clamp: radius %d outside 0..3", radius);
        return SVGF_ERR_INVALID_ARG;
    }
    if (!(sigma_scale >= 0.0f) || sigma_scale > 3.402823466e38f) {      // NaN, negative, +inf
        snprintf(c->err, sizeof(c->err), "svgf_set_history_clamp: sigma_scale %g is not a finite number >= 0", (double)sigma_scale);
        return SVGF_ERR_INVALID_ARG;
    }
    c->clamp_radius = radius; c->clamp_k = sigma_scale;
    return SVGF_OK;
}

extern "C" int svgf_get_history_clamp(const svgf_ctx *c, int *radius, float *sigma_scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (radius) *radius = c->clamp_radius;
    if (sigma_scale) *sigma_scale = c->clamp_k;
    return SVGF_OK;
}

// Firefly filter of the input colour (include/svgf.h).  Host state only, like the clamp.
extern "C" int svgf_set_firefly_filter(svgf_ctx *c, int rank, float scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (rank < 0 || rank > 3) {
        snprintf(c->err, sizeof(c->err), "svgf_set_firefly_filter: rank %d outside 0..3", rank);
        return SVGF_ERR_INVALID_ARG;
    }
    if (!(scale >= 0.0f) || scale > 3.402823466e38f) {      // NaN, negative, +inf
        snprintf(c->err, sizeof(c->err), "svgf_set_firefly_filter: scale %g is not a finite number >= 0", (double)scale);
        return SVGF_ERR_INVALID_ARG;
    }
    c->firefly_rank = rank; c->firefly_scale = scale;
    return SVGF_OK;
}

extern "C" int svgf_get_firefly_filter(const svgf_ctx *c, int *rank, float *scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (rank) *rank = c->firefly_rank;
    if (scale) *scale = c->firefly_scale;
    return SVGF_OK;
}

// Per-object rigid motion of the temporal pass (include/svgf.h).  Host state only, like the clamp: the table is the caller's memory.
extern "C" int svgf_set_object_motion(svgf_ctx *c, const float *geom_xf_dev, int n_geoms)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (n_geoms < 0) {
        snprintf(c->err, sizeof(c->err), "svgf_set_object_motion: n_geoms %d is negative", n_geoms);
        return SVGF_ERR_INVALID_ARG;
    }
    if (!geom_xf_dev && n_geoms > 0) {
        snprintf(c->err, sizeof(c->err), "svgf_set_object_motion: null table with n_geoms %d", n_geoms);
        return SVGF_ERR_INVALID_ARG;
    }
    if ((uintptr_t)geom_xf_dev & 15) {      // the kernel loads a row of a map as one 16-byte value
        snprintf(c->err, sizeof(c->err), "svgf_set_object_motion: the table at %p is not 16-byte aligned", (const void *)geom_xf_dev);
        return SVGF_ERR_INVALID_ARG;
    }
    c->xf_dev = geom_xf_dev; c->xf_n = n_geoms;
    return SVGF_OK;
}

extern "C" int svgf_get_object_motion(const svgf_ctx *c, const float **geom_xf_dev, int *n_geoms)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (geom_xf_dev) *geom_xf_dev = c->xf_dev;
    if (n_geoms) *n_geoms = c->xf_n;
    return SVGF_OK;
}

// Output TAA (include/svgf.h).  Configuration like the clamp, but the first call that turns it on allocates the pass's three planes.
extern "C" int svgf_set_output_taa(svgf_ctx *c, float alpha, float sigma_scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (!(alpha >= 0.0f && alpha <= 1.0f)) {      // NaN included
        snprintf(c->err, sizeof(c->err), "svgf_set_output_taa: alpha %g outside 0..1", (double)alpha);
        return SVGF_ERR_INVALID_ARG;
    }
    if (!(sigma_scale >= 0.0f) || sigma_scale > 3.402823466e38f) {      // NaN, negative, +inf
        snprintf(c->err, sizeof(c->err), "svgf_set_output_taa: sigma_scale %g is not a finite number >= 0", (double)sigma_scale);
        return SVGF_ERR_INVALID_ARG;
    }
    if (alpha > 0.0f && !c->taa_pre) {
        SVGF_ENTER(c);
        float *pre = nullptr;
        float4 *h[2] = { nullptr, nullptr };
        const bool ok = hipMalloc((void **)&pre, c->n * 3 * sizeof(float)) == hipSuccess &&
                        hipMalloc((void **)&h[0], c->n * sizeof(float4)) == hipSuccess &&
                        hipMalloc((void **)&h[1], c->n * sizeof(float4)) == hipSuccess;
        // (cleared once, on the legacy stream, and complete before the call returns: a frame may follow on a non-blocking stream)
        const bool cleared = ok && hipMemset(pre, 0, c->n * 3 * sizeof(float)) == hipSuccess && hipMemset(h[0], 0, c->n * sizeof(float4)) == hipSuccess &&
                             hipMemset(h[1], 0, c->n * sizeof(float4)) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
        if (!cleared) {
            if (pre) (void)hipFree(pre);
            for (int k = 0; k < 2; k++) if (h[k]) (void)hipFree(h[k]);
            (void)hipGetLastError();
            snprintf(c->err, sizeof(c->err), "svgf_set_output_taa: %s for the output pass's planes (%zu bytes)", ok ? "hipMemset failed" : "hipMalloc failed", c->n * 44);
            return ok ? SVGF_ERR_HIP : SVGF_ERR_OOM;
        }
        c->taa_pre = pre; c->taa_hist[0] = h[0]; c->taa_hist[1] = h[1];
    }
    if (alpha > 0.0f && !(c->taa_alpha > 0.0f)) c->taa_valid = 0;      // turned on: the first frame behind this call has no output history
    c->taa_alpha = alpha; c->taa_k = sigma_scale;
    return SVGF_OK;
}

extern "C" int svgf_get_output_taa(const svgf_ctx *c, float *alpha, float *sigma_scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (alpha) *alpha = c->taa_alpha;
    if (sigma_scale) *sigma_scale = c->taa_k;
    return SVGF_OK;
}

extern "C" int svgf_is_pipelined(const svgf_ctx *c) { return (c && c->pipelined && c->piped_mode) ? 1 : 0; }
extern "C" int svgf_pipeline_status(const svgf_ctx *c) { return !c || !c->pipelined ? 0 : (c->pipe_serial ? 2 : 1); }

extern "C" int svgf_enable_pipeline(svgf_ctx *c)
{
    SVGF_ENTER(c);
    return enable_pipeline(c);
}

extern "C" int svgf_sync(svgf_ctx *c)
{
    SVGF_ENTER(c);
    HIPC(c, hipDeviceSynchronize());
    return SVGF_OK;
}

// Stream-scoped completion: wait for what has been enqueued on `stream` (this context's frames included) and nothing else.
extern "C" int svgf_sync_stream(svgf_ctx *c, void *stream)
{
    SVGF_ENTER(c);
    HIPC(c, hipStreamSynchronize((hipStream_t)stream));
    return SVGF_OK;
}

extern "C" const char *svgf_last_error(const svgf_ctx *c) { return c ? c->err : g_create_err; }
extern "C" int svgf_width(const svgf_ctx *c) { return c ? c->W : 0; }
#ifdef SVGF_BUILD_EXPERIMENTS
// The a-trous levels of the context's last frame, in order: the kernel each ran (0 fused first level, 1 lane, 2 lane with two
// y-phases, 3 strip, 4 lattice, 5 gather), its step, and the lane / strip estimates (us) the automatic choice compared for that
// step (NaN where kernel_variant != 0 or the choice was not made between those two).  Writes min(n, levels) entries of every
// non-null array; returns the number of levels (0 for a frame without a cascade), or a negative error.
extern "C" int svgf_exp_level_kernels(const svgf_ctx *c, int *kinds, int *steps, double *lane_us, double *strip_us, int n)
{
    if (!c || n < 0) return SVGF_ERR_INVALID_ARG;
    for (int k = 0; k < c->lk_n && k < n; k++) {
        if (kinds) kinds[k] = c->lk_kind[k];
        if (steps) steps[k] = c->lk_step[k];
        if (lane_us) lane_us[k] = c->lk_asked[k] ? c->est_lane_us[step_log2(c->lk_step[k])] : __builtin_nan("");
        if (strip_us) strip_us[k] = c->lk_asked[k] ? c->est_strip_us[step_log2(c->lk_step[k])] : __builtin_nan("");
    }
    return c->lk_n;
}
#endif
extern "C" int svgf_height(const svgf_ctx *c) { return c ? c->H : 0; }

extern "C" int svgf_set_capture(svgf_ctx *c, int on)
{
    SVGF_ENTER(c);
    if (on && !c->cv_capture) {
        HIPC(c, hipMalloc((void **)&c->cv_capture, c->n * sizeof(float4)));
        HIPC(c, hipMemset(c->cv_capture, 0, c->n * sizeof(float4)));
    }
    c->capture = on ? 1 : 0;
    return SVGF_OK;
}

// ---- profiling ---------------------------------------------------------------------------------------------

extern "C" int svgf_profile_enable(svgf_ctx *c, int nframes)
{
    if (!c || nframes < 0) return SVGF_ERR_INVALID_ARG;
    SVGF_ENTER(c);
    if (c->ev && nframes == c->prof_frames) {
        // Same number of slots as before: only the counters restart, the events are reused.  Creating a few hundred events takes
        // 0.2-2 ms, and a benchmark that re-arms the profiler between its warm-up and its timed frames would let the GPU idle for
        // that long: 2 ms of idle time cost the following 20 frames 3 % (profiles/r04_clock_states.txt).
        c->prof_count = 0; c->frame_no = 0;
        memset(c->ev_n, 0, sizeof(int) * (size_t)nframes);
        return SVGF_OK;
    }
    profile_free(c, (long long)c->prof_frames * SVGF_MAX_KERNELS_PER_FRAME * 2);
    c->prof_frames = 0; c->prof_count = 0; c->frame_no = 0;
    if (c->prof_stride < 1) c->prof_stride = 1;
    if (nframes == 0) return SVGF_OK;
    const long long ne = (long long)nframes * SVGF_MAX_KERNELS_PER_FRAME * 2;
    c->ev = (hipEvent_t *)calloc(ne, sizeof(hipEvent_t));
    c->ev_kind = (int *)calloc((size_t)nframes * SVGF_MAX_KERNELS_PER_FRAME, sizeof(int));
    c->ev_n = (int *)calloc(nframes, sizeof(int));
    if (!c->ev || !c->ev_kind || !c->ev_n) { profile_free(c, 0); return SVGF_ERR_OOM; }
    for (long long k = 0; k < ne; k++) {
        hipError_t e = hipEventCreate(&c->ev[k]);
        if (e != hipSuccess) {          // give back what was created: profiling stays off
            profile_free(c, k);
            snprintf(c->err, sizeof(c->err), "svgf_profile_enable: hipEventCreate failed: %s", hipGetErrorString(e));
            return SVGF_ERR_HIP;
        }
    }
    c->prof_frames = nframes;
    return SVGF_OK;
}

extern "C" int svgf_profile_stride(svgf_ctx *c, int k)
{
    if (!c || k < 1) return SVGF_ERR_INVALID_ARG;
    c->prof_stride = k;
    return SVGF_OK;
}

extern "C" long long svgf_profile_frames(const svgf_ctx *c) { return c ? c->prof_count : 0; }

extern "C" int svgf_profile_read(svgf_ctx *c, int slot, int max_entries, int *kinds, float *ms, int *n_out)
{
    if (!c || !n_out || slot < 0 || slot >= c->prof_frames) return SVGF_ERR_INVALID_ARG;
    SVGF_ENTER(c);
    const int nk = c->ev_n[slot];
    int w = 0;
    for (int k = 0; k < nk && w < max_entries; k++, w++) {
        const long long base = ((long long)slot * SVGF_MAX_KERNELS_PER_FRAME + k) * 2;
        float t = 0.0f;
        HIPC(c, hipEventElapsedTime(&t, c->ev[base], c->ev[base + 1]));
        if (kinds) kinds[w] = c->ev_kind[slot * SVGF_MAX_KERNELS_PER_FRAME + k];
        if (ms) ms[w] = t;
    }
    *n_out = w;
    return SVGF_OK;
}

namespace {
// Times one launch when profiling is on: the event pair of the slot is armed for the next kernel launch of this thread and
// the launcher's SVGF_LAUNCH_KERNEL attaches it to the dispatch (svgf_kernels.h).  Nothing is recorded on the stream.
struct KernelTimer {
    svgf_ctx *c; hipStream_t s; int slot; int k; bool on;
    bool begin(int kind) {
        if (!on) return true;
        k = c->ev_n[slot];
        if (k >= SVGF_MAX_KERNELS_PER_FRAME) return true;
        const long long e = (long long)slot * SVGF_MAX_KERNELS_PER_FRAME + k;
        c->ev_kind[e] = kind;
        g_svgf_launch_events = SvgfLaunchEvents{ c->ev[e * 2], c->ev[e * 2 + 1] };
        return true;
    }
    bool end() {
        if (!on || k >= SVGF_MAX_KERNELS_PER_FRAME) return true;
        const bool consumed = (g_svgf_launch_events.start == nullptr);      // a launcher that did not go through the macro: no entry
        g_svgf_launch_events = SvgfLaunchEvents{ nullptr, nullptr };
        if (consumed) c->ev_n[slot] = k + 1;
        return true;
    }
};
}  // namespace

thread_local SvgfLaunchEvents g_svgf_launch_events = { nullptr, nullptr };

#define LAUNCH(kind, expr)                                                                           \
    do {                                                                                             \
        timer.begin(kind);                                                                           \
        const hipError_t le__ = (expr);                                                              \
        timer.end();          /* (also disarms the event pair when the launcher failed before launching) */ \
        if (le__ != hipSuccess) {                                                                    \
            snprintf(c->err, sizeof(c->err), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(le__), __FILE__, __LINE__); \
            return SVGF_ERR_HIP;                                                                     \
        }                                                                                            \
    } while (0)

// ---- the frame ------------------------------------------------------------------------------------------------

// ---- the frame pipeline's resources: second plane set, two internal streams, events; and the probe that decides whether the
// promise (inputs_ready = 1) can be honoured.  Called by svgf_create_ex(SVGF_CREATE_PIPELINED) or svgf_enable_pipeline, never by
// svgf_denoise: it allocates and synchronises the device.
__global__ void k_svgf_spin(unsigned long long ticks)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// Do kernels on pipe[0] and pipe[1] overlap?  The HIP runtime spreads a process's streams over GPU_MAX_HW_QUEUES hardware queues
// (default 4, read when the runtime starts); two streams that land on the same queue run their kernels one after the other, and
// pipelined frames are then 8-10 % SLOWER than ordered ones (the cross-stream events cost, nothing overlaps: profiles/r05_exp_pipeline.log).
// Two one-wave spin kernels of ~200 us, one per stream: together they take ~200 us on two queues and ~400 us on one.
static hipError_t probe_two_streams(int device, hipStream_t sa, hipStream_t sb, bool *overlap, double *ratio_out)
{
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) khz = 100000;
    const double spin_us = 200.0;
    const unsigned long long ticks = (unsigned long long)(spin_us * 1e-6 * khz * 1e3);
    hipEvent_t e[4] = { nullptr, nullptr, nullptr, nullptr };
    hipError_t rc = hipSuccess;
    for (int k = 0; k < 4 && rc == hipSuccess; k++) rc = hipEventCreate(&e[k]);
    double best = 1e30;
#define SVGF_PROBE(call) do { if (rc == hipSuccess) rc = (call); } while (0)
    // (one probe at a time in this process: two contexts created from two host threads would time each other's spin kernels.  Work of
    // OTHER origin on the device can still delay one of the two kernels: up to eight trials, the best one counts, a clear answer ends it)
    static std::mutex probe_mu;
    std::lock_guard<std::mutex> probe_lock(probe_mu);
    for (int trial = 0; trial < 9 && rc == hipSuccess && best > 1.2; trial++) {       // trial 0 loads the code object
        SVGF_PROBE(hipDeviceSynchronize());
        SVGF_PROBE(hipEventRecord(e[0], sa));
        if (rc == hipSuccess) hipLaunchKernelGGL(k_svgf_spin, dim3(1), dim3(64), 0, sa, trial ? ticks : 1ull);
        SVGF_PROBE(hipEventRecord(e[1], sa));
        SVGF_PROBE(hipEventRecord(e[2], sb));
        if (rc == hipSuccess) hipLaunchKernelGGL(k_svgf_spin, dim3(1), dim3(64), 0, sb, trial ? ticks : 1ull);
        SVGF_PROBE(hipEventRecord(e[3], sb));
        SVGF_PROBE(hipGetLastError());
        SVGF_PROBE(hipDeviceSynchronize());
        if (!trial || rc != hipSuccess) continue;
        // span from the earlier start to the later end, on the device's own clock
        float a01 = 0, a23 = 0, a03 = 0, a21 = 0;
        SVGF_PROBE(hipEventElapsedTime(&a01, e[0], e[1]));
        SVGF_PROBE(hipEventElapsedTime(&a23, e[2], e[3]));
        SVGF_PROBE(hipEventElapsedTime(&a03, e[0], e[3]));
        SVGF_PROBE(hipEventElapsedTime(&a21, e[2], e[1]));
        double span = a03 > a21 ? a03 : a21;
        if (a01 > span) span = a01;
        if (a23 > span) span = a23;
        const double one = (a01 < a23 ? a01 : a23);
        if (one > 0 && span / one < best) best = span / one;
    }
#undef SVGF_PROBE
    for (int k = 0; k < 4; k++) if (e[k]) (void)hipEventDestroy(e[k]);
    *ratio_out = best;
    *overlap = best < 1.5;          // 1.0: side by side; 2.0: one after the other
    return rc;
}

static int probe_streams_overlap(svgf_ctx *c, bool *overlap, double *ratio_out)
{
    HIPC(c, probe_two_streams(c->device, c->pipe[0], c->pipe[1], overlap, ratio_out));
    return SVGF_OK;
}

// The same probe for a CALLER's two streams (inputs_ready = 2: the library runs such frames on the streams it is given and cannot
// know how the runtime mapped them to hardware queues).  Synchronises the device: call it once, at set-up.
extern "C" int svgf_streams_overlap(int device, void *stream_a, void *stream_b)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return SVGF_ERR_NO_DEVICE;
    if (stream_a == stream_b) return 0;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    bool overlap = false;
    double ratio = 0.0;
    if (probe_two_streams(device, (hipStream_t)stream_a, (hipStream_t)stream_b, &overlap, &ratio) != hipSuccess) return SVGF_ERR_HIP;
    return overlap ? 1 : 0;
}

static int enable_pipeline(svgf_ctx *c)
{
    if (c->pipelined) return SVGF_OK;
    for (int k = 3; k < 6; k++) {
        char *raw = nullptr;
        if (!c->cv[k]) {
            if (hipMalloc((void **)&raw, c->n * sizeof(float4) + 2 * kPlanePad) != hipSuccess) { snprintf(c->err, sizeof(c->err), "svgf_enable_pipeline: hipMalloc failed for the pipeline's planes"); return SVGF_ERR_OOM; }
            c->cv[k] = reinterpret_cast<float4 *>(raw + kPlanePad);
            HIPC(c, hipMemset(raw, 0, c->n * sizeof(float4) + 2 * kPlanePad));
        }
        if (!c->vp[k]) {
            const size_t vb = (size_t)(c->W + 2) * (c->H + 2) * sizeof(float) + 64;
            if (hipMalloc((void **)&c->vp[k], vb) != hipSuccess) { snprintf(c->err, sizeof(c->err), "svgf_enable_pipeline: hipMalloc failed for the pipeline's planes"); return SVGF_ERR_OOM; }
            HIPC(c, hipMemset(c->vp[k], 0, vb));
        }
    }
    for (int q = 0; q < 2; q++) {
        if (!c->pipe[q]) HIPC(c, hipStreamCreateWithFlags(&c->pipe[q], hipStreamNonBlocking));
        for (svgf_ctx::PipeEvent *e : { &c->ev_hist[q], &c->ev_done[q], &c->ev_tdone[q] })
            if (!e->ev) HIPC(c, hipEventCreateWithFlags(&e->ev, hipEventDisableTiming));
    }
    if (!c->ev_in) HIPC(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
    bool overlap = true;
    double ratio = 0.0;
    if (const int rc = probe_streams_overlap(c, &overlap, &ratio); rc != SVGF_OK) return rc;
    // The runtime hands out hardware queues in an order of its own, and two streams created one after the other can land on ONE queue
    // even when the process has several (seen in fresh C++ processes under the default GPU_MAX_HW_QUEUES = 4, examples/): replace
    // the second stream until the pair overlaps, a few times; with ONE queue in all, no replacement helps and the promise is refused.
    hipStream_t rejected[5];
    int n_rejected = 0;
    for (int k = 0; k < 5 && !overlap; k++) {
        hipStream_t cand = nullptr;
        if (hipStreamCreateWithFlags(&cand, hipStreamNonBlocking) != hipSuccess) break;
        rejected[n_rejected++] = c->pipe[1];
        c->pipe[1] = cand;
        if (const int rc = probe_streams_overlap(c, &overlap, &ratio); rc != SVGF_OK) break;
    }
    for (int k = 0; k < n_rejected; k++) (void)hipStreamDestroy(rejected[k]);
    HIPC(c, hipDeviceSynchronize());
    c->pipelined = 1;
    c->pipe_serial = overlap ? 0 : 1;
    c->piped_mode = overlap ? 1 : 0;      // (refused: frames stay plain ordered frames until one asks for inputs_ready = 2)
    pipe_reset(c);
    if (!overlap)
        snprintf(c->err, sizeof(c->err), "frame pipeline: the context's internal streams share a hardware queue (six candidate pairs; two 200 us kernels took %.2fx one): "
                 "the inputs_ready = 1 promise is refused and such frames run ordered on the caller's stream; start the process with "
                 "GPU_MAX_HW_QUEUES=8 (read by the HIP runtime at initialisation)", ratio);
    return SVGF_OK;
}

// The automatic choice between the two fast a-trous kernels for steps 2-32: the one whose launch geometry is estimated cheaper runs
// (the cost model: svgf_atrous_geometry.hip).  The estimates depend on the image size and the device only, so they are asked for
// once per context and step.
static bool lane_pays(svgf_ctx *c, const AtrousArgs &a)
{
    const int l = step_log2(a.step);
    if (c->lane_cheaper[l] < 0) {
        const double lane = atrous_lane_estimate_us(a, c->n_cu), strip = atrous_strip_estimate_us(a, c->n_cu);
        c->lane_cheaper[l] = lane <= strip ? 1 : 0;
#ifdef SVGF_BUILD_EXPERIMENTS
        c->est_lane_us[l] = lane; c->est_strip_us[l] = strip;
#endif
    }
    return c->lane_cheaper[l] != 0;
}

#ifdef SVGF_BUILD_EXPERIMENTS
// Temporal pass + first level as ONE kernel (svgf_atrous_fused.hip), or as two?  The fused kernel works on 240-column strips
// with both y-phases of a strip in one workgroup and pays the same rounds x (rows + 6) launch geometry as the lane kernel; what
// it saves is the temporal kernel (HBM-bound, 25.6 ns per kilopixel at 1080p) and 56 B/px of traffic between the two.  It runs
// when its estimate is below the estimate of the level it replaces plus the temporal pass.
static bool fuse_pays(svgf_ctx *c, const AtrousArgs &a)
{
    if (c->fuse_pays < 0) {
        const double lane = atrous_lane_supported(a) ? atrous_lane_estimate_us(a, c->n_cu) : 1e30;
        const double strip = atrous_strip_supported(a) ? atrous_strip_estimate_us(a, c->n_cu) : 1e30;
        const double level = lane < strip ? lane : strip;
        const double temporal_us = 0.0256e-3 * (double)c->W * (double)c->H;
        c->fuse_pays = (kFusedRowFactor * atrous_fused_estimate_us(a, c->n_cu) <= level + temporal_us && level < 1e29) ? 1 : 0;
    }
    return c->fuse_pays != 0;
}
#endif

// ---- the frame: plan (every decision, nothing enqueued), enqueue (walks the plan), commit (the context's state behind it) ----
enum KernelKind { K_FUSED, K_LANE, K_LANE2Y, K_STRIP, K_LATTICE, K_GATHER };      // (the numbering svgf_exp_level_kernels reports)
enum FrameExit { EXIT_CASCADE, EXIT_DEBUG_HLEN, EXIT_DEBUG_VAR, EXIT_COPY };

#ifdef SVGF_BUILD_EXPERIMENTS
// The launch geometry of one a-trous level on one kernel (0 fused first level, 1 lane, 2 lane with two y-phases, 3 strip,
// 4 lattice: the numbering of svgf_exp_level_kernels) for a W x H frame on a device of n_cu compute units, as the launcher would
// compute it (svgf_atrous_geometry.h) — host arithmetic only, no device is touched.  out[0..7]: supported, n_strips, seg_rows,
// n_segs, n_groups, grid blocks, block threads, LDS bytes (lattice: supported, log2k, pstride, band_rows, n_bands, grid blocks,
// block threads, LDS bytes); all zero where the kernel does not run such a level.  *estimate_us: what the automatic choice compares (lane, strip,
// fused), NaN for the others.  For the two-y-phase kernels "supported" is the geometry's own condition (step 2, the lane
// kernel's limits), not the fused kernel's conditions on the context's planes.
extern "C" int svgf_exp_atrous_geometry(int kernel, int W, int H, int step, int blur_variance, int has_variance_plane, int n_cu,
                                        int *out, double *estimate_us)
{
    if (!out || !estimate_us || W < 1 || H < 1 || step < 1 || n_cu < 1) return SVGF_ERR_INVALID_ARG;
    static const float plane = 0.0f;      // a.var is only tested for null here
    AtrousArgs a;
    memset(&a, 0, sizeof(a));
    a.W = W; a.H = H; a.step = step; a.blur_variance = blur_variance; a.var = has_variance_plane ? &plane : nullptr;
    for (int k = 0; k < 8; k++) out[k] = 0;
    *estimate_us = __builtin_nan("");
    SegmentGeom gm;
    int threads = 0, lds = 0;
    switch (kernel) {
    case K_LANE:
        if (!atrous_lane_supported(a)) return SVGF_OK;
        (void)lane_geometry(a, 1, n_cu, &gm);
        *estimate_us = atrous_lane_estimate_us(a, n_cu);
        atrous_lane_block(a, &threads, &lds);
        break;
    case K_FUSED: case K_LANE2Y:
        if (step != 2 || !atrous_lane_supported(a)) return SVGF_OK;
        (void)lane_geometry(a, 2, n_cu, &gm);
        if (kernel == K_FUSED) *estimate_us = atrous_fused_estimate_us(a, n_cu);
        atrous_lane2y_block(kernel == K_FUSED, &threads, &lds);
        break;
    case K_STRIP: {
        if (!atrous_strip_supported(a)) return SVGF_OK;
        int tx, rows;
        strip_pick(atrous_step_log2(step), tx, rows);
        (void)strip_geometry(a, tx, rows, n_cu, &gm);
        *estimate_us = atrous_strip_estimate_us(a, n_cu);
        threads = strip_shape::block_threads(tx, rows); lds = (int)strip_shape::lds_bytes(step, tx, rows);
        break;
    }
    case K_LATTICE: {
        LatticeTiles lt;
        if (!lattice_geometry(a, lt)) return SVGF_OK;
        const int v[8] = { 1, lt.log2k, lt.pstride, lt.band_rows, lt.n_bands, (int)lattice_grid_blocks(lt), kLatticeThreads, (int)lattice_lds_bytes(lt) };
        memcpy(out, v, sizeof(v));
        return SVGF_OK;
    }
    default:
        return SVGF_ERR_INVALID_ARG;
    }
    const int v[8] = { 1, gm.n_strips, gm.seg_rows, gm.n_segs, gm.n_groups, segment_grid_blocks(gm), threads, lds };
    memcpy(out, v, sizeof(v));
    return SVGF_OK;
}
#endif

struct LevelPlan {
    KernelKind kind;
    AtrousArgs a;
    int dst;                        // cv index the level writes; -1: the last level writes `out` only
    bool keep, last, asked;         // keep: the output becomes the colour history (:391); asked: the automatic choice compared the estimates of this step
};
struct FramePlan {
    bool flip, piped, promise;      // the pipeline decision (see plan_frame); flip: the context goes into piped mode with this frame
    bool wait_in_first;             // a promised frame that runs behind the caller's stream position as a whole
    unsigned long long cap_id;      // != 0: `stream` is being captured into a graph
    int pq;                         // parity: plane set, internal stream and events of this frame
    hipStream_t s, s_user;
    int hist_release;               // ev_hist[pq] is recorded behind level [hist_release]; -1: behind the temporal pass; n_levels: at the frame's end
    bool timed; int slot;           // profiling brackets this frame's kernels, in slot `slot`
    bool temporal, fused, split_fused, tdone, capture;      // what runs before the cascade; tdone: the temporal pass re-arms ev_tdone[pq] (planar frames)
    int svf;                        // SvgfParams::spatial_variance_frames
    TemporalArgs t;
    FrameExit exit;
    float *out;
    float *out_c;                   // where the last level / the pass-through copy writes the image: `out`, or the output pass's `pre` plane
    bool taa;                       // svgf_set_output_taa: the output pass runs, last
    OutputTaaArgs o;
    int taa_cur, taa_valid;         // the context's output history after the frame
    int n_levels;
    LevelPlan lv[SVGF_MAX_LEVELS];
    int acc, hist, cur, gcur, last_modulated;      // the context's plane roles after the frame
    unsigned vp_valid;
};

// The kernel of one a-trous level: the ONE place that chooses between the six.
static KernelKind level_kernel(svgf_ctx *c, const SvgfParams *p, const AtrousArgs &a, bool fuse_here)
{
    if (fuse_here) return K_FUSED;
    const int kv = p->kernel_variant;
    if (kv != 1 && atrous_strip_supported(a)) {
#ifdef SVGF_BUILD_EXPERIMENTS
        if (a.step == 2 && kv == 5 && atrous_lane_supported(a)) return K_LANE2Y;
#endif
        if (atrous_lane_supported(a) && (kv >= 4 || (kv == 0 && lane_pays(c, a)))) return K_LANE;
        return K_STRIP;
    }
    if (kv != 1 && kv != 2 && atrous_lattice_supported(a)) return K_LATTICE;     // steps 64, 128, ...
    return K_GATHER;
}

// gbuffer_dev == nullptr: the planar path (svgf_denoise_planar) — the current-frame planes nrm/pos/gid[1 - gcur] (and `albedo`)
// were filled in place by the producer.
// Every level is decided and validated here, before anything is enqueued or any context state changes: a failure half-way
// through the cascade would leave the colour history of this frame next to the G-buffer / moments of the previous one.  The
// context is only read (the memoised estimates of lane_pays / fuse_pays aside).
// motion_dev != nullptr: the temporal pass reads the previous-frame coordinates from the caller's plane (svgf_denoise_motion); an
// input like the colour image, read by that pass only.
static int plan_frame(svgf_ctx *c, void *out_rgb_dev, const void *in_rgb_dev, const void *gbuffer_dev,
                      const void *motion_dev, int motion_format, const SvgfParams *p, void *stream, FramePlan &pl)
{
    if (p->atrous_nlevel < 0 || p->atrous_nlevel > SVGF_MAX_LEVELS) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: atrous_nlevel %d outside 0..%d", p->atrous_nlevel, SVGF_MAX_LEVELS);
        return SVGF_ERR_INVALID_ARG;
    }
    if (p->kernel_variant < 0 || p->kernel_variant > 6 || p->kernel_variant == 3) {
        snprintf(c->err, sizeof(c->err), p->kernel_variant == 3
                 ? "svgf_denoise: kernel_variant %d (experimental shared-weight kernel) is no longer part of the library, see tools/experiments/"
                 : "svgf_denoise: kernel_variant %d unknown", p->kernel_variant);
        return SVGF_ERR_INVALID_ARG;
    }
#ifndef SVGF_BUILD_EXPERIMENTS
    if (p->kernel_variant == 5 || p->kernel_variant == 6) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: kernel_variant %d is a parked experiment (two-y-phase geometry / temporal pass fused into "
                 "the first level) and is not part of this build; build libsvgf_hip_exp.so (-DSVGF_BUILD_EXPERIMENTS)", p->kernel_variant);
        return SVGF_ERR_UNSUPPORTED;
    }
#endif
    if (motion_dev && !temporal_motion_format_known(motion_format)) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise_motion: motion_format %d unknown", motion_format);
        return SVGF_ERR_INVALID_ARG;
    }
    const bool motion = motion_dev && p->temporal_enable;      // (a non-temporal frame has no history to look up: the plane is ignored)
#ifdef SVGF_BUILD_EXPERIMENTS
    if (motion && (p->kernel_variant == 6 || c->use_split_fused)) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise_motion: the parked fused temporal kernels (kernel_variant 6, split_fused) take no motion plane");
        return SVGF_ERR_UNSUPPORTED;
    }
#endif
    const bool clamp = c->clamp_radius > 0 && p->temporal_enable;      // svgf_set_history_clamp (a non-temporal frame gathers no history)
    if (clamp && !temporal_clamp_supported(c->W, c->H)) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: the history clamp (svgf_set_history_clamp) is limited to images of at most 262140 rows, this context has %d", c->H);
        return SVGF_ERR_UNSUPPORTED;
    }
#ifdef SVGF_BUILD_EXPERIMENTS
    if (clamp && (p->kernel_variant == 6 || c->use_split_fused)) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: the parked fused temporal kernels (kernel_variant 6, split_fused) have no history clamp (svgf_set_history_clamp)");
        return SVGF_ERR_UNSUPPORTED;
    }
#endif
    const bool xform = c->xf_dev && c->xf_n > 0 && p->temporal_enable;      // svgf_set_object_motion (a non-temporal frame tests no history)
#ifdef SVGF_BUILD_EXPERIMENTS
    if (xform && (p->kernel_variant == 6 || c->use_split_fused)) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: the parked fused temporal kernels (kernel_variant 6, split_fused) take no object motion table (svgf_set_object_motion)");
        return SVGF_ERR_UNSUPPORTED;
    }
#endif
    const bool firefly = c->firefly_rank > 0;      // svgf_set_firefly_filter: temporal and non-temporal frames alike
    if (firefly && !temporal_clamp_supported(c->W, c->H)) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: the firefly filter (svgf_set_firefly_filter) is limited to images of at most 262140 rows, this context has %d", c->H);
        return SVGF_ERR_UNSUPPORTED;
    }
#ifdef SVGF_BUILD_EXPERIMENTS
    if (firefly && (p->kernel_variant == 6 || c->use_split_fused)) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: the parked fused temporal kernels (kernel_variant 6, split_fused) have no firefly filter (svgf_set_firefly_filter)");
        return SVGF_ERR_UNSUPPORTED;
    }
#endif
    // svgf_set_output_taa: every frame that writes the image (debug views are written as they are and drop the output history)
    const bool taa = pl.taa = c->taa_alpha > 0.0f && p->right_view_option != 1 && p->right_view_option != 2;
    if (taa && !temporal_clamp_supported(c->W, c->H)) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: the output pass (svgf_set_output_taa) is limited to images of at most 262140 rows, this context has %d", c->H);
        return SVGF_ERR_UNSUPPORTED;
    }
#ifdef SVGF_BUILD_EXPERIMENTS
    if (taa && (p->kernel_variant == 6 || c->use_split_fused)) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: the parked fused temporal kernels (kernel_variant 6, split_fused) have no output pass (svgf_set_output_taa)");
        return SVGF_ERR_UNSUPPORTED;
    }
#endif
    const float *in = (const float *)in_rgb_dev, *g = (const float *)gbuffer_dev;
    pl.out = (float *)out_rgb_dev; pl.out_c = taa ? c->taa_pre : pl.out; pl.s_user = (hipStream_t)stream; pl.cap_id = 0;
    // Pipelined frames (see svgf_ctx::pipelined).  The promise behind inputs_ready = 1: at call time the inputs are complete (and stay
    // untouched until the work of this call is done) — so the frame need not order itself behind the caller's stream, which has
    // waited for the PREVIOUS frame's end, and runs on an internal stream; only the kernel that writes `out` waits for the caller's
    // stream position (readers of that buffer enqueued behind earlier calls).
    // Without the promise a frame of a pipelined context runs on the caller's stream, like any frame of any context, behind the last
    // frame that used its plane set and the history of the frame before it; under stream capture nothing is promised (the frame is
    // recorded on the capturing stream).  The planar path and the experiments build's fused temporal pass never pipeline.
    // (The promise is a permission: it is used where there is something to overlap — a temporal pass and a cascade of two or more
    // levels.  A one-launch frame like BASELINE configs[0] loses more to the four cross-stream events of a pipelined frame than it
    // can gain: 0.0247 -> 0.0342 ms measured, profiles/r05_exp_pipeline.log.)
    // Nor where nothing CAN overlap: with the colour history taken from the LAST level the next temporal pass needs the whole frame.
    // inputs_ready == 2 asks for the pipeline WITHOUT the promise: the frame is ordered behind `stream` like any other work (its
    // inputs may be produced there, its output consumed there), and a caller that alternates TWO streams from frame to frame gets
    // the same overlap with nothing but stream semantics — a stream only ever waits for the frames that were given to it.
    // (planar frames too, ABI 0.9: the promise then covers the context's own current-frame planes — written, complete, and not
    // rewritten before the work of this call is done; a producer that refills them every frame takes the pointers through
    // svgf_planar_gbuffer_stream, which orders it behind the frames that still read them)
    const bool worth = p->temporal_enable && p->spatial_enable && p->atrous_nlevel >= 2 &&
                       p->right_view_option != 1 && p->right_view_option != 2 && p->history_level != p->atrous_nlevel;
    // Only a context whose pipeline resources exist (svgf_create_ex(SVGF_CREATE_PIPELINED) / svgf_enable_pipeline) takes either form up:
    // svgf_denoise never allocates.  The promise additionally needs the two internal streams on different hardware queues (probed when
    // the resources were created, svgf_pipeline_status() == 1): refused, a promised frame is a plain ordered frame.
    bool promise = (p->inputs_ready == 1) && worth && c->pipelined && !c->pipe_serial;
    bool want_pipeline = promise || ((p->inputs_ready == 2) && worth && c->pipelined);
    if (want_pipeline || c->piped_mode) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        unsigned long long id = 0;
        if (pl.s_user && hipStreamGetCaptureInfo(pl.s_user, &cs, &id) == hipSuccess && cs != hipStreamCaptureStatusNone) { pl.cap_id = id ? id : 1; promise = false; }
        // a frame recorded into a graph did not run when it was recorded: the eager frames behind it order themselves behind the
        // caller's stream (where the graph is launched) until both parities' events are eager ones again
        if (!pl.cap_id && (c->ev_hist[0].cap || c->ev_hist[1].cap)) promise = false;
    }
#ifdef SVGF_BUILD_EXPERIMENTS
    if (p->kernel_variant == 6 || p->kernel_variant == 5 || c->use_reuse || c->use_split_fused) { promise = false; want_pipeline = false; }
#endif
    pl.flip = want_pipeline && !pl.cap_id && !c->piped_mode;
    const bool piped = pl.piped = c->piped_mode || pl.flip;
    const long long pipe_frames = pl.flip ? 0 : c->pipe_frames;
    const int pq = pl.pq = piped ? (int)(pipe_frames & 1) : 0;
    const int pbase = piped ? 3 * pq : 0;          // this frame's plane set
    // A promised frame runs on the context's stream of its parity.  Every other frame of a pipelined context runs on the caller's own
    // stream, behind the previous frame of the same parity (same plane set), wherever that one ran: with one stream that is what an
    // ordered frame always was; with two streams used in turn (inputs_ready = 2) the caller's streams ARE the pipeline.
    pl.promise = piped && promise;
    pl.s = pl.promise ? c->pipe[pq] : pl.s_user;
    // the first pipelined frame: all of it behind the caller's stream.  So is every promised frame of a context that has ever
    // been recorded into a graph: a replay of that graph on the caller's stream touches the same planes and is visible to this
    // frame only through the caller's stream position
    pl.wait_in_first = pipe_frames == 0 || c->ever_captured;
    pl.timed = c->prof_frames && (c->frame_no % (c->prof_stride > 0 ? c->prof_stride : 1)) == 0;
    pl.slot = pl.timed ? (int)(c->prof_count % c->prof_frames) : 0;

    // 1) temporal accumulation, or constant variance (reference :360-371).  Writes a cv plane `acc` that does not hold the
    //    colour history, and the current-frame G-buffer planes.  When the frame runs the a-trous cascade on the fast path the
    //    temporal pass is not launched at all: the first level's loader waves accumulate the pixels they stage (fused
    //    kernel, svgf_atrous_fused.hip) and `acc` stays unwritten unless something other than that level needs it.
    //    (Rounds 1-3 ran this pass alone on a side stream beside the previous frame's trailing levels — it lost 3-8 % once the lane
    //    kernel ran all five levels; round 5's frame pipeline, above, runs whole frames of alternating parity on two streams.)
    const int old_hist = c->hist;
    const int acc = pl.acc = piped ? (pbase == old_hist ? pbase + 1 : pbase) : (old_hist + 1) % 3;
    const int gnew = pl.gcur = 1 - c->gcur;
    const bool cascade = !(p->right_view_option == 1 || p->right_view_option == 2 || p->atrous_nlevel == 0 || !p->spatial_enable);
    TemporalArgs &t = pl.t;
    memset(&t, 0, sizeof(t));
    pl.temporal = p->temporal_enable != 0; pl.fused = pl.split_fused = false; pl.svf = p->spatial_variance_frames;
    t.in_rgb = in; t.gbuf = g; t.cv_acc = c->cv[acc];
    t.nrm_cur = c->nrm[gnew]; t.gid_cur = c->gid[gnew]; t.pos_cur = c->pos[gnew];
    t.W = c->W; t.H = c->H;
    if (firefly) { t.firefly_rank = c->firefly_rank; t.firefly_scale = c->firefly_scale; }
    AtrousArgs probe;
    memset(&probe, 0, sizeof(probe));
    probe.W = c->W; probe.H = c->H; probe.step = 2;
    if (pl.temporal) {
        t.cv_hist = c->cv[c->hist];
        t.mom_hist = c->mom[c->cur]; t.mom_acc = c->mom[1 - c->cur];
        t.hlen = c->hlen[c->cur]; t.hlen_upd = c->hlen[1 - c->cur];
        t.nrm_prev = c->nrm[c->gcur]; t.gid_prev = c->gid[c->gcur];
        memcpy(t.M, c->view_prev, sizeof(t.M));
        t.color_alpha_min = p->color_alpha; t.moment_alpha_min = p->moment_alpha;
        t.reproj_sx = p->reproj_scale[0]; t.reproj_sy = p->reproj_scale[1];
        t.pos_prev = c->pos[c->gcur]; t.pos_tol = p->reproj_position_tol;
        t.dump = c->dump; t.arena = c->arena; t.arena_bytes = c->arena_bytes;
        if (motion) { t.motion = motion_dev; t.motion_format = motion_format; }
        if (clamp) { t.clamp_radius = c->clamp_radius; t.clamp_k = c->clamp_k; }
        if (xform) { t.xf = c->xf_dev; t.n_geoms = c->xf_n; }
#ifdef SVGF_BUILD_EXPERIMENTS      // parked: the temporal pass in the first level's loaders, DESIGN.md 5.8
        if (!motion && !clamp && !xform && !firefly && cascade && (p->kernel_variant == 0 || p->kernel_variant == 6) && !p->paper_steps && p->spatial_variance_frames <= 0)
            pl.fused = atrous_fused_supported(probe, t) && (p->kernel_variant == 6 || fuse_pays(c, probe));
#endif
    } else if (g && !firefly && cascade && (p->kernel_variant == 0 || p->kernel_variant == 6) && !p->paper_steps) {
        // Non-temporal mode.  On the AoS boundary the prepare pass (variance = 10, colour copy, G-buffer split) is loads and
        // stores only and rides in the first level's loader waves when the cascade starts with the lane kernel at step 2
        // (svgf_atrous_fused.hip, FUSED = 3): no prepare launch, no colour plane written and read back.  (Not with the firefly filter:
        // those loaders stage no neighbourhood of the input; the frame then runs the tiled prepare kernel, one launch more.)
        pl.fused = atrous_prepare_fused_supported(probe, t) && atrous_strip_supported(probe) && atrous_lane_supported(probe) &&
                   (p->kernel_variant == 6 || (kPrepareFusedByDefault && lane_pays(c, probe)));
    }
    pl.tdone = piped && !g && !pl.cap_id; pl.capture = c->capture != 0;
    unsigned vp_valid = c->vp_valid & ~(1u << acc);     // the temporal / prepare pass writes no variance plane: the first level gathers cv.w
    int hist = acc;                                    // color_history <- color_acc / input (:366,370)

    // 2) debug views, pass-through or the a-trous cascade (:373-394)
    pl.exit = p->right_view_option == 1 ? EXIT_DEBUG_HLEN : p->right_view_option == 2 ? EXIT_DEBUG_VAR : !cascade ? EXIT_COPY : EXIT_CASCADE;
    pl.n_levels = cascade ? p->atrous_nlevel : 0;
    int src = hist;
#ifdef SVGF_BUILD_EXPERIMENTS
    int terms_out[SVGF_MAX_LEVELS];      // tp[] index a level stores its geometric terms in for the next one, -1: none
#endif
    for (int i = 0; i < pl.n_levels; i++) {
        LevelPlan &lv = pl.lv[i];
        AtrousArgs &a = lv.a;
        const int level = i + 1;
        lv.last = (level == p->atrous_nlevel);
        lv.keep = (level == p->history_level);
        const bool fuse_here = pl.fused && level == 1;
        int dst = -1;
        if (!lv.last || lv.keep) {
            // (the fused level reads the OLD colour history while it writes: its destination is the third plane)
            for (int k = pbase; k < pbase + 3; k++) if (k != src && k != hist && !(fuse_here && k == old_hist)) { dst = k; break; }
        }
        lv.dst = dst;
        a.src = c->cv[src]; a.dst = dst >= 0 ? c->cv[dst] : nullptr; a.out_rgb = lv.last ? pl.out_c : nullptr;
        a.nrm = c->nrm[gnew]; a.pos = c->pos[gnew]; a.gbuf = g; a.albedo = c->albedo;
        a.W = c->W; a.H = c->H;
        a.step = 1 << (p->paper_steps ? level - 1 : level);   // reference: level starts at 1 => steps 2,4,8,16,32 (:98,386)
        a.sigma_c = p->sigma_l; a.sigma_n = p->sigma_n; a.sigma_x = p->sigma_x;
        a.blur_variance = p->blur_variance ? 1 : 0;
        a.modulate = (lv.last && p->sepcolor && p->addcolor) ? 1 : 0;
        // pre-blur source of steps >= 16: the zero-margined 4-byte variance plane the producer level wrote next to its colour
        // plane (see below); the lane kernel at those steps REQUIRES it (its loaders blur the variance from it)
        a.var = (c->use_vplane && a.step >= 16 && ((vp_valid >> src) & 1u)) ? c->vp[src] : nullptr;
        a.var_dst = nullptr;
        a.tin = nullptr; a.tout = nullptr; a.t_m = 0; a.t_m_out = 0;
        lv.kind = level_kernel(c, p, a, fuse_here);
        if (p->kernel_variant == 2 && lv.kind != K_STRIP) {
            snprintf(c->err, sizeof(c->err), "svgf_denoise: strip kernel does not support %dx%d step %d", c->W, c->H, a.step);
            return SVGF_ERR_UNSUPPORTED;
        }
        lv.asked = p->kernel_variant == 0 && (lv.kind == K_FUSED || lv.kind == K_LANE || lv.kind == K_STRIP) && c->lane_cheaper[step_log2(a.step)] >= 0;
        // Pre-blur rows (y-1, y+1 of the full-resolution image) of the lane / strip kernels.  At steps >= 16 they are
        // read as 4-byte gathers out of 16-byte colour texels whose lines nobody else on the XCD touches (PMC: 75.6 /
        // 72.6 B/px fetched against 40 algorithmic); there the kernels read them from a zero-margined 4-byte variance plane
        // that the producer level writes next to its colour plane (51.3 / 48.8 B/px, +4 B/px written).  At steps 2-8
        // the neighbouring rows are the sibling y-phases' own rows, already in L2: a plane would ADD 8 B/px (measured,
        // profiles/r02_pmc_hbm.txt), so those levels keep reading colour.w and only the level feeding a step-16 level
        // writes the plane.
        if (lv.kind != K_LANE && lv.kind != K_STRIP) a.var = nullptr;
        else if (c->use_vplane && dst >= 0 && !lv.last && a.step >= 8) a.var_dst = c->vp[dst];
        if (dst >= 0) { if (a.var_dst) vp_valid |= 1u << dst; else vp_valid &= ~(1u << dst); }
#ifdef SVGF_BUILD_EXPERIMENTS
        terms_out[i] = -1;
        // Cross-level reuse of the geometric terms (svgf_atrous_lane_reuse.hip): a lane-kernel level stores four terms for the next
        // level if that one runs the lane kernel at twice its step, and that level reads them.
        if (c->use_reuse && i > 0 && lv.kind == K_LANE && pl.lv[i - 1].kind == K_LANE && a.step == 2 * pl.lv[i - 1].a.step && a.step <= 32) {
            terms_out[i - 1] = (i >= 2 && terms_out[i - 2] == 0) ? 1 : 0;
            a.tin = pl.lv[i - 1].a.tout = c->tp[terms_out[i - 1]];
            pl.lv[i - 1].a.t_m_out = a.t_m = (c->W + a.step - 1) / a.step;
        }
#endif
        // the accumulated plane itself is only written by the fused level when something besides that level reads it: a later
        // frame (the history is not this level's output) or a test (svgf_set_capture)
        if (fuse_here) t.cv_acc = (!lv.keep || c->capture) ? c->cv[acc] : nullptr;
        if (lv.keep) hist = dst;
        src = dst;
    }
#ifdef SVGF_BUILD_EXPERIMENTS
    // The G-buffer split alone can ride in the first level's loaders (svgf_atrous_fused.hip, FUSED = 4): the temporal pass then
    // writes 28 B/px less.  Only where that level runs the lane kernel at step 2 and nothing reads the planes before it does.
    pl.split_fused = pl.temporal && !pl.fused && c->use_split_fused && g && cascade && p->kernel_variant == 0 && !p->paper_steps &&
                     p->spatial_variance_frames <= 0 && pl.lv[0].kind == K_LANE && atrous_split_fused_supported(pl.lv[0].a, t);
#endif
    t.skip_split = pl.split_fused ? 1 : 0;
    // The other stream's next temporal pass may go on once everything it reads of this frame is final: behind the level that
    // writes the colour history; behind the temporal pass where no level of the cascade writes it (it IS the accumulated plane then,
    // which no level of this frame overwrites, and everything else was final before); frames without a cascade (debug views,
    // pass-through) and non-temporal frames without such a level release it at their end: they read state that pass rewrites.
    pl.hist_release = pl.n_levels;
    if (cascade && p->history_level >= 1 && p->history_level <= p->atrous_nlevel) pl.hist_release = p->history_level - 1;
    else if (cascade && pl.temporal) pl.hist_release = -1;
    pl.hist = hist; pl.vp_valid = vp_valid;
    pl.cur = pl.temporal ? 1 - c->cur : c->cur;      // 3) history rotation (:396-399): planes swap roles instead of being copied
    pl.last_modulated = (cascade && p->sepcolor && p->addcolor) ? 1 : 0;
    // The output pass.  It reads this frame's position / geomId planes (written by the temporal or prepare pass, the first level's
    // loaders or the producer), the call's motion plane even on a frame with temporal_enable == 0, and the output history of the
    // last frame if that frame left one; a frame without the pass drops the history.
    pl.taa_cur = c->taa_cur; pl.taa_valid = 0;
    if (taa) {
        OutputTaaArgs &o = pl.o;
        memset(&o, 0, sizeof(o));
        o.pre = c->taa_pre; o.out = pl.out;
        o.hist = c->taa_valid ? c->taa_hist[c->taa_cur] : nullptr; o.hist_new = c->taa_hist[1 - c->taa_cur];
        o.pos = c->pos[gnew]; o.gid = c->gid[gnew];
        if (motion_dev) { o.motion = motion_dev; o.motion_format = motion_format; }
        if (c->xf_dev && c->xf_n > 0) { o.xf = c->xf_dev; o.n_geoms = c->xf_n; }
        memcpy(o.M, c->view_prev, sizeof(o.M));
        o.W = c->W; o.H = c->H;
        o.reproj_sx = p->reproj_scale[0]; o.reproj_sy = p->reproj_scale[1];
        o.alpha = c->taa_alpha; o.k = c->taa_k;
        pl.taa_cur = 1 - c->taa_cur; pl.taa_valid = 1;
    }
    return SVGF_OK;
}

// Walks the plan.  Of the context it writes the pipeline's event records (and the switch into piped mode), and the profiling slot.
static int enqueue_frame(svgf_ctx *c, const FramePlan &pl)
{
    const int pq = pl.pq, n = (int)c->n;
    const hipStream_t s = pl.s; const TemporalArgs &t = pl.t;
    if (pl.flip) { c->piped_mode = 1; pipe_reset(c); }      // (a state flip, nothing is allocated: the colour history lies in plane set 0)
    if (pl.piped) {
        c->ev_tdone[pq].valid = 0;      // (re-armed below by a planar frame's temporal pass)
        if (pl.promise) {
            HIPC(c, hipEventRecord(c->ev_in, pl.s_user));      // the caller's stream position at hand-over: the last level waits for it (`out`)
            if (pl.wait_in_first) HIPC(c, hipStreamWaitEvent(s, c->ev_in, 0));
        }
        HIPC(c, pipe_wait(s, c->ev_done[pq], pl.cap_id));
    }
    KernelTimer timer{ c, s, pl.slot, 0, pl.timed };
    if (pl.timed) c->ev_n[pl.slot] = 0;
    // the other stream's frame: this frame's temporal pass (and everything behind it) starts when that frame's colour history,
    // moments, history lengths and G-buffer planes are final
    if (pl.piped) HIPC(c, pipe_wait(s, c->ev_hist[1 - pq], pl.cap_id));
    if (pl.temporal && !pl.fused) {
        LAUNCH(SVGF_KERNEL_TEMPORAL, launch_temporal(t, s));
        if (pl.tdone) HIPC(c, pipe_record(c->ev_tdone[pq], s, 0));
        if (pl.svf > 0)      // f4 extension: spatial variance estimate for short histories (its own profiling slot, same kind)
            LAUNCH(SVGF_KERNEL_TEMPORAL, launch_spatial_variance(t.cv_acc, t.mom_acc, t.hlen_upd, t.nrm_cur, t.gid_cur, t.W, t.H, pl.svf, s));
    } else if (!pl.fused) {
        if (t.firefly_rank) LAUNCH(SVGF_KERNEL_PREPARE, launch_prepare_filtered(t.in_rgb, t.gbuf, t.cv_acc, t.nrm_cur, t.gid_cur, t.pos_cur, t.W, t.H,
                                                                                t.firefly_rank, t.firefly_scale, s));
        else LAUNCH(SVGF_KERNEL_PREPARE, launch_prepare(t.in_rgb, t.gbuf, t.cv_acc, t.nrm_cur, t.gid_cur, t.pos_cur, t.W, t.H, s));
    }
    // (before the early release below: the next frame's copy into the one capture buffer must not overtake this one)
    if (pl.capture && !pl.fused) HIPC(c, hipMemcpyAsync(c->cv_capture, c->cv[pl.acc], c->n * sizeof(float4), hipMemcpyDeviceToDevice, s));
    if (pl.piped && pl.hist_release < 0) HIPC(c, pipe_record(c->ev_hist[pq], s, pl.cap_id));
    switch (pl.exit) {
    case EXIT_DEBUG_HLEN: LAUNCH(SVGF_KERNEL_DEBUGVIEW, launch_debug_hlen(c->hlen[c->cur], pl.out, n, 100.0f, s)); break;   // pre-update lengths (:374)
    case EXIT_DEBUG_VAR:  LAUNCH(SVGF_KERNEL_DEBUGVIEW, launch_debug_var(c->cv[pl.acc], pl.out, n, 0.1f, s)); break;         // (:377)
    case EXIT_COPY:                                                                                                          // (:382)
        if (pl.taa && pl.piped) HIPC(c, pipe_wait(s, c->ev_done[1 - pq], pl.cap_id));      // (`pre`: see the last level below)
        LAUNCH(SVGF_KERNEL_COPYOUT, launch_copy_rgb(c->cv[pl.acc], pl.out_c, n, s));
        break;
    case EXIT_CASCADE:    break;
    }
    for (int i = 0; i < pl.n_levels; i++) {
        const LevelPlan &lv = pl.lv[i]; const AtrousArgs &a = lv.a;
        // The one kernel of a promised frame that writes the caller's `out`: behind what the caller's stream held when the frame
        // was handed over (a reader of the same buffer enqueued behind an earlier call, for instance).  The promise is about the
        // INPUTS only; the output buffer is protected by stream order like everywhere else.
        // With the output pass that kernel is the pass itself (below); the last level writes the ONE `pre` plane instead, which the
        // other parity's output pass reads: behind that frame's end (long past by now where frames overlap at all).
        if (pl.promise && lv.last && !pl.taa) HIPC(c, hipStreamWaitEvent(s, c->ev_in, 0));
        if (pl.taa && pl.piped && lv.last) HIPC(c, pipe_wait(s, c->ev_done[1 - pq], pl.cap_id));
        switch (lv.kind) {
        case K_FUSED:
#ifdef SVGF_BUILD_EXPERIMENTS
            if (pl.temporal) LAUNCH(SVGF_KERNEL_FUSED, launch_atrous_fused(a, t, s));
            else
#endif
            LAUNCH(SVGF_KERNEL_FUSED, launch_atrous_prepare_fused(a, t, s));
            if (pl.capture) HIPC(c, hipMemcpyAsync(c->cv_capture, c->cv[pl.acc], c->n * sizeof(float4), hipMemcpyDeviceToDevice, s));
            break;
        case K_LANE:       // steps 2 .. 32: symmetric terms evaluated once
#ifdef SVGF_BUILD_EXPERIMENTS
            if (pl.split_fused && i == 0) { LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_split_fused(a, t, s)); break; }
            if (a.tin || a.tout) { LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_lane_reuse(a, s)); break; }
#endif
            LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_lane(a, s));
            break;
#ifdef SVGF_BUILD_EXPERIMENTS
        case K_LANE2Y:  LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_lane_2y(a, s)); break;  // A/B partner of the fused kernel's geometry
#endif
        case K_STRIP:   LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_strip(a, s)); break;
        case K_LATTICE: LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_lattice(a, s)); break;
        default:        LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_gather(a, s)); break;
        }
        if (pl.piped && i == pl.hist_release) HIPC(c, pipe_record(c->ev_hist[pq], s, pl.cap_id));
    }
    if (pl.piped && pl.hist_release == pl.n_levels) HIPC(c, pipe_record(c->ev_hist[pq], s, pl.cap_id));
    if (pl.taa) {
        // reads the output history the other parity's frame wrote and overwrites the one it read: behind that frame's end (the
        // writer of `pre` above has waited for it already where the frame is pipelined); writes the caller's `out`
        if (pl.promise) HIPC(c, hipStreamWaitEvent(s, c->ev_in, 0));
        LAUNCH(SVGF_KERNEL_OUTPUT_TAA, launch_output_taa(pl.o, s));
    }
    if (pl.piped) {
        HIPC(c, pipe_record(c->ev_done[pq], s, pl.cap_id));
        if (s != pl.s_user) HIPC(c, hipStreamWaitEvent(pl.s_user, c->ev_done[pq].ev, 0));      // what the caller enqueues behind this call sees `out`
    }
    return SVGF_OK;
}

// The context behind a frame whose every call was accepted: the planes' roles rotate, the counters advance.
static void commit_frame(svgf_ctx *c, const FramePlan &pl, const SvgfCamera *cam)
{
    c->acc = pl.acc; c->hist = pl.hist; c->cur = pl.cur; c->gcur = pl.gcur; c->vp_valid = pl.vp_valid; c->last_modulated = pl.last_modulated;
    c->taa_cur = pl.taa_cur; c->taa_valid = pl.taa_valid;
    if (pl.piped) { c->pipe_frames++; if (pl.cap_id) c->ever_captured = 1; }
    view_matrix_from_camera(cam, c->view_prev);
    if (pl.timed) c->prof_count++;
    c->frame_no++;
#ifdef SVGF_BUILD_EXPERIMENTS
    c->lk_n = pl.n_levels;
    for (int i = 0; i < pl.n_levels; i++) { c->lk_kind[i] = (int)pl.lv[i].kind; c->lk_step[i] = pl.lv[i].a.step; c->lk_asked[i] = pl.lv[i].asked; }
#endif
}

static int denoise_frame(svgf_ctx *c, void *out_rgb_dev, const void *in_rgb_dev, const void *gbuffer_dev,
                         const void *motion_dev, int motion_format, const SvgfCamera *cam, const SvgfParams *p, void *stream)
{
    if (!out_rgb_dev || !in_rgb_dev || !cam || !p) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: null argument");
        return SVGF_ERR_INVALID_ARG;
    }
    SVGF_ENTER(c);
    FramePlan pl;
    int rc = plan_frame(c, out_rgb_dev, in_rgb_dev, gbuffer_dev, motion_dev, motion_format, p, stream, pl);
    if (rc == SVGF_OK) rc = enqueue_frame(c, pl);
    if (rc == SVGF_OK) commit_frame(c, pl, cam);
    return rc;
}

extern "C" int svgf_denoise_motion(svgf_ctx *c, void *out_rgb_dev, const void *in_rgb_dev, const void *gbuffer_dev,
                                   const void *motion_dev, int motion_format, const SvgfCamera *cam, const SvgfParams *p, void *stream)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (!gbuffer_dev) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise: null argument");
        return SVGF_ERR_INVALID_ARG;
    }
    return denoise_frame(c, out_rgb_dev, in_rgb_dev, gbuffer_dev, motion_dev, motion_format, cam, p, stream);
}

extern "C" int svgf_denoise(svgf_ctx *c, void *out_rgb_dev, const void *in_rgb_dev, const void *gbuffer_dev,
                            const SvgfCamera *cam, const SvgfParams *p, void *stream)
{
    return svgf_denoise_motion(c, out_rgb_dev, in_rgb_dev, gbuffer_dev, nullptr, 0, cam, p, stream);
}

// The motion plane of a frame whose geometry moved rigidly, written with the camera path's own projection (k_motion_reproject,
// svgf_kernels.hip) and the view matrix svgf_denoise would have retained for `prev_cam`.  Stateless.
extern "C" int svgf_motion_reproject(int device, void *motion_out_dev, int motion_format, const void *gbuffer_dev,
                                     const float *position_dev, const int *geom_id_dev, int width, int height,
                                     const SvgfCamera *prev_cam, const float reproj_scale[2], const float *geom_xf_dev, int n_geoms,
                                     void *stream)
{
    if (!motion_out_dev || !temporal_motion_format_known(motion_format) || (!gbuffer_dev && (!position_dev || !geom_id_dev)) ||
        width <= 0 || height <= 0 || !prev_cam || n_geoms < 0)
        return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    MotionReprojArgs a;
    memset(&a, 0, sizeof(a));
    a.out = motion_out_dev; a.format = motion_format;
    a.gbuf = (const float *)gbuffer_dev; a.pos = position_dev; a.gid = geom_id_dev;
    view_matrix_from_camera(prev_cam, a.M);
    a.W = width; a.H = height;
    a.reproj_sx = reproj_scale ? reproj_scale[0] : 0.0f; a.reproj_sy = reproj_scale ? reproj_scale[1] : 0.0f;
    a.xf = n_geoms > 0 ? geom_xf_dev : nullptr; a.n_geoms = a.xf ? n_geoms : 0;
    return launch_motion_reproject(a, (hipStream_t)stream) == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

// Guided upsampling (k_upsample, svgf_upsample.hip): the full-size image from a reduced-size denoise.  Stateless; every argument is
// answered before the first HIP call.
static bool upsample_guide_ok(const SvgfGuide *g) { return g->gbuffer || (g->normal && g->position && g->geom_id); }
static UpsampleGuide upsample_guide(const SvgfGuide *g)
{
    UpsampleGuide u;
    u.gbuf = (const float *)g->gbuffer;
    u.nrm = g->normal; u.pos = g->position; u.gid = g->geom_id; u.albedo = g->albedo;
    return u;
}
extern "C" int svgf_upsample(int device, void *out_rgb_hi_dev, const SvgfGuide *hi, int width_hi, int height_hi,
                             const void *rgb_lo_dev, const SvgfGuide *lo, int width_lo, int height_lo,
                             const SvgfUpsampleParams *up, void *stream)
{
    if (!out_rgb_hi_dev || !rgb_lo_dev || !hi || !lo || !up) return SVGF_ERR_INVALID_ARG;
    if (!upsample_guide_ok(hi) || !upsample_guide_ok(lo)) return SVGF_ERR_INVALID_ARG;
    if (up->modulate != 0 && up->modulate != 1) return SVGF_ERR_INVALID_ARG;
    if (up->modulate && !hi->gbuffer && !hi->albedo) return SVGF_ERR_INVALID_ARG;
    if (width_hi <= 0 || height_hi <= 0 || width_lo <= 0 || height_lo <= 0 || width_lo > width_hi || height_lo > height_hi)
        return SVGF_ERR_INVALID_ARG;
    if (!(up->sigma_n >= 0.0f) || !(up->sigma_x >= 0.0f) || std::isinf(up->sigma_n) || std::isinf(up->sigma_x)) return SVGF_ERR_INVALID_ARG;
    if ((long long)width_hi * height_hi >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    UpsampleArgs a;
    memset(&a, 0, sizeof(a));
    a.out = (float *)out_rgb_hi_dev; a.rgb_lo = (const float *)rgb_lo_dev;
    a.hi = upsample_guide(hi); a.lo = upsample_guide(lo);
    a.Wh = width_hi; a.Hh = height_hi; a.Wl = width_lo; a.Hl = height_lo;
    a.rx = (float)width_lo / (float)width_hi; a.ry = (float)height_lo / (float)height_hi;
    a.sigma_n = up->sigma_n; a.sigma_x = up->sigma_x; a.modulate = up->modulate;
    return launch_upsample(a, (hipStream_t)stream) == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

// History transfer (k_transfer_history, svgf_transfer.hip): everything dst's next frame reads as history becomes src's, resampled to
// dst's size.  One launch on `stream`; the planes written are the ones the indices hist, cur, gcur and taa_cur name.  Not a frame: no
// profile entry, frame_no unchanged.  On contexts without pipeline resources it neither synchronises nor allocates.
extern "C" int svgf_transfer_history(svgf_ctx *dst, svgf_ctx *src, void *stream)
{
    if (!dst || !src) return SVGF_ERR_INVALID_ARG;      // (neither context is touched)
    if (dst == src) {
        snprintf(dst->err, sizeof(dst->err), "svgf_transfer_history: dst and src are the same context");
        return SVGF_ERR_INVALID_ARG;
    }
    if (dst->device != src->device) {
        snprintf(dst->err, sizeof(dst->err), "svgf_transfer_history: dst lives on device %d, src on device %d", dst->device, src->device);
        return SVGF_ERR_UNSUPPORTED;
    }
    SVGF_ENTER(dst);
    const hipStream_t s = (hipStream_t)stream;
    if (s) {      // (the legacy stream cannot be captured)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            snprintf(dst->err, sizeof(dst->err), "svgf_transfer_history: `stream` is being captured into a graph; the call changes host state a replay would not");
            return SVGF_ERR_UNSUPPORTED;
        }
    }
    // Frames of a pipelined context may be running on its internal streams or on another stream of the caller's: wait for the device,
    // as svgf_planar_gbuffer does.  dst's events are forgotten: its next frame orders itself behind the caller's stream as a whole
    // (pipe_frames == 0), that is, behind the launch below.
    const bool piped = dst->pipelined || src->pipelined;
    if (piped) {
        HIPC(dst, hipDeviceSynchronize());
        pipe_reset(dst);
    }
    TransferArgs a;
    memset(&a, 0, sizeof(a));
    a.cv_s = src->cv[src->hist]; a.mom_s = src->mom[src->cur]; a.hlen_s = src->hlen[src->cur];
    a.nrm_s = src->nrm[src->gcur]; a.pos_s = src->pos[src->gcur]; a.gid_s = src->gid[src->gcur];
    a.cv_d = dst->cv[dst->hist]; a.mom_d = dst->mom[dst->cur]; a.hlen_d = dst->hlen[dst->cur];
    a.nrm_d = dst->nrm[dst->gcur]; a.pos_d = dst->pos[dst->gcur]; a.gid_d = dst->gid[dst->gcur];
    // the output history moves when dst has the pass on and src holds one; otherwise dst has none afterwards
    const bool taa = dst->taa_hist[0] && dst->taa_alpha != 0.0f && src->taa_valid && src->taa_hist[0];
    if (taa) { a.taa_s = src->taa_hist[src->taa_cur]; a.taa_d = dst->taa_hist[dst->taa_cur]; }
    a.Ws = src->W; a.Hs = src->H; a.Wd = dst->W; a.Hd = dst->H;
    a.rx = (float)src->W / (float)dst->W; a.ry = (float)src->H / (float)dst->H;
    a.identity = (src->W == dst->W && src->H == dst->H) ? 1 : 0;
    HIPC(dst, launch_transfer_history(a, s));
    // the internal streams of a pipelined context carry its promised frames: whatever they run next runs behind the launch
    for (svgf_ctx *c : { dst, src }) {
        if (!c->pipelined) continue;
        HIPC(dst, hipEventRecord(c->ev_in, s));
        for (int q = 0; q < 2; q++) HIPC(dst, hipStreamWaitEvent(c->pipe[q], c->ev_in, 0));
    }
    memcpy(dst->view_prev, src->view_prev, sizeof(dst->view_prev));
    dst->vp_valid = 0;      // derived from planes that hold something else now
    dst->taa_valid = taa ? 1 : 0;
    return SVGF_OK;
}

// ---- the planar path (the AoS -> plane repack fused into the producer) -----------------------
static int planar_gbuffer(svgf_ctx *c, SvgfPlanarGBuffer *out, bool have_stream, hipStream_t stream)
{
    if (!c || !out) return SVGF_ERR_INVALID_ARG;
    SVGF_ENTER(c);
    if (!c->albedo) {
        // (first call only.  The clear runs on the legacy stream; the producer that fills the plane may run on a non-blocking
        // stream that does not order itself behind it: the clear is complete before the pointer leaves this function.)
        HIPC(c, hipMalloc((void **)&c->albedo, c->n * 3 * sizeof(float)));
        HIPC(c, hipMemset(c->albedo, 0, c->n * 3 * sizeof(float)));
        HIPC(c, hipStreamSynchronize(nullptr));
    }
    // The planes handed out were the CURRENT planes of the frame before last (its levels read them) and are the PREVIOUS planes of
    // the last frame (its temporal pass reads them); the producer writes them on a stream of its own choosing.  On an ordered context
    // that stream has waited for every frame (stream order).  Frames of a PIPELINED context may still be running on another stream of
    // the caller's or on the context's own: svgf_planar_gbuffer waits for the device; svgf_planar_gbuffer_stream makes `stream` wait
    // for exactly the two things that still read the planes — the end of the frame before last and the temporal pass of the last
    // frame (and the last frame's end when its last level read the one albedo plane) — so that the producer of frame n+1 runs
    // beside the levels of frame n.
    if (c->piped_mode) {
        if (!have_stream) HIPC(c, hipDeviceSynchronize());
        else {
            const int pq = (int)(c->pipe_frames & 1);      // parity of the NEXT frame = parity of the frame before last
            const svgf_ctx::PipeEvent &last_done = c->ev_done[1 - pq];      // (events recorded under a capture are not waited for: cap id 0)
            HIPC(c, pipe_wait(stream, c->ev_done[pq], 0));
            if (pipe_live(c->ev_tdone[1 - pq], 0)) HIPC(c, pipe_wait(stream, c->ev_tdone[1 - pq], 0));
            else HIPC(c, pipe_wait(stream, last_done, 0));      // (the last frame was not a planar one)
            if (c->last_modulated) HIPC(c, pipe_wait(stream, last_done, 0));
        }
    }
    const int gnew = 1 - c->gcur;        // the planes the next frame's temporal / prepare pass treats as "current"
    out->normal = c->nrm[gnew]; out->position = c->pos[gnew]; out->geom_id = c->gid[gnew]; out->albedo = c->albedo;
    return SVGF_OK;
}

extern "C" int svgf_planar_gbuffer(svgf_ctx *c, SvgfPlanarGBuffer *out) { return planar_gbuffer(c, out, false, nullptr); }
extern "C" int svgf_planar_gbuffer_stream(svgf_ctx *c, SvgfPlanarGBuffer *out, void *stream) { return planar_gbuffer(c, out, true, (hipStream_t)stream); }

extern "C" int svgf_denoise_planar(svgf_ctx *c, void *out_rgb_dev, const void *in_rgb_dev, const SvgfCamera *cam, const SvgfParams *p, void *stream)
{
    return svgf_denoise_planar_motion(c, out_rgb_dev, in_rgb_dev, nullptr, 0, cam, p, stream);
}

extern "C" int svgf_denoise_planar_motion(svgf_ctx *c, void *out_rgb_dev, const void *in_rgb_dev, const void *motion_dev, int motion_format,
                                          const SvgfCamera *cam, const SvgfParams *p, void *stream)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (p && p->sepcolor && p->addcolor && !c->albedo) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise_planar: sepcolor && addcolor needs the albedo plane of svgf_planar_gbuffer");
        return SVGF_ERR_INVALID_ARG;
    }
    return denoise_frame(c, out_rgb_dev, in_rgb_dev, nullptr, motion_dev, motion_format, cam, p, stream);
}

extern "C" int svgf_denoise_host(svgf_ctx *c, float *out_rgb_host, const float *in_rgb_host,
                                 const SvgfGBufferTexel *gbuffer_host, const SvgfCamera *cam, const SvgfParams *p)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (!out_rgb_host || !in_rgb_host || !gbuffer_host) {
        snprintf(c->err, sizeof(c->err), "svgf_denoise_host: null argument");
        return SVGF_ERR_INVALID_ARG;
    }
    SVGF_ENTER(c);
    if (!c->st_in) HIPC(c, hipMalloc((void **)&c->st_in, c->n * 3 * sizeof(float)));
    if (!c->st_out) HIPC(c, hipMalloc((void **)&c->st_out, c->n * 3 * sizeof(float)));
    if (!c->st_g) HIPC(c, hipMalloc((void **)&c->st_g, c->n * sizeof(SvgfGBufferTexel)));
    HIPC(c, hipMemcpy(c->st_in, in_rgb_host, c->n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->st_g, gbuffer_host, c->n * sizeof(SvgfGBufferTexel), hipMemcpyHostToDevice));
    int rc = svgf_denoise(c, c->st_out, c->st_in, c->st_g, cam, p, nullptr);
    if (rc != SVGF_OK) return rc;
    HIPC(c, hipDeviceSynchronize());
    HIPC(c, hipMemcpy(out_rgb_host, c->st_out, c->n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return SVGF_OK;
}

// ---- state inspection -------------------------------------------------------------------------------------------

extern "C" int svgf_read_state(svgf_ctx *c, int which, void *host_dst, unsigned long long host_bytes)
{
    if (!c || !host_dst) return SVGF_ERR_INVALID_ARG;
    SVGF_ENTER(c);
    HIPC(c, hipDeviceSynchronize());
    const size_t n = c->n;
    auto need = [&](size_t b) -> bool {
        if (host_bytes < b) { snprintf(c->err, sizeof(c->err), "svgf_read_state: buffer too small (%llu < %zu)", host_bytes, b); return false; }
        return true;
    };
    switch (which) {
    case SVGF_STATE_HISTORY_LENGTH:
        if (!need(n * sizeof(int))) return SVGF_ERR_INVALID_ARG;
        HIPC(c, hipMemcpy(host_dst, c->hlen[c->cur], n * sizeof(int), hipMemcpyDeviceToHost));
        return SVGF_OK;
    case SVGF_STATE_MOMENTS:
        if (!need(n * 2 * sizeof(float))) return SVGF_ERR_INVALID_ARG;
        HIPC(c, hipMemcpy(host_dst, c->mom[c->cur], n * 2 * sizeof(float), hipMemcpyDeviceToHost));
        return SVGF_OK;
    case SVGF_STATE_COLOR_HISTORY:
    case SVGF_STATE_COLOR_ACC:
    case SVGF_STATE_VARIANCE_TEMPORAL: {
        const bool is_hist = (which == SVGF_STATE_COLOR_HISTORY);
        if (!is_hist && !c->cv_capture) {
            snprintf(c->err, sizeof(c->err), "svgf_read_state: enable svgf_set_capture before the frame");
            return SVGF_ERR_INVALID_ARG;
        }
        const size_t out_bytes = (which == SVGF_STATE_VARIANCE_TEMPORAL) ? n * sizeof(float) : n * 3 * sizeof(float);
        if (!need(out_bytes)) return SVGF_ERR_INVALID_ARG;
        float4 *tmp = (float4 *)malloc(n * sizeof(float4));
        if (!tmp) return SVGF_ERR_OOM;
        hipError_t e = hipMemcpy(tmp, is_hist ? c->cv[c->hist] : c->cv_capture, n * sizeof(float4), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { free(tmp); snprintf(c->err, sizeof(c->err), "hipMemcpy: %s", hipGetErrorString(e)); return SVGF_ERR_HIP; }
        float *d = (float *)host_dst;
        if (which == SVGF_STATE_VARIANCE_TEMPORAL) for (size_t k = 0; k < n; k++) d[k] = tmp[k].w;
        else for (size_t k = 0; k < n; k++) { d[3 * k] = tmp[k].x; d[3 * k + 1] = tmp[k].y; d[3 * k + 2] = tmp[k].z; }
        free(tmp);
        return SVGF_OK;
    }
    case SVGF_STATE_PREV_NORMAL:
    case SVGF_STATE_PREV_POSITION:
        if (!need(n * 3 * sizeof(float))) return SVGF_ERR_INVALID_ARG;
        HIPC(c, hipMemcpy(host_dst, which == SVGF_STATE_PREV_NORMAL ? c->nrm[c->gcur] : c->pos[c->gcur], n * 3 * sizeof(float), hipMemcpyDeviceToHost));
        return SVGF_OK;
    case SVGF_STATE_PREV_GEOM_ID:
        if (!need(n * sizeof(int))) return SVGF_ERR_INVALID_ARG;
        HIPC(c, hipMemcpy(host_dst, c->gid[c->gcur], n * sizeof(int), hipMemcpyDeviceToHost));
        return SVGF_OK;
    case SVGF_STATE_OUTPUT_HISTORY:
        if (!c->taa_valid || !c->taa_hist[c->taa_cur]) {
            snprintf(c->err, sizeof(c->err), "svgf_read_state: the context has no output history");
            return SVGF_ERR_INVALID_ARG;
        }
        if (!need(n * sizeof(float4))) return SVGF_ERR_INVALID_ARG;
        HIPC(c, hipMemcpy(host_dst, c->taa_hist[c->taa_cur], n * sizeof(float4), hipMemcpyDeviceToHost));
        return SVGF_OK;
    default:
        snprintf(c->err, sizeof(c->err), "svgf_read_state: unknown state %d", which);
        return SVGF_ERR_INVALID_ARG;
    }
}
