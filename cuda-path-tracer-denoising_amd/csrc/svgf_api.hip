// svgf_api.hip — the context of libsvgf_hip.so: lifetime, the plane arena, settings, state read-back, and the stateless entry points.
// The frame itself is svgf_frame.hip; the frame pipeline's resources svgf_pipeline.hip; the profiler svgf_profiler.hip.
//
// Mirrors the host sequence of reference denoise() (src/denoise.cu:349-402) with two structural changes that
// do not alter results:
//   * no device-to-device copies: the five per-frame cudaMemcpy's (src/denoise.cu:366,391,396-398) become
//     index rotation over ping-pong planes;
//   * variance is never updated in place: each a-trous level reads {colour,variance} plane A and writes plane B,
//     which is the "snapshot" semantics the parity contract fixes (SURVEY.md §7 hard parts, §8c).
#include <new>

#include "svgf_context.h"

static_assert(SVGF_MOTION_PREV_COORD_F32 == SVGF_MOTION_FMT_COORD && SVGF_MOTION_DELTA_F32 == SVGF_MOTION_FMT_D32 &&
              SVGF_MOTION_DELTA_F16 == SVGF_MOTION_FMT_D16, "include/svgf.h and svgf_kernels.h name the same motion formats");

static char g_create_err[512] = "";

extern "C" int svgf_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }
// 1: this library was built with -DSVGF_BUILD_EXPERIMENTS (parked kernel variants 5 / 6, tuning table); the product build says 0
extern "C" int svgf_build_has_experiments(void) { return kExperimentsBuild ? 1 : 0; }
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

hipError_t ctx_alloc(svgf_ctx *c, void **p, size_t bytes)
{
    void *q = nullptr;
    if (c->n_owned >= (int)(sizeof(c->owned) / sizeof(c->owned[0])) || hipMalloc(&q, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return hipErrorOutOfMemory;
    }
    hipError_t e = hipMemset(q, 0, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { (void)hipFree(q); return e; }
    c->owned[c->n_owned++] = *p = q;
    return hipSuccess;
}

// The context's planes live in ONE allocation (the arena), each with kPlanePad bytes in front of and behind its W*H elements:
//   * the fused temporal + first-level kernel reads the 3x3 window around a reprojected position as three 3-element row
//     pieces, and a piece that starts one element left of an image row's first pixel (or ends one right of its last) must stay
//     inside memory the context owns at the plane's two ends;
//   * it addresses every plane as arena + 32-bit byte offset (svgf_atrous_lane_impl.h: LaneFused), which needs them within
//     4 GiB of one base — true by construction up to the sizes atrous_fused_supported() admits.
static const size_t kPlaneAlign = 4096;
static size_t plane_span(size_t bytes) { return (bytes + 2 * kPlanePad + kPlaneAlign - 1) / kPlaneAlign * kPlaneAlign; }
static void *plane_carve(Planes &b, size_t *cursor, size_t bytes)
{
    char *p = b.arena + *cursor + kPlanePad;
    *cursor += plane_span(bytes);
    return p;
}

static void free_all(svgf_ctx *c)
{
    for (int k = 0; k < c->n_owned; k++) (void)hipFree(c->owned[k]);
    pipeline_free(c->pipe);
    profiler_free(c->prof);
}

extern "C" int svgf_reset(svgf_ctx *c)
{
    SVGF_ENTER(c);
    HIPC(c, hipDeviceSynchronize());
    Planes &b = c->planes;
    HIPC(c, hipMemset(b.arena, 0, b.arena_bytes));      // cv[0..2] and both sets of nrm, gid, mom, hlen, pos
    for (int k = 3; k < 6; k++) if (b.cv[k]) HIPC(c, hipMemset(b.cv[k], 0, c->n * sizeof(float4)));
    for (int k = 0; k < 6; k++) if (b.vp[k]) HIPC(c, hipMemset(b.vp[k], 0, variance_plane_bytes(c)));
    b.vp_valid = 0;
    c->pipe.reset();
    // gcur is deliberately NOT reset: the pointers svgf_planar_gbuffer handed out (planes 1 - gcur) stay the ones the next
    // frame reads, so planar_gbuffer() -> reset() -> producer -> denoise_planar() works (both plane sets are zero again)
    b.hist = 0; b.acc = 0; b.cur = 0;
    c->taa.valid = 0;      // (the output history is dropped; svgf_set_output_taa's setting stays)
    // The clears above run on the legacy stream; a caller may enqueue the next svgf_denoise on a non-blocking stream that does not
    // order itself behind them: they are complete before svgf_reset returns.
    HIPC(c, hipStreamSynchronize(nullptr));
    return SVGF_OK;
}

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
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cu < 8) c->n_cu = 256;
    memset(c->lane_cheaper, -1, sizeof(c->lane_cheaper));
    Planes &b = c->planes;
    const size_t n = c->n;
    b.arena_bytes = 3 * plane_span(n * sizeof(float4)) + 2 * (2 * plane_span(n * 3 * sizeof(float)) + 2 * plane_span(n * sizeof(int)) + plane_span(n * sizeof(float2)))
                    + plane_span(4096);
    bool ok = ctx_alloc(c, (void **)&b.arena, b.arena_bytes) == hipSuccess;
    if (ok) {
        size_t cur = 0;
        for (int k = 0; k < 3; k++) b.cv[k] = (float4 *)plane_carve(b, &cur, n * sizeof(float4));
        for (int k = 0; k < 2; k++) {
            b.nrm[k] = (float *)plane_carve(b, &cur, n * 3 * sizeof(float));
            b.gid[k] = (int *)plane_carve(b, &cur, n * sizeof(int));
            b.mom[k] = (float2 *)plane_carve(b, &cur, n * sizeof(float2));
            b.hlen[k] = (int *)plane_carve(b, &cur, n * sizeof(int));
            b.pos[k] = (float *)plane_carve(b, &cur, n * 3 * sizeof(float));
        }
        b.dump = plane_carve(b, &cur, 4096);
        if (cur != b.arena_bytes) ok = false;         // (the size formula above and the carving below it disagree)
    }
    for (int k = 0; k < 3 && ok; k++) ok = ctx_alloc(c, (void **)&b.vp[k], variance_plane_bytes(c)) == hipSuccess;
    if (ok) ok = exp_create(c) == hipSuccess;
    int rc = ok ? SVGF_OK : SVGF_ERR_OOM;
    if (ok && (flags & SVGF_CREATE_PIPELINED)) rc = svgf_enable_pipeline(c);
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

// ---- settings (include/svgf.h).  Host state only: no device work, nothing to order. ----
static bool finite_nonneg(float x) { return x >= 0.0f && x <= 3.402823466e38f; }      // false for NaN, negative, +inf

extern "C" int svgf_set_history_clamp(svgf_ctx *c, int radius, float sigma_scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (radius < 0 || radius > 3) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_set_history_clamp: radius %d outside 0..3", radius);
    if (!finite_nonneg(sigma_scale))
        return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_set_history_clamp: sigma_scale %g is not a finite number >= 0", (double)sigma_scale);
    c->set.clamp_radius = radius; c->set.clamp_k = sigma_scale;
    return SVGF_OK;
}

extern "C" int svgf_get_history_clamp(const svgf_ctx *c, int *radius, float *sigma_scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (radius) *radius = c->set.clamp_radius;
    if (sigma_scale) *sigma_scale = c->set.clamp_k;
    return SVGF_OK;
}

extern "C" int svgf_set_firefly_filter(svgf_ctx *c, int rank, float scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (rank < 0 || rank > 3) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_set_firefly_filter: rank %d outside 0..3", rank);
    if (!finite_nonneg(scale)) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_set_firefly_filter: scale %g is not a finite number >= 0", (double)scale);
    c->set.firefly_rank = rank; c->set.firefly_scale = scale;
    return SVGF_OK;
}

extern "C" int svgf_get_firefly_filter(const svgf_ctx *c, int *rank, float *scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (rank) *rank = c->set.firefly_rank;
    if (scale) *scale = c->set.firefly_scale;
    return SVGF_OK;
}

// (the table is the caller's memory)
extern "C" int svgf_set_object_motion(svgf_ctx *c, const float *geom_xf_dev, int n_geoms)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (n_geoms < 0) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_set_object_motion: n_geoms %d is negative", n_geoms);
    if (!geom_xf_dev && n_geoms > 0) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_set_object_motion: null table with n_geoms %d", n_geoms);
    if ((uintptr_t)geom_xf_dev & 15)      // the kernel loads a row of a map as one 16-byte value
        return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_set_object_motion: the table at %p is not 16-byte aligned", (const void *)geom_xf_dev);
    c->set.xf_dev = geom_xf_dev; c->set.xf_n = n_geoms;
    return SVGF_OK;
}

extern "C" int svgf_get_object_motion(const svgf_ctx *c, const float **geom_xf_dev, int *n_geoms)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (geom_xf_dev) *geom_xf_dev = c->set.xf_dev;
    if (n_geoms) *n_geoms = c->set.xf_n;
    return SVGF_OK;
}

// Configuration like the clamp, but the first call that turns it on allocates the pass's three planes.
extern "C" int svgf_set_output_taa(svgf_ctx *c, float alpha, float sigma_scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_set_output_taa: alpha %g outside 0..1", (double)alpha);      // NaN included
    if (!finite_nonneg(sigma_scale))
        return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_set_output_taa: sigma_scale %g is not a finite number >= 0", (double)sigma_scale);
    OutputTaa &taa = c->taa;
    if (alpha > 0.0f && !taa.hist[1]) {
        SVGF_ENTER(c);
        hipError_t e = taa.pre ? hipSuccess : ctx_alloc(c, (void **)&taa.pre, c->n * 3 * sizeof(float));
        for (int k = 0; k < 2 && e == hipSuccess; k++) if (!taa.hist[k]) e = ctx_alloc(c, (void **)&taa.hist[k], c->n * sizeof(float4));
        const bool oom = e == hipErrorOutOfMemory;
        if (e != hipSuccess)
            return refuse(c, oom ? SVGF_ERR_OOM : SVGF_ERR_HIP, "svgf_set_output_taa: %s for the output pass's planes (%zu bytes)", oom ? "hipMalloc failed" : "hipMemset failed", c->n * 44);
    }
    if (alpha > 0.0f && !(taa.alpha > 0.0f)) taa.valid = 0;      // turned on: the first frame behind this call has no output history
    taa.alpha = alpha; taa.k = sigma_scale;
    return SVGF_OK;
}

extern "C" int svgf_get_output_taa(const svgf_ctx *c, float *alpha, float *sigma_scale)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (alpha) *alpha = c->taa.alpha;
    if (sigma_scale) *sigma_scale = c->taa.k;
    return SVGF_OK;
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
extern "C" int svgf_height(const svgf_ctx *c) { return c ? c->H : 0; }

extern "C" int svgf_set_capture(svgf_ctx *c, int on)
{
    SVGF_ENTER(c);
    if (on && !c->cv_capture) HIPC(c, ctx_alloc(c, (void **)&c->cv_capture, c->n * sizeof(float4)));
    c->capture = on ? 1 : 0;
    return SVGF_OK;
}

// ---- stateless entry points ----

// The motion plane of a frame whose geometry moved rigidly, written with the camera path's own projection (k_motion_reproject,
// svgf_kernels.hip) and the view matrix svgf_denoise would have retained for `prev_cam`.
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

// Guided upsampling (k_upsample, svgf_upsample.hip): the full-size image from a reduced-size denoise.  Every argument is
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
    if (!finite_nonneg(up->sigma_n) || !finite_nonneg(up->sigma_x)) return SVGF_ERR_INVALID_ARG;
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
// dst's size.  One launch on `stream`; the planes written are the ones the indices hist, cur, gcur and taa.cur name.  Not a frame: no
// profile entry, frame_no unchanged.  On contexts without pipeline resources it neither synchronises nor allocates.
extern "C" int svgf_transfer_history(svgf_ctx *dst, svgf_ctx *src, void *stream)
{
    if (!dst || !src) return SVGF_ERR_INVALID_ARG;      // (neither context is touched)
    if (dst == src) return refuse(dst, SVGF_ERR_INVALID_ARG, "svgf_transfer_history: dst and src are the same context");
    if (dst->device != src->device)
        return refuse(dst, SVGF_ERR_UNSUPPORTED, "svgf_transfer_history: dst lives on device %d, src on device %d", dst->device, src->device);
    SVGF_ENTER(dst);
    const hipStream_t s = (hipStream_t)stream;
    if (s) {      // (the legacy stream cannot be captured)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return refuse(dst, SVGF_ERR_UNSUPPORTED, "svgf_transfer_history: `stream` is being captured into a graph; the call changes host state a replay would not");
    }
    // Frames of a pipelined context may be running on its internal streams or on another stream of the caller's: wait for the device,
    // as svgf_planar_gbuffer does.  dst's events are forgotten: its next frame orders itself behind the caller's stream as a whole
    // (pipe.frames == 0), that is, behind the launch below.
    if (dst->pipe.pipelined || src->pipe.pipelined) {
        HIPC(dst, hipDeviceSynchronize());
        dst->pipe.reset();
    }
    const Planes &sp = src->planes, &dp = dst->planes;
    TransferArgs a;
    memset(&a, 0, sizeof(a));
    a.cv_s = sp.cv[sp.hist]; a.mom_s = sp.mom[sp.cur]; a.hlen_s = sp.hlen[sp.cur];
    a.nrm_s = sp.nrm[sp.gcur]; a.pos_s = sp.pos[sp.gcur]; a.gid_s = sp.gid[sp.gcur];
    a.cv_d = dp.cv[dp.hist]; a.mom_d = dp.mom[dp.cur]; a.hlen_d = dp.hlen[dp.cur];
    a.nrm_d = dp.nrm[dp.gcur]; a.pos_d = dp.pos[dp.gcur]; a.gid_d = dp.gid[dp.gcur];
    // the output history moves when dst has the pass on and src holds one; otherwise dst has none afterwards
    const bool taa = dst->taa.hist[0] && dst->taa.alpha != 0.0f && src->taa.valid && src->taa.hist[0];
    if (taa) { a.taa_s = src->taa.hist[src->taa.cur]; a.taa_d = dst->taa.hist[dst->taa.cur]; }
    a.Ws = src->W; a.Hs = src->H; a.Wd = dst->W; a.Hd = dst->H;
    a.rx = (float)src->W / (float)dst->W; a.ry = (float)src->H / (float)dst->H;
    a.identity = (src->W == dst->W && src->H == dst->H) ? 1 : 0;
    HIPC(dst, launch_transfer_history(a, s));
    // the internal streams of a pipelined context carry its promised frames: whatever they run next runs behind the launch
    for (svgf_ctx *c : { dst, src }) {
        if (!c->pipe.pipelined) continue;
        HIPC(dst, hipEventRecord(c->pipe.ev_in, s));
        for (int q = 0; q < 2; q++) HIPC(dst, hipStreamWaitEvent(c->pipe.stream[q], c->pipe.ev_in, 0));
    }
    memcpy(dst->view_prev, src->view_prev, sizeof(dst->view_prev));
    dst->planes.vp_valid = 0;      // derived from planes that hold something else now
    dst->taa.valid = taa ? 1 : 0;
    return SVGF_OK;
}

// ---- host round trip and state inspection ----

extern "C" int svgf_denoise_host(svgf_ctx *c, float *out_rgb_host, const float *in_rgb_host,
                                 const SvgfGBufferTexel *gbuffer_host, const SvgfCamera *cam, const SvgfParams *p)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (!out_rgb_host || !in_rgb_host || !gbuffer_host) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_denoise_host: null argument");
    SVGF_ENTER(c);
    if (!c->st_in) HIPC(c, ctx_alloc(c, (void **)&c->st_in, c->n * 3 * sizeof(float)));
    if (!c->st_out) HIPC(c, ctx_alloc(c, (void **)&c->st_out, c->n * 3 * sizeof(float)));
    if (!c->st_g) HIPC(c, ctx_alloc(c, &c->st_g, c->n * sizeof(SvgfGBufferTexel)));
    HIPC(c, hipMemcpy(c->st_in, in_rgb_host, c->n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->st_g, gbuffer_host, c->n * sizeof(SvgfGBufferTexel), hipMemcpyHostToDevice));
    int rc = svgf_denoise(c, c->st_out, c->st_in, c->st_g, cam, p, nullptr);
    if (rc != SVGF_OK) return rc;
    HIPC(c, hipDeviceSynchronize());
    HIPC(c, hipMemcpy(out_rgb_host, c->st_out, c->n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return SVGF_OK;
}

extern "C" int svgf_read_state(svgf_ctx *c, int which, void *host_dst, unsigned long long host_bytes)
{
    if (!c || !host_dst) return SVGF_ERR_INVALID_ARG;
    SVGF_ENTER(c);
    HIPC(c, hipDeviceSynchronize());
    const size_t n = c->n;
    const Planes &b = c->planes;
    auto too_small = [&](size_t need) { return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_read_state: buffer too small (%llu < %zu)", host_bytes, need); };
    const void *src = nullptr;      // the states that are read as they lie: the plane and its size
    size_t bytes = 0;
    switch (which) {
    case SVGF_STATE_HISTORY_LENGTH: src = b.hlen[b.cur]; bytes = n * sizeof(int); break;
    case SVGF_STATE_MOMENTS:        src = b.mom[b.cur];  bytes = n * 2 * sizeof(float); break;
    case SVGF_STATE_PREV_NORMAL:    src = b.nrm[b.gcur]; bytes = n * 3 * sizeof(float); break;
    case SVGF_STATE_PREV_POSITION:  src = b.pos[b.gcur]; bytes = n * 3 * sizeof(float); break;
    case SVGF_STATE_PREV_GEOM_ID:   src = b.gid[b.gcur]; bytes = n * sizeof(int); break;
    case SVGF_STATE_OUTPUT_HISTORY:
        if (!c->taa.valid || !c->taa.hist[c->taa.cur]) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_read_state: the context has no output history");
        src = c->taa.hist[c->taa.cur]; bytes = n * sizeof(float4);
        break;
    case SVGF_STATE_COLOR_HISTORY:
    case SVGF_STATE_COLOR_ACC:
    case SVGF_STATE_VARIANCE_TEMPORAL: {      // unpacked from a {colour, variance} plane
        const bool is_hist = (which == SVGF_STATE_COLOR_HISTORY);
        if (!is_hist && !c->cv_capture) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_read_state: enable svgf_set_capture before the frame");
        const size_t out_bytes = (which == SVGF_STATE_VARIANCE_TEMPORAL) ? n * sizeof(float) : n * 3 * sizeof(float);
        if (host_bytes < out_bytes) return too_small(out_bytes);
        float4 *tmp = (float4 *)malloc(n * sizeof(float4));
        if (!tmp) return SVGF_ERR_OOM;
        hipError_t e = hipMemcpy(tmp, is_hist ? b.cv[b.hist] : c->cv_capture, n * sizeof(float4), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { free(tmp); return refuse(c, SVGF_ERR_HIP, "hipMemcpy: %s", hipGetErrorString(e)); }
        float *d = (float *)host_dst;
        if (which == SVGF_STATE_VARIANCE_TEMPORAL) for (size_t k = 0; k < n; k++) d[k] = tmp[k].w;
        else for (size_t k = 0; k < n; k++) { d[3 * k] = tmp[k].x; d[3 * k + 1] = tmp[k].y; d[3 * k + 2] = tmp[k].z; }
        free(tmp);
        return SVGF_OK;
    }
    default: return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_read_state: unknown state %d", which);
    }
    if (host_bytes < bytes) return too_small(bytes);
    HIPC(c, hipMemcpy(host_dst, src, bytes, hipMemcpyDeviceToHost));
    return SVGF_OK;
}
