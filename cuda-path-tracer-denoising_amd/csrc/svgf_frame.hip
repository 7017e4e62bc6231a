// svgf_frame.hip — one frame: plan (every decision, nothing enqueued), enqueue (walks the plan), commit (the context's state behind
// it); the kernel choice; and the svgf_denoise* / planar entry points.  FramePlan: svgf_context.h.
#include "svgf_context.h"

// ---- host copy of the view-matrix construction (reference GetViewMatrix src/denoise.cu:342-347) -------------
// inverse of the column-major matrix [right|0, up|0, view|0, position|1] by 2x2-minor (cofactor) expansion in the
// operation order of glm 0.9.6.3 (external/include/glm/detail/type_mat4x4.inl:37-92), so fp32 rounding matches.
void view_matrix_from_camera(const SvgfCamera *cam, float *out)
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

// ---- the kernel choice ----

// The automatic choice between the two fast a-trous kernels for steps 2-32: the one whose launch geometry is estimated cheaper runs
// (the cost model: svgf_atrous_geometry.hip).  The estimates depend on the image size and the device only, so they are asked for
// once per context and step.
static bool lane_pays(svgf_ctx *c, const AtrousArgs &a)
{
    const int l = step_log2(a.step);
    if (c->lane_cheaper[l] < 0) {
        const double lane = atrous_lane_estimate_us(a, c->n_cu), strip = atrous_strip_estimate_us(a, c->n_cu);
        c->lane_cheaper[l] = lane <= strip ? 1 : 0;
        exp_note_estimates(c, l, lane, strip);
    }
    return c->lane_cheaper[l] != 0;
}

// The kernel of one a-trous level: the ONE place that chooses between the six.  (kernel_variant 5 gets here in the experiments
// build only: frame_demands refuses it in the product.)
static KernelKind level_kernel(svgf_ctx *c, const SvgfParams *p, const AtrousArgs &a, bool fuse_here)
{
    if (fuse_here) return K_FUSED;
    const int kv = p->kernel_variant;
    if (kv != 1 && atrous_strip_supported(a)) {
        if (a.step == 2 && kv == 5 && atrous_lane_supported(a)) return K_LANE2Y;
        if (atrous_lane_supported(a) && (kv >= 4 || (kv == 0 && lane_pays(c, a)))) return K_LANE;
        return K_STRIP;
    }
    if (kv != 1 && kv != 2 && atrous_lattice_supported(a)) return K_LATTICE;     // steps 64, 128, ...
    return K_GATHER;
}

// ---- the plan.  Every level is decided and validated here, before anything is enqueued or any context state changes: a failure
// half-way through the cascade would leave the colour history of this frame next to the G-buffer / moments of the previous one.
// The context is only read (the memoised estimates of lane_pays / fuse_pays aside). ----

// What the frame's settings demand, and whether this context can honour them.
static int frame_demands(svgf_ctx *c, FrameAsk &q)
{
    const SvgfParams *p = q.p;
    if (p->atrous_nlevel < 0 || p->atrous_nlevel > SVGF_MAX_LEVELS)
        return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_denoise: atrous_nlevel %d outside 0..%d", p->atrous_nlevel, SVGF_MAX_LEVELS);
    if (p->kernel_variant == 3)
        return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_denoise: kernel_variant %d (experimental shared-weight kernel) is no longer part of the library, see tools/experiments/", p->kernel_variant);
    if (p->kernel_variant < 0 || p->kernel_variant > 6) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_denoise: kernel_variant %d unknown", p->kernel_variant);
    if (!kExperimentsBuild && (p->kernel_variant == 5 || p->kernel_variant == 6))
        return refuse(c, SVGF_ERR_UNSUPPORTED, "svgf_denoise: kernel_variant %d is a parked experiment (two-y-phase geometry / temporal pass fused into "
                      "the first level) and is not part of this build; build libsvgf_hip_exp.so (-DSVGF_BUILD_EXPERIMENTS)", p->kernel_variant);
    if (q.motion_dev && !temporal_motion_format_known(q.motion_format))
        return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_denoise_motion: motion_format %d unknown", q.motion_format);
    // A non-temporal frame has no history to look up, gather or test: the motion plane, the clamp and the object table are ignored.
    // The firefly filter acts on temporal and non-temporal frames alike; the output pass on every frame that writes the image
    // (debug views are written as they are and drop the output history).
    const bool temporal = p->temporal_enable != 0, debug_view = p->right_view_option == 1 || p->right_view_option == 2;
    q.f[F_MOTION]  = { q.motion_dev && temporal, false, "svgf_denoise_motion", "motion plane", "take" };
    q.f[F_CLAMP]   = { c->set.clamp_radius > 0 && temporal, true, "svgf_denoise", "history clamp (svgf_set_history_clamp)", "have" };
    q.f[F_XFORM]   = { c->set.xf_dev && c->set.xf_n > 0 && temporal, false, "svgf_denoise", "object motion table (svgf_set_object_motion)", "take" };
    q.f[F_FIREFLY] = { c->set.firefly_rank > 0, true, "svgf_denoise", "firefly filter (svgf_set_firefly_filter)", "have" };
    q.f[F_TAA]     = { c->taa.alpha > 0.0f && !debug_view, true, "svgf_denoise", "output pass (svgf_set_output_taa)", "have" };
    for (const FrameFeature &f : q.f) {
        if (!f.active) continue;
        if (f.tiled && !temporal_clamp_supported(c->W, c->H))
            return refuse(c, SVGF_ERR_UNSUPPORTED, "svgf_denoise: the %s is limited to images of at most 262140 rows, this context has %d", f.name, c->H);
        if (const int rc = exp_refuse_feature(c, p, f); rc != SVGF_OK) return rc;
    }
    q.cascade = !(debug_view || p->atrous_nlevel == 0 || !p->spatial_enable);
    return SVGF_OK;
}

// Pipelined frames (see Pipeline).  The promise behind inputs_ready = 1: at call time the inputs are complete (and stay
// untouched until the work of this call is done) — so the frame need not order itself behind the caller's stream, which has
// waited for the PREVIOUS frame's end, and runs on an internal stream; only the kernel that writes `out` waits for the caller's
// stream position (readers of that buffer enqueued behind earlier calls).
// Without the promise a frame of a pipelined context runs on the caller's stream, like any frame of any context, behind the last
// frame that used its plane set and the history of the frame before it; under stream capture nothing is promised (the frame is
// recorded on the capturing stream).  The experiments build's parked kernels never pipeline.
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
static void plan_pipeline(const svgf_ctx *c, const FrameAsk &q, FramePlan &pl)
{
    const SvgfParams *p = q.p;
    const Pipeline &pp = c->pipe;
    const bool worth = p->temporal_enable && p->spatial_enable && p->atrous_nlevel >= 2 &&
                       p->right_view_option != 1 && p->right_view_option != 2 && p->history_level != p->atrous_nlevel;
    // Only a context whose pipeline resources exist (svgf_create_ex(SVGF_CREATE_PIPELINED) / svgf_enable_pipeline) takes either form up:
    // svgf_denoise never allocates.  The promise additionally needs the two internal streams on different hardware queues (probed when
    // the resources were created, svgf_pipeline_status() == 1): refused, a promised frame is a plain ordered frame.
    bool promise = (p->inputs_ready == 1) && worth && pp.pipelined && !pp.serial;
    bool want_pipeline = promise || ((p->inputs_ready == 2) && worth && pp.pipelined);
    pl.cap_id = 0;
    if (want_pipeline || pp.piped_mode) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        unsigned long long id = 0;
        if (pl.s_user && hipStreamGetCaptureInfo(pl.s_user, &cs, &id) == hipSuccess && cs != hipStreamCaptureStatusNone) { pl.cap_id = id ? id : 1; promise = false; }
        // a frame recorded into a graph did not run when it was recorded: the eager frames behind it order themselves behind the
        // caller's stream (where the graph is launched) until both parities' events are eager ones again
        if (!pl.cap_id && (pp.ev_hist[0].captured() || pp.ev_hist[1].captured())) promise = false;
    }
    if (exp_never_pipelines(c, p)) { promise = false; want_pipeline = false; }
    pl.flip = want_pipeline && !pl.cap_id && !pp.piped_mode;
    pl.piped = pp.piped_mode || pl.flip;
    const long long pipe_frames = pl.flip ? 0 : pp.frames;
    pl.pq = pl.piped ? (int)(pipe_frames & 1) : 0;
    // A promised frame runs on the context's stream of its parity.  Every other frame of a pipelined context runs on the caller's own
    // stream, behind the previous frame of the same parity (same plane set), wherever that one ran: with one stream that is what an
    // ordered frame always was; with two streams used in turn (inputs_ready = 2) the caller's streams ARE the pipeline.
    pl.promise = pl.piped && promise;
    pl.s = pl.promise ? pp.stream[pl.pq] : pl.s_user;
    // the first pipelined frame: all of it behind the caller's stream.  So is every promised frame of a context that has ever
    // been recorded into a graph: a replay of that graph on the caller's stream touches the same planes and is visible to this
    // frame only through the caller's stream position
    pl.wait_in_first = pipe_frames == 0 || pp.ever_captured;
}

// 1) temporal accumulation, or constant variance (reference :360-371).  Writes a cv plane `acc` that does not hold the
//    colour history, and the current-frame G-buffer planes.  In the non-temporal mode on the AoS boundary the pass is not launched
//    at all where the cascade starts with the lane kernel at step 2: the first level's loader waves do its work (pl.fused).
//    (Rounds 1-3 ran this pass alone on a side stream beside the previous frame's trailing levels — it lost 3-8 % once the lane
//    kernel ran all five levels; round 5's frame pipeline, above, runs whole frames of alternating parity on two streams.)
static void plan_first_pass(svgf_ctx *c, const FrameAsk &q, FramePlan &pl)
{
    const SvgfParams *p = q.p;
    const Planes &b = c->planes;
    const int pbase = pl.piped ? 3 * pl.pq : 0;          // this frame's plane set
    const int acc = pl.acc = pl.piped ? (pbase == b.hist ? pbase + 1 : pbase) : (b.hist + 1) % 3;
    const int gnew = pl.gcur = 1 - b.gcur;
    const bool firefly = q.f[F_FIREFLY].active;
    TemporalArgs &t = pl.t;
    memset(&t, 0, sizeof(t));
    pl.temporal = p->temporal_enable != 0; pl.fused = pl.split_fused = false; pl.svf = p->spatial_variance_frames;
    t.in_rgb = q.in; t.gbuf = q.g; t.cv_acc = b.cv[acc];
    t.nrm_cur = b.nrm[gnew]; t.gid_cur = b.gid[gnew]; t.pos_cur = b.pos[gnew];
    t.W = c->W; t.H = c->H;
    if (firefly) { t.firefly_rank = c->set.firefly_rank; t.firefly_scale = c->set.firefly_scale; }
    AtrousArgs probe;
    memset(&probe, 0, sizeof(probe));
    probe.W = c->W; probe.H = c->H; probe.step = 2;
    if (pl.temporal) {
        t.cv_hist = b.cv[b.hist];
        t.mom_hist = b.mom[b.cur]; t.mom_acc = b.mom[1 - b.cur];
        t.hlen = b.hlen[b.cur]; t.hlen_upd = b.hlen[1 - b.cur];
        t.nrm_prev = b.nrm[b.gcur]; t.gid_prev = b.gid[b.gcur];
        memcpy(t.M, c->view_prev, sizeof(t.M));
        t.color_alpha_min = p->color_alpha; t.moment_alpha_min = p->moment_alpha;
        t.reproj_sx = p->reproj_scale[0]; t.reproj_sy = p->reproj_scale[1];
        t.pos_prev = b.pos[b.gcur]; t.pos_tol = p->reproj_position_tol;
        t.dump = b.dump; t.arena = b.arena; t.arena_bytes = b.arena_bytes;
        if (q.f[F_MOTION].active) { t.motion = q.motion_dev; t.motion_format = q.motion_format; }
        if (q.f[F_CLAMP].active) { t.clamp_radius = c->set.clamp_radius; t.clamp_k = c->set.clamp_k; }
        if (q.f[F_XFORM].active) { t.xf = c->set.xf_dev; t.n_geoms = c->set.xf_n; }
        exp_plan_first_pass(c, q, probe, pl);
    } else if (q.g && !firefly && q.cascade && (p->kernel_variant == 0 || p->kernel_variant == 6) && !p->paper_steps) {
        // Non-temporal mode.  On the AoS boundary the prepare pass (variance = 10, colour copy, G-buffer split) is loads and
        // stores only and rides in the first level's loader waves when the cascade starts with the lane kernel at step 2
        // (svgf_atrous_prepare_fused.hip, FUSED = 3): no prepare launch, no colour plane written and read back — wherever the first
        // level runs the lane kernel anyway (measured: profiles/r04_exp_prepare_fused.log).  (Not with the firefly filter:
        // those loaders stage no neighbourhood of the input; the frame then runs the tiled prepare kernel, one launch more.)
        pl.fused = atrous_prepare_fused_supported(probe, t) && atrous_strip_supported(probe) && atrous_lane_supported(probe) &&
                   (p->kernel_variant == 6 || lane_pays(c, probe));
    }
    pl.tdone = pl.piped && !q.g && !pl.cap_id; pl.capture = c->capture != 0;
}

// 2) debug views, pass-through or the a-trous cascade (:373-394), and 3) the history rotation (:396-399): planes swap roles
//    instead of being copied.
static int plan_cascade(svgf_ctx *c, const FrameAsk &q, FramePlan &pl)
{
    const SvgfParams *p = q.p;
    const Planes &b = c->planes;
    const int pbase = pl.piped ? 3 * pl.pq : 0, old_hist = b.hist, gnew = pl.gcur;
    unsigned vp_valid = b.vp_valid & ~(1u << pl.acc);     // the temporal / prepare pass writes no variance plane: the first level gathers cv.w
    int hist = pl.acc;                                    // color_history <- color_acc / input (:366,370)
    pl.exit = p->right_view_option == 1 ? EXIT_DEBUG_HLEN : p->right_view_option == 2 ? EXIT_DEBUG_VAR : !q.cascade ? EXIT_COPY : EXIT_CASCADE;
    pl.n_levels = q.cascade ? p->atrous_nlevel : 0;
    int src = hist;
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
        a.src = b.cv[src]; a.dst = dst >= 0 ? b.cv[dst] : nullptr; a.out_rgb = lv.last ? pl.out_c : nullptr;
        a.nrm = b.nrm[gnew]; a.pos = b.pos[gnew]; a.gbuf = q.g; a.albedo = b.albedo;
        a.W = c->W; a.H = c->H;
        a.step = 1 << (p->paper_steps ? level - 1 : level);   // reference: level starts at 1 => steps 2,4,8,16,32 (:98,386)
        a.sigma_c = p->sigma_l; a.sigma_n = p->sigma_n; a.sigma_x = p->sigma_x;
        a.blur_variance = p->blur_variance ? 1 : 0;
        a.modulate = (lv.last && p->sepcolor && p->addcolor) ? 1 : 0;
        // pre-blur source of steps >= 16: the zero-margined 4-byte variance plane the producer level wrote next to its colour
        // plane (see below); the lane kernel at those steps REQUIRES it (its loaders blur the variance from it)
        a.var = (c->use_vplane && a.step >= 16 && ((vp_valid >> src) & 1u)) ? b.vp[src] : nullptr;
        a.var_dst = nullptr;
        a.tin = nullptr; a.tout = nullptr; a.t_m = 0; a.t_m_out = 0;
        lv.kind = level_kernel(c, p, a, fuse_here);
        if (p->kernel_variant == 2 && lv.kind != K_STRIP)
            return refuse(c, SVGF_ERR_UNSUPPORTED, "svgf_denoise: strip kernel does not support %dx%d step %d", c->W, c->H, a.step);
        lv.asked = p->kernel_variant == 0 && (lv.kind == K_FUSED || lv.kind == K_LANE || lv.kind == K_STRIP) && c->lane_cheaper[step_log2(a.step)] >= 0;
        // Pre-blur rows (y-1, y+1 of the full-resolution image) of the lane / strip kernels.  At steps >= 16 they are
        // read as 4-byte gathers out of 16-byte colour texels whose lines nobody else on the XCD touches (PMC: 75.6 /
        // 72.6 B/px fetched against 40 algorithmic); there the kernels read them from a zero-margined 4-byte variance plane
        // that the producer level writes next to its colour plane (51.3 / 48.8 B/px, +4 B/px written).  At steps 2-8
        // the neighbouring rows are the sibling y-phases' own rows, already in L2: a plane would ADD 8 B/px (measured,
        // profiles/r02_pmc_hbm.txt), so those levels keep reading colour.w and only the level feeding a step-16 level
        // writes the plane.
        if (lv.kind != K_LANE && lv.kind != K_STRIP) a.var = nullptr;
        else if (c->use_vplane && dst >= 0 && !lv.last && a.step >= 8) a.var_dst = b.vp[dst];
        if (dst >= 0) { if (a.var_dst) vp_valid |= 1u << dst; else vp_valid &= ~(1u << dst); }
        // the accumulated plane itself is only written by the fused level when something besides that level reads it: a later
        // frame (the history is not this level's output) or a test (svgf_set_capture)
        if (fuse_here) pl.t.cv_acc = (!lv.keep || c->capture) ? b.cv[pl.acc] : nullptr;
        if (lv.keep) hist = dst;
        src = dst;
    }
    exp_plan_cascade(c, q, pl);
    pl.t.skip_split = pl.split_fused ? 1 : 0;
    // The other stream's next temporal pass may go on once everything it reads of this frame is final: behind the level that
    // writes the colour history; behind the temporal pass where no level of the cascade writes it (it IS the accumulated plane then,
    // which no level of this frame overwrites, and everything else was final before); frames without a cascade (debug views,
    // pass-through) and non-temporal frames without such a level release it at their end: they read state that pass rewrites.
    pl.hist_release = pl.n_levels;
    if (q.cascade && p->history_level >= 1 && p->history_level <= p->atrous_nlevel) pl.hist_release = p->history_level - 1;
    else if (q.cascade && pl.temporal) pl.hist_release = -1;
    pl.hist = hist; pl.vp_valid = vp_valid;
    pl.cur = pl.temporal ? 1 - b.cur : b.cur;
    pl.last_modulated = (q.cascade && p->sepcolor && p->addcolor) ? 1 : 0;
    return SVGF_OK;
}

// The output pass.  It reads this frame's position / geomId planes (written by the temporal or prepare pass, the first level's
// loaders or the producer), the call's motion plane even on a frame with temporal_enable == 0, and the output history of the
// last frame if that frame left one; a frame without the pass drops the history.
static void plan_output_pass(const svgf_ctx *c, const FrameAsk &q, FramePlan &pl)
{
    const OutputTaa &taa = c->taa;
    pl.taa_cur = taa.cur; pl.taa_valid = 0;
    if (!pl.taa) return;
    OutputTaaArgs &o = pl.o;
    memset(&o, 0, sizeof(o));
    o.pre = taa.pre; o.out = pl.out;
    o.hist = taa.valid ? taa.hist[taa.cur] : nullptr; o.hist_new = taa.hist[1 - taa.cur];
    o.pos = c->planes.pos[pl.gcur]; o.gid = c->planes.gid[pl.gcur];
    if (q.motion_dev) { o.motion = q.motion_dev; o.motion_format = q.motion_format; }
    if (c->set.xf_dev && c->set.xf_n > 0) { o.xf = c->set.xf_dev; o.n_geoms = c->set.xf_n; }
    memcpy(o.M, c->view_prev, sizeof(o.M));
    o.W = c->W; o.H = c->H;
    o.reproj_sx = q.p->reproj_scale[0]; o.reproj_sy = q.p->reproj_scale[1];
    o.alpha = taa.alpha; o.k = taa.k;
    pl.taa_cur = 1 - taa.cur; pl.taa_valid = 1;
}

static int plan_frame(svgf_ctx *c, FrameAsk &q, void *out_rgb_dev, void *stream, FramePlan &pl)
{
    if (const int rc = frame_demands(c, q); rc != SVGF_OK) return rc;
    pl.taa = q.f[F_TAA].active;
    pl.out = (float *)out_rgb_dev; pl.out_c = pl.taa ? c->taa.pre : pl.out; pl.s_user = (hipStream_t)stream;
    plan_pipeline(c, q, pl);
    const Profiler &pr = c->prof;
    pl.timed = pr.frames && (pr.frame_no % (pr.stride > 0 ? pr.stride : 1)) == 0;
    pl.slot = pl.timed ? (int)(pr.count % pr.frames) : 0;
    plan_first_pass(c, q, pl);
    if (const int rc = plan_cascade(c, q, pl); rc != SVGF_OK) return rc;
    plan_output_pass(c, q, pl);
    return SVGF_OK;
}

// Walks the plan.  Of the context it writes the pipeline's event records (and the switch into piped mode), and the profiling slot.
static int enqueue_frame(svgf_ctx *c, const FramePlan &pl)
{
    const int pq = pl.pq, n = (int)c->n;
    const hipStream_t s = pl.s; const TemporalArgs &t = pl.t;
    const Planes &b = c->planes;
    Pipeline &pp = c->pipe;
    if (pl.flip) { pp.piped_mode = 1; pp.reset(); }      // (a state flip, nothing is allocated: the colour history lies in plane set 0)
    if (pl.piped) {
        pp.ev_tdone[pq].disarm();      // (re-armed below by a planar frame's temporal pass)
        if (pl.promise) {
            HIPC(c, hipEventRecord(pp.ev_in, pl.s_user));      // the caller's stream position at hand-over: the last level waits for it (`out`)
            if (pl.wait_in_first) HIPC(c, hipStreamWaitEvent(s, pp.ev_in, 0));
        }
        HIPC(c, pp.ev_done[pq].wait(s, pl.cap_id));
    }
    KernelTimer timer{ &c->prof, pl.slot, 0, pl.timed };
    if (pl.timed) c->prof.ev_n[pl.slot] = 0;
    // the other stream's frame: this frame's temporal pass (and everything behind it) starts when that frame's colour history,
    // moments, history lengths and G-buffer planes are final
    if (pl.piped) HIPC(c, pp.ev_hist[1 - pq].wait(s, pl.cap_id));
    if (pl.temporal && !pl.fused) {
        LAUNCH(SVGF_KERNEL_TEMPORAL, launch_temporal(t, s));
        if (pl.tdone) HIPC(c, pp.ev_tdone[pq].record(s, 0));
        if (pl.svf > 0)      // f4 extension: spatial variance estimate for short histories (its own profiling slot, same kind)
            LAUNCH(SVGF_KERNEL_TEMPORAL, launch_spatial_variance(t.cv_acc, t.mom_acc, t.hlen_upd, t.nrm_cur, t.gid_cur, t.W, t.H, pl.svf, s));
    } else if (!pl.fused) {
        if (t.firefly_rank) LAUNCH(SVGF_KERNEL_PREPARE, launch_prepare_filtered(t.in_rgb, t.gbuf, t.cv_acc, t.nrm_cur, t.gid_cur, t.pos_cur, t.W, t.H,
                                                                                t.firefly_rank, t.firefly_scale, s));
        else LAUNCH(SVGF_KERNEL_PREPARE, launch_prepare(t.in_rgb, t.gbuf, t.cv_acc, t.nrm_cur, t.gid_cur, t.pos_cur, t.W, t.H, s));
    }
    // (before the early release below: the next frame's copy into the one capture buffer must not overtake this one)
    if (pl.capture && !pl.fused) HIPC(c, hipMemcpyAsync(c->cv_capture, b.cv[pl.acc], c->n * sizeof(float4), hipMemcpyDeviceToDevice, s));
    if (pl.piped && pl.hist_release < 0) HIPC(c, pp.ev_hist[pq].record(s, pl.cap_id));
    switch (pl.exit) {
    case EXIT_DEBUG_HLEN: LAUNCH(SVGF_KERNEL_DEBUGVIEW, launch_debug_hlen(b.hlen[b.cur], pl.out, n, 100.0f, s)); break;   // pre-update lengths (:374)
    case EXIT_DEBUG_VAR:  LAUNCH(SVGF_KERNEL_DEBUGVIEW, launch_debug_var(b.cv[pl.acc], pl.out, n, 0.1f, s)); break;         // (:377)
    case EXIT_COPY:                                                                                                          // (:382)
        if (pl.taa && pl.piped) HIPC(c, pp.ev_done[1 - pq].wait(s, pl.cap_id));      // (`pre`: see the last level below)
        LAUNCH(SVGF_KERNEL_COPYOUT, launch_copy_rgb(b.cv[pl.acc], pl.out_c, n, s));
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
        if (pl.promise && lv.last && !pl.taa) HIPC(c, hipStreamWaitEvent(s, pp.ev_in, 0));
        if (pl.taa && pl.piped && lv.last) HIPC(c, pp.ev_done[1 - pq].wait(s, pl.cap_id));
        const int parked = exp_launch_level(c, pl, i, timer);      // (the experiments build's parked kernels; 1: not one of theirs)
        if (parked < 0) return parked;
        if (parked) switch (lv.kind) {
        case K_FUSED:   LAUNCH(SVGF_KERNEL_FUSED, launch_atrous_prepare_fused(a, t, s)); break;
        case K_LANE:    LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_lane(a, s)); break;       // steps 2 .. 32: symmetric terms evaluated once
        case K_STRIP:   LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_strip(a, s)); break;
        case K_LATTICE: LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_lattice(a, s)); break;
        default:        LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_gather(a, s)); break;
        }
        if (lv.kind == K_FUSED && pl.capture) HIPC(c, hipMemcpyAsync(c->cv_capture, b.cv[pl.acc], c->n * sizeof(float4), hipMemcpyDeviceToDevice, s));
        if (pl.piped && i == pl.hist_release) HIPC(c, pp.ev_hist[pq].record(s, pl.cap_id));
    }
    if (pl.piped && pl.hist_release == pl.n_levels) HIPC(c, pp.ev_hist[pq].record(s, pl.cap_id));
    if (pl.taa) {
        // reads the output history the other parity's frame wrote and overwrites the one it read: behind that frame's end (the
        // writer of `pre` above has waited for it already where the frame is pipelined); writes the caller's `out`
        if (pl.promise) HIPC(c, hipStreamWaitEvent(s, pp.ev_in, 0));
        LAUNCH(SVGF_KERNEL_OUTPUT_TAA, launch_output_taa(pl.o, s));
    }
    if (pl.piped) {
        HIPC(c, pp.ev_done[pq].record(s, pl.cap_id));
        if (s != pl.s_user) HIPC(c, pp.ev_done[pq].wait(pl.s_user, pl.cap_id));      // what the caller enqueues behind this call sees `out`
    }
    return SVGF_OK;
}

// The context behind a frame whose every call was accepted: the planes' roles rotate, the counters advance.
static void commit_frame(svgf_ctx *c, const FramePlan &pl, const SvgfCamera *cam)
{
    Planes &b = c->planes;
    b.acc = pl.acc; b.hist = pl.hist; b.cur = pl.cur; b.gcur = pl.gcur; b.vp_valid = pl.vp_valid; b.last_modulated = pl.last_modulated;
    c->taa.cur = pl.taa_cur; c->taa.valid = pl.taa_valid;
    if (pl.piped) { c->pipe.frames++; if (pl.cap_id) c->pipe.ever_captured = 1; }
    view_matrix_from_camera(cam, c->view_prev);
    if (pl.timed) c->prof.count++;
    c->prof.frame_no++;
    exp_commit_frame(c, pl);
}

// gbuffer_dev == nullptr: the planar path (svgf_denoise_planar) — the current-frame planes nrm/pos/gid[1 - gcur] (and `albedo`)
// were filled in place by the producer.
// motion_dev != nullptr: the temporal pass reads the previous-frame coordinates from the caller's plane (svgf_denoise_motion); an
// input like the colour image, read by that pass only.
static int denoise_frame(svgf_ctx *c, void *out_rgb_dev, const void *in_rgb_dev, const void *gbuffer_dev,
                         const void *motion_dev, int motion_format, const SvgfCamera *cam, const SvgfParams *p, void *stream)
{
    if (!out_rgb_dev || !in_rgb_dev || !cam || !p) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_denoise: null argument");
    SVGF_ENTER(c);
    FrameAsk q;
    q.p = p; q.in = (const float *)in_rgb_dev; q.g = (const float *)gbuffer_dev; q.motion_dev = motion_dev; q.motion_format = motion_format;
    FramePlan pl;
    int rc = plan_frame(c, q, out_rgb_dev, stream, pl);
    if (rc == SVGF_OK) rc = enqueue_frame(c, pl);
    if (rc == SVGF_OK) commit_frame(c, pl, cam);
    return rc;
}

extern "C" int svgf_denoise_motion(svgf_ctx *c, void *out_rgb_dev, const void *in_rgb_dev, const void *gbuffer_dev,
                                   const void *motion_dev, int motion_format, const SvgfCamera *cam, const SvgfParams *p, void *stream)
{
    if (!c) return SVGF_ERR_INVALID_ARG;
    if (!gbuffer_dev) return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_denoise: null argument");
    return denoise_frame(c, out_rgb_dev, in_rgb_dev, gbuffer_dev, motion_dev, motion_format, cam, p, stream);
}

extern "C" int svgf_denoise(svgf_ctx *c, void *out_rgb_dev, const void *in_rgb_dev, const void *gbuffer_dev,
                            const SvgfCamera *cam, const SvgfParams *p, void *stream)
{
    return svgf_denoise_motion(c, out_rgb_dev, in_rgb_dev, gbuffer_dev, nullptr, 0, cam, p, stream);
}

// ---- the planar path (the AoS -> plane repack fused into the producer) -----------------------
static int planar_gbuffer(svgf_ctx *c, SvgfPlanarGBuffer *out, bool have_stream, hipStream_t stream)
{
    if (!c || !out) return SVGF_ERR_INVALID_ARG;
    SVGF_ENTER(c);
    Planes &b = c->planes;
    if (!b.albedo) HIPC(c, ctx_alloc(c, (void **)&b.albedo, c->n * 3 * sizeof(float)));      // (first call only)
    if (const int rc = pipeline_wait_gbuffer_readers(c, have_stream, stream); rc != SVGF_OK) return rc;
    const int gnew = 1 - b.gcur;        // the planes the next frame's temporal / prepare pass treats as "current"
    out->normal = b.nrm[gnew]; out->position = b.pos[gnew]; out->geom_id = b.gid[gnew]; out->albedo = b.albedo;
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
    if (p && p->sepcolor && p->addcolor && !c->planes.albedo)
        return refuse(c, SVGF_ERR_INVALID_ARG, "svgf_denoise_planar: sepcolor && addcolor needs the albedo plane of svgf_planar_gbuffer");
    return denoise_frame(c, out_rgb_dev, in_rgb_dev, nullptr, motion_dev, motion_format, cam, p, stream);
}
