// svgf_experiments.hip — EXPERIMENTS build only (libsvgf_hip_exp.so): the tuning table behind SVGF_TUNE(), the introspection entry
// points, and everything the frame path (svgf_frame.hip) knows about the parked kernels — kernel_variant 5 / 6, split_fused and the
// cross-level term reuse (measured losses).  The product build compiles the exp_* calls to nothing (svgf_context.h).
#include <mutex>

#include "svgf_context.h"

#ifndef SVGF_BUILD_EXPERIMENTS
#error "svgf_experiments.hip holds the experiments build's host side: compile it with -DSVGF_BUILD_EXPERIMENTS (build.py: build_hip(experiments=True))"
#endif

// a row of the fused temporal + first-level kernel against a row of the plain lane kernel, as measured at 1920x1080 (DESIGN.md
// 5.8, profiles/r04_exp_fused_*.log: 176 us in its last version against 42.7 for the plain level, i.e. the fused kernel LOSES to
// temporal pass + level, 55 + 46 us): with this factor the automatic choice never fuses; kernel_variant 6 forces it
static const double kFusedRowFactor = 4.1;

// ---- the tuning table: name -> int, process-wide.  The product build has neither the table nor the entry point: SVGF_TUNE() is
// its default there and no environment variable is read anywhere in the library. ----
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

// ---- introspection ----

// The a-trous levels of the context's last frame, in order: the kernel each ran (0 fused first level, 1 lane, 2 lane with two
// y-phases, 3 strip, 4 lattice, 5 gather), its step, and the lane / strip estimates (us) the automatic choice compared for that
// step (NaN where kernel_variant != 0 or the choice was not made between those two).  Writes min(n, levels) entries of every
// non-null array; returns the number of levels (0 for a frame without a cascade), or a negative error.
extern "C" int svgf_exp_level_kernels(const svgf_ctx *c, int *kinds, int *steps, double *lane_us, double *strip_us, int n)
{
    if (!c || n < 0) return SVGF_ERR_INVALID_ARG;
    const Experiments &x = c->exp;
    for (int k = 0; k < x.lk_n && k < n; k++) {
        if (kinds) kinds[k] = x.lk_kind[k];
        if (steps) steps[k] = x.lk_step[k];
        if (lane_us) lane_us[k] = x.lk_asked[k] ? x.est_lane_us[step_log2(x.lk_step[k])] : __builtin_nan("");
        if (strip_us) strip_us[k] = x.lk_asked[k] ? x.est_strip_us[step_log2(x.lk_step[k])] : __builtin_nan("");
    }
    return x.lk_n;
}

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

// ---- the frame path's calls ----

hipError_t exp_create(svgf_ctx *c)
{
    Experiments &x = c->exp;
    x.use_reuse = SVGF_TUNE("reuse", 0) ? 1 : 0;
    x.use_split_fused = SVGF_TUNE("split_fused", 0) ? 1 : 0;      // (FUSED = 4: a measured loss)
    x.fuse_pays = -1;
    // (the terms planes of the parked cross-level reuse: allocated here, never in the middle of a frame)
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess && x.use_reuse; k++) e = ctx_alloc(c, (void **)&x.tp[k], (size_t)(c->W + 64) * c->H * sizeof(float4));
    return e;
}

static bool parked_temporal(const svgf_ctx *c, const SvgfParams *p) { return p->kernel_variant == 6 || c->exp.use_split_fused; }

int exp_refuse_feature(svgf_ctx *c, const SvgfParams *p, const FrameFeature &f)
{
    if (!parked_temporal(c, p)) return SVGF_OK;
    return refuse(c, SVGF_ERR_UNSUPPORTED, "%s: the parked fused temporal kernels (kernel_variant 6, split_fused) %s no %s", f.entry, f.parked_verb, f.name);
}

bool exp_never_pipelines(const svgf_ctx *c, const SvgfParams *p) { return p->kernel_variant == 5 || c->exp.use_reuse || parked_temporal(c, p); }

void exp_note_estimates(svgf_ctx *c, int l, double lane_us, double strip_us) { c->exp.est_lane_us[l] = lane_us; c->exp.est_strip_us[l] = strip_us; }

// Temporal pass + first level as ONE kernel (svgf_atrous_fused.hip), or as two?  The fused kernel works on 240-column strips
// with both y-phases of a strip in one workgroup and pays the same rounds x (rows + 6) launch geometry as the lane kernel; what
// it saves is the temporal kernel (HBM-bound, 25.6 ns per kilopixel at 1080p) and 56 B/px of traffic between the two.  It runs
// when its estimate is below the estimate of the level it replaces plus the temporal pass.
static bool fuse_pays(svgf_ctx *c, const AtrousArgs &a)
{
    if (c->exp.fuse_pays < 0) {
        const double lane = atrous_lane_supported(a) ? atrous_lane_estimate_us(a, c->n_cu) : 1e30;
        const double strip = atrous_strip_supported(a) ? atrous_strip_estimate_us(a, c->n_cu) : 1e30;
        const double level = lane < strip ? lane : strip;
        const double temporal_us = 0.0256e-3 * (double)c->W * (double)c->H;
        c->exp.fuse_pays = (kFusedRowFactor * atrous_fused_estimate_us(a, c->n_cu) <= level + temporal_us && level < 1e29) ? 1 : 0;
    }
    return c->exp.fuse_pays != 0;
}

// parked: the temporal pass in the first level's loaders, DESIGN.md 5.8.  When the frame runs the a-trous cascade on that path the
// temporal pass is not launched at all: the first level's loader waves accumulate the pixels they stage (svgf_atrous_fused.hip)
// and `acc` stays unwritten unless something other than that level needs it.
void exp_plan_first_pass(svgf_ctx *c, const FrameAsk &q, const AtrousArgs &probe, FramePlan &pl)
{
    const SvgfParams *p = q.p;
    bool plain = q.cascade && (p->kernel_variant == 0 || p->kernel_variant == 6) && !p->paper_steps && p->spatial_variance_frames <= 0;
    for (const int k : { F_MOTION, F_CLAMP, F_XFORM, F_FIREFLY }) if (q.f[k].active) plain = false;
    if (plain) pl.fused = atrous_fused_supported(probe, pl.t) && (p->kernel_variant == 6 || fuse_pays(c, probe));
}

void exp_plan_cascade(svgf_ctx *c, const FrameAsk &q, FramePlan &pl)
{
    const SvgfParams *p = q.p;
    // Cross-level reuse of the geometric terms (svgf_atrous_lane_reuse.hip): a lane-kernel level stores four terms for the next
    // level if that one runs the lane kernel at twice its step, and that level reads them.
    int terms_out[SVGF_MAX_LEVELS];      // tp[] index a level stores its geometric terms in for the next one, -1: none
    for (int i = 0; i < pl.n_levels; i++) {
        AtrousArgs &a = pl.lv[i].a;
        terms_out[i] = -1;
        if (c->exp.use_reuse && i > 0 && pl.lv[i].kind == K_LANE && pl.lv[i - 1].kind == K_LANE && a.step == 2 * pl.lv[i - 1].a.step && a.step <= 32) {
            terms_out[i - 1] = (i >= 2 && terms_out[i - 2] == 0) ? 1 : 0;
            a.tin = pl.lv[i - 1].a.tout = c->exp.tp[terms_out[i - 1]];
            pl.lv[i - 1].a.t_m_out = a.t_m = (c->W + a.step - 1) / a.step;
        }
    }
    // The G-buffer split alone can ride in the first level's loaders (svgf_atrous_fused.hip, FUSED = 4): the temporal pass then
    // writes 28 B/px less.  Only where that level runs the lane kernel at step 2 and nothing reads the planes before it does.
    pl.split_fused = pl.temporal && !pl.fused && c->exp.use_split_fused && q.g && q.cascade && p->kernel_variant == 0 && !p->paper_steps &&
                     p->spatial_variance_frames <= 0 && pl.lv[0].kind == K_LANE && atrous_split_fused_supported(pl.lv[0].a, pl.t);
}

int exp_launch_level(svgf_ctx *c, const FramePlan &pl, int i, KernelTimer &timer)
{
    const LevelPlan &lv = pl.lv[i]; const AtrousArgs &a = lv.a; const TemporalArgs &t = pl.t;
    const hipStream_t s = pl.s;
    if (lv.kind == K_FUSED && pl.temporal) LAUNCH(SVGF_KERNEL_FUSED, launch_atrous_fused(a, t, s));
    else if (lv.kind == K_LANE && pl.split_fused && i == 0) LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_split_fused(a, t, s));
    else if (lv.kind == K_LANE && (a.tin || a.tout)) LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_lane_reuse(a, s));
    else if (lv.kind == K_LANE2Y) LAUNCH(SVGF_KERNEL_ATROUS, launch_atrous_lane_2y(a, s));  // A/B partner of the fused kernel's geometry
    else return 1;
    return SVGF_OK;
}

void exp_commit_frame(svgf_ctx *c, const FramePlan &pl)
{
    Experiments &x = c->exp;
    x.lk_n = pl.n_levels;
    for (int i = 0; i < pl.n_levels; i++) { x.lk_kind[i] = (int)pl.lv[i].kind; x.lk_step[i] = pl.lv[i].a.step; x.lk_asked[i] = pl.lv[i].asked; }
}
