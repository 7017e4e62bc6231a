// svgf_context.h — the context behind include/svgf.h's handle, grouped by the file that owns each part, the plan of one frame, and
// the few functions that cross the host files: svgf_api.hip (context, settings, read-back), svgf_pipeline.hip, svgf_profiler.hip,
// svgf_frame.hip and, in the experiments build, svgf_experiments.hip.  Internal.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/svgf.h"
#include "svgf_atrous_geometry.h"

#define SVGF_MAX_KERNELS_PER_FRAME (SVGF_MAX_LEVELS + 4)
#pragma GCC visibility push(hidden)      // (what crosses the host files is not exported; to the end of this file)

// An event of the frame pipeline: recorded at least once since the last reset (`valid`), and the stream-capture id it was last
// recorded under (0: eagerly).
class PipeEvent {
    hipEvent_t ev; int valid; unsigned long long cap;
public:
    hipError_t create() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    void destroy() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t record(hipStream_t s, unsigned long long cap_id)
    {
        const hipError_t rc = hipEventRecord(ev, s);
        if (rc == hipSuccess) { valid = 1; cap = cap_id; }
        return rc;
    }
    // (an event recorded under another capture, or eagerly while the waiting frame is captured, or vice versa, is not waited for: such
    // frames are ordered through the caller's stream)
    bool live(unsigned long long cap_id) const { return valid && cap == cap_id; }
    hipError_t wait(hipStream_t s, unsigned long long cap_id) const { return live(cap_id) ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
    bool captured() const { return cap != 0; }
    void disarm() { valid = 0; }
    void forget() { valid = 0; cap = 0; }
};

// Frame pipeline (SvgfParams::inputs_ready, round 5).  A frame's temporal pass needs of the previous frame only what exists
// once the level feeding the colour history has run (level 1 with the reference's defaults); levels 2-5 of frame n and the
// temporal pass + level 1 of frame n+1 are independent.  A pipelined context runs even frames on stream[0] with planes 0-2 and
// odd frames on stream[1] with planes 3-5; ev_hist[q] (recorded behind the level that writes the history of a frame of parity q)
// is all that the other stream's next temporal pass waits for, and the caller's stream waits for ev_done[q] at the end of the
// call.  The kernels of two consecutive frames then share the chip: one frame's level tails, launch gaps and opening bursts
// lie under the other's tap rows (two INDEPENDENT sequences on two streams: +9-10 % in aggregate,
// profiles/r05_exp_two_sequences.log — the ceiling of this).
struct Pipeline {
    int pipelined;         // the second plane set, the internal streams and the events exist (svgf_create_ex / svgf_enable_pipeline)
    int piped_mode;        // frames alternate between the two plane sets (every frame of the context, once on)
    int serial;            // the probe at enable time found the two internal streams on ONE hardware queue: the promise is refused
    int ever_captured;     // a frame of this context has been recorded into a graph: promised frames order themselves behind `stream`
    hipStream_t stream[2];
    PipeEvent ev_hist[2], ev_done[2];
    PipeEvent ev_tdone[2];    // planar frames: behind the temporal pass (the last reader of the PREVIOUS frame's G-buffer planes, which the next producer overwrites)
    hipEvent_t ev_in;
    long long frames;      // frames since the context became pipelined (parity = stream and plane set)
    void reset();          // forgets every event and restarts the parity (a pipelined context stays pipelined)
};

struct Profiler {
    int frames;            // slots; 0 = off
    int stride;            // bracket every stride-th frame
    long long frame_no;    // frames denoised since profile_enable
    long long count;       // frames recorded since enable
    hipEvent_t *ev;        // frames * SVGF_MAX_KERNELS_PER_FRAME * 2
    int *ev_kind;          // frames * SVGF_MAX_KERNELS_PER_FRAME
    int *ev_n;             // frames
};

// The planes and which of them plays which role.  cv[0..2], nrm, gid, mom, hlen, pos and dump are carved from ONE allocation (the
// arena, svgf_api.hip); everything else the context holds on the device comes from ctx_alloc.
struct Planes {
    char *arena;
    size_t arena_bytes;
    float4 *cv[6];         // colour + variance planes: history, source, destination of a level (roles rotate).  [3..5]: the second
                           // set of a PIPELINED context, allocated by svgf_enable_pipeline
    float *vp[6];          // zero-margined (W+2) x (H+2) copies of cv[k].w: what the step-16/32 levels take their 3x3 variance pre-blur from
    unsigned vp_valid;     // bit k: vp[k] holds the variance of cv[k]
    void *dump;            // 4 KB of scrap for the fused kernel (TemporalArgs::dump)
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
    int last_modulated;    // the last frame's last level read the (single) albedo plane
};

// Configuration, not history (svgf_reset keeps it); read by plan_frame when a frame is enqueued.
struct Settings {
    int clamp_radius;      // svgf_set_history_clamp; 0 = off
    float clamp_k;
    int firefly_rank;      // svgf_set_firefly_filter; 0 = off.  Temporal and non-temporal frames alike run on F(in_rgb)
    float firefly_scale;
    const float *xf_dev;   // svgf_set_object_motion: the caller's table, read by the temporal kernel; null or xf_n == 0: off
    int xf_n;
};

// svgf_set_output_taa: the setting (kept by svgf_reset) and the pass's state; the planes exist from the first call that turns it on
struct OutputTaa {
    float alpha;           // 0 = off
    float k;
    float *pre;            // packed rgb: the frame's image, written by the last level / the pass-through copy in place of `out`
    float4 *hist[2];       // {output, geomId bits}: the previous frame's and the one being written
    int cur;               // hist index the next frame reads
    int valid;             // hist[cur] holds the last frame's output (history, not configuration: svgf_reset clears it)
};

#ifdef SVGF_BUILD_EXPERIMENTS
struct Experiments {       // what only svgf_experiments.hip reads
    float4 *tp[2];         // cross-level reuse of the geometric terms: four terms per pixel, written by level L for level L+1 (lane kernels
                           // only, svgf_atrous_lane_reuse.hip); allocated by svgf_create when use_reuse is set
    int use_split_fused;   // svgf_exp_set("split_fused", 1): the G-buffer split of temporal frames in the first level's loaders
    int use_reuse;         // svgf_exp_set("reuse", 1) before svgf_create: measured a loss, profiles/r04_ab_reuse_*.log
    signed char fuse_pays; // -1 not evaluated yet, 1: the fused temporal + first-level kernel is the cheaper way through both
    double est_lane_us[8], est_strip_us[8];   // per log2(step): the two estimates lane_cheaper[] was decided from
    // the a-trous levels of the last frame (svgf_exp_level_kernels), a copy of its plan: kernel (K_FUSED ..), step, and whether the
    // automatic choice compared the estimates of that step
    int lk_n;
    int lk_kind[SVGF_MAX_LEVELS], lk_step[SVGF_MAX_LEVELS], lk_asked[SVGF_MAX_LEVELS];
};
#endif

struct svgf_ctx {
    int device, W, H;
    size_t n;
    int n_cu;              // compute units of the context's device (launch-geometry cost model of the kernel choice)
    signed char lane_cheaper[8];   // per log2(step): -1 not evaluated yet, 1 the lane kernel's estimate is the lower one
    int use_vplane;        // 0 only for A/B measurements (experiments build: svgf_exp_set("no_variance_plane", 1) before svgf_create)
    void *owned[24];       // every device allocation of the context (ctx_alloc), in the order made: what svgf_destroy frees
    int n_owned;
    Planes planes;
    float view_prev[16];   // column-major; identity until the first frame (reference src/denoise.cu:15)
    Pipeline pipe;
    Profiler prof;
    Settings set;
    OutputTaa taa;
#ifdef SVGF_BUILD_EXPERIMENTS
    Experiments exp;
#endif
    // state capture for tests
    int capture;
    float4 *cv_capture;
    // staging for svgf_denoise_host
    float *st_in, *st_out; void *st_g;
    char err[512];
};

// The message svgf_last_error returns, and the code the entry point answers with: `return refuse(c, SVGF_ERR_..., "...", ...)`.
__attribute__((format(printf, 3, 4))) static inline int refuse(svgf_ctx *c, int rc, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(c->err, sizeof(c->err), fmt, ap);
    va_end(ap);
    return rc;
}

#define HIPC(ctx, call)                                                                             \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess)                                                                       \
            return refuse(ctx, SVGF_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

// Entry preamble: a null context is an invalid argument; the call runs on the context's device (SvgfDeviceGuard) or fails.
#define SVGF_ENTER(ctx)                                                                              \
    if (!(ctx)) return SVGF_ERR_INVALID_ARG;                                                         \
    SvgfDeviceGuard dev_guard((ctx)->device);                                                        \
    if (!dev_guard.ok) return refuse(ctx, SVGF_ERR_HIP, "hipSetDevice(%d) failed", (ctx)->device);

static inline int step_log2(int step) { const int l = atrous_step_log2(step); return l < 7 ? l : 7; }      // index of lane_cheaper[] / est_*_us[]

// ---- svgf_api.hip ----
// Each plane has kPlanePad bytes in front of and behind its W*H elements (see the arena).
static const size_t kPlanePad = 128;
// (+64 bytes: the step-16/32 lane kernel reads the variance plane in 16-byte pieces that may end 8 bytes behind the last margin)
static inline size_t variance_plane_bytes(const svgf_ctx *c) { return (size_t)(c->W + 2) * (c->H + 2) * sizeof(float) + 64; }
// The one way the context gets device memory: allocated, cleared on the legacy stream, and the clear complete before the call
// returns (the next frame may run on a non-blocking stream that does not order itself behind it).  *p is set on success only;
// hipErrorOutOfMemory: the allocation failed, any other error: the clear did — nothing stays allocated then.  svgf_destroy frees it.
hipError_t ctx_alloc(svgf_ctx *c, void **p, size_t bytes);

// ---- svgf_pipeline.hip ----
void pipeline_free(Pipeline &pp);
// svgf_planar_gbuffer(_stream): the producer's stream (or the host) waits for the frames that still read the planes handed out
int  pipeline_wait_gbuffer_readers(svgf_ctx *c, bool have_stream, hipStream_t stream);

// ---- svgf_profiler.hip ----
void profiler_free(Profiler &pr);
// Times one launch when profiling is on: the event pair of the slot is armed for the next kernel launch of this thread and
// the launcher's SVGF_LAUNCH_KERNEL attaches it to the dispatch (svgf_kernels.h).  Nothing is recorded on the stream.
struct KernelTimer {
    Profiler *pr; int slot; int k; bool on;
    struct Launch {          // armed for as long as it lives (its end also disarms the pair when the launcher failed before launching)
        KernelTimer &t;
        Launch(KernelTimer &timer, int kind);
        ~Launch();
    };
};
// (needs `c` and `timer` in scope)
#define LAUNCH(kind, expr) do { KernelTimer::Launch timed__(timer, kind); HIPC(c, expr); } while (0)

// ---- svgf_frame.hip: the plan of one frame (every decision, nothing enqueued) ----
void view_matrix_from_camera(const SvgfCamera *cam, float *out);

enum KernelKind { K_FUSED, K_LANE, K_LANE2Y, K_STRIP, K_LATTICE, K_GATHER };      // (the numbering svgf_exp_level_kernels reports)
enum FrameExit { EXIT_CASCADE, EXIT_DEBUG_HLEN, EXIT_DEBUG_VAR, EXIT_COPY };
struct LevelPlan {
    KernelKind kind;
    AtrousArgs a;
    int dst;                        // cv index the level writes; -1: the last level writes `out` only
    bool keep, last, asked;         // keep: the output becomes the colour history (:391); asked: the automatic choice compared the estimates of this step
};
struct FramePlan {
    bool flip, piped, promise;      // the pipeline decision (plan_pipeline); flip: the context goes into piped mode with this frame
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
// What the call and the context's settings ask of a frame (frame_demands).  The features are one table: a row that is active may be
// refused for the image's size (the tiled kernels' grids) or, in the experiments build, by a parked kernel that lacks it.
struct FrameFeature { bool active, tiled; const char *entry, *name, *parked_verb; };
enum { F_MOTION, F_CLAMP, F_XFORM, F_FIREFLY, F_TAA, F_COUNT };
struct FrameAsk {
    const SvgfParams *p;
    const float *in, *g;            // g == nullptr: the planar path
    const void *motion_dev; int motion_format;
    bool cascade;
    FrameFeature f[F_COUNT];
};

// ---- svgf_experiments.hip: where the product's frame path meets the parked kernels.  Empty in the product build. ----
#ifdef SVGF_BUILD_EXPERIMENTS
static const bool kExperimentsBuild = true;
hipError_t exp_create(svgf_ctx *c);                                      // the knobs read at creation, the terms planes
int  exp_refuse_feature(svgf_ctx *c, const SvgfParams *p, const FrameFeature &f);      // frame_demands: a parked kernel was asked for and lacks `f`
bool exp_never_pipelines(const svgf_ctx *c, const SvgfParams *p);
void exp_note_estimates(svgf_ctx *c, int l, double lane_us, double strip_us);
void exp_plan_first_pass(svgf_ctx *c, const FrameAsk &q, const AtrousArgs &probe, FramePlan &pl);      // behind the temporal arguments: fuse?
void exp_plan_cascade(svgf_ctx *c, const FrameAsk &q, FramePlan &pl);                                  // behind the cascade: term reuse, split_fused
int  exp_launch_level(svgf_ctx *c, const FramePlan &pl, int i, KernelTimer &timer);                    // 1: not a parked kernel's level
void exp_commit_frame(svgf_ctx *c, const FramePlan &pl);
#else
static const bool kExperimentsBuild = false;
static inline hipError_t exp_create(svgf_ctx *) { return hipSuccess; }
static inline int  exp_refuse_feature(svgf_ctx *, const SvgfParams *, const FrameFeature &) { return SVGF_OK; }
static inline bool exp_never_pipelines(const svgf_ctx *, const SvgfParams *) { return false; }
static inline void exp_note_estimates(svgf_ctx *, int, double, double) {}
static inline void exp_plan_first_pass(svgf_ctx *, const FrameAsk &, const AtrousArgs &, FramePlan &) {}
static inline void exp_plan_cascade(svgf_ctx *, const FrameAsk &, FramePlan &) {}
static inline int  exp_launch_level(svgf_ctx *, const FramePlan &, int, KernelTimer &) { return 1; }
static inline void exp_commit_frame(svgf_ctx *, const FramePlan &) {}
#endif
#pragma GCC visibility pop
