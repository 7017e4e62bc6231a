/*
 * svgf.h — C ABI of the MI355X-native SVGF denoiser (libsvgf_hip.so).
 *
 * This is the drop-in boundary for the reference's denoiser entry points
 *     void denoiseInit(Scene *scene);                         (reference src/denoise.h:6,  src/denoise.cu:31-61)
 *     void denoiseFree();                                     (reference src/denoise.h:7,  src/denoise.cu:63-74)
 *     void denoise(glm::vec3 *out, glm::vec3 *in,
 *                  GBufferTexel *gbuffer);                    (reference src/denoise.h:8,  src/denoise.cu:349-402)
 * The reference keeps its state in file-static globals and reads 13 `ui_*`
 * globals + `scene->state.camera` at call time (src/main.h:39-69, src/denoise.cu:350-399).
 * Here the same information crosses the boundary explicitly: a context handle
 * (so one context per GPU can coexist), a camera block and a parameter block.
 * `cuda-path-tracer-denoising_amd/csrc/denoise_compat.cpp` rebuilds the three legacy functions (declared by the
 * renderer's own denoise.h) on top of these entry points; INTEGRATION.md shows the binding.
 *
 * Every entry point switches to its context's device and restores the caller's current device before it returns.
 * Contexts are independent: one per GPU (or several per GPU) may be driven from different host threads; one context
 * must not be used from two threads at once.
 *
 * Plain C: pointers and sizes only, no C++/torch types.  All image pointers are
 * DEVICE pointers unless the function name ends in `_host`.
 *
 * Wire formats (kept bit-identical to the reference):
 *   colour image : W*H packed float[3]  (glm::vec3, 12 B), index p = x + y*W   (src/pathtrace.cu:193)
 *   G-buffer     : W*H SvgfGBufferTexel (52 B, align 4)                        (src/sceneStructs.h:113-119)
 */
#ifndef SVGF_H_
#define SVGF_H_

#ifdef __cplusplus
extern "C" {
#endif

#define SVGF_VERSION_MAJOR 0
#define SVGF_VERSION_MINOR 9

/* ---- error codes (every entry point returns one of these; the library never exits) ---- */
#define SVGF_OK                 0
#define SVGF_ERR_INVALID_ARG   -1
#define SVGF_ERR_NO_DEVICE     -2   /* no usable HIP device / HIP runtime error at create */
#define SVGF_ERR_OOM           -3
#define SVGF_ERR_HIP           -4   /* a HIP call or kernel launch failed; see svgf_last_error */
#define SVGF_ERR_UNSUPPORTED   -5

/* G-buffer texel, layout of reference `struct GBufferTexel` (src/sceneStructs.h:113-119):
 * normal@0 position@12 albedo@24 ialbedo@36 geomId@48, sizeof == 52, alignof == 4.
 * geomId == -1 marks a ray miss (src/pathtrace.cu:317-323). */
typedef struct SvgfGBufferTexel {
    float normal[3];
    float position[3];
    float albedo[3];
    float ialbedo[3];
    int   geomId;
} SvgfGBufferTexel;

/* The camera fields `denoise()` reads from `scene->state.camera`
 * (src/sceneStructs.h:74-83; used at src/denoise.cu:33-34,343-346,350-351).
 * right/up are NOT normalised in the reference app (src/main.cpp:180-184); pass them as they are. */
typedef struct SvgfCamera {
    float right[3];
    float up[3];
    float view[3];
    float position[3];
} SvgfCamera;

/* The `ui_*` globals `denoise()` reads (src/main.h:39-69, defaults src/main.cpp:49-62). */
typedef struct SvgfParams {
    int   temporal_enable;    /* ui_temporal_enable  (default 0) */
    int   spatial_enable;     /* ui_spatial_enable   (default 0) */
    float color_alpha;        /* ui_color_alpha      (0.2)  */
    float moment_alpha;       /* ui_moment_alpha     (0.2)  */
    int   blur_variance;      /* ui_blurvariance     (1)    */
    float sigma_l;            /* ui_sigmal           (0.45) luminance edge-stop */
    float sigma_x;            /* ui_sigmax           (0.35) position  edge-stop */
    float sigma_n;            /* ui_sigman           (0.2)  normal    edge-stop */
    int   atrous_nlevel;      /* ui_atrous_nlevel    (5), 0..SVGF_MAX_LEVELS */
    int   history_level;      /* ui_history_level    (1)    */
    int   sepcolor;           /* ui_sepcolor         (0)    */
    int   addcolor;           /* ui_addcolor         (0)    */
    int   right_view_option;  /* ui_right_view_option (0): 0 image, 1 history length, 2 variance */
    /* --- extensions; 0 == reference behaviour --- */
    int   kernel_variant;     /* 0 auto (steps 2-32: the cheaper of the lane-marching and the LDS strip kernel by their
                                 launch-geometry cost model — lane at 1920, 3840, 1600, 3440 columns ..., strip at 1024,
                                 2048 ..., for frames taller than about six lattice rows per level (H / step >= 6); shorter
                                 ones mostly take the strip kernel at the coarse steps; the choice can differ per level
                                 (1280 x 720: strip at step 16 only); the lane kernel at steps 16-32 also needs the
                                 variance plane the previous level leaves; lattice sub-image kernel for steps >= 64; gather where none applies; on NON-temporal
                                 frames the prepare pass (variance fill + G-buffer split) rides in the first level's loader
                                 waves whenever that level runs the lane kernel at step 2 on the AoS boundary: one launch
                                 less, +39 % on BASELINE configs[0]),
                                 1 strict gather kernel on every level,
                                 2 LDS strip kernel for every step 2-32 (error if a step is unsupported, raised before
                                 anything is enqueued),
                                 4 lane-marching kernel wherever it is supported (steps 2-32) whatever the image width,
                                 strip / lattice for the rest; the temporal (or prepare) pass is always its own kernel.
                                 3 is retired (SVGF_ERR_INVALID_ARG).  5 and 6 name parked experiments (two-y-phase geometry;
                                 temporal pass fused into the first level — measured losses) that exist only in
                                 the experiments build of these sources (libsvgf_hip_exp.so, -DSVGF_BUILD_EXPERIMENTS): this
                                 library answers SVGF_ERR_UNSUPPORTED, before anything is enqueued. */
    int   inputs_ready;       /* The FRAME PIPELINE (ABI 0.8; explicit resources since 0.9).  Only a context whose pipeline resources
                                 exist — svgf_create_ex(.., SVGF_CREATE_PIPELINED, ..) or svgf_enable_pipeline(ctx): a second set of colour
                                 planes (+60 B/px), two internal streams, events — looks at this field; any other context orders every
                                 frame on `stream`, and svgf_denoise never allocates or synchronises.
                                 1 is a promise about THIS call: the inputs (colour, G-buffer) are COMPLETE at call time — not merely
                                 enqueued on `stream` — and stay untouched until the work of this call is done.  The library then does
                                 not order the frame behind `stream`: it runs even and odd frames on its two internal streams with
                                 two sets of colour planes, starts a frame's temporal pass as soon as the level that feeds the
                                 previous frame's colour history has run (history_level 1: the previous frame's levels 2-5 and this
                                 frame's temporal pass + level 1 share the GPU), lets only the kernel that writes `output` wait for
                                 what `stream` held at call time (readers of the same buffer behind earlier calls), and makes
                                 `stream` wait for the frame's end — so what the caller enqueues behind the call sees `output`,
                                 exactly as without the promise.  Results are bit-identical to ordered frames
                                 (tests/test_pipeline_gpu.py).  What it is worth depends on the box: +5-10 % at 1080p where the socket
                                 has power headroom, nothing where the ordered frames already run at the power limit.
                                 The promise NEEDS the two internal streams on different hardware queues of the HIP runtime
                                 (GPU_MAX_HW_QUEUES, default 4, read by the runtime when the process starts; a process that also holds
                                 an RCCL communicator or many streams of its own should export 8): on one queue pipelined frames are
                                 8-10 % SLOWER than ordered ones.  The library probes this when the resources are created (two 200 us
                                 kernels, one per stream: side by side or one after the other?), replaces its second stream up to five
                                 times when the pair serialises, and REFUSES the promise when they still
                                 serialise — svgf_pipeline_status() == 2, svgf_last_error() says why, promised frames run as
                                 ordinary ordered frames.
                                 0 = everything ordered on `stream` (the reference's behaviour).
                                 2 = the pipeline WITHOUT the promise: the frame is ordered behind `stream` like any other work
                                 (inputs produced there, output consumed there), and a caller that alternates TWO streams from
                                 frame to frame — each with its own input / output buffers — gets the same overlap from plain
                                 stream semantics, because a stream only waits for the frames that were given to it
                                 (examples/pipeline.cpp: producer + denoiser of consecutive frames overlapping, no events).
                                 Planar frames (svgf_denoise_planar) take both forms up too (ABI 0.9): the promise then covers the
                                 context's own current-frame planes — filled, complete, and not refilled before the work of the
                                 call is done; a producer that refills them every frame takes the pointers through
                                 svgf_planar_gbuffer_stream.  Ignored — the frame is ordered on `stream` — while `stream` is being
                                 captured into a graph.  Once a frame of the context HAS been captured, promised frames order
                                 themselves behind `stream` entirely (a replay of the graph on `stream` uses the same planes): mix
                                 graph replay and the promise only if that is acceptable.  One-launch frames (temporal off, one level)
                                 and frames whose colour history is the LAST level's output have nothing to overlap and never take
                                 the pipeline up. */
    float reproj_scale[2];    /* "next" row f4, paper-faithful reprojection: if > 0, the previous-frame clip
                                 coordinate is divided by it before the ndc mapping: (tan(FOVY) * W / H, tan(FOVY)) =
                                 (pixelLength.x * W / 2, pixelLength.y * H / 2) makes the reprojection exact for any field
                                 of view and aspect ratio.  0 = the reference's mapping (src/denoise.cu:202-203: "no
                                 tan(fov), no aspect", exact only for tan(FOVY) = 1 and W = H; at 16:9 a static camera
                                 keeps its history on ~16 % of the pixels) */
    int   paper_steps;        /* "next" row f4: 1 = a-trous level k (1-based) uses dilation 2^(k-1) = 1, 2, 4, ... as in the
                                 SVGF paper; 0 = the reference's 2^k = 2, 4, 8, ... (its level counter starts at 1,
                                 src/denoise.cu:98,386).  Appended in ABI 0.2 (sizeof(SvgfParams) 68 -> 72). */
    float reproj_position_tol;/* "next" row f4, the consistency test the reference's README (:39) names but isReprjValid
                                 (src/denoise.cu:172-182) does not have: if > 0, a history tap is also rejected when the world
                                 position stored for it in the previous frame lies further than this from the current
                                 pixel's position (Schied et al. 2017 test depth; world position is what the G-buffer of this
                                 renderer carries).  0 = the reference's test (bounds, geomId, normal).  ABI 0.3. */
    int   spatial_variance_frames; /* "next" row f4, the spatial variance estimate the reference leaves as a TODO
                                 (src/denoise.cu:326, EstimateVariance is a constant): if K > 0, a pixel whose updated history
                                 is shorter than K frames takes its variance from the luminance moments of its 7x7
                                 neighbourhood instead of from its own (Schied et al. 2017, section 4.2): taps that pass the
                                 reference's own consistency predicate (same geomId, |n_q - n_p| <= 0.1) count with weight 1,
                                 variance = max(0, mean(m2) - mean(m1)^2) * max(1, 4 / history length).
                                 The pixel itself always counts, whatever its normal; the predicate is evaluated in float32
                                 on sqrt((dx dx + dy dy) + dz dz), so a distance of exactly 0.1f passes, the next float above
                                 it does not, and a tap with a NaN in its normal is skipped; ray misses (geomId -1) pass for
                                 one another; taps outside the image are left out (16 taps in a corner, 28 at the middle of
                                 an edge); the sums run over the taps in raster order in float32; a NaN moment in the window
                                 gives a variance of 0 and a second-moment sum that overflows beside a finite squared mean
                                 gives +inf, never a negative value; a pixel whose updated history has K frames or more
                                 keeps the temporal pass's variance, so K <= 1 acts on no pixel; K belongs to the call, the
                                 context keeps nothing of it.
                                 0 = reference (temporal variance, 100 without history).  ABI 0.3 (sizeof(SvgfParams) 72 -> 80). */
} SvgfParams;

#define SVGF_MAX_LEVELS 10

typedef struct svgf_ctx svgf_ctx;

/* Library / ABI version: (major << 16) | minor. */
int svgf_version(void);

/* Fill *p with the reference defaults of src/main.cpp:49-62. */
int svgf_params_default(SvgfParams *p);

/* denoiseInit equivalent: allocate per-pixel history state for a width x height image on HIP
 * device `device` and zero the history (src/denoise.cu:31-61).  *out receives the handle. */
int svgf_create(int device, int width, int height, svgf_ctx **out);

/* svgf_create with flags (ABI 0.9).  SVGF_CREATE_PIPELINED: also create the frame pipeline's resources now (see
 * SvgfParams::inputs_ready) — second colour-plane set, two internal streams, events, the hardware-queue probe — so that no frame of
 * the sequence ever allocates or synchronises.  Unknown flag bits are SVGF_ERR_INVALID_ARG. */
#define SVGF_CREATE_PIPELINED 1u
int svgf_create_ex(int device, int width, int height, unsigned flags, svgf_ctx **out);

/* The same resources for an existing context, between frames (allocates, synchronises the device; not under stream capture).
 * Idempotent.  Returns SVGF_OK also when the probe refuses the promise: ask svgf_pipeline_status. */
int svgf_enable_pipeline(svgf_ctx *ctx);

/* 0: the context has no pipeline resources (inputs_ready is ignored); 1: it has, and promised frames run on the internal streams;
 * 2: it has, but the two internal streams share a hardware queue of the HIP runtime — the promise (inputs_ready = 1) is refused and
 *    such frames run ordered on the caller's stream (inputs_ready = 2, the caller's own two streams, still works);
 *    svgf_last_error(ctx) holds the explanation right after svgf_create_ex / svgf_enable_pipeline. */
int svgf_pipeline_status(const svgf_ctx *ctx);

/* The library's queue probe for a CALLER's two streams (what inputs_ready = 2 runs on): 1 = kernels enqueued on `stream_a` and `stream_b`
 * run side by side, 0 = the HIP runtime has put the two streams on one hardware queue and they run one after the other (frames in
 * turn on them then gain nothing and pay a few per cent: use one stream and inputs_ready = 0 instead, as examples/farm.cpp and
 * examples/pipeline.cpp do), < 0 = error.  Two 200 us one-wave kernels and two device synchronisations: call it once, at set-up. */
int svgf_streams_overlap(int device, void *stream_a, void *stream_b);

/* denoiseFree equivalent (src/denoise.cu:63-74).  NULL is accepted. */
int svgf_destroy(svgf_ctx *ctx);

/* denoiseFree + denoiseInit on the same size (what runCuda() does on reset, src/main.cpp:192-201):
 * history length, moments and variance go back to zero; nothing is reallocated. */
int svgf_reset(svgf_ctx *ctx);

/* denoise() equivalent (src/denoise.cu:349-402).  Enqueues the whole frame on `stream`
 * (a hipStream_t, NULL = default stream) and returns WITHOUT synchronising; the legacy
 * shim adds the hipDeviceSynchronize() the reference ends with (src/denoise.cu:401).
 * `cam` is the camera of THIS frame; it is retained as the previous view for the next call
 * (src/denoise.cu:399). */
int svgf_denoise(svgf_ctx *ctx, void *out_rgb_dev, const void *in_rgb_dev,
                 const void *gbuffer_dev, const SvgfCamera *cam, const SvgfParams *params,
                 void *stream);

/* Convenience for tests/tools: same call with HOST pointers (uploads, runs, downloads, syncs). */
int svgf_denoise_host(svgf_ctx *ctx, float *out_rgb_host, const float *in_rgb_host,
                      const SvgfGBufferTexel *gbuffer_host, const SvgfCamera *cam,
                      const SvgfParams *params);

/* Block until everything enqueued on the context's DEVICE has finished (hipDeviceSynchronize: what the reference's denoise()
 * ends with, src/denoise.cu:401, and what the legacy shim calls). */
int svgf_sync(svgf_ctx *ctx);

/* Stream-scoped completion (ABI 0.7): block until what has been enqueued on `stream` — the stream the frames were given to
 * svgf_denoise with — has finished, and nothing else: a renderer with several streams does not stall the others.
 * svgf_denoise itself never synchronises and never allocates (the frame pipeline's resources are created by svgf_create_ex /
 * svgf_enable_pipeline, ABI 0.9); frames without the inputs_ready promise touch no stream but `stream`, so such a frame may be captured
 * into a hipGraph (hipStreamBeginCapture .. svgf_denoise .. hipStreamEndCapture) and replayed: the launches are recorded with the plane
 * roles of the captured call, so replay a graph of TWO consecutive frames (or any even number) to keep the context's rotation
 * consistent (tests/test_stream_gpu.py).  Promised frames (inputs_ready = 1 on a pipelined context) run on the context's internal
 * streams and `stream` waits for their end. */
int svgf_sync_stream(svgf_ctx *ctx, void *stream);

/* 1 while the context's frames alternate between its two plane sets (the frame pipeline is in use: resources created and either the
 * probe accepted the promise or a frame has asked for inputs_ready = 2), else 0. */
int svgf_is_pipelined(const svgf_ctx *ctx);

/* 0 for this (product) build; 1 for the experiments build of the same sources, which additionally accepts kernel_variant 5 / 6
 * and exports a tuning entry point that is deliberately not declared here. */
int svgf_build_has_experiments(void);

/* Message of the last error on this context (or of the last failed svgf_create if ctx == NULL). */
const char *svgf_last_error(const svgf_ctx *ctx);

int svgf_width(const svgf_ctx *ctx);
int svgf_height(const svgf_ctx *ctx);

/* ---- state inspection (tests, sequence goldens).  All copy W*H elements to HOST memory, synchronously. ---- */
#define SVGF_STATE_HISTORY_LENGTH   0   /* int32[W*H]   history length that the NEXT frame will read (src/denoise.cu:398) */
#define SVGF_STATE_MOMENTS          1   /* float[2*W*H] moment history of the NEXT frame (src/denoise.cu:397) */
#define SVGF_STATE_COLOR_HISTORY    2   /* float[3*W*H] colour history of the NEXT frame (src/denoise.cu:366,370,391) */
#define SVGF_STATE_VARIANCE_TEMPORAL 3  /* float[W*H]   variance after the temporal pass of the LAST frame (src/denoise.cu:306,315,327) */
#define SVGF_STATE_COLOR_ACC        4   /* float[3*W*H] colour after the temporal pass of the LAST frame (src/denoise.cu:297,313) */
int svgf_read_state(svgf_ctx *ctx, int which, void *host_dst, unsigned long long host_bytes);

/* Keep a copy of the temporal pass output of every following frame so that SVGF_STATE_VARIANCE_TEMPORAL and
 * SVGF_STATE_COLOR_ACC can be read back (costs one extra 16 B/px device copy per frame; tests only). */
int svgf_set_capture(svgf_ctx *ctx, int on);

/* ---- per-kernel timing with HIP events on the launch stream (bench / roofline) ----
 * svgf_profile_enable(ctx, nframes): allocate event pairs for `nframes` frames (0 = off) and restart the frame
 * counter; every following svgf_denoise brackets each kernel it launches with an event pair in slot
 * (frame_counter % nframes).  No synchronisation happens inside svgf_denoise.
 * svgf_profile_read(ctx, slot, ...): after a sync, returns for that slot the kernels launched, in launch order:
 * kind code (SVGF_KERNEL_*) and elapsed milliseconds. */
#define SVGF_KERNEL_TEMPORAL   1
#define SVGF_KERNEL_PREPARE    2   /* non-temporal variance fill + G-buffer split */
#define SVGF_KERNEL_ATROUS     3
#define SVGF_KERNEL_DEBUGVIEW  4
#define SVGF_KERNEL_COPYOUT    5
#define SVGF_KERNEL_FUSED      6   /* prepare pass of a NON-temporal frame + first a-trous level in one launch (ABI 0.6): such a frame reports
                                      one FUSED entry in place of PREPARE + the first ATROUS; temporal frames never do in this build */
/* Timing source: an event pair attached to each kernel dispatch (hipExtLaunchKernelGGL): the kernel's own begin / end
 * timestamps, nothing recorded on the stream.
 * svgf_profile_stride(ctx, k): time only every k-th frame (k >= 1, default 1).
 * svgf_profile_enable(ctx, n) with the n already armed restarts the counters without re-creating events. */
int svgf_profile_enable(svgf_ctx *ctx, int nframes);
int svgf_profile_stride(svgf_ctx *ctx, int every_kth_frame);
long long svgf_profile_frames(const svgf_ctx *ctx);
int svgf_profile_read(svgf_ctx *ctx, int slot, int max_entries, int *kinds, float *ms, int *n_out);

/* ---- "next" row f1: device-side producer of the denoiser's inputs ---------------------------------
 * In the reference the 1-spp colour and the G-buffer are produced on the device by the path tracer (primary rays
 * src/pathtrace.cu:187-208, first-hit G-buffer fill src/pathtrace.cu:317-323) and handed to denoise() as device
 * pointers (src/pathtrace.cu:436-438).  These two entry points stand in for that producer with the analytic
 * Cornell-like scene of SURVEY.md 8(d): svgf_synth_camera replaces runCuda()'s camera update (src/main.cpp:154-190,
 * pixelLength of src/scene.cpp:159-166), svgf_synth_render replaces generateRayFromCamera + the first-bounce G-buffer
 * write + the 1-spp radiance.  Stateless; outputs are packed rgb (12 B/px) and SvgfGBufferTexel (52 B/px) in device
 * memory, ready for svgf_denoise on the same stream. */
typedef struct SvgfSynthParams {
    int   frame;             /* frame index: noise stream, and camera phase when the camera moves */
    int   seed;              /* sequence seed */
    float noise;             /* multiplicative noise amplitude (0.6) */
    float fireflies;         /* fraction of pixels 6x brighter (0.02) */
    float pixel_length[2];   /* Camera::pixelLength, as svgf_synth_camera returns it */
} SvgfSynthParams;
int svgf_synth_camera(int frame, int moving, int width, int height, SvgfCamera *cam, float pixel_length[2]);
int svgf_synth_render(int device, void *out_rgb_dev, void *out_gbuffer_dev, int width, int height,
                      const SvgfCamera *cam, const SvgfSynthParams *sp, void *stream);

/* ---- "next" row f1, second half: the AoS -> plane repack fused into the producer ---------
 * svgf_denoise reads the reference's 52-byte AoS texel (src/sceneStructs.h:113-119) once per frame and splits it into the
 * planes every later kernel works on (packed float3 normals, packed float3 positions, int geomId): 52 B/px fetched, 28 B/px
 * written, only because the producer and the consumer do not share a layout.  A producer that can write planes gets the
 * context's OWN current-frame planes from svgf_planar_gbuffer and fills them in place (src/pathtrace.cu:317-323 is where
 * the reference fills its texel); svgf_denoise_planar then runs the frame without touching an AoS G-buffer at all.
 *   normal, position: packed float3 per pixel; geom_id: int per pixel (-1 = miss); albedo: packed float3 per pixel holding
 *   albedo * ialbedo (only read on the last level when sepcolor && addcolor; may be left unwritten otherwise).
 * The pointers are valid for exactly ONE svgf_denoise_planar call on this context (the planes rotate with the history: ask
 * again for the next frame); producer and svgf_denoise_planar must be ordered on the same stream.  svgf_reset between
 * svgf_planar_gbuffer and svgf_denoise_planar is allowed: it clears both plane sets (so fill the planes AFTER the reset) but
 * does not change which set the pointers name.  Results are bit-identical
 * to svgf_denoise on the same texels (tests/test_planar_inputs.py).  AoS and planar frames may alternate on one context. */
typedef struct SvgfPlanarGBuffer {
    float *normal;
    float *position;
    int   *geom_id;
    float *albedo;
} SvgfPlanarGBuffer;
int svgf_planar_gbuffer(svgf_ctx *ctx, SvgfPlanarGBuffer *out);
/* The same for a PIPELINED context whose producer runs on `stream` (ABI 0.9): instead of waiting for the device (what
 * svgf_planar_gbuffer does on a pipelined context) it makes `stream` wait for exactly what still reads the planes it hands out — the
 * end of the frame before last, whose levels read them as the current G-buffer, and the temporal pass of the last frame, which reads
 * them as the previous one — so that the producer of frame n+1 runs beside the levels of frame n.  Use with inputs_ready = 2 and
 * two streams in turn (producer, svgf_denoise_planar and the consumer of `output` of one frame on one stream).  Not under capture. */
int svgf_planar_gbuffer_stream(svgf_ctx *ctx, SvgfPlanarGBuffer *out, void *stream);
int svgf_denoise_planar(svgf_ctx *ctx, void *out_rgb_dev, const void *in_rgb_dev, const SvgfCamera *cam, const SvgfParams *p, void *stream);
/* svgf_synth_render writing those planes instead of the AoS texel (same pixels, same values) */
int svgf_synth_render_planar(int device, void *out_rgb_dev, const SvgfPlanarGBuffer *out_planes, int width, int height,
                             const SvgfCamera *cam, const SvgfSynthParams *sp, void *stream);
/* sizeof(SvgfParams) of THIS build of the library: the struct has grown at its tail (ABI 0.2: 72 bytes, 0.3: 80) and
 * svgf_denoise reads all of it, so a binding compiled against an older header must not be mixed with a newer library:
 * compare this with the size of your own struct at load time (the Python binding and denoise_compat.cpp do). */
int svgf_params_sizeof(void);

/* ---- "next" row f3: scene-driven producer --------------------------------------------------------
 * The reference's scenes are transformed unit cubes / spheres (src/scene.cpp:47-117, src/intersections.h:50,104) and OBJ
 * triangle meshes (svgf_scene_render_mesh below).  The host side (scene.py: the MATERIAL / OBJECT / CAMERA text format)
 * builds these records; svgf_scene_render casts the primary rays against them and writes colour + G-buffer like
 * svgf_synth_render does for its built-in scene.  geomId = index into `geoms`.  `geoms` and `light` are host memory:
 * the library has read them completely when the call returns (it waits for its own uploads; the kernel behind them stays
 * asynchronous on `stream`). */
#define SVGF_SCENE_MAX_GEOMS 64
typedef struct SvgfSceneGeom {
    int   type;              /* 0 cube [-0.5,0.5]^3, 1 sphere r = 0.5 (object space) */
    int   material;          /* material id of the scene file (informational) */
    float albedo[3];         /* material RGB */
    float emittance;         /* > 0: emitter */
    float xf[12];            /* object -> world, 3x4 row-major: T * Rx * Ry * Rz * S (src/utilities.cpp:65-72) */
    float inv[12];           /* world -> object */
    float invT[9];           /* transpose of inv's 3x3 block (normals of curved primitives) */
} SvgfSceneGeom;
int svgf_scene_render(int device, void *out_rgb_dev, void *out_gbuffer_dev, int width, int height,
                      const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneGeom *geoms, int n_geoms,
                      const float light[3], void *stream);
/* The same with the scene's triangle meshes (Scene::loadMesh's world-space triangles, src/scene.cpp:234-311; host arrays, read
 * completely before the call returns like `geoms`; every triangle is tested for every pixel — no BVH here (row f14 below has one), the reference's
 * scenes have 38 .. 4 968 triangles — so n_tris x width x height is what a call costs): `tris` = n_tris x 3 vertices x {pos[3], normal[3], uv[2]}, `tri_ids` = the object index written as
 * geomId for each triangle, `tri_albedo` = n_tris x rgb (the mesh's material colour), `geom_ids` = the object index written
 * as geomId for each primitive (NULL: its position in `geoms`).  Textures (n_tex may be 0): `tex_data` = 8-bit RGB images, rows
 * top to bottom, `tex_desc` = n_tex x {byte offset into tex_data, width, height}, `tri_tex` = texture index per triangle or -1
 * (anything outside [-1, n_tex) is SVGF_ERR_INVALID_ARG);
 * a textured triangle's albedo is Texture::getColor at the interpolated uv (src/sceneStructs.h:208-219, :162-164).  First hit as the
 * reference's computeIntersection (src/pathtrace.cu:211-276): nearest of primitives and the nearest triangle of the scene
 * (glm::intersectRayTriangle), mesh normal interpolated with Triangle::Intersect's corner weights (src/sceneStructs.h:168-172). */
#define SVGF_SCENE_MAX_TRIS (1 << 20)
int svgf_scene_render_mesh(int device, void *out_rgb_dev, void *out_gbuffer_dev, int width, int height,
                           const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneGeom *geoms, int n_geoms,
                           const int *geom_ids, const float *tris, const int *tri_ids, const float *tri_albedo, int n_tris,
                           const int *tri_tex, const int *tex_desc, const unsigned char *tex_data, int n_tex,
                           const float light[3], void *stream);
/* The same frame written into the planes of svgf_planar_gbuffer instead of AoS texels (same pixels, same values; n_geoms and
 * n_tris may each be 0): the producer side of svgf_denoise_planar for scenes in the reference's format. */
int svgf_scene_render_mesh_planar(int device, void *out_rgb_dev, const SvgfPlanarGBuffer *out_planes, int width, int height,
                                  const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneGeom *geoms, int n_geoms,
                                  const int *geom_ids, const float *tris, const int *tri_ids, const float *tri_albedo, int n_tris,
                                  const int *tri_tex, const int *tex_desc, const unsigned char *tex_data, int n_tex,
                                  const float light[3], void *stream);

/* ---- "next" row f5: per-pixel motion vectors (added after 0.9; probe the symbol) ----------------------------------
 * The temporal pass finds a pixel's history at the coordinate the caller gives instead of projecting the pixel's position
 * through the previous camera: history survives on geometry that moved.  `motion_dev`: W*H elements in device memory, an
 * INPUT like the colour image (inputs_ready covers it); NULL = exactly svgf_denoise / svgf_denoise_planar.  Ignored when
 * temporal_enable == 0.  Any float is defined: NaN, +-inf and off-screen values mean "no history".  INTEGRATION.md has
 * the conventions (pixel centres at integers; `prev` is where this pixel's surface point was in the previous frame). */
#define SVGF_MOTION_PREV_COORD_F32 1   /* float[2]: prev.x, prev.y */
#define SVGF_MOTION_DELTA_F32      2   /* float[2]: prev - (x, y) */
#define SVGF_MOTION_DELTA_F16      3   /* __half[2]: the same, converted to float first */
int svgf_denoise_motion(svgf_ctx *ctx, void *out_rgb_dev, const void *in_rgb_dev, const void *gbuffer_dev,
                        const void *motion_dev, int motion_format, const SvgfCamera *cam, const SvgfParams *params,
                        void *stream);
/* added after 0.9; probe the symbol.  svgf_denoise_planar with the motion plane of svgf_denoise_motion. */
int svgf_denoise_planar_motion(svgf_ctx *ctx, void *out_rgb_dev, const void *in_rgb_dev, const void *motion_dev,
                               int motion_format, const SvgfCamera *cam, const SvgfParams *params, void *stream);
/* added after 0.9; probe the symbol.  Writes such a plane for rigid motion: per pixel the texel's position (AoS texels, or
 * NULL and the two planes), mapped by geom_xf_dev[geomId] (3x4 row-major, this frame's world -> the previous frame's; NULL /
 * out-of-range id: unmoved), through the camera path's own projection with `prev_cam` and `reproj_scale` (NULL = 0, 0).
 * geomId == -1 gets NaN.  With n_geoms = 0 the plane reproduces svgf_denoise bit for bit (SVGF_MOTION_PREV_COORD_F32).
 * Stateless, asynchronous on `stream`, allocates nothing. */
int svgf_motion_reproject(int device, void *motion_out_dev, int motion_format, const void *gbuffer_dev,
                          const float *position_dev, const int *geom_id_dev, int width, int height,
                          const SvgfCamera *prev_cam, const float reproj_scale[2], const float *geom_xf_dev, int n_geoms,
                          void *stream);

/* ---- "next" row f6: history clamp of the temporal pass (added after 0.9; probe the symbol) ------------------------
 * Variance clipping: where the temporal pass found a usable history value, its COLOUR is clamped per channel to
 * mean +- sigma_scale * sigma of the current frame's in_rgb over the (2 radius + 1)^2 window around the pixel, before the blend.
 * History whose shading is no longer plausible (a shadow that moved on, a light switched) stops ghosting; moments, history
 * length and validity are untouched.  Normative arithmetic, float32 without contraction: taps (x+xx, y+yy), yy outer, xx inner,
 * inside the image only (n of them, centre included); s = sum v; m = s / n; q = sum (v - m)(v - m); sd = sqrtf(q / n);
 * lo = m - k sd; hi = m + k sd; if (pc < lo) pc = lo; if (pc > hi) pc = hi (NaN history or bounds: unchanged).
 * radius 0 = off (the default), 1..3; sigma_scale finite and >= 0; otherwise SVGF_ERR_INVALID_ARG, as for a NULL context.
 * Configuration of the context, not history: svgf_reset keeps it.  Read when a frame is enqueued, by all four svgf_denoise*
 * entry points and every inputs_ready mode; frames with temporal_enable == 0 ignore it.  Host state only, no device work.
 * (A clamped temporal frame on a context of more than 262140 rows answers SVGF_ERR_UNSUPPORTED.)
 * INTEGRATION.md 5b says which values to start from. */
int svgf_set_history_clamp(svgf_ctx *ctx, int radius, float sigma_scale);
/* added after 0.9; probe the symbol.  Either pointer may be NULL. */
int svgf_get_history_clamp(const svgf_ctx *ctx, int *radius, float *sigma_scale);

/* ---- "next" row f8: firefly filter of the input colour (added after 0.9; probe the symbol) -----------------------
 * Rank clamp of the CURRENT frame's colour: with the filter on, the frame runs exactly as if in_rgb had been the filtered image
 * F(in_rgb) - the colour that is blended and the luminance that feeds the moments, the window statistics of the history clamp
 * (svgf_set_history_clamp) when one is set, and the colour the non-temporal prepare pass copies.  in_rgb itself is never written.
 * Normative arithmetic of F, float32 without contraction, per pixel p = (x, y) with colour c; L is the library's luminance,
 * (float)((0.2126 (double)r + 0.7152 (double)g) + 0.0722 (double)b):
 *   Lp = L(c_p);  t[0..rank-1] = -inf;  n = 0
 *   for yy = -1..1 (outer), xx = -1..1 (inner), (xx, yy) != (0, 0), (x+xx, y+yy) inside the image:
 *       v = L(c_q);  if (v == v) { n += 1;  for j = 0..rank-1: if (v > t[j]) swap(v, t[j]); }
 *   if (n == 0) unchanged
 *   B = t[min(rank, n) - 1]          the min(rank, n)-th largest neighbour luminance; the centre is excluded, NaN is not counted
 *   bound = scale * B
 *   if (Lp > bound) { s = bound / Lp;  c_p = (r s, g s, b s); }          a NaN Lp or bound: unchanged
 * Every float is a defined input and the arithmetic runs as written (an infinite centre over a finite bound: s = 0, inf * 0 = NaN).
 * rank 0 = off (the default), 1..3; scale finite and >= 0; otherwise SVGF_ERR_INVALID_ARG, as for a NULL context, and the
 * setting is unchanged.  Configuration of the context, not history: svgf_reset keeps it.  Read when a frame is enqueued (a frame
 * already recorded into a graph keeps what it was recorded with), by all four svgf_denoise* entry points, svgf_denoise_host,
 * every inputs_ready mode, AoS and planar frames, temporal frames AND frames with temporal_enable == 0.  Host state only.
 * A temporal frame stays one temporal launch; a non-temporal frame runs its prepare pass as a launch of its own instead of inside
 * the first level.  (A filtered frame on a context of more than 262140 rows answers SVGF_ERR_UNSUPPORTED.)
 * INTEGRATION.md 5d says which values to start from and what they cost. */
int svgf_set_firefly_filter(svgf_ctx *ctx, int rank, float scale);
/* added after 0.9; probe the symbol.  Either pointer may be NULL. */
int svgf_get_firefly_filter(const svgf_ctx *ctx, int *rank, float *scale);

/* ---- "next" row f7: rigid object motion in the temporal pass (added after 0.9; probe the symbol) -------------------
 * Gives the temporal pass the per-object rigid maps of the current frame, the table svgf_motion_reproject takes:
 * geom_xf_dev is device memory of n_geoms x 12 floats, 3x4 row-major, indexed by geomId; each map takes this frame's world
 * space to the previous frame's, xf_prev[g] * inverse(xf_cur[g]).  A geomId outside [0, n_geoms) is unmoved.  NULL or
 * n_geoms == 0 = off (the default).  SVGF_ERR_INVALID_ARG (setting unchanged) for a NULL context, n_geoms < 0, NULL with
 * n_geoms > 0 and a pointer that is not 16-byte aligned (a row of a map is loaded as one 16-byte value).
 * Normative arithmetic, float32 without contraction, per pixel with 0 <= geomId < n_geoms that looks history up, M = X[geomId],
 * p / n the texel's position / normal:
 *   q[r] = ((M[4r] px + M[4r+1] py) + M[4r+2] pz) + M[4r+3]      (svgf_motion_reproject's own sequence)
 *   m[r] = (M[4r] nx + M[4r+1] ny) + M[4r+2] nz                  (linear block only, not renormalised)
 * every other pixel: q = p, m = n, through a branch (no multiplication by an identity).  Effect:
 *   1. svgf_denoise / svgf_denoise_planar (no motion plane): history is looked up at the projection of q through the previous
 *      camera — bit for bit the coordinate svgf_motion_reproject(X) would have written and svgf_denoise_motion read.
 *      With a motion plane the plane gives the coordinate and the table serves the two tests only.
 *   2. the normal test of all nine taps compares the tap's previous normal with m,
 *   3. the position test (SvgfParams::reproj_position_tol > 0) the tap's previous position with q.
 * Nothing else moves: the planes the pass keeps for the next frame hold the true normal and position; blend, moments, clamp
 * and every a-trous level are as they are.  The maps must be rigid (rotation + translation; not checked).  Every float in the
 * table is a defined input: the arithmetic runs as written and the existing predicates see its results.
 * Configuration of the context, like the history clamp: svgf_reset keeps it; host state only, no device work.  Pointer and
 * count are read when a frame is enqueued (a frame recorded into a graph keeps what it was recorded with); the CONTENTS are
 * read by the temporal kernel when it runs: refresh the table on the frame's stream before each frame.  inputs_ready = 1
 * covers the table (complete at call time, untouched until the frame is done).  Honoured by all four svgf_denoise* entry
 * points, svgf_denoise_host and every inputs_ready mode; frames with temporal_enable == 0 ignore it.
 * INTEGRATION.md 5c says when to use the table alone and when table + plane. */
int svgf_set_object_motion(svgf_ctx *ctx, const float *geom_xf_dev, int n_geoms);
/* added after 0.9; probe the symbol.  Either pointer may be NULL. */
int svgf_get_object_motion(const svgf_ctx *ctx, const float **geom_xf_dev, int *n_geoms);

/* ---- "next" row f9: output TAA, the last stage of the SVGF pipeline (added after 0.9; probe the symbol) --------------------
 * Temporal anti-aliasing of the FILTERED image (Schied et al. 2017, the step behind the a-trous cascade): with the feature on, the
 * image the frame would have written to `out` - call it C: the last level's output, its sepcolor && addcolor modulation included,
 * or the pass-through copy where there is no cascade - is blended with the previous frame's OUTPUT, found at the temporal pass's
 * previous-frame coordinate and clipped to C's 3x3 neighbourhood.  One more launch at the end of the frame (SVGF_KERNEL_OUTPUT_TAA
 * in svgf_profile_read, always the last entry).  Normative arithmetic, float32 without contraction, every float a defined input;
 * per pixel p = (x, y) with c = C[p] and g = this frame's geomId[p]:
 *   1. no history - o = c - when g == -1 or the context has no output history (the first frame after svgf_create, svgf_reset or
 *      the call that turned the feature on, and any frame after one that dropped it, below);
 *   2. previous coordinate, the temporal pass's own rule: the call's motion plane in its format (svgf_denoise_motion /
 *      svgf_denoise_planar_motion; the output pass reads the plane on frames with temporal_enable == 0 too, where the temporal
 *      side ignores it), else the projection of the pixel's position through the previous camera with params->reproj_scale, the
 *      position first moved by svgf_set_object_motion's map when one is set and 0 <= g < n_geoms; fx = floor, frac = coord - floor;
 *      no history unless 0 <= fx < W and 0 <= fy < H (NaN and +-inf fail);
 *   3. taps k = 0..3 at (fx + (k & 1), fy + (k >> 1)), weights w = {(1-fracx)(1-fracy), fracx (1-fracy), (1-fracx) fracy, fracx fracy};
 *      a tap counts when it lies inside the image and the geomId stored with the output history at that texel equals g; for the
 *      counted taps in order of k: h += w[k] * hist, sumw += w[k]; if ((double)sumw >= 0.01) h = h / sumw, else no history;
 *   4. h is clamped per channel to mean +- sigma_scale * sigma of C over the 3x3 window around p, exactly the arithmetic of
 *      svgf_set_history_clamp with radius 1 (taps inside the image only; comparisons, so NaN leaves h as it is);
 *   5. o = (alpha * c) + ((1.0f - alpha) * h);
 *   6. out[p] = o, and (o, g) is the output history at p for the next frame.
 * No normal or position test: the clip bounds a wrong history, the geomId test keeps colour from crossing objects.  The pass
 * reads no plane of the previous frame's G-buffer (the output history carries its geomId).
 * alpha == 0 = off (the default); otherwise 0 < alpha <= 1; sigma_scale finite and >= 0 in either case.  Anything else, NaN
 * included, is SVGF_ERR_INVALID_ARG, as is a NULL context: the setting is unchanged and svgf_get_output_taa writes nothing.
 * The first call that turns the feature on allocates the pass's planes (+44 B/px: one packed-rgb plane for C, two 16 B/px output
 * histories; they live until svgf_destroy): it may synchronise the device and must not be made under stream capture, like
 * svgf_enable_pipeline.  SVGF_ERR_OOM when the allocation fails, the setting unchanged.
 * Configuration of the context, not history: svgf_reset keeps alpha and sigma_scale and drops the output history.  Read when a
 * frame is enqueued: a frame recorded into a graph keeps what it was recorded with, including which history plane it reads and
 * whether a history exists (replay graphs of an even number of frames, as svgf_sync_stream's text asks).  Honoured by all four
 * svgf_denoise* entry points and svgf_denoise_host, AoS and planar frames, every inputs_ready mode, temporal and non-temporal
 * frames and every kernel_variant of this build, whenever right_view_option is not a debug view.  Debug views (right_view_option
 * 1 or 2) are written as they are and drop the output history; so does a frame enqueued while the feature is off.  With the
 * feature off a frame enqueues exactly what it did before the feature existed.
 * (A frame with the feature on, on a context of more than 262140 rows, answers SVGF_ERR_UNSUPPORTED before anything is enqueued.)
 * INTEGRATION.md 5e says which values to start from and what the pass costs. */
int svgf_set_output_taa(svgf_ctx *ctx, float alpha, float sigma_scale);
/* added after 0.9; probe the symbol.  Either pointer may be NULL. */
int svgf_get_output_taa(const svgf_ctx *ctx, float *alpha, float *sigma_scale);
#define SVGF_KERNEL_OUTPUT_TAA 7   /* svgf_profile_read: the output pass, the last entry of a frame that runs it */

/* ---- "next" row f10: guided upsampling (added after 0.9; probe the symbol) -------------------------------------------------
 * The full-size image rebuilt from a reduced-size denoise and the full-size G-buffer of the same frame: a renderer traces and
 * denoises the illumination at W_lo x H_lo, keeps its W_hi x H_hi G-buffer (which costs it almost nothing), and multiplies the
 * albedo back at full size, so textures and object edges stay sharp.  `rgb_lo` is the `out` of a svgf_denoise* run on the small
 * frame WITHOUT the final modulation (sepcolor = 1, addcolor = 0), `lo` that frame's G-buffer, `hi` the full-size one.
 * Stateless, asynchronous on `stream`, allocates nothing, one launch.  All image pointers are device pointers; colour images are
 * packed rgb.  Normative arithmetic, float32 without contraction, every float a defined input; per hi pixel P = (x, y) with
 * g, n, p its geomId, normal and position:
 *   rx = (float)width_lo / (float)width_hi, ry = (float)height_lo / (float)height_hi             (float32 divisions)
 *   u = ((float)x + 0.5f) * rx - 0.5f, v = ((float)y + 0.5f) * ry - 0.5f;  fx = floorf(u), ax = u - fx;  fy = floorf(v), ay = v - fy
 *   wb = {(1-ax)(1-ay), ax (1-ay), (1-ax) ay, ax ay};  tap k = 0..3 at (fx + (k & 1), fy + (k >> 1)), INSIDE when it lies in the lo image
 *   pass A (guided): a tap counts when it is inside and geomId_lo == g.  w = wb[k]; if g != -1:
 *       if sigma_n > 0: d = n_lo - n; s = (d.x d.x + d.y d.y) + d.z d.z; t = 1 - sqrtf(s) / sigma_n; if (!(t > 0)) t = 0; w = w t
 *       if sigma_x > 0: d = p_lo - p; s = (n.x d.x + n.y d.y) + n.z d.z; t = 1 - fabsf(s) / sigma_x; if (!(t > 0)) t = 0; w = w t
 *     in order of k: acc[c] += w * rgb_lo[c], sumw += w.  If (double)sumw >= 0.01: o = acc / sumw (a NaN sumw fails the test).
 *   pass B (same object), only if A did not accept: the same sum with w = wb[k] over the inside taps with geomId_lo == g; the same test.
 *   pass C (plain), only if B did not accept: the same sum over all inside taps; the same test; otherwise o = 0.  (With lo <= hi the
 *     nearest inside tap weighs about 0.25 or more: C accepts.)
 *   if modulate: o = o * a per channel, a = albedo * ialbedo of the hi texel (AoS) or the hi albedo plane's value
 *   out[P] = o
 * SVGF_ERR_INVALID_ARG, answered before any device work: a NULL out, rgb_lo, hi, lo or up; a guide with neither `gbuffer` nor all
 * three of normal, position and geom_id; modulate with a planar hi guide whose albedo is NULL; modulate other than 0 or 1; a size
 * <= 0; width_lo > width_hi or height_lo > height_hi; a sigma that is negative, NaN or infinite.  SVGF_ERR_UNSUPPORTED for
 * width_hi * height_hi >= 2^31 / 16, as svgf_motion_reproject answers.
 * INTEGRATION.md 5f says what to feed it; sigma_x is in the scene's world units. */
typedef struct SvgfGuide {          /* one resolution's G-buffer: AoS texels, or planes (gbuffer != NULL wins) */
    const void  *gbuffer;           /* W*H SvgfGBufferTexel, or NULL */
    const float *normal, *position; /* packed float3 per pixel (svgf_planar_gbuffer's layout) */
    const int   *geom_id;
    const float *albedo;            /* packed float3 holding albedo * ialbedo; only read on the hi side with modulate */
} SvgfGuide;
typedef struct SvgfUpsampleParams {
    float sigma_n;   /* width of the normal term, 0 = term off */
    float sigma_x;   /* width of the plane-distance term (world units), 0 = term off */
    int   modulate;  /* 1: multiply the result by the hi side's albedo * ialbedo */
} SvgfUpsampleParams;
int svgf_upsample(int device, void *out_rgb_hi_dev, const SvgfGuide *hi, int width_hi, int height_hi,
                  const void *rgb_lo_dev, const SvgfGuide *lo, int width_lo, int height_lo,
                  const SvgfUpsampleParams *up, void *stream);

/* ---- "next" row f11: history transfer across a resolution change (added after 0.9; probe the symbol) ----------------------------
 * A renderer that denoises at a reduced size (row f10) changes that size from frame to frame; a context is bound to one size for
 * life.  svgf_transfer_history carries the whole history of `src` into `dst`, a context of a different (or the same) size on the same
 * device: everything the next frame of `dst` reads as history becomes `src`'s, resampled to `dst`'s size - the colour history, the
 * moments and history lengths, the previous normals, positions and geomIds, the previous view matrix (copied on the host) and, when
 * both contexts have one, f9's output history.  Whatever `dst` held before is gone, as after svgf_reset(dst).  One launch on
 * `stream`; at equal sizes a bit-exact clone of a sequence.
 * What does not move: `dst`'s configuration (history clamp, firefly filter, object motion, output-TAA settings, pipeline resources,
 * profiling, capture) is unchanged; `src` is only read - a frame given to it afterwards is bit-identical to that frame on a `src` that
 * was never transferred from; data derived from the planes written (the variance copies of the coarse levels) is invalidated, not
 * transferred; the call is not a frame: no profile entry, the frame counters are unchanged.
 * Normative arithmetic, float32 without contraction, every float a defined input; Ws x Hs = src's size, Wd x Hd = dst's:
 *   Ws == Wd && Hs == Hd: every plane is copied bit for bit.  No arithmetic touches the values: NaN and inf survive unchanged.
 *   otherwise, per dst pixel P = (x, y):
 *     rx = (float)Ws / (float)Wd;  ry = (float)Hs / (float)Hd                                      (float32 divisions)
 *     u = ((float)x + 0.5f) * rx - 0.5f;  v = ((float)y + 0.5f) * ry - 0.5f                        (svgf_upsample's mapping)
 *     anchor A = (min(max((int)floorf(u + 0.5f), 0), Ws - 1), min(max((int)floorf(v + 0.5f), 0), Hs - 1))
 *     g = gid_s[A]
 *     gid_d[P] = g;  normal_d[P] = normal_s[A];  position_d[P] = position_s[A];  hlen_d[P] = hlen_s[A]    (bit copies: true texels, never blends)
 *     fx = floorf(u), ax = u - fx;  fy = floorf(v), ay = v - fy;  w = {(1-ax)(1-ay), ax (1-ay), (1-ax) ay, ax ay}
 *     tap k = 0..3 at (fx + (k & 1), fy + (k >> 1)); a tap counts when it lies inside the src image and gid_s[tap] == g
 *     in order of k over the counted taps:  col += w[k] * colour_s[tap];  mom += w[k] * moments_s[tap];  sumw += w[k]
 *     if ((double)sumw >= 0.01) { colour_d[P] = col / sumw;  moments_d[P] = mom / sumw }  else  { the anchor's values, bit copies }
 *     (the anchor is always one of the four taps, with weight about 0.25 or more: the else branch is there for NaN weights only)
 *   the fourth component of the colour plane (the variance the history plane carries along) is the anchor's.
 *   The history length is the anchor's on purpose: a weighted mean truncated to int can lose 1 to rounding on a constant field, and a
 *   transfer must neither age nor rejuvenate a sequence.
 *   Output history: when `dst` has f9 on (svgf_set_output_taa with alpha != 0) and `src` holds a valid output history, the same gather
 *   runs on the output history's rgb, the anchor and g taken from the geomId bits stored with src's output history, and {result, g} is
 *   written to the plane dst's next frame reads: dst's output history is valid.  In every other case `dst` has no output history
 *   afterwards and its next frame takes f9's rule 1.
 * Ratios above 2 subsample (the footprint stays 2 x 2 src texels).  The previous positions are texels of src's grid: with
 * SvgfParams::reproj_position_tol > 0 a transferred tap sits up to half a src texel away from where a native previous frame of dst's
 * size would have put it - choose the tolerance with that in mind.  Motion vectors of dst's next frame are in
 * dst's pixel units, as always.
 * Errors, answered before any device work: NULL dst or src, and dst == src: SVGF_ERR_INVALID_ARG; contexts on different devices:
 * SVGF_ERR_UNSUPPORTED; a `stream` that is being captured into a graph: SVGF_ERR_UNSUPPORTED (the call changes host state that a
 * replay would not).  Pixel indices are 64-bit: every size svgf_create accepts is supported.
 * Ordering: the launch is enqueued on `stream` (a hipStream_t, NULL = default stream).  The caller's contract: frames of both contexts
 * that are not complete have been given to `stream` (or `stream` has been ordered behind them), and dst's next frame goes to `stream`
 * or is ordered behind it; so is whatever overwrites src's history (its frame after next).  On contexts without pipeline resources
 * the call never synchronises and never allocates.  If either context has pipeline resources the call first waits for the device, as
 * svgf_planar_gbuffer does on such a context, forgets dst's pipeline events - dst's next frame runs behind `stream` as a whole, like
 * the first frame after svgf_reset; whether dst alternates its plane sets stays as it is - and orders the internal streams of
 * both contexts behind the launch.  It writes exactly the planes dst's next frame reads.
 * The planes are read back through svgf_read_state kinds 0-2 and 5-8 below; INTEGRATION.md 5g has the recipe (one context per
 * resolution step), examples/dynres.cpp a loop. */
int svgf_transfer_history(svgf_ctx *dst, svgf_ctx *src, void *stream);
/* added after 0.9; probe the symbol (SVGF_ERR_INVALID_ARG from a library that lacks them).  More svgf_read_state kinds. */
#define SVGF_STATE_PREV_NORMAL     5   /* float[3*W*H] the normals the NEXT frame tests its taps against */
#define SVGF_STATE_PREV_POSITION   6   /* float[3*W*H] */
#define SVGF_STATE_PREV_GEOM_ID    7   /* int32[W*H]   */
#define SVGF_STATE_OUTPUT_HISTORY  8   /* float[4*W*H] {r, g, b, geomId bits}: f9's output history; SVGF_ERR_INVALID_ARG while the context has none */

/* ---- "next" row f2: the step right after denoise() ------------------------------------------------
 * svgf_display_pack: reference sendTwoImagesToPBO (src/pathtrace.cu:45-77, launched at :446): `left` (the 1-spp
 *   image) and `right` (the denoised image), both packed rgb floats in device memory, side by side into a
 *   (2*width) x height RGBA8 buffer in device memory; channel = clamp((int)(v * 255.0), 0, 255), alpha 0.
 * svgf_save_png: reference saveImage + image::savePNG (src/main.cpp:131-152, src/image.cpp:22-39) for a HOST image:
 *   clamp(v, 0, 1) * 255.f truncated to a byte, 8-bit RGB PNG; mirror_x != 0 flips the image in x as saveImage does. */
int svgf_display_pack(int device, void *pbo_rgba8_dev, const void *left_rgb_dev, const void *right_rgb_dev, int width,
                      int height, void *stream);
int svgf_save_png(const char *path, const float *rgb_host, int width, int height, int mirror_x);

/* ---- "next" row f12: HDR display - luminance histogram, auto-exposure, tone-mapped pack (added after 0.9; probe the symbol) ------
 * Everything upstream of svgf_display_pack is HDR radiance and the pack clips it at 1.  These entry points meter an image (a
 * log-luminance histogram over the whole chip), keep an exposure that follows the metered average, and pack with that exposure, a
 * tone curve and a display transfer.  All three device entry points are stateless (the exposure lives in SVGF_EXPOSURE_STATE_WORDS
 * 32-bit words of DEVICE memory the caller owns, 4-byte aligned), asynchronous on `stream` and allocate nothing; calls on one stream
 * are ordered.  Normative arithmetic: float32 without contraction, integers otherwise, every float a defined input, no
 * transcendental anywhere.
 * State words: [0..255] accumulating histogram, zero between meterings; [256..511] histogram of the last metered image; [512] n;
 *   [513] m; [514] Lbits; [515] target (float); [516] exposure (float); [517] meterings since reset; [518..519] 0.
 * svgf_exposure_reset (one launch) writes all 520 words: zero, except [515] = [516] = 1.0f.
 * svgf_exposure_meter, launch 1, per pixel of `rgb_dev` (packed rgb, width x height):
 *   L = the library's luminance, (float)((0.2126 (double)r + 0.7152 (double)g) + 0.0722 (double)b)
 *   the pixel is counted iff L == L && L > 0 && L < +inf
 *   bin = min(max((int)(bits(L) >> 20) - 888, 0), 255)      sign, exponent and three mantissa bits: eight bins per octave from
 *                                                            2^-16; bin 0 also takes everything smaller, bin 255 everything from 61440 up
 *   word[bin] += 1                                           integers: the result does not depend on arrival order
 * launch 2 (one workgroup):
 *   h = word[0..255];  n = sum h
 *   lo = (n * trim_low_1024) >> 10;  hi = (n * trim_high_1024) >> 10                                (64-bit products)
 *   P[0] = 0;  P[b+1] = P[b] + h[b];  c[b] = max(0, min(P[b+1], n - hi) - max(P[b], lo));  m = sum c
 *   if m > 0:  S = sum c[b] * (2 * (888 + b) + 1) (64 bits);  Lbits = (uint32)(((S << 19) + (m >> 1)) / m);  Lavg = as_float(Lbits)
 *              (the mean of the bins' centre bit patterns: the inverse of the piecewise-linear logarithm the binning uses)
 *              t = key / Lavg;  if (t < min_exposure) t = min_exposure;  if (t > max_exposure) t = max_exposure
 *   if m == 0: Lbits = 0;  t = (word[517] > 0) ? as_float(word[516]) : 1.0f
 *   prev = as_float(word[516]);  e = (word[517] == 0) ? t : prev + ((t - prev) * adapt)
 *   writes: word[256 + b] = h[b];  word[b] = 0;  [512] = n;  [513] = m;  [514] = Lbits;  [515] = t;  [516] = e;
 *           [517] = min(word[517] + 1, 2^31 - 1);  [518] = [519] = 0
 *   The second launch zeroes the accumulating bins: consecutive meterings on one stream are independent and the caller never clears
 *   anything after the one reset.
 * svgf_display_tonemap (one launch):
 *   e = state_dev ? exposure_bias * as_float(state[516]) : exposure_bias                            (multiplied on the device)
 *   iw2 = white > 0 ? 1.0f / (white * white) : 0.0f                                                 (on the host)
 *   per channel v of either image:  x = v * e
 *   op 0: y = x.   ops 1 and 2 first:  if (!(x > 0.0f)) x = 0.0f;  if (x > 65504.0f) x = 65504.0f
 *   op 1: y = (x * (1.0f + x * iw2)) / (1.0f + x)
 *   op 2: y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)
 *   transfer 0: byte = clamp((int)((double)y * 255.0), 0, 255); the conversion saturates and maps NaN to 0: svgf_display_pack's
 *   transfer 1: the same conversion of sqrtf(y)
 *   transfer 2: byte = #{k in 1..255 : y >= T[k]}, T[k] the float32 nearest to the sRGB decode of k / 255 computed in double
 *               (c / 12.92 for c <= 0.04045, else ((c + 0.055) / 1.055)^2.4); the 256 values are literals of the library, which
 *               never calls pow; svgf_tonemap_srgb_table returns them
 *   alpha = 0.  left_rgb_dev == NULL: the buffer is width x height and holds `right` alone; otherwise it is (2 width) x height, side
 *   by side as svgf_display_pack packs, and both halves get the same mapping.
 * SVGF_ERR_INVALID_ARG, answered before any device work: a NULL state_dev (reset and meter), rgb_dev, pbo_rgba8_dev, right_rgb_dev,
 * ep, tp or thresholds; a size <= 0; key, min_exposure or max_exposure that is not finite and > 0, or min_exposure > max_exposure;
 * adapt outside (0, 1]; a trim outside [0, 1023] or trim_low_1024 + trim_high_1024 > 1023 (within the limit m >= 1 whenever
 * n >= 1); op or transfer outside 0..2; exposure_bias or white negative, NaN or infinite.  SVGF_ERR_UNSUPPORTED:
 * width * height >= 2^31 / 16.  INTEGRATION.md 6a says what to meter and which values to start from. */
#define SVGF_EXPOSURE_STATE_WORDS 520            /* 2080 bytes of DEVICE memory the caller owns, 4-byte aligned */
typedef struct SvgfExposureParams {              /* 24 bytes */
    float key;              /* luminance the metered average is mapped to (0.18) */
    int   trim_low_1024;    /* darkest  share of the counted pixels left out, in 1/1024 (51)  */
    int   trim_high_1024;   /* brightest share left out, in 1/1024 (51) */
    float min_exposure, max_exposure;            /* clamp of the target (1/64, 64) */
    float adapt;            /* share of the way to the target taken per metering, (0, 1]; the caller turns dt into it */
} SvgfExposureParams;
typedef struct SvgfTonemapParams {               /* 16 bytes */
    int   op;               /* 0 none, 1 extended Reinhard per channel, 2 ACES fit (Narkowicz) */
    int   transfer;         /* 0 linear (the reference), 1 gamma 2.0 (sqrtf), 2 sRGB by threshold table */
    float exposure_bias;    /* multiplies the metered exposure (or stands alone when state == NULL) */
    float white;            /* op 1: white point, 0 = plain Reinhard */
} SvgfTonemapParams;
int svgf_exposure_reset (int device, void *state_dev, void *stream);
int svgf_exposure_meter (int device, void *state_dev, const void *rgb_dev, int width, int height,
                         const SvgfExposureParams *ep, void *stream);
int svgf_display_tonemap(int device, void *pbo_rgba8_dev, const void *left_rgb_dev, const void *right_rgb_dev,
                         int width, int height, const SvgfTonemapParams *tp, const void *state_dev, void *stream);
int svgf_tonemap_srgb_table(float thresholds[256]);      /* host only: the table transfer 2 uses */

/* ---- "next" row f13: image-quality meter - MSE / PSNR, largest error, windowed SSIM of two device images (added after 0.9; probe the symbol) ----
 * svgf_quality_meter compares two packed-rgb DEVICE images, `a` the image under test and `b` the reference (width x height pixels,
 * 4-byte aligned), and leaves the totals in device memory.  It is stateless, asynchronous on `stream`, allocates nothing and takes
 * two launches (a tile kernel and a one-workgroup resolve); it changes nothing a frame enqueues.
 * state_dev: svgf_quality_state_bytes(width, height) bytes of DEVICE memory the caller owns, 8-byte aligned.  It needs NO
 *   initialisation: a call rewrites everything it later reads.  The first 64 bytes are the result block, eight 8-byte words:
 *     [0] n_pixels (integer)  [1] n_windows (integer)  [2] sum_se  [3] sum_ssim  [4] max_abs  [5] min_ssim  [6] (double)peak
 *     [7] (double)e                                                                                     ([2]..[7] are doubles)
 *   the rest is the kernels' scratch (six 8-byte words per 64 x 32-pixel tile).
 * exposure_state_dev: NULL, or f12's 520-word state; then e = scale * as_float(word[516]) in float32, multiplied on the device as
 *   svgf_display_tonemap does.  NULL: e = scale.
 * se_map_dev (width x height floats) and ssim_map_dev (nwx x nwy floats, svgf_quality_windows) are optional outputs, 4-byte aligned.
 * Normative arithmetic - every float is a defined input; float32 where stated, DOUBLE elsewhere, nothing contracted.
 * Per pixel:
 *   for each of the six channel values v: t = v * e in float32.  The pixel is COUNTED iff all six t are finite.
 *   if clamp: if (t < 0) t = 0; if (t > peak) t = peak
 *   d_c = (double)ta_c - (double)tb_c;  se = (d_r d_r + d_g d_g) + d_b d_b
 *   La, Lb = the library's luminance of the transformed channels, (float)((0.2126 (double)r + 0.7152 (double)g) + 0.0722 (double)b)
 *   over counted pixels: n_pixels; sum_se = sum of se; max_abs = max |d_c| (0 when no pixel is counted)
 *   se_map[p] = (float)se; the bit pattern 0x7FC00000 for a pixel that is not counted
 * Windows: 8 x 8 at stride 4 (x264's layout), origins (4 i, 4 j), i < nwx, j < nwy, n = (d >= 8) ? (d - 8) / 4 + 1 : 0.  Pixels right
 *   of or below the last window belong to no window (they still count for the error).  A window is counted iff all 64 of its pixels
 *   are.  It is built from four 4 x 4 CELLS.  A cell's five sums, in double: La, Lb, La La, Lb Lb, La Lb (products of the floats
 *   widened to double); a row of a cell is ((v0 + v1) + v2) + v3, the cell ((r0 + r1) + r2) + r3; the window ((c00 + c10) + c01) + c11
 *   with cells c[x][y].  Then
 *     k = 0.015625;  ma = sa k;  mb = sb k;  va = saa k - ma ma;  vb = sbb k - mb mb;  cv = sab k - ma mb
 *     C1 = (0.01 (double)peak)^2;  C2 = (0.03 (double)peak)^2
 *     ssim = ((2.0 ma mb + C1) (2.0 cv + C2)) / (((ma ma + mb mb) + C1) ((va + vb) + C2))
 *   over counted windows: n_windows; sum_ssim; min_ssim (+inf when no window is counted)
 *   ssim_map[i + j nwx] = (float)ssim; the bit pattern 0x7FC00000 for a window that is not counted
 *   In double the form gives exactly 1.0 for a == b and is exactly symmetric in (a, b); in float32 the cancellation in
 *   saa / 64 - ma ma costs up to 2.6e-4 of a window's value on near-flat bright images - which is what a denoised image is.
 * The two sums: workgroups write per-tile partials into the state and the resolve adds them in index order (contiguous runs of
 *   tiles, then the runs); the order is fixed and no floating-point atomic is used, so two calls on the same inputs leave the same
 *   64 bytes.  Against the exact sum of the per-pixel / per-window doubles above, a sum of n terms differs by at most
 *   n 2^-52 sum |term| (any order of n - 1 double additions errs by at most (n - 1) 2^-53 sum |term| to first order; the bound
 *   doubles that).  Everything else in the block is exact: the counts, the max, the min.
 * svgf_quality_read copies the block on `stream`, waits for that stream only, and fills the HOST struct:
 *   mse = sum_se / (3.0 n_pixels);  psnr_db = 10 log10(peak^2 / mse), +inf for mse == 0;  mean_ssim = sum_ssim / n_windows;
 *   NaN where n_pixels == 0 (mse, psnr_db) or n_windows == 0 (mean_ssim).
 * SVGF_ERR_INVALID_ARG, answered before any device work: a NULL state_dev, a_rgb_dev, b_rgb_dev, qp or out_host; a size <= 0; peak
 * or scale that is not finite and > 0; clamp other than 0 or 1.  SVGF_ERR_UNSUPPORTED: width * height >= 2^31 / 16;
 * svgf_quality_state_bytes returns 0 for those sizes and for a size <= 0.  INTEGRATION.md 6b says what to compare with what. */
typedef struct SvgfQualityParams {               /* 12 bytes */
    float peak;             /* the signal's white: PSNR's peak, SSIM's dynamic range L; finite, > 0 */
    float scale;            /* multiplies every channel of both images first (an exposure); finite, > 0 */
    int   clamp;            /* 1: channels clamped to [0, peak] after scaling (display-referred metric); 0: as they are */
} SvgfQualityParams;
typedef struct SvgfQualityResult {               /* 88 bytes, HOST */
    unsigned long long n_pixels, n_windows;
    double sum_se, sum_ssim, max_abs, min_ssim, peak, scale;      /* the eight device words; scale is e, the effective one */
    double mse, psnr_db, mean_ssim;                                /* formed by svgf_quality_read on the host */
} SvgfQualityResult;
unsigned long long svgf_quality_state_bytes(int width, int height);      /* host; a multiple of 8, >= 64; 0 for a size <= 0 or an unsupported one */
int svgf_quality_windows(int width, int height, int *nwx, int *nwy);     /* host; either pointer may be NULL; SVGF_ERR_INVALID_ARG for a size <= 0 */
int svgf_quality_meter(int device, void *state_dev, const void *a_rgb_dev, const void *b_rgb_dev, int width, int height,
                       const SvgfQualityParams *qp, const void *exposure_state_dev, float *se_map_dev, float *ssim_map_dev,
                       void *stream);
int svgf_quality_read (int device, const void *state_dev, SvgfQualityResult *out_host, void *stream);

/* ---- "next" row f14: resident scene - upload once, BVH over the triangles, draw per frame (added after 0.9; probe the symbol) ----
 * svgf_scene_render_mesh uploads the whole scene, waits for that upload and tests every triangle for every pixel on EVERY call.
 * A resident scene is the same scene kept on the device with a bounding-volume hierarchy over its triangles: svgf_scene_create
 * validates, builds and uploads once; svgf_scene_draw / svgf_scene_draw_planar are exactly one launch on `stream` - no allocation,
 * no upload, no host synchronisation, legal under stream capture.  What moves from frame to frame is the camera, the light,
 * SvgfSynthParams and - with row f15 below - rigid per-object poses; topology, textures and the set of objects are fixed at creation.
 * svgf_scene_create: the scene arguments are svgf_scene_render_mesh's (host arrays, read completely before it returns), with the
 *   same validation and error codes, and in addition SVGF_ERR_INVALID_ARG for a vertex POSITION that is not finite (normals and uvs
 *   may be anything), for bp->max_leaf_tris outside 0..8, bp->split outside 0..1 and a NULL `out`; device outside 0..63:
 *   SVGF_ERR_UNSUPPORTED.  All of that is answered before any device work.  One device allocation holds the scene's arrays, the
 *   nodes, the triangle order and the padded triangle boxes.  It allocates and synchronises: not under capture.
 * svgf_scene_destroy waits for the device first (draws in flight read the allocation); NULL is accepted.
 * svgf_scene_draw*: SVGF_ERR_INVALID_ARG for a NULL scene, output, cam, sp or light, a planar target without normal, position and
 *   geom_id, a size <= 0; SVGF_ERR_UNSUPPORTED for width * height >= 2^31 / 16; all before any device work.
 * Normative semantics - a GATED brute force; every tree gives the same frame.  float32, one rounding per operation, no contraction:
 *   Padded box of triangle i, computed by this one formula, on the host at creation and on the device by a pose (row f15).  Per axis c:
 *     mn = min(min(v0, v1), v2), mx likewise;  ext = max over c of (mx_c - mn_c)
 *     pad_c = (ext * 2^-8) + (2^-16 * max(1, |mn_c|, |mx_c|));  lo_c = mn_c - pad_c;  hi_c = mx_c + pad_c
 *   Slab test S(box, ray) -> (pass, tn), ray origin o and direction d:  tn = 0, tf = +inf; per axis c:
 *     if fabsf(d_c) < 2^-100: the axis passes iff lo_c <= o_c <= hi_c, and leaves the interval alone;
 *     otherwise inv = 1.0f / d_c; t1 = (lo_c - o_c) * inv; t2 = (hi_c - o_c) * inv; tn = max(tn, min(t1, t2)); tf = min(tf, max(t1, t2))
 *     pass = every axis passes && tn <= tf.  No NaN arises from finite inputs.
 *   Triangle i COUNTS for a ray iff svgf_scene_render_mesh's own intersection arithmetic gives a t > 0, S(padded box i) passes, and
 *     t >= tn_i.  Among the counting triangles with t below the primitives' nearest hit the smallest t wins; equal t: the lowest
 *     index; a primitive keeps a tie with a triangle.  Everything else - primitives, corner weights, textures, shading, noise, the
 *     stores - is svgf_scene_render_mesh's, the same device code.
 *   A node's box is the exact union (min / max, no arithmetic) of the stored padded boxes below it; a node is skipped iff S(node)
 *     fails or tn_node > the nearest t so far.  Subtraction, multiplication by an `inv` of fixed sign, min and max are monotone, so a
 *     larger box never has a larger tn nor fails where a smaller one passes: skipping is exact and the visiting order is free.
 *   Wherever the winner of svgf_scene_render_mesh's ungated loop passes its own gate - every pixel of every scene the tests hold,
 *   the reference's recorded scenes included - the frame equals svgf_scene_render_mesh's bit for bit.  The gate exists because the
 *   float32 intersection test accepts, at grazing incidence, hits that lie off the triangle, which no box can promise to keep.
 * Builder: binned SAH over the centroids (split 0) or equal counts along the widest centroid axis (split 1); a split that is
 *   degenerate, or whose sides would not fit the depth left, is replaced by equal counts by position in the list.  For every input up
 *   to SVGF_SCENE_MAX_TRIS: depth <= SVGF_SCENE_MAX_DEPTH (root = 0), every leaf holds 1..max_leaf_tris triangles, n_nodes =
 *   2 * n_leaves - 1, and the same input gives the same nodes.  n_tris == 0: n_nodes = 0, and a draw skips the triangle part.
 * INTEGRATION.md 5h has the frame loop and what it costs, examples/resident_scene.cpp runs it. */
typedef struct svgf_scene svgf_scene;
typedef struct SvgfSceneBuildParams {
    int max_leaf_tris;       /* 1..8, 0 = default 4 */
    int split;               /* 0 binned SAH, 1 equal counts on the widest centroid axis */
} SvgfSceneBuildParams;
typedef struct SvgfSceneInfo {
    int n_geoms, n_tris, n_tex, n_nodes, n_leaves, depth, max_leaf_tris;
    unsigned long long device_bytes;
} SvgfSceneInfo;
#define SVGF_SCENE_MAX_DEPTH 48
int svgf_scene_create(int device, const SvgfSceneGeom *geoms, int n_geoms, const int *geom_ids, const float *tris, const int *tri_ids,
                      const float *tri_albedo, int n_tris, const int *tri_tex, const int *tex_desc, const unsigned char *tex_data,
                      int n_tex, const SvgfSceneBuildParams *bp /* NULL = defaults */, svgf_scene **out);
int svgf_scene_destroy(svgf_scene *scene);
int svgf_scene_info(const svgf_scene *scene, SvgfSceneInfo *out);
int svgf_scene_draw(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev, int width, int height,
                    const SvgfCamera *cam, const SvgfSynthParams *sp, const float light[3], void *stream);
int svgf_scene_draw_planar(const svgf_scene *scene, void *out_rgb_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                           const SvgfCamera *cam, const SvgfSynthParams *sp, const float light[3], void *stream);
/* The builder by itself: host only, no device needed.  count > 0: a leaf over triangles order[first .. first + count);
 * count == 0: an inner node with children first and first + 1; node 0 is the root.  `tris` as svgf_scene_render_mesh takes them
 * (24 floats per triangle; positions must be finite); `nodes` has room for 2 * max(n_tris, 1), `order` for n_tris. */
typedef struct SvgfBvhNode { float lo[3]; int first; float hi[3]; int count; } SvgfBvhNode;   /* 32 bytes */
int svgf_bvh_build_host(const float *tris, int n_tris, const SvgfSceneBuildParams *bp, SvgfBvhNode *nodes, int *n_nodes,
                        int *order, int *depth);

/* ---- "next" row f15: animated resident scene - pose objects and refit the BVH on the device (added after 0.9; probe the symbol) ----
 * A resident scene whose objects move rigidly: per frame the caller hands over a DEVICE table of per-object poses, and
 * svgf_scene_pose re-poses the triangles and primitives from their rest state, recomputes the padded triangle boxes, refits the
 * node boxes and writes row f7's motion table for the same frame - at most three launches on `stream`, no allocation, no upload, no
 * host wait, legal under stream capture.  Nothing of row f14's contract moves: the frame is the gated brute force over the POSED
 * triangles, which every tree reproduces, so a refitted tree draws the frame a tree rebuilt at that pose would.
 * What stays static: the topology (nodes' first / count, the triangle order - the tree is refitted, never re-split, however loose its
 * boxes become; row f24 below lets a scene adopt a tree rebuilt elsewhere), the textures, and the set of objects.  Row f26 below
 * lets renderer-side code move vertices independently of each other (include/svgf_deform.h).
 * svgf_scene_enable_pose(scene, n_objects): allocates the animation side once - posed copies of the triangles, triangle boxes, nodes
 *   and primitives, the HELD pose table (identity) and the refit plan.  The arrays svgf_scene_create uploaded become the REST state
 *   and are never written again; the posed copies start as bit copies of them and the draws read them from now on.  Allocates and
 *   synchronises: not under capture (like svgf_enable_pipeline).  A second call with the same n_objects is a no-op; a different
 *   n_objects, n_objects outside 1..SVGF_SCENE_MAX_POSED or a NULL scene is SVGF_ERR_INVALID_ARG, before any device work.  A scene
 *   that never calls it is byte for byte row f14's.  svgf_scene_info's device_bytes grows by the second allocation.
 * svgf_scene_pose(scene, pose_dev, n_objects, motion_out_dev, stream): one call per frame, ahead of the draw, on the draw's stream.
 *   pose_dev: n_objects SvgfScenePose records in device memory, whose CONTENTS the kernels read when they run (row f7's rule: a
 *   captured pose replays with whatever the table holds then).  Object id k is tri_ids / geom_ids (a primitive's index where geom_ids
 *   was NULL); an id outside [0, n_objects) keeps its rest state through a branch (a bit copy, no arithmetic).  Poses apply to the
 *   REST state, never to the previous pose: the same table twice leaves the same bytes, nothing drifts.
 *   SVGF_ERR_INVALID_ARG, before any device work, the scene untouched: a NULL scene or table, n_objects other than what was enabled,
 *   a scene without svgf_scene_enable_pose, a pose_dev or motion_out_dev that is not 16-byte aligned.
 * Normative arithmetic - float32, one rounding per operation, no contraction; M = pose[id].xf:
 *   vertex position  p'[r] = ((M[4r] px + M[4r+1] py) + M[4r+2] pz) + M[4r+3]
 *   vertex normal    n'[r] = (M[4r] nx + M[4r+1] ny) + M[4r+2] nz         (linear block, not renormalised: row f7's rule)
 *   uv, albedo, texture index, id: untouched.
 *   Padded box of a posed triangle: row f14's formula on the posed positions - computed by that one formula, on the host at creation
 *   and on the device by a pose.
 *   C = A o B of two 3x4 maps: C[r][c] = (A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c], and for c == 3 "+ A[r][3]" last.
 *   Primitive with a posed id: xf' = pose.xf o xf_rest; inv' = inv_rest o pose.inv; invT' = transpose of inv's 3x3 block; the rest copied.
 *   Motion table: motion_out_dev non-NULL: row k < n_objects (12 floats) = held[k].xf o pose[k].inv - this frame's world to the
 *   previous frame's, what svgf_set_object_motion and svgf_motion_reproject take.  Then held := pose (also with NULL), on the device in
 *   stream order, so a replayed graph chains.  held is the identity after svgf_scene_enable_pose.
 *   Node boxes: a leaf = fminf / fmaxf union of the posed boxes of order[first .. first + count); an inner node = the union of its two
 *   children.  A pose is expected to be finite and rigid (not checked); every float is a defined input to the above, and because the
 *   topology is fixed a NaN or inf cannot make a draw loop or read out of bounds.
 * svgf_scene_read: a blocking read-back (tests, debugging; like svgf_read_state).  Kinds: 0 triangles as drawn (96 B each),
 *   1 padded triangle boxes as drawn (SvgfBvhNode: first = i, count = 1), 2 nodes, 3 primitives as drawn (SvgfSceneGeom), 4 order,
 *   5 the held pose table (posed scenes only).  host_bytes must be the array's size exactly; otherwise, or for another kind,
 *   SVGF_ERR_INVALID_ARG.  Works on a static scene (what was created).
 * svgf_pose_rigid (host only): rotation by angle_rad about `axis` through `pivot`, then `translate`; computed in double, inv the
 *   analytic inverse (R^T, -R^T t), each of the 24 values rounded to float32 once.  A zero axis or a non-finite argument:
 *   SVGF_ERR_INVALID_ARG.
 * svgf_bvh_refit_plan_host (host only, no device needed): the partition svgf_scene_pose refits by, from the nodes alone.  A TREELET
 *   is a whole subtree of at most `cap` nodes whose parent's subtree is larger: node `root` and its descendants, nodes
 *   [begin, begin + count); `levels` = 1 + the deepest local level (root = 0) that holds an inner node, 0 for a single leaf.  The TOP
 *   is every node whose subtree exceeds `cap`, listed deepest first in n_top_depths segments top[top_seg[s] .. top_seg[s + 1]), one
 *   per depth: a top node's children are treelet roots or stand in an earlier segment.  level[k] = the local level of a treelet node,
 *   the depth of a top node.  Room: treelets, level, top: n_nodes; top_seg: SVGF_SCENE_MAX_DEPTH + 2.  SVGF_ERR_INVALID_ARG for
 *   arrays that are no binary tree by the SvgfBvhNode rules (a child at or before its parent, two parents, an unreached node, a
 *   negative first / count) or cap < 1; SVGF_ERR_UNSUPPORTED for a depth above SVGF_SCENE_MAX_DEPTH or a tree not laid out as the
 *   builder lays it out (children in pairs, a node's descendants in one index range starting at its first child).
 * INTEGRATION.md 5i has the frame loop and what a pose costs, examples/animated_scene.cpp runs it. */
typedef struct SvgfScenePose { float xf[12]; float inv[12]; } SvgfScenePose;  /* rest world -> this frame's world, and back; 3x4 row-major */
#define SVGF_SCENE_MAX_POSED 1024
#define SVGF_SCENE_REFIT_CAP 1024    /* nodes per treelet of svgf_scene_pose's refit (32 KB of LDS) */
typedef struct SvgfRefitTreelet { int root, begin, count, levels; } SvgfRefitTreelet;
typedef struct SvgfRefitPlanInfo { int n_treelets, n_top, n_top_depths, cap; } SvgfRefitPlanInfo;
int svgf_scene_enable_pose(svgf_scene *scene, int n_objects);
int svgf_scene_pose(svgf_scene *scene, const SvgfScenePose *pose_dev, int n_objects, float *motion_out_dev, void *stream);
int svgf_scene_read(const svgf_scene *scene, int which, void *host_dst, unsigned long long host_bytes);
int svgf_pose_rigid(const float axis[3], float angle_rad, const float pivot[3], const float translate[3], SvgfScenePose *out);
int svgf_bvh_refit_plan_host(const SvgfBvhNode *nodes, int n_nodes, int cap, SvgfRefitTreelet *treelets, unsigned char *level,
                             int *top, int *top_seg, SvgfRefitPlanInfo *info);

/* ---- "next" row f16: shadowed resident scene - stochastic shadow rays through the BVH (added after 0.9; probe the symbol) ----
 * svgf_scene_draw shades every hit towards a point light whatever stands in between.  svgf_scene_draw_shadowed draws the same
 * frame and, per pixel, casts `samples` shadow rays from the surface towards points of a parallelogram light: the one-sample
 * visibility estimate of an area light, the noise SVGF was designed for (a penumbra pixel is lit or dark in any one frame, the
 * truth is the mean over frames).  One launch on `stream`, no allocation, no upload, no host wait, legal under stream capture; on a
 * static scene and on a posed one (row f15), where it reads the posed arrays exactly as svgf_scene_draw does.
 * Exactly one of out_gbuffer_dev (AoS texels) and planes (svgf_planar_gbuffer's layout) is non-NULL.
 * Errors: svgf_scene_draw's, and in addition SVGF_ERR_INVALID_ARG for a NULL light, samples outside
 *   1..SVGF_SCENE_MAX_SHADOW_SAMPLES, a light field that is not finite, both targets given or neither; all before any device work.
 * Normative semantics - float32, one rounding per operation, no contraction:
 *   G-buffer: every field (AoS or planes) is what svgf_scene_draw writes with light = centre, bit for bit.  Shadows touch colour only.
 *   A miss (geomId < 0) and an emissive hit (emittance > 0) cast no ray and get svgf_scene_draw's colour.
 *   Every other pixel p (= y * width + x), pos its G-buffer position, sample s = 0 .. samples - 1:
 *     u = hash(seed, frame, p, 8 + 2s), v = hash(seed, frame, p, 9 + 2s)    (svgf_synth_render's hash; streams 0..4 stay the noise)
 *     L_c = (centre_c + (2u - 1) * edge_u_c) + (2v - 1) * edge_v_c;   q_c = L_c - pos_c;   dl = sqrtf((q0 q0 + q1 q1) + q2 q2)
 *     !(dl > 0): the sample is unoccluded, no ray is formed.  Otherwise d_c = q_c / dl, t_lo = 2^-10 * fmaxf(1, dl), t_hi = dl - t_lo,
 *     and the sample is OCCLUDED iff an occluder counts on the ray (pos, d) with t_lo < t < t_hi.  Occluders:
 *       triangle i: row f14's rule on that ray - svgf_scene_render_mesh's intersection arithmetic (back-face cull included) gives t,
 *         S(padded box i) passes and t >= tn_i;
 *       primitive k with emittance == 0: its cube / sphere test - the one the primary ray runs - reports a hit and the world-space
 *         distance tw of that hit lies in the interval.  Every primitive, not only the nearest.  An emitter never occludes.
 *   Occlusion is an OR over the counting occluders, so it does not depend on visiting order, tree or leaf size: a node is skipped
 *     iff S(node) fails or tn_node > t_hi (exact by row f14's monotonicity argument), and leaving at the first occluder is free.
 *   Colour: vis = (float)unoccluded / (float)samples, and the shade of svgf_scene_draw becomes
 *     0.15f + vis * ((30.0f * lam) / (4.0f + dist2))        lam, dist2 from `centre` exactly as svgf_scene_draw forms them;
 *     everything behind the shade (noise multiplier, fireflies, chroma, stores) is unchanged.  With nothing in the way vis = 1 and
 *     the colour is svgf_scene_draw's on every bit.  edge_u = edge_v = 0 is a point light: vis is 0 or 1, hard shadows.
 * INTEGRATION.md 5j has the frame loop and what a shadow ray costs, examples/shadowed_scene.cpp runs it. */
typedef struct SvgfSceneLight {
    float centre[3];      /* what svgf_scene_draw takes as `light`: the Lambert term and the fall-off use it, unchanged */
    float edge_u[3];      /* half-edges of a parallelogram light around centre; both zero = a point light, hard shadows */
    float edge_v[3];
    int   samples;        /* shadow rays per pixel and frame, 1..SVGF_SCENE_MAX_SHADOW_SAMPLES */
} SvgfSceneLight;
#define SVGF_SCENE_MAX_SHADOW_SAMPLES 64
int svgf_scene_draw_shadowed(const svgf_scene *scene, void *out_rgb_dev, void *out_gbuffer_dev /* or NULL */,
                             const SvgfPlanarGBuffer *planes /* or NULL */, int width, int height, const SvgfCamera *cam,
                             const SvgfSynthParams *sp, const SvgfSceneLight *light, void *stream);

/* ---- "next" row f17: a read-only view of the resident scene (added after 0.9; probe the symbol) ----
 * What svgf_scene_draw* read, for renderer-side code that traces its own rays through the same scene: the companion library
 * libsvgf_trace.so (include/svgf_trace.h: a one-bounce path-traced draw) reaches the scene through this call and nothing else.
 * Host only, no device work.  On a posed scene (row f15) the pointers are the posed arrays, exactly what svgf_scene_draw reads;
 * `geom_ids` is NULL where svgf_scene_create got none, `tri_tex` where the scene has no texture.  nodes / tri_boxes are SvgfBvhNode
 * records (a triangle's padded box: first = i, count = 1).  The view is valid until svgf_scene_destroy or svgf_scene_enable_pose
 * (which moves the draws to the posed copies); the arrays' CONTENTS change with every svgf_scene_pose, in stream order.
 * A NULL argument: SVGF_ERR_INVALID_ARG. */
typedef struct SvgfSceneView {
    int device, n_geoms, n_tris, n_tex, n_nodes, depth;
    const SvgfSceneGeom *geoms;
    const int *geom_ids;
    const float *tris;              /* 24 floats per triangle */
    const int *tri_ids;
    const float *tri_albedo;
    const int *tri_tex;
    const int *tex_desc;
    const unsigned char *tex;
    const SvgfBvhNode *nodes;
    const int *order;
    const SvgfBvhNode *tri_boxes;
} SvgfSceneView;                    /* 112 bytes */
int svgf_scene_view(const svgf_scene *scene, SvgfSceneView *out);

/* ---- "next" row f24: draw with a tree of the caller's (added after 0.9; probe the symbol) ----
 * Row f14's frame is a gated brute force that every valid tree reproduces, so a scene can walk any tree over its triangles without
 * a pixel changing.  svgf_scene_adopt_tree hands it one: from this call on every draw (svgf_scene_draw*, and the companion libraries
 * through svgf_scene_view) reads nodes_dev / order_dev instead of the scene's own arrays; svgf_scene_view hands them out,
 * svgf_scene_info reports n_nodes, n_leaves and depth = depth_bound, svgf_scene_read kinds 2 and 4 read them back.  Host only: no
 * device work, no allocation, no synchronisation - the caller orders whatever builds the arrays ahead of the draws on the stream,
 * and keeps them alive and valid (a binary tree by the SvgfBvhNode rules over order_dev, a permutation of 0 .. n_tris - 1, no
 * deeper than depth_bound; exact boxes) while they are adopted.  libsvgf_lbvh.so (include/svgf_lbvh.h) builds such a tree on the
 * device from the triangle boxes as drawn.
 * nodes_dev == NULL detaches: the scene is back on its own tree and its own info.
 * SVGF_ERR_INVALID_ARG, the scene untouched: a NULL scene; a scene with n_tris == 0; n_leaves outside 1..n_tris; n_nodes other than
 *   2 * n_leaves - 1; depth_bound outside 0..SVGF_SCENE_MAX_DEPTH (the draws' stack); a pointer that is not 16-byte aligned; a NULL
 *   order_dev with non-NULL nodes.
 * svgf_scene_pose on a scene with an adopted tree launches the pose kernel only (triangles, padded boxes, primitives, motion table,
 *   held) and skips both refit launches: THE ADOPTED TREE IS THEN STALE - its boxes no longer bound the posed triangles - until the
 *   caller rebuilds it, and a draw in between may miss triangles.  The frame loop is pose, build, draw.  The refit plan and the
 *   scene's own posed nodes stay valid: after a detach the next svgf_scene_pose refits them from the posed boxes as before (until
 *   that pose they are as stale as the last refit left them).
 * A scene that never adopts a tree is row f23's on every byte. */
int svgf_scene_adopt_tree(svgf_scene *scene, const SvgfBvhNode *nodes_dev, const int *order_dev, int n_nodes, int n_leaves,
                          int depth_bound);

/* ---- "next" row f26: write the triangles as drawn, refit on request (added after 0.9; probe the symbol) ----
 * Rows f15 and f24 let svgf_scene_pose alone change the triangles as drawn: one rigid map per object.  These two host-side entry
 * points let renderer-side code move vertices independently of each other - libsvgf_deform.so (include/svgf_deform.h) skins triangles
 * with them - while the frame stays row f14's gated brute force over the triangles as they stand.
 * svgf_scene_drawn_arrays(scene, tris_dev, tri_boxes_dev): WRITABLE device pointers to the posed copies, 96 bytes per triangle and 32
 *   bytes per padded box (SvgfBvhNode: first = i, count = 1) - the arrays the draws and svgf_scene_view read.  Host only: no device
 *   work, no allocation, no synchronisation; the pointers hold until svgf_scene_destroy.  SVGF_ERR_INVALID_ARG, nothing written: a
 *   NULL argument; a scene without svgf_scene_enable_pose - its arrays are the REST state and are never written.
 *   A WRITER OWES THE SCENE row f14's padded box for every triangle it writes, computed by that one formula (the literals and nesting
 *   of svgf_bvh_tri_box), in stream order ahead of the tree and the draw; uv, albedo, texture index and id are not the writer's.
 *   svgf_scene_pose rewrites every triangle and box from the rest state: a writer runs behind it, on triangles whose id stands
 *   outside the pose table.
 * svgf_scene_refit(scene, stream): exactly the two refit launches of svgf_scene_pose (treelets, then the top) on the scene's OWN nodes,
 *   from the padded boxes as drawn, and nothing else - no pose, no motion table, held untouched.  No allocation, no host wait; legal
 *   under stream capture.  Allowed while a tree is adopted: the adopted tree is not touched, and the scene's own tree is valid again
 *   after a detach.  The topology stays what svgf_scene_create built: a refitted tree is exact and as loose as the deformation makes
 *   it; re-splitting is rows f24 and f25.  SVGF_ERR_INVALID_ARG for a NULL scene or one without svgf_scene_enable_pose.
 * A scene that never calls either is row f25's on every byte; no kernel changed.
 * THE TWO PROTOTYPES stand in include/svgf_scene_write.h, which includes this header: the functions this header declares are the set
 * the Python binding's EXPORTS table is pinned to (tests/test_abi.py, tests/test_binding_surface.py), and these two are bound by
 * deform.py beside the library that uses them. */

#ifdef __cplusplus
}
#endif
#endif /* SVGF_H_ */
