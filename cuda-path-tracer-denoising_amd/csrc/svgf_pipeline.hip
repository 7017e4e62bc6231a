// svgf_pipeline.hip — the frame pipeline's resources: second plane set, two internal streams, events; and the probe that decides
// whether the promise (inputs_ready = 1) can be honoured.  Set up by svgf_enable_pipeline (svgf_create_ex(SVGF_CREATE_PIPELINED)
// calls it), never by svgf_denoise: it allocates and synchronises the device.
#include <mutex>

#include "svgf_context.h"

void Pipeline::reset()
{
    frames = 0;
    for (int q = 0; q < 2; q++) { ev_hist[q].forget(); ev_done[q].forget(); ev_tdone[q].forget(); }
}

void pipeline_free(Pipeline &pp)
{
    for (int q = 0; q < 2; q++) {
        if (pp.stream[q]) (void)hipStreamDestroy(pp.stream[q]);
        pp.ev_hist[q].destroy(); pp.ev_done[q].destroy(); pp.ev_tdone[q].destroy();
    }
    if (pp.ev_in) (void)hipEventDestroy(pp.ev_in);
}

__global__ void k_svgf_spin(unsigned long long ticks)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// Do kernels on streams sa and sb overlap?  The HIP runtime spreads a process's streams over GPU_MAX_HW_QUEUES hardware queues
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

// (svgf_create_ex calls it with the context's device current already: the guard nests)
extern "C" int svgf_enable_pipeline(svgf_ctx *c)
{
    SVGF_ENTER(c);
    Pipeline &pp = c->pipe;
    if (pp.pipelined) return SVGF_OK;
    for (int k = 3; k < 6; k++) {
        void *raw = nullptr;
        hipError_t e = c->planes.cv[k] ? hipSuccess : ctx_alloc(c, &raw, c->n * sizeof(float4) + 2 * kPlanePad);
        if (raw) c->planes.cv[k] = reinterpret_cast<float4 *>(static_cast<char *>(raw) + kPlanePad);
        if (e == hipSuccess && !c->planes.vp[k]) e = ctx_alloc(c, (void **)&c->planes.vp[k], variance_plane_bytes(c));
        if (e == hipErrorOutOfMemory) return refuse(c, SVGF_ERR_OOM, "svgf_enable_pipeline: hipMalloc failed for the pipeline's planes");
        HIPC(c, e);
    }
    for (int q = 0; q < 2; q++) {
        if (!pp.stream[q]) HIPC(c, hipStreamCreateWithFlags(&pp.stream[q], hipStreamNonBlocking));
        for (PipeEvent *e : { &pp.ev_hist[q], &pp.ev_done[q], &pp.ev_tdone[q] }) HIPC(c, e->create());
    }
    if (!pp.ev_in) HIPC(c, hipEventCreateWithFlags(&pp.ev_in, hipEventDisableTiming));
    bool overlap = true;
    double ratio = 0.0;
    HIPC(c, probe_two_streams(c->device, pp.stream[0], pp.stream[1], &overlap, &ratio));
    // The runtime hands out hardware queues in an order of its own, and two streams created one after the other can land on ONE queue
    // even when the process has several (seen in fresh C++ processes under the default GPU_MAX_HW_QUEUES = 4, examples/): replace
    // the second stream until the pair overlaps, a few times; with ONE queue in all, no replacement helps and the promise is refused.
    hipStream_t rejected[5];
    int n_rejected = 0;
    for (int k = 0; k < 5 && !overlap; k++) {
        hipStream_t cand = nullptr;
        if (hipStreamCreateWithFlags(&cand, hipStreamNonBlocking) != hipSuccess) break;
        rejected[n_rejected++] = pp.stream[1];
        pp.stream[1] = cand;
        if (probe_two_streams(c->device, pp.stream[0], pp.stream[1], &overlap, &ratio) != hipSuccess) break;
    }
    for (int k = 0; k < n_rejected; k++) (void)hipStreamDestroy(rejected[k]);
    HIPC(c, hipDeviceSynchronize());
    pp.pipelined = 1;
    pp.serial = overlap ? 0 : 1;
    pp.piped_mode = overlap ? 1 : 0;      // (refused: frames stay plain ordered frames until one asks for inputs_ready = 2)
    pp.reset();
    if (!overlap)
        snprintf(c->err, sizeof(c->err), "frame pipeline: the context's internal streams share a hardware queue (six candidate pairs; two 200 us kernels took %.2fx one): "
                 "the inputs_ready = 1 promise is refused and such frames run ordered on the caller's stream; start the process with "
                 "GPU_MAX_HW_QUEUES=8 (read by the HIP runtime at initialisation)", ratio);
    return SVGF_OK;
}

extern "C" int svgf_is_pipelined(const svgf_ctx *c) { return (c && c->pipe.pipelined && c->pipe.piped_mode) ? 1 : 0; }
extern "C" int svgf_pipeline_status(const svgf_ctx *c) { return !c || !c->pipe.pipelined ? 0 : (c->pipe.serial ? 2 : 1); }

// The planes svgf_planar_gbuffer hands out were the CURRENT planes of the frame before last (its levels read them) and are the
// PREVIOUS planes of the last frame (its temporal pass reads them); the producer writes them on a stream of its own choosing.  On an
// ordered context that stream has waited for every frame (stream order).  Frames of a PIPELINED context may still be running on
// another stream of the caller's or on the context's own: svgf_planar_gbuffer waits for the device; svgf_planar_gbuffer_stream makes
// `stream` wait for exactly the two things that still read the planes — the end of the frame before last and the temporal pass of
// the last frame (and the last frame's end when its last level read the one albedo plane) — so that the producer of frame n+1 runs
// beside the levels of frame n.
int pipeline_wait_gbuffer_readers(svgf_ctx *c, bool have_stream, hipStream_t stream)
{
    const Pipeline &pp = c->pipe;
    if (!pp.piped_mode) return SVGF_OK;
    if (!have_stream) { HIPC(c, hipDeviceSynchronize()); return SVGF_OK; }
    const int pq = (int)(pp.frames & 1);      // parity of the NEXT frame = parity of the frame before last
    const PipeEvent &last_done = pp.ev_done[1 - pq];      // (events recorded under a capture are not waited for: cap id 0)
    HIPC(c, pp.ev_done[pq].wait(stream, 0));
    if (pp.ev_tdone[1 - pq].live(0)) HIPC(c, pp.ev_tdone[1 - pq].wait(stream, 0));
    else HIPC(c, last_done.wait(stream, 0));      // (the last frame was not a planar one)
    if (c->planes.last_modulated) HIPC(c, last_done.wait(stream, 0));
    return SVGF_OK;
}
