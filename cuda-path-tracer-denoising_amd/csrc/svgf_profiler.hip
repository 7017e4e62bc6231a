// svgf_profiler.hip — svgf_profile_*: per-kernel timings of every stride-th frame, taken from the dispatches themselves.
#include "svgf_context.h"

thread_local SvgfLaunchEvents g_svgf_launch_events = { nullptr, nullptr };

// the arrays and every event created so far (calloc: the others are null); profiling is off afterwards
void profiler_free(Profiler &pr)
{
    for (long long k = 0; pr.ev && k < (long long)pr.frames * SVGF_MAX_KERNELS_PER_FRAME * 2; k++) if (pr.ev[k]) (void)hipEventDestroy(pr.ev[k]);
    free(pr.ev); free(pr.ev_kind); free(pr.ev_n);
    pr.ev = nullptr; pr.ev_kind = nullptr; pr.ev_n = nullptr;
    pr.frames = 0;
}

extern "C" int svgf_profile_enable(svgf_ctx *c, int nframes)
{
    if (!c || nframes < 0) return SVGF_ERR_INVALID_ARG;
    SVGF_ENTER(c);
    Profiler &pr = c->prof;
    if (pr.ev && nframes == pr.frames) {
        // Same number of slots as before: only the counters restart, the events are reused.  Creating a few hundred events takes
        // 0.2-2 ms, and a benchmark that re-arms the profiler between its warm-up and its timed frames would let the GPU idle for
        // that long: 2 ms of idle time cost the following 20 frames 3 % (profiles/r04_clock_states.txt).
        pr.count = 0; pr.frame_no = 0;
        memset(pr.ev_n, 0, sizeof(int) * (size_t)nframes);
        return SVGF_OK;
    }
    profiler_free(pr);
    pr.count = 0; pr.frame_no = 0;
    if (pr.stride < 1) pr.stride = 1;
    if (nframes == 0) return SVGF_OK;
    const long long ne = (long long)nframes * SVGF_MAX_KERNELS_PER_FRAME * 2;
    pr.ev = (hipEvent_t *)calloc(ne, sizeof(hipEvent_t));
    pr.ev_kind = (int *)calloc((size_t)nframes * SVGF_MAX_KERNELS_PER_FRAME, sizeof(int));
    pr.ev_n = (int *)calloc(nframes, sizeof(int));
    if (!pr.ev || !pr.ev_kind || !pr.ev_n) { profiler_free(pr); return SVGF_ERR_OOM; }
    pr.frames = nframes;
    for (long long k = 0; k < ne; k++) {
        hipError_t e = hipEventCreate(&pr.ev[k]);
        if (e != hipSuccess) {          // give back what was created: profiling stays off
            pr.ev[k] = nullptr;
            profiler_free(pr);
            return refuse(c, SVGF_ERR_HIP, "svgf_profile_enable: hipEventCreate failed: %s", hipGetErrorString(e));
        }
    }
    return SVGF_OK;
}

extern "C" int svgf_profile_stride(svgf_ctx *c, int k)
{
    if (!c || k < 1) return SVGF_ERR_INVALID_ARG;
    c->prof.stride = k;
    return SVGF_OK;
}

extern "C" long long svgf_profile_frames(const svgf_ctx *c) { return c ? c->prof.count : 0; }

extern "C" int svgf_profile_read(svgf_ctx *c, int slot, int max_entries, int *kinds, float *ms, int *n_out)
{
    if (!c || !n_out || slot < 0 || slot >= c->prof.frames) return SVGF_ERR_INVALID_ARG;
    SVGF_ENTER(c);
    const Profiler &pr = c->prof;
    const int nk = pr.ev_n[slot];
    int w = 0;
    for (int k = 0; k < nk && w < max_entries; k++, w++) {
        const long long base = ((long long)slot * SVGF_MAX_KERNELS_PER_FRAME + k) * 2;
        float t = 0.0f;
        HIPC(c, hipEventElapsedTime(&t, pr.ev[base], pr.ev[base + 1]));
        if (kinds) kinds[w] = pr.ev_kind[slot * SVGF_MAX_KERNELS_PER_FRAME + k];
        if (ms) ms[w] = t;
    }
    *n_out = w;
    return SVGF_OK;
}

KernelTimer::Launch::Launch(KernelTimer &timer, int kind) : t(timer)
{
    if (!t.on) return;
    t.k = t.pr->ev_n[t.slot];
    if (t.k >= SVGF_MAX_KERNELS_PER_FRAME) return;
    const long long e = (long long)t.slot * SVGF_MAX_KERNELS_PER_FRAME + t.k;
    t.pr->ev_kind[e] = kind;
    g_svgf_launch_events = SvgfLaunchEvents{ t.pr->ev[e * 2], t.pr->ev[e * 2 + 1] };
}

KernelTimer::Launch::~Launch()
{
    if (!t.on || t.k >= SVGF_MAX_KERNELS_PER_FRAME) return;
    const bool consumed = (g_svgf_launch_events.start == nullptr);      // a launcher that did not go through the macro: no entry
    g_svgf_launch_events = SvgfLaunchEvents{ nullptr, nullptr };
    if (consumed) t.pr->ev_n[t.slot] = t.k + 1;
}
