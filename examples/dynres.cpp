// examples/dynres.cpp — a renderer's loop under dynamic resolution: the size the frame is traced and denoised at changes every few
// frames, the displayed size does not (svgf_transfer_history + svgf_upsample, include/svgf.h rows f11 and f10), in C++ through the
// C ABI.
//
// A context is bound to one size for life, so the loop keeps one context per resolution step (three here: 3/4, 2/3 and 1/2 of the
// displayed size).  At a switch, all on one stream:
//   * svgf_transfer_history(next, current, stream): colour history, moments, history lengths, the previous G-buffer planes and the
//     previous view of the sequence, resampled to the new size - the sequence goes on instead of starting again from 1-spp colour;
//   * svgf_denoise on the new context with sepcolor = 1, addcolor = 0 (illumination out);
//   * svgf_upsample(modulate = 1) to the displayed size, as in examples/upsample.cpp.
// The loop runs twice, with the transfer and with what a renderer without it would do (svgf_reset of the context it switches to),
// and prints after the first frame behind each switch the fraction of pixels whose history length is 2 or more.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/dynres.cpp -L cuda-path-tracer-denoising_amd -lsvgf_hip \
//         -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/dynres
//   examples/dynres [frames=24] [width=1920] [height=1080] [period=4]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svgf.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); return 1; } } while (0)
#define SVGF_OKAY(x) do { int rc__ = (x); if (rc__ != SVGF_OK) { fprintf(stderr, "%s failed (%d): %s\n", #x, rc__, svgf_last_error(ctx[cur])); return 1; } } while (0)

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 24, W = argc > 2 ? atoi(argv[2]) : 1920, H = argc > 3 ? atoi(argv[3]) : 1080;
    const int period = argc > 4 ? atoi(argv[4]) : 4;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "dynres: no HIP device (the library has no CPU path)\n"); return 2; }
    if (frames < 1 || W < 4 || H < 4 || period < 1) { fprintf(stderr, "usage: dynres [frames >= 1] [width >= 4] [height >= 4] [period >= 1]\n"); return 2; }
    HIP_OK(hipSetDevice(0));
    const int NS = 3;
    const int w[NS] = { W * 3 / 4, W * 2 / 3, W / 2 }, h[NS] = { H * 3 / 4, H * 2 / 3, H / 2 };      // the resolution steps, largest first
    const size_t N = (size_t)W * H, n_max = (size_t)w[0] * h[0];

    svgf_ctx *ctx[NS] = { nullptr, nullptr, nullptr };
    int cur = 0;
    for (int k = 0; k < NS; k++) { cur = k; SVGF_OKAY(svgf_create(0, w[k], h[k], &ctx[k])); }      // one context per step: 140 B/px of its size each
    float *rgb_lo, *ill_lo, *rgb_hi, *out_hi;
    void *gb_lo, *gb_hi;
    HIP_OK(hipMalloc((void **)&rgb_lo, n_max * 12)); HIP_OK(hipMalloc((void **)&ill_lo, n_max * 12)); HIP_OK(hipMalloc(&gb_lo, n_max * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc((void **)&rgb_hi, N * 12)); HIP_OK(hipMalloc((void **)&out_hi, N * 12)); HIP_OK(hipMalloc(&gb_hi, N * sizeof(SvgfGBufferTexel)));
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));

    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1;
    p.sepcolor = 1; p.addcolor = 0;                                 // illumination out: svgf_upsample multiplies the albedo back at full size
    const SvgfUpsampleParams up = { 0.5f, 0.5f, 1 };
    SvgfGuide lo = { gb_lo, nullptr, nullptr, nullptr, nullptr }, hi = { gb_hi, nullptr, nullptr, nullptr, nullptr };
    std::vector<int> hlen(n_max), gid(n_max);
    std::vector<float> host(3 * N);
    size_t bad = 0;

    for (int transfer = 1; transfer >= 0; transfer--) {
        cur = 0;
        for (int k = 0; k < NS; k++) { cur = k; SVGF_OKAY(svgf_reset(ctx[k])); }
        cur = 0;
        for (int f = 0; f < frames; f++) {
            const int step = (f / period) % NS;
            const bool switched = step != cur;
            if (switched) {
                // the sequence moves to the context of the new size; motion vectors, where a renderer gives them, are in the NEW
                // context's pixel units from this frame on
                if (transfer) { const int from = cur; cur = step; SVGF_OKAY(svgf_transfer_history(ctx[step], ctx[from], s)); }
                else { cur = step; SVGF_OKAY(svgf_sync_stream(ctx[cur], s)); SVGF_OKAY(svgf_reset(ctx[cur])); }
            }
            SvgfCamera cam;
            SvgfSynthParams sp_lo = { f, 7, 0.6f, 0.02f, { 0.0f, 0.0f } }, sp_hi = sp_lo;
            SVGF_OKAY(svgf_synth_camera(f, /*moving=*/1, w[cur], h[cur], &cam, sp_lo.pixel_length));
            SVGF_OKAY(svgf_synth_camera(f, /*moving=*/1, W, H, &cam, sp_hi.pixel_length));      // one camera, two pixel sizes
            // the exact reprojection at any aspect (SvgfParams::reproj_scale): a history survives the moving camera
            p.reproj_scale[0] = sp_lo.pixel_length[0] * (float)w[cur] / 2.0f; p.reproj_scale[1] = sp_lo.pixel_length[1] * (float)h[cur] / 2.0f;
            SVGF_OKAY(svgf_synth_render(0, rgb_lo, gb_lo, w[cur], h[cur], &cam, &sp_lo, s));
            SVGF_OKAY(svgf_synth_render(0, rgb_hi, gb_hi, W, H, &cam, &sp_hi, s));
            SVGF_OKAY(svgf_denoise(ctx[cur], ill_lo, rgb_lo, gb_lo, &cam, &p, s));
            SVGF_OKAY(svgf_upsample(0, out_hi, &hi, W, H, ill_lo, &lo, w[cur], h[cur], &up, s));
            if (switched) {
                const size_t n = (size_t)w[cur] * h[cur];
                SVGF_OKAY(svgf_read_state(ctx[cur], SVGF_STATE_HISTORY_LENGTH, hlen.data(), n * sizeof(int)));      // (synchronises)
                SVGF_OKAY(svgf_read_state(ctx[cur], SVGF_STATE_PREV_GEOM_ID, gid.data(), n * sizeof(int)));          // this frame's geomIds: -1 = ray miss
                size_t kept = 0, hit = 0;
                for (size_t k = 0; k < n; k++) { kept += hlen[k] >= 2; hit += gid[k] != -1; }
                printf("dynres: frame %3d, switch to %4dx%-4d %s: history length >= 2 on %5.1f %% of the pixels (%5.1f %% of them hit the scene)\n",
                       f, w[cur], h[cur], transfer ? "with the transfer" : "after a reset    ", 100.0 * (double)kept / (double)n, 100.0 * (double)hit / (double)n);
            }
        }
        SVGF_OKAY(svgf_sync_stream(ctx[cur], s));
        HIP_OK(hipMemcpy(host.data(), out_hi, 3 * N * sizeof(float), hipMemcpyDeviceToHost));
        double sum = 0.0;
        for (float v : host) { if (v == v && v >= 0.0f && v < 1e6f) sum += v; else bad++; }
        printf("dynres: %d frames %s, %dx%d displayed: mean of the last image %.4f, %zu values out of range\n", frames,
               transfer ? "with the transfer" : "with a reset at every switch", W, H, sum / (3.0 * N), bad);
    }
    for (int k = 0; k < NS; k++) svgf_destroy(ctx[k]);
    (void)hipFree(rgb_lo); (void)hipFree(ill_lo); (void)hipFree(gb_lo); (void)hipFree(rgb_hi); (void)hipFree(out_hi); (void)hipFree(gb_hi);
    (void)hipStreamDestroy(s);
    return bad ? 1 : 0;
}
