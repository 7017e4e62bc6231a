// examples/upsample.cpp — a renderer's loop that denoises at a reduced size and rebuilds the full-size image (svgf_upsample,
// include/svgf.h row f10), in C++ through the C ABI.
//
// Per frame, all on one stream:
//   * the PRODUCER (the path tracer's role; here svgf_synth_render) writes the 1-spp colour and the G-buffer at the small size, and
//     the G-buffer at the full size from the same camera (a real renderer rasterises or traces primary rays for it);
//   * svgf_denoise on the small frame with sepcolor = 1, addcolor = 0: the output is the filtered ILLUMINATION, albedo divided out;
//   * svgf_upsample(modulate = 1): the four small-frame taps around each full-size pixel, weighted by how well their G-buffer agrees
//     with the pixel's own, times the full-size albedo: textures and object edges stay at full resolution;
//   * svgf_display_pack: the full-size 1-spp image beside the result.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/upsample.cpp -L cuda-path-tracer-denoising_amd -lsvgf_hip \
//         -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/upsample
//   examples/upsample [frames=100] [width=3840] [height=2160] [divisor=2]
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svgf.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); return 1; } } while (0)
#define SVGF_OKAY(x) do { int rc__ = (x); if (rc__ != SVGF_OK) { fprintf(stderr, "%s failed (%d): %s\n", #x, rc__, svgf_last_error(ctx)); return 1; } } while (0)

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 100, W = argc > 2 ? atoi(argv[2]) : 3840, H = argc > 3 ? atoi(argv[3]) : 2160;
    const int div = argc > 4 ? atoi(argv[4]) : 2;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "upsample: no HIP device (the library has no CPU path)\n"); return 2; }
    if (frames < 1 || W <= 0 || H <= 0 || div < 1 || W / div < 1 || H / div < 1) { fprintf(stderr, "usage: upsample [frames >= 1] [width] [height] [divisor >= 1]\n"); return 2; }
    HIP_OK(hipSetDevice(0));
    const int w = W / div, h = H / div;
    const size_t N = (size_t)W * H, n = (size_t)w * h;

    svgf_ctx *ctx = nullptr;
    SVGF_OKAY(svgf_create(0, w, h, &ctx));                          // the denoiser's state lives at the SMALL size
    float *rgb_lo, *ill_lo, *rgb_hi, *out_hi;
    void *gb_lo, *gb_hi, *pbo;
    HIP_OK(hipMalloc((void **)&rgb_lo, n * 12)); HIP_OK(hipMalloc((void **)&ill_lo, n * 12)); HIP_OK(hipMalloc(&gb_lo, n * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc((void **)&rgb_hi, N * 12)); HIP_OK(hipMalloc((void **)&out_hi, N * 12)); HIP_OK(hipMalloc(&gb_hi, N * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc(&pbo, 2 * N * 4));
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));

    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1;
    p.sepcolor = 1; p.addcolor = 0;                                 // illumination out: svgf_upsample multiplies the albedo back at full size
    const SvgfUpsampleParams up = { 0.5f, 0.5f, 1 };                // sigma_x in the scene's world units (the room is 10 units wide)
    SvgfGuide lo = { gb_lo, nullptr, nullptr, nullptr, nullptr }, hi = { gb_hi, nullptr, nullptr, nullptr, nullptr };

    const auto t0 = std::chrono::steady_clock::now();
    for (int f = 0; f < frames; f++) {
        SvgfCamera cam;
        SvgfSynthParams sp_lo = { f, 7, 0.6f, 0.02f, { 0.0f, 0.0f } }, sp_hi = sp_lo;
        SVGF_OKAY(svgf_synth_camera(f, /*moving=*/1, w, h, &cam, sp_lo.pixel_length));
        SVGF_OKAY(svgf_synth_camera(f, /*moving=*/1, W, H, &cam, sp_hi.pixel_length));      // one camera, two pixel sizes
        SVGF_OKAY(svgf_synth_render(0, rgb_lo, gb_lo, w, h, &cam, &sp_lo, s));
        SVGF_OKAY(svgf_synth_render(0, rgb_hi, gb_hi, W, H, &cam, &sp_hi, s));              // (its colour only feeds the left half of the display)
        SVGF_OKAY(svgf_denoise(ctx, ill_lo, rgb_lo, gb_lo, &cam, &p, s));
        SVGF_OKAY(svgf_upsample(0, out_hi, &hi, W, H, ill_lo, &lo, w, h, &up, s));
        SVGF_OKAY(svgf_display_pack(0, pbo, rgb_hi, out_hi, W, H, s));
    }
    SVGF_OKAY(svgf_sync_stream(ctx, s));
    const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / frames * 1e3;

    std::vector<float> host(3 * N);
    HIP_OK(hipMemcpy(host.data(), out_hi, 3 * N * sizeof(float), hipMemcpyDeviceToHost));
    double sum = 0.0;
    size_t bad = 0;
    for (float v : host) { if (v == v && v >= 0.0f && v < 1e6f) sum += v; else bad++; }
    printf("upsample: %dx%d denoised, %dx%d displayed, %d frames (producers + denoiser + upsample + pack): %.4f ms per frame; mean of the last image %.4f, %zu values out of range\n",
           w, h, W, H, frames, ms, sum / (3.0 * N), bad);
    svgf_destroy(ctx);
    (void)hipFree(rgb_lo); (void)hipFree(ill_lo); (void)hipFree(gb_lo); (void)hipFree(rgb_hi); (void)hipFree(out_hi); (void)hipFree(gb_hi); (void)hipFree(pbo);
    (void)hipStreamDestroy(s);
    return bad ? 1 : 0;
}
