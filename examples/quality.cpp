// examples/quality.cpp — scoring a denoiser setting on the device with the image-quality meter (include/svgf.h row f13), in C++
// through the C ABI.
//
// Per frame, all on one stream:
//   * the PRODUCER (svgf_synth_render, the synthetic static scene) writes the 1-spp frame, and once more with noise = 0 and
//     fireflies = 0: the clean frame, the reference a renderer gets from a converged render of the same view;
//   * svgf_denoise with temporal + spatial on;
//   * svgf_quality_meter three times: noisy against clean, denoised against clean, and this output against the previous one (the
//     flicker figure: on a static view everything it sees is the denoiser's own frame-to-frame change);
//   * svgf_quality_read of the three 64-byte blocks.
// The last frame is also scored the way a display shows it: svgf_exposure_meter on the clean frame, then the meter with that state,
// peak 1 and clamp = 1.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/quality.cpp -L cuda-path-tracer-denoising_amd -lsvgf_hip \
//         -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/quality
//   examples/quality [frames=8] [width=1280] [height=720]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <utility>

#include "svgf.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); return 1; } } while (0)
#define SVGF_OKAY(x) do { int rc__ = (x); if (rc__ != SVGF_OK) { fprintf(stderr, "%s failed (%d): %s\n", #x, rc__, svgf_last_error(ctx)); return 1; } } while (0)

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 8, W = argc > 2 ? atoi(argv[2]) : 1280, H = argc > 3 ? atoi(argv[3]) : 720;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "quality: no HIP device (the library has no CPU path)\n"); return 2; }
    const unsigned long long state_bytes = frames >= 1 ? svgf_quality_state_bytes(W, H) : 0;
    if (state_bytes == 0) { fprintf(stderr, "usage: quality [frames >= 1] [width] [height]\n"); return 2; }
    HIP_OK(hipSetDevice(0));
    const size_t N = (size_t)W * H;

    svgf_ctx *ctx = nullptr;
    SVGF_OKAY(svgf_create(0, W, H, &ctx));
    float *noisy, *clean, *out, *prev;
    void *gb, *gb_clean, *q_noisy, *q_out, *q_flicker, *exposure;
    HIP_OK(hipMalloc((void **)&noisy, N * 12)); HIP_OK(hipMalloc((void **)&clean, N * 12));
    HIP_OK(hipMalloc((void **)&out, N * 12)); HIP_OK(hipMalloc((void **)&prev, N * 12));
    HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel))); HIP_OK(hipMalloc(&gb_clean, N * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc(&q_noisy, state_bytes)); HIP_OK(hipMalloc(&q_out, state_bytes)); HIP_OK(hipMalloc(&q_flicker, state_bytes));      // never initialised
    HIP_OK(hipMalloc(&exposure, SVGF_EXPOSURE_STATE_WORDS * 4));
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));

    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1;
    const SvgfQualityParams scene_referred = { /*peak=*/1.0f, /*scale=*/1.0f, /*clamp=*/0 };
    int nwx = 0, nwy = 0;
    SVGF_OKAY(svgf_quality_windows(W, H, &nwx, &nwy));
    printf("%d x %d, %d x %d windows, %llu bytes of state per comparison\n", W, H, nwx, nwy, state_bytes);

    SvgfQualityResult rn, ro, rf;
    for (int f = 0; f < frames; f++) {
        SvgfCamera cam;
        SvgfSynthParams sp = { f, 7, 0.6f, 0.02f, { 0.0f, 0.0f } }, sp_clean = sp;
        sp_clean.noise = 0.0f; sp_clean.fireflies = 0.0f;
        SVGF_OKAY(svgf_synth_camera(f, /*moving=*/0, W, H, &cam, sp.pixel_length));
        sp_clean.pixel_length[0] = sp.pixel_length[0]; sp_clean.pixel_length[1] = sp.pixel_length[1];
        std::swap(out, prev);
        SVGF_OKAY(svgf_synth_render(0, noisy, gb, W, H, &cam, &sp, s));
        SVGF_OKAY(svgf_synth_render(0, clean, gb_clean, W, H, &cam, &sp_clean, s));
        SVGF_OKAY(svgf_denoise(ctx, out, noisy, gb, &cam, &p, s));
        SVGF_OKAY(svgf_quality_meter(0, q_noisy, noisy, clean, W, H, &scene_referred, nullptr, nullptr, nullptr, s));
        SVGF_OKAY(svgf_quality_meter(0, q_out, out, clean, W, H, &scene_referred, nullptr, nullptr, nullptr, s));
        if (f > 0) SVGF_OKAY(svgf_quality_meter(0, q_flicker, out, prev, W, H, &scene_referred, nullptr, nullptr, nullptr, s));
        SVGF_OKAY(svgf_quality_read(0, q_noisy, &rn, s));
        SVGF_OKAY(svgf_quality_read(0, q_out, &ro, s));
        printf("frame %2d: noisy %6.2f dB / SSIM %.4f   denoised %6.2f dB / SSIM %.4f", f, rn.psnr_db, rn.mean_ssim, ro.psnr_db, ro.mean_ssim);
        if (f > 0) {
            SVGF_OKAY(svgf_quality_read(0, q_flicker, &rf, s));
            printf("   against the previous output %6.2f dB / SSIM %.4f (worst window %.4f)\n", rf.psnr_db, rf.mean_ssim, rf.min_ssim);
        } else {
            printf("   (no previous output)\n");
        }
    }
    // the last frame as a display shows it: the clean frame's metered exposure, white at 1, channels clamped to [0, 1]
    const SvgfExposureParams ep = { 0.18f, 614, 51, 1.0f / 64.0f, 64.0f, 1.0f };      // low trim: the ray misses' share
    const SvgfQualityParams display_referred = { 1.0f, 1.0f, 1 };
    SVGF_OKAY(svgf_exposure_reset(0, exposure, s));
    SVGF_OKAY(svgf_exposure_meter(0, exposure, clean, W, H, &ep, s));
    SVGF_OKAY(svgf_quality_meter(0, q_noisy, noisy, clean, W, H, &display_referred, exposure, nullptr, nullptr, s));
    SVGF_OKAY(svgf_quality_meter(0, q_out, out, clean, W, H, &display_referred, exposure, nullptr, nullptr, s));
    SVGF_OKAY(svgf_quality_read(0, q_noisy, &rn, s));
    SVGF_OKAY(svgf_quality_read(0, q_out, &ro, s));
    printf("last frame at the metered exposure %.4f, clamped to [0, 1]: noisy %6.2f dB / SSIM %.4f   denoised %6.2f dB / SSIM %.4f\n",
           ro.scale, rn.psnr_db, rn.mean_ssim, ro.psnr_db, ro.mean_ssim);

    svgf_destroy(ctx);
    (void)hipFree(noisy); (void)hipFree(clean); (void)hipFree(out); (void)hipFree(prev); (void)hipFree(gb); (void)hipFree(gb_clean);
    (void)hipFree(q_noisy); (void)hipFree(q_out); (void)hipFree(q_flicker); (void)hipFree(exposure);
    (void)hipStreamDestroy(s);
    return 0;
}
