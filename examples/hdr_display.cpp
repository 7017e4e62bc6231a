// examples/hdr_display.cpp — a renderer's loop with an emitter far above 1 and the HDR display side (include/svgf.h row f12), in
// C++ through the C ABI.
//
// Per frame, all on one stream:
//   * the PRODUCER (the path tracer's role; here svgf_scene_render on a small room: floor, three walls, ceiling, a sphere and a
//     hanging lamp of emittance 40) writes the 1-spp colour and the G-buffer;
//   * svgf_denoise;
//   * svgf_exposure_meter on the denoised image: luminance histogram, trimmed log-average, one step of the exposure towards
//     key / average (adapt = 1 - exp(-dt / tau), here dt = 1/60 s and tau = 0.25 s);
//   * svgf_display_tonemap with the metered exposure, the ACES fit and the sRGB transfer; and, for comparison, svgf_display_pack,
//     the reference's linear pack, which clips everything above 1.
// Each frame prints the exposure and the share of colour bytes at 255 in either buffer.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/hdr_display.cpp -L cuda-path-tracer-denoising_amd -lsvgf_hip \
//         -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/hdr_display
//   examples/hdr_display [frames=8] [width=1280] [height=720]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "svgf.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); return 1; } } while (0)
#define SVGF_OKAY(x) do { int rc__ = (x); if (rc__ != SVGF_OK) { fprintf(stderr, "%s failed (%d): %s\n", #x, rc__, svgf_last_error(ctx)); return 1; } } while (0)

// an axis-aligned primitive: scale, then translate (object -> world and back are diagonal + offset)
static SvgfSceneGeom box(int type, float cx, float cy, float cz, float sx, float sy, float sz, float r, float g, float b, float emit)
{
    SvgfSceneGeom q;
    memset(&q, 0, sizeof(q));
    q.type = type; q.albedo[0] = r; q.albedo[1] = g; q.albedo[2] = b; q.emittance = emit;
    const float s[3] = { sx, sy, sz }, c[3] = { cx, cy, cz };
    for (int i = 0; i < 3; i++) {
        q.xf[4 * i + i] = s[i];         q.xf[4 * i + 3] = c[i];
        q.inv[4 * i + i] = 1.0f / s[i]; q.inv[4 * i + 3] = -c[i] / s[i];
        q.invT[3 * i + i] = 1.0f / s[i];
    }
    return q;
}

static double share_at_255(const std::vector<unsigned char> &rgba)
{
    size_t hit = 0;
    for (size_t i = 0; i < rgba.size(); i += 4) hit += (rgba[i] == 255) + (rgba[i + 1] == 255) + (rgba[i + 2] == 255);
    return (double)hit / (double)(rgba.size() / 4 * 3);
}

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 8, W = argc > 2 ? atoi(argv[2]) : 1280, H = argc > 3 ? atoi(argv[3]) : 720;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "hdr_display: no HIP device (the library has no CPU path)\n"); return 2; }
    if (frames < 1 || W <= 0 || H <= 0) { fprintf(stderr, "usage: hdr_display [frames >= 1] [width] [height]\n"); return 2; }
    HIP_OK(hipSetDevice(0));
    const size_t N = (size_t)W * H;

    svgf_ctx *ctx = nullptr;
    SVGF_OKAY(svgf_create(0, W, H, &ctx));
    float *rgb, *out;
    void *gb, *pbo_plain, *pbo_mapped, *state;
    HIP_OK(hipMalloc((void **)&rgb, N * 12)); HIP_OK(hipMalloc((void **)&out, N * 12)); HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc(&pbo_plain, 2 * N * 4)); HIP_OK(hipMalloc(&pbo_mapped, N * 4));
    HIP_OK(hipMalloc(&state, SVGF_EXPOSURE_STATE_WORDS * 4));
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));

    const SvgfSceneGeom geoms[] = {
        // a room wider and taller than the camera's view of its open front (the camera stands at z = 10.5 and looks at y = 5)
        box(0, 0.0f, -2.0f, 0.0f, 24.0f, 0.02f, 12.0f, 0.8f, 0.8f, 0.8f, 0.0f),     // floor
        box(0, 0.0f, 12.0f, 0.0f, 24.0f, 0.02f, 12.0f, 0.8f, 0.8f, 0.8f, 0.0f),     // ceiling
        box(0, 0.0f, 5.0f, -6.0f, 24.0f, 14.0f, 0.02f, 0.8f, 0.8f, 0.8f, 0.0f),     // back wall
        box(0, -12.0f, 5.0f, 0.0f, 0.02f, 14.0f, 12.0f, 0.85f, 0.35f, 0.35f, 0.0f), // left wall
        box(0, 12.0f, 5.0f, 0.0f, 0.02f, 14.0f, 12.0f, 0.35f, 0.85f, 0.35f, 0.0f),  // right wall
        box(1, -2.0f, 0.0f, -1.0f, 4.0f, 4.0f, 4.0f, 0.9f, 0.9f, 0.9f, 0.0f),       // sphere
        box(0, 0.0f, 6.5f, -1.0f, 4.0f, 0.3f, 4.0f, 1.0f, 1.0f, 1.0f, 40.0f),       // a hanging lamp: 40 x what the display can show
    };
    const int n_geoms = (int)(sizeof(geoms) / sizeof(geoms[0]));
    const float light[3] = { 0.0f, 6.0f, -1.0f };                                   // the shading's point light, just below the lamp

    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1;
    const float dt = 1.0f / 60.0f, tau = 0.25f;
    // the trims: ray misses leave the cascade near-black but positive, so they are counted, in the lowest bin; the low trim has to
    // cover their share of the frame.  This room leaves almost none: 10 % is ample.
    const SvgfExposureParams ep = { 0.18f, 102, 51, 1.0f / 64.0f, 64.0f, 1.0f - expf(-dt / tau) };
    const SvgfTonemapParams tp = { /*op=*/2, /*transfer=*/2, /*exposure_bias=*/1.0f, /*white=*/0.0f };
    SVGF_OKAY(svgf_exposure_reset(0, state, s));

    std::vector<unsigned char> plain(2 * N * 4), mapped(N * 4), right(N * 4);
    unsigned words[SVGF_EXPOSURE_STATE_WORDS];
    for (int f = 0; f < frames; f++) {
        SvgfCamera cam;
        SvgfSynthParams sp = { f, 7, 0.6f, 0.02f, { 0.0f, 0.0f } };
        SVGF_OKAY(svgf_synth_camera(f, /*moving=*/1, W, H, &cam, sp.pixel_length));
        SVGF_OKAY(svgf_scene_render(0, rgb, gb, W, H, &cam, &sp, geoms, n_geoms, light, s));
        SVGF_OKAY(svgf_denoise(ctx, out, rgb, gb, &cam, &p, s));
        SVGF_OKAY(svgf_exposure_meter(0, state, out, W, H, &ep, s));
        SVGF_OKAY(svgf_display_tonemap(0, pbo_mapped, nullptr, out, W, H, &tp, state, s));
        SVGF_OKAY(svgf_display_pack(0, pbo_plain, rgb, out, W, H, s));
        // (a renderer hands the buffer to its display here; the example reads it back to count)
        SVGF_OKAY(svgf_sync_stream(ctx, s));
        HIP_OK(hipMemcpy(plain.data(), pbo_plain, plain.size(), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(mapped.data(), pbo_mapped, mapped.size(), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(words, state, sizeof(words), hipMemcpyDeviceToHost));
        for (int y = 0; y < H; y++) memcpy(&right[(size_t)y * W * 4], &plain[((size_t)y * 2 * W + W) * 4], (size_t)W * 4);      // the denoised half
        float target, exposure;
        memcpy(&target, &words[515], 4); memcpy(&exposure, &words[516], 4);
        printf("frame %2d: %u of %zu pixels counted, %u in the darkest bin, %u metered after the trims; exposure %.4f (target %.4f); "
               "bytes at 255: plain pack %.2f %%, tone-mapped %.2f %%\n",
               f, words[512], N, words[256], words[513], exposure, target, 100.0 * share_at_255(right), 100.0 * share_at_255(mapped));
    }
    svgf_destroy(ctx);
    (void)hipFree(rgb); (void)hipFree(out); (void)hipFree(gb); (void)hipFree(pbo_plain); (void)hipFree(pbo_mapped); (void)hipFree(state);
    (void)hipStreamDestroy(s);
    return 0;
}
