// examples/shadowed_scene.cpp — stochastic soft shadows on the animated resident scene (include/svgf.h row f16), in C++ through the C ABI.
//
// The room of examples/animated_scene.cpp without its sphere: four cubes, the light's emitting slab under the ceiling and the block,
// which turns 9 degrees about y and slides in x per frame.  The light is the slab's lower face as a parallelogram.  noise = 0, so the
// one-sample visibility estimate is the ONLY noise.  Per frame, on one stream: svgf_scene_pose with a motion table, a 1-sample
// svgf_scene_draw_shadowed, svgf_denoise in two contexts (history clamp off / on, both with the motion table), and a 64-sample draw as
// the reference.  Printed per frame: svgf_quality_meter's PSNR / SSIM against the reference of the noisy frame, the denoised one and
// the denoised one with the clamp; and the flicker - the mean squared difference of consecutive outputs - over the whole frame and
// inside the moving shadow (the pixels on which two consecutive references differ).
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/shadowed_scene.cpp -L cuda-path-tracer-denoising_amd -lsvgf_hip \
//         -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/shadowed_scene
//   examples/shadowed_scene [frames=8] [width=640] [height=360] [moving=1]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "svgf.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); return 1; } } while (0)
#define SVGF_OKAY(x) do { int rc__ = (x); if (rc__ != SVGF_OK) { fprintf(stderr, "%s failed (%d)\n", #x, rc__); return 1; } } while (0)

// an axis-aligned cube: centre t, edge lengths s
static SvgfSceneGeom box(float tx, float ty, float tz, float sx, float sy, float sz, float r, float g, float b, float emit)
{
    SvgfSceneGeom q = {};
    const float t[3] = { tx, ty, tz }, s[3] = { sx, sy, sz };
    q.type = 0; q.albedo[0] = r; q.albedo[1] = g; q.albedo[2] = b; q.emittance = emit;
    for (int k = 0; k < 3; k++) {
        q.xf[4 * k + k] = s[k]; q.xf[4 * k + 3] = t[k];
        q.inv[4 * k + k] = 1.0f / s[k]; q.inv[4 * k + 3] = -t[k] / s[k];
        q.invT[3 * k + k] = 1.0f / s[k];
    }
    return q;
}

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 8, W = argc > 2 ? atoi(argv[2]) : 640, H = argc > 3 ? atoi(argv[3]) : 360;
    const int moving = argc > 4 ? atoi(argv[4]) : 1;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "shadowed_scene: no HIP device (the library has no CPU path)\n"); return 2; }
    const unsigned long long state_bytes = frames >= 2 ? svgf_quality_state_bytes(W, H) : 0;
    if (state_bytes == 0) { fprintf(stderr, "usage: shadowed_scene [frames >= 2] [width] [height] [moving 0/1]\n"); return 2; }
    HIP_OK(hipSetDevice(0));

    const int BLOCK = 5, N_OBJECTS = 6;
    const float block_at[3] = { -2.5f, 1.1f, 0.0f };
    const std::vector<SvgfSceneGeom> geoms = { box(0, 0, 0, 12, 0.2f, 12, 0.8f, 0.8f, 0.8f, 0), box(0, 5, -6, 12, 10, 0.2f, 0.8f, 0.8f, 0.7f, 0),
                                               box(-6, 5, 0, 0.2f, 10, 12, 0.8f, 0.3f, 0.3f, 0), box(6, 5, 0, 0.2f, 10, 12, 0.3f, 0.8f, 0.3f, 0),
                                               box(0, 9.9f, 0, 3, 0.1f, 3, 1, 1, 1, 5),
                                               box(block_at[0], block_at[1], block_at[2], 2, 2, 2, 0.3f, 0.4f, 0.9f, 0) };
    SvgfSceneLight light = { { 0.0f, 9.5f, 0.0f }, { 1.5f, 0.0f, 0.0f }, { 0.0f, 0.0f, 1.5f }, 1 }, light_ref = light;
    light_ref.samples = SVGF_SCENE_MAX_SHADOW_SAMPLES;

    svgf_scene *scene = nullptr;
    SVGF_OKAY(svgf_scene_create(0, geoms.data(), (int)geoms.size(), nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &scene));
    SVGF_OKAY(svgf_scene_enable_pose(scene, N_OBJECTS));
    svgf_ctx *ctx[2] = { nullptr, nullptr };        // 0: history clamp off; 1: on
    const size_t N = (size_t)W * H;
    float *noisy, *ref, *ref_prev, *out[2], *prev[2], *motion, *se_map;
    void *gb, *gb_ref, *q;
    SvgfScenePose *pose_dev, *pose_host;
    HIP_OK(hipMalloc((void **)&noisy, N * 12)); HIP_OK(hipMalloc((void **)&ref, N * 12)); HIP_OK(hipMalloc((void **)&ref_prev, N * 12));
    HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel))); HIP_OK(hipMalloc(&gb_ref, N * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc((void **)&motion, sizeof(float) * 12 * N_OBJECTS)); HIP_OK(hipMalloc((void **)&se_map, N * 4)); HIP_OK(hipMalloc(&q, state_bytes));
    HIP_OK(hipMalloc((void **)&pose_dev, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames));
    HIP_OK(hipHostMalloc((void **)&pose_host, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames, hipHostMallocDefault));
    for (int k = 0; k < 2; k++) {
        SVGF_OKAY(svgf_create(0, W, H, &ctx[k]));
        HIP_OK(hipMalloc((void **)&out[k], N * 12)); HIP_OK(hipMalloc((void **)&prev[k], N * 12));
        SVGF_OKAY(svgf_set_object_motion(ctx[k], motion, N_OBJECTS));
    }
    SVGF_OKAY(svgf_set_history_clamp(ctx[1], 1, 1.5f));
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1;
    SvgfCamera cam;
    float pixel_length[2];
    SVGF_OKAY(svgf_synth_camera(0, /*moving=*/0, W, H, &cam, pixel_length));
    p.reproj_scale[0] = pixel_length[0] * (float)W / 2.0f; p.reproj_scale[1] = pixel_length[1] * (float)H / 2.0f;
    const SvgfQualityParams qp = { 1.0f, 1.0f, 0 };
    const float y_axis[3] = { 0, 1, 0 }, zero[3] = { 0, 0, 0 }, PI = 3.14159265f;
    std::vector<float> h_ref(3 * N), h_ref_prev(3 * N), h_se(N);

    printf("%d frames of %dx%d, the block %s; 1 shadow ray per pixel against a %d-ray reference; clamp radius 1, 1.5 sigma\n", frames, W, H,
           moving ? "turning and sliding" : "at rest", light_ref.samples);
    for (int f = 0; f < frames; f++) {
        SvgfScenePose *table = pose_host + (size_t)f * N_OBJECTS;
        for (int k = 0; k < N_OBJECTS; k++) SVGF_OKAY(svgf_pose_rigid(y_axis, 0.0f, zero, zero, &table[k]));
        const float slide[3] = { moving ? 0.25f * (float)f : 0.0f, 0, 0 };
        SVGF_OKAY(svgf_pose_rigid(y_axis, moving ? 9.0f * PI / 180.0f * (float)f : 0.0f, block_at, slide, &table[BLOCK]));
        HIP_OK(hipMemcpyAsync(pose_dev + (size_t)f * N_OBJECTS, table, sizeof(SvgfScenePose) * N_OBJECTS, hipMemcpyHostToDevice, s));
        const SvgfSynthParams sp = { f, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
        std::swap(ref, ref_prev); std::swap(h_ref, h_ref_prev);
        SVGF_OKAY(svgf_scene_pose(scene, pose_dev + (size_t)f * N_OBJECTS, N_OBJECTS, motion, s));
        SVGF_OKAY(svgf_scene_draw_shadowed(scene, noisy, gb, nullptr, W, H, &cam, &sp, &light, s));
        SVGF_OKAY(svgf_scene_draw_shadowed(scene, ref, gb_ref, nullptr, W, H, &cam, &sp, &light_ref, s));
        SvgfQualityResult r[3];
        SVGF_OKAY(svgf_quality_meter(0, q, noisy, ref, W, H, &qp, nullptr, nullptr, nullptr, s));
        SVGF_OKAY(svgf_quality_read(0, q, &r[0], s));
        HIP_OK(hipMemcpyAsync(h_ref.data(), ref, N * 12, hipMemcpyDeviceToHost, s));
        double flicker[2][2] = { { 0, 0 }, { 0, 0 } };       // [context][whole frame, moving shadow]
        size_t n_shadow = 0;
        for (int k = 0; k < 2; k++) {
            std::swap(out[k], prev[k]);
            SVGF_OKAY(svgf_denoise(ctx[k], out[k], noisy, gb, &cam, &p, s));
            SVGF_OKAY(svgf_quality_meter(0, q, out[k], ref, W, H, &qp, nullptr, nullptr, nullptr, s));
            SVGF_OKAY(svgf_quality_read(0, q, &r[1 + k], s));
            if (f == 0) continue;
            SvgfQualityResult rf;
            SVGF_OKAY(svgf_quality_meter(0, q, out[k], prev[k], W, H, &qp, nullptr, se_map, nullptr, s));
            SVGF_OKAY(svgf_quality_read(0, q, &rf, s));
            HIP_OK(hipMemcpyAsync(h_se.data(), se_map, N * 4, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            flicker[k][0] = rf.mse;
            double sum = 0.0;
            n_shadow = 0;
            for (size_t i = 0; i < N; i++) {
                float d = 0.0f;
                for (int c = 0; c < 3; c++) d = fmaxf(d, fabsf(h_ref[3 * i + c] - h_ref_prev[3 * i + c]));
                if (d > 0.01f && std::isfinite(h_se[i])) { sum += h_se[i]; n_shadow++; }
            }
            flicker[k][1] = n_shadow ? sum / (3.0 * (double)n_shadow) : 0.0;
        }
        printf("frame %2d: noisy %6.2f dB / SSIM %.4f   denoised %6.2f dB / %.4f   with the clamp %6.2f dB / %.4f", f, r[0].psnr_db, r[0].mean_ssim,
               r[1].psnr_db, r[1].mean_ssim, r[2].psnr_db, r[2].mean_ssim);
        if (f > 0) printf("   flicker (mse x 1e4) whole frame %.3f / %.3f, moving shadow (%zu px) %.3f / %.3f", 1e4 * flicker[0][0], 1e4 * flicker[1][0],
                          n_shadow, 1e4 * flicker[0][1], 1e4 * flicker[1][1]);
        printf("\n");
    }

    HIP_OK(hipStreamSynchronize(s));
    SVGF_OKAY(svgf_scene_destroy(scene));
    for (int k = 0; k < 2; k++) { svgf_destroy(ctx[k]); (void)hipFree(out[k]); (void)hipFree(prev[k]); }
    (void)hipFree(noisy); (void)hipFree(ref); (void)hipFree(ref_prev); (void)hipFree(gb); (void)hipFree(gb_ref); (void)hipFree(motion);
    (void)hipFree(se_map); (void)hipFree(q); (void)hipFree(pose_dev); (void)hipHostFree(pose_host); (void)hipStreamDestroy(s);
    return 0;
}
