// examples/restir_gi/restir_gi_scene.cpp — the whole resampled pipeline on the room of examples/traced_scene.cpp: the direct term D by
// row f27 (include/svgf_restir.h), the indirect term I by row f28 (include/svgf_restir_gi.h), one svgf_denoise context each, then
// svgf_trace_compose.  C++ through the C ABI of four libraries: libsvgf_hip.so (scene, pose, denoiser, quality meter),
// libsvgf_restir.so, libsvgf_restir_gi.so and libsvgf_split.so (svgf_trace_compose, and svgf_trace_draw_split for the truth).
//
// Per frame, on one stream: svgf_scene_pose, svgf_scene_draw for the G-buffer, svgf_motion_reproject with the pose's motion rows for
// the previous-coordinate plane, ONE svgf_restir_frame (a table of one light: the scene's own 3 x 3 light at power 30, so D is the
// split draw's direct term with a resampled light point), and the indirect term I drawn four ways, each with a state of its own:
//   1 sample     candidates = 1, no reuse: svgf_trace_draw_split's I at bounce_samples = 1 on bits
//   8 cand.      candidates = 8, no reuse
//   reuse        candidates = 1, the history tap and 3 neighbours within 30 pixels, jacobian_max 10
//   4 + reuse    candidates = 4, the same reuse
// Each I goes through one svgf_denoise context (sepcolor = 1, addcolor = 0) and svgf_trace_compose with the denoised D.
// svgf_quality_meter scores I and the composed frame, noisy and denoised, against a truth: the mean of svgf_trace_draw_split's D and I
// at 8 bounce samples and 64 shadow rays over `seeds` = 16 frame seeds.  That is 128 bounce samples per pixel: the truth's own standard
// error is 1 / sqrt(128) = 0.088 of the one-sample error, below a tenth.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/restir_gi/restir_gi_scene.cpp -L cuda-path-tracer-denoising_amd -lsvgf_restir_gi \
//         -lsvgf_restir -lsvgf_split -lsvgf_hip -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/restir_gi/restir_gi_scene
//   examples/restir_gi/restir_gi_scene [frames=8] [width=640] [height=360] [moving=1] [seeds=16]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svgf_restir.h"
#include "svgf_restir_gi.h"
#include "svgf_split.h"

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
    const int moving = argc > 4 ? atoi(argv[4]) : 1, seeds = argc > 5 ? atoi(argv[5]) : 16;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "restir_gi_scene: no HIP device (the libraries have no CPU path)\n"); return 2; }
    const unsigned long long state_bytes = frames >= 1 && seeds >= 1 ? svgf_quality_state_bytes(W, H) : 0;
    if (state_bytes == 0) { fprintf(stderr, "usage: restir_gi_scene [frames >= 1] [width] [height] [moving 0/1] [seeds >= 1]\n"); return 2; }
    if (svgf_restir_gi_version() != svgf_version() || svgf_restir_version() != svgf_version()) {
        fprintf(stderr, "restir_gi_scene: the resamplers and libsvgf_hip.so disagree on the ABI\n");
        return 2;
    }
    HIP_OK(hipSetDevice(0));

    const int BLOCK = 5, N_OBJECTS = 6, N_WAYS = 4;
    const float block_at[3] = { -2.5f, 1.1f, 0.0f }, ambient = 0.15f;
    const std::vector<SvgfSceneGeom> geoms = { box(0, 0, 0, 12, 0.2f, 12, 0.8f, 0.8f, 0.8f, 0), box(0, 5, -6, 12, 10, 0.2f, 0.8f, 0.8f, 0.7f, 0),
                                               box(-6, 5, 0, 0.2f, 10, 12, 0.8f, 0.3f, 0.3f, 0), box(6, 5, 0, 0.2f, 10, 12, 0.3f, 0.8f, 0.3f, 0),
                                               box(0, 9.9f, 0, 3, 0.1f, 3, 1, 1, 1, 5),
                                               box(block_at[0], block_at[1], block_at[2], 2, 2, 2, 0.3f, 0.4f, 0.9f, 0) };
    SvgfSceneLight light = { { 0.0f, 9.5f, 0.0f }, { 1.5f, 0.0f, 0.0f }, { 0.0f, 0.0f, 1.5f }, 1 }, light_ref = light;
    light_ref.samples = SVGF_SCENE_MAX_SHADOW_SAMPLES;
    const SvgfLight lamp = { { 0.0f, 9.5f, 0.0f }, { 1.5f, 0.0f, 0.0f }, { 0.0f, 0.0f, 1.5f }, { 30.0f, 30.0f, 30.0f } };
    const SvgfTraceParams tp_ref = { SVGF_TRACE_MAX_BOUNCE_SAMPLES, ambient, 1 };
    const SvgfRestirParams rp = { 1, 1, 20.0f, 3, 30.0f, 0.9f };
    const SvgfRestirGIParams ways[N_WAYS] = { { 1, 0, 20.0f, 0, 30.0f, 0.9f, 10.0f, ambient, 1 }, { 8, 0, 20.0f, 0, 30.0f, 0.9f, 10.0f, ambient, 1 },
                                              { 1, 1, 20.0f, 3, 30.0f, 0.9f, 10.0f, ambient, 1 }, { 4, 1, 20.0f, 3, 30.0f, 0.9f, 10.0f, ambient, 1 } };
    const char *way_name[N_WAYS] = { "1 sample", "8 cand.", "reuse", "4 + reuse" };

    svgf_scene *scene = nullptr;
    svgf_lights *table = nullptr;
    svgf_restir *direct_state = nullptr;
    svgf_restir_gi *state[N_WAYS] = { nullptr, nullptr, nullptr, nullptr };
    svgf_ctx *ctx_d = nullptr, *ctx[N_WAYS] = { nullptr, nullptr, nullptr, nullptr };
    SVGF_OKAY(svgf_scene_create(0, geoms.data(), (int)geoms.size(), nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &scene));
    SVGF_OKAY(svgf_scene_enable_pose(scene, N_OBJECTS));
    SVGF_OKAY(svgf_lights_create(0, &lamp, 1, &table));
    SVGF_OKAY(svgf_restir_create(scene, W, H, &direct_state));
    const size_t N = (size_t)W * H;
    float *rgb, *D, *out_d, *I[N_WAYS], *out_i[N_WAYS], *img, *ref_d, *ref_i, *ref, *motion, *coord;
    void *gb, *gb_ref, *q;
    SvgfScenePose *pose_dev, *pose_host;
    HIP_OK(hipMalloc((void **)&rgb, N * 12)); HIP_OK(hipMalloc((void **)&D, N * 12)); HIP_OK(hipMalloc((void **)&out_d, N * 12));
    HIP_OK(hipMalloc((void **)&img, N * 12)); HIP_OK(hipMalloc((void **)&ref_d, N * 12)); HIP_OK(hipMalloc((void **)&ref_i, N * 12));
    HIP_OK(hipMalloc((void **)&ref, N * 12));
    HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel))); HIP_OK(hipMalloc(&gb_ref, N * sizeof(SvgfGBufferTexel))); HIP_OK(hipMalloc((void **)&coord, N * 8));
    HIP_OK(hipMalloc((void **)&motion, sizeof(float) * 12 * N_OBJECTS)); HIP_OK(hipMalloc(&q, state_bytes));
    HIP_OK(hipMalloc((void **)&pose_dev, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames));
    HIP_OK(hipHostMalloc((void **)&pose_host, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames, hipHostMallocDefault));
    SVGF_OKAY(svgf_create(0, W, H, &ctx_d));
    SVGF_OKAY(svgf_set_object_motion(ctx_d, motion, N_OBJECTS));
    for (int k = 0; k < N_WAYS; k++) {
        SVGF_OKAY(svgf_restir_gi_create(scene, W, H, &state[k]));
        SVGF_OKAY(svgf_create(0, W, H, &ctx[k]));
        SVGF_OKAY(svgf_set_object_motion(ctx[k], motion, N_OBJECTS));
        HIP_OK(hipMalloc((void **)&I[k], N * 12)); HIP_OK(hipMalloc((void **)&out_i[k], N * 12));
    }
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1;
    p.sepcolor = 1; p.addcolor = 0;                                 // a demodulated term in, the filtered term out: the caller modulates
    const SvgfGuide guide = { gb, nullptr, nullptr, nullptr, nullptr };
    SvgfCamera cam;
    float pixel_length[2];
    SVGF_OKAY(svgf_synth_camera(0, /*moving=*/0, W, H, &cam, pixel_length));
    p.reproj_scale[0] = pixel_length[0] * (float)W / 2.0f; p.reproj_scale[1] = pixel_length[1] * (float)H / 2.0f;
    const SvgfQualityParams qp = { 1.0f, 1.0f, 0 };
    const float y_axis[3] = { 0, 1, 0 }, zero[3] = { 0, 0, 0 }, PI = 3.14159265f;
    std::vector<float> h_d(3 * N), h_i(3 * N);
    std::vector<double> sum_d(3 * N), sum_i(3 * N);

    printf("%d frames of %dx%d, the block %s; D by svgf_restir_frame, I by svgf_restir_gi_frame, against the mean of %d draws of "
           "svgf_trace_draw_split at %d bounce samples and %d shadow rays (%d bounce samples per pixel)\n", frames, W, H,
           moving ? "turning and sliding" : "at rest", seeds, tp_ref.bounce_samples, light_ref.samples, seeds * tp_ref.bounce_samples);
    for (int f = 0; f < frames; f++) {
        SvgfScenePose *pose = pose_host + (size_t)f * N_OBJECTS;
        for (int k = 0; k < N_OBJECTS; k++) SVGF_OKAY(svgf_pose_rigid(y_axis, 0.0f, zero, zero, &pose[k]));
        const float slide[3] = { moving ? 0.25f * (float)f : 0.0f, 0, 0 };
        SVGF_OKAY(svgf_pose_rigid(y_axis, moving ? 9.0f * PI / 180.0f * (float)f : 0.0f, block_at, slide, &pose[BLOCK]));
        HIP_OK(hipMemcpyAsync(pose_dev + (size_t)f * N_OBJECTS, pose, sizeof(SvgfScenePose) * N_OBJECTS, hipMemcpyHostToDevice, s));
        const SvgfSynthParams sp = { f, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
        SVGF_OKAY(svgf_scene_pose(scene, pose_dev + (size_t)f * N_OBJECTS, N_OBJECTS, motion, s));
        SVGF_OKAY(svgf_scene_draw(scene, rgb, gb, W, H, &cam, &sp, light.centre, s));           // the G-buffer; its colour is not used
        SVGF_OKAY(svgf_motion_reproject(0, coord, SVGF_MOTION_PREV_COORD_F32, gb, nullptr, nullptr, W, H, &cam, p.reproj_scale, motion, N_OBJECTS, s));
        SVGF_OKAY(svgf_restir_frame(direct_state, table, gb, nullptr, coord, &rp, &sp, ambient, D, s));
        SVGF_OKAY(svgf_denoise(ctx_d, out_d, D, gb, &cam, &p, s));
        for (int k = 0; k < N_WAYS; k++) {
            SVGF_OKAY(svgf_restir_gi_frame(state[k], &light, gb, nullptr, coord, &ways[k], &sp, I[k], s));
            SVGF_OKAY(svgf_denoise(ctx[k], out_i[k], I[k], gb, &cam, &p, s));
        }
        if (f != 0 && f != 1 && f != 3 && f != 7 && f != frames - 1) continue;
        // the truth: the same pose under `seeds` other frame seeds, D and I averaged in double on the host
        for (size_t i = 0; i < 3 * N; i++) { sum_d[i] = 0.0; sum_i[i] = 0.0; }
        for (int k = 0; k < seeds; k++) {
            const SvgfSynthParams sp_ref = { 1000 + f * seeds + k, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
            SVGF_OKAY(svgf_trace_draw_split(scene, ref_d, ref_i, nullptr, gb_ref, nullptr, W, H, &cam, &sp_ref, &light_ref, &tp_ref, s));
            HIP_OK(hipMemcpyAsync(h_d.data(), ref_d, N * 12, hipMemcpyDeviceToHost, s));
            HIP_OK(hipMemcpyAsync(h_i.data(), ref_i, N * 12, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            for (size_t i = 0; i < 3 * N; i++) { sum_d[i] += h_d[i]; sum_i[i] += h_i[i]; }
        }
        for (size_t i = 0; i < 3 * N; i++) { h_d[i] = (float)(sum_d[i] / seeds); h_i[i] = (float)(sum_i[i] / seeds); }
        HIP_OK(hipMemcpyAsync(ref_d, h_d.data(), N * 12, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(ref_i, h_i.data(), N * 12, hipMemcpyHostToDevice, s));
        SVGF_OKAY(svgf_trace_compose(0, ref, ref_d, ref_i, &guide, W, H, s));
        printf("frame %2d:\n", f);
        for (int k = 0; k < N_WAYS; k++) {
            // I noisy, I denoised, the composed frame noisy, the composed frame denoised
            SvgfQualityResult r[4];
            for (int i = 0; i < 4; i++) {
                const float *scored = i == 0 ? I[k] : i == 1 ? out_i[k] : img;
                if (i >= 2) SVGF_OKAY(svgf_trace_compose(0, img, i == 2 ? D : out_d, i == 2 ? I[k] : out_i[k], &guide, W, H, s));
                SVGF_OKAY(svgf_quality_meter(0, q, scored, i < 2 ? ref_i : ref, W, H, &qp, nullptr, nullptr, nullptr, s));
                SVGF_OKAY(svgf_quality_read(0, q, &r[i], s));
            }
            printf("   %-9s I noisy %6.2f dB / SSIM %.4f, denoised %6.2f dB / %.4f;   composed noisy %6.2f dB / %.4f, denoised %6.2f dB / %.4f\n", way_name[k],
                   r[0].psnr_db, r[0].mean_ssim, r[1].psnr_db, r[1].mean_ssim, r[2].psnr_db, r[2].mean_ssim, r[3].psnr_db, r[3].mean_ssim);
        }
    }

    HIP_OK(hipStreamSynchronize(s));
    for (int k = 0; k < N_WAYS; k++) { svgf_restir_gi_destroy(state[k]); svgf_destroy(ctx[k]); (void)hipFree(I[k]); (void)hipFree(out_i[k]); }
    svgf_restir_destroy(direct_state); svgf_destroy(ctx_d);
    svgf_lights_destroy(table);
    SVGF_OKAY(svgf_scene_destroy(scene));
    (void)hipFree(rgb); (void)hipFree(D); (void)hipFree(out_d); (void)hipFree(img); (void)hipFree(ref_d); (void)hipFree(ref_i); (void)hipFree(ref);
    (void)hipFree(gb); (void)hipFree(gb_ref); (void)hipFree(coord); (void)hipFree(motion); (void)hipFree(q);
    (void)hipFree(pose_dev); (void)hipHostFree(pose_host); (void)hipStreamDestroy(s);
    return 0;
}
