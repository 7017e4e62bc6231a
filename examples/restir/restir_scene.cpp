// examples/restir/restir_scene.cpp — a room under 64 small lamps at ONE shadow ray per pixel (include/svgf_restir.h, row f27), in C++
// through the C ABI of three libraries: libsvgf_hip.so (scene, pose, denoiser, quality meter), libsvgf_restir.so (the light table,
// svgf_restir_frame, svgf_lights_draw_all) and libsvgf_split.so (svgf_trace_compose).
//
// The scene is the turning block's room of examples/split_scene.cpp; the lamps are an 8 x 8 grid of small parallelogram lights under
// where its ceiling would be.  Per frame, on one stream: svgf_scene_pose, svgf_scene_draw for the G-buffer, svgf_motion_reproject
// with the pose's motion rows for the previous-coordinate plane, and the direct term D drawn three ways, each with a state of its own:
//   uniform     candidates = 1, no reuse: a uniformly chosen lamp
//   32 cand.    candidates = 32, no reuse
//   full reuse  candidates = 8, the history tap and 3 neighbours within 30 pixels
// Each D goes through one svgf_denoise context (sepcolor = 1, addcolor = 0) and svgf_trace_compose with a zero indirect term, and
// svgf_quality_meter scores the noisy and the denoised image against svgf_lights_draw_all with 64 samples per lamp, composed alike.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/restir/restir_scene.cpp -L cuda-path-tracer-denoising_amd -lsvgf_restir \
//         -lsvgf_split -lsvgf_hip -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/restir/restir_scene
//   examples/restir/restir_scene [frames=8] [width=640] [height=360] [moving=1]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svgf_restir.h"
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
    const int moving = argc > 4 ? atoi(argv[4]) : 1;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "restir_scene: no HIP device (the libraries have no CPU path)\n"); return 2; }
    const unsigned long long state_bytes = frames >= 1 ? svgf_quality_state_bytes(W, H) : 0;
    if (state_bytes == 0) { fprintf(stderr, "usage: restir_scene [frames >= 1] [width] [height] [moving 0/1]\n"); return 2; }
    if (svgf_restir_version() != svgf_version()) { fprintf(stderr, "restir_scene: libsvgf_restir.so and libsvgf_hip.so disagree on the ABI\n"); return 2; }
    HIP_OK(hipSetDevice(0));

    const int BLOCK = 5, N_OBJECTS = 6, N_WAYS = 3, N_LAMPS = 64;
    const float block_at[3] = { -2.5f, 1.1f, 0.0f }, ambient = 0.15f;
    const std::vector<SvgfSceneGeom> geoms = { box(0, 0, 0, 12, 0.2f, 12, 0.8f, 0.8f, 0.8f, 0), box(0, 5, -6, 12, 10, 0.2f, 0.8f, 0.8f, 0.7f, 0),
                                               box(-6, 5, 0, 0.2f, 10, 12, 0.8f, 0.3f, 0.3f, 0), box(6, 5, 0, 0.2f, 10, 12, 0.3f, 0.8f, 0.3f, 0),
                                               box(0, 9.9f, 0, 3, 0.1f, 3, 1, 1, 1, 5),
                                               box(block_at[0], block_at[1], block_at[2], 2, 2, 2, 0.3f, 0.4f, 0.9f, 0) };
    std::vector<SvgfLight> lamps(N_LAMPS);
    for (int k = 0; k < N_LAMPS; k++) {             // an 8 x 8 grid at y = 6, warm and cool lamps in a chequerboard, a few of them strong
        const int i = k % 8, j = k / 8;
        const float strong = (k % 11 == 0) ? 6.0f : 1.0f, warm = ((i + j) & 1) ? 1.0f : 0.6f;
        lamps[k] = SvgfLight{ { -4.9f + 1.4f * (float)i, 6.0f, -4.9f + 1.4f * (float)j }, { 0.15f, 0, 0 }, { 0, 0, 0.15f },
                              { 1.5f * strong, 1.5f * strong * (0.7f + 0.3f * warm), 1.5f * strong * warm } };
    }
    const SvgfRestirParams ways[N_WAYS] = { { 1, 0, 20.0f, 0, 30.0f, 0.9f }, { 32, 0, 20.0f, 0, 30.0f, 0.9f }, { 8, 1, 20.0f, 3, 30.0f, 0.9f } };
    const char *way_name[N_WAYS] = { "uniform", "32 cand.", "full reuse" };

    svgf_scene *scene = nullptr;
    svgf_lights *table = nullptr;
    svgf_restir *state[N_WAYS] = { nullptr, nullptr, nullptr };
    svgf_ctx *ctx[N_WAYS] = { nullptr, nullptr, nullptr };
    SVGF_OKAY(svgf_scene_create(0, geoms.data(), (int)geoms.size(), nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &scene));
    SVGF_OKAY(svgf_scene_enable_pose(scene, N_OBJECTS));
    SVGF_OKAY(svgf_lights_create(0, lamps.data(), N_LAMPS, &table));
    const size_t N = (size_t)W * H;
    float *rgb, *D[N_WAYS], *noisy[N_WAYS], *out[N_WAYS], *ref, *zero_term, *motion, *coord;
    void *gb, *q;
    SvgfScenePose *pose_dev, *pose_host;
    HIP_OK(hipMalloc((void **)&rgb, N * 12)); HIP_OK(hipMalloc((void **)&ref, N * 12)); HIP_OK(hipMalloc((void **)&zero_term, N * 12));
    HIP_OK(hipMemset(zero_term, 0, N * 12));
    HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel))); HIP_OK(hipMalloc((void **)&coord, N * 8));
    HIP_OK(hipMalloc((void **)&motion, sizeof(float) * 12 * N_OBJECTS)); HIP_OK(hipMalloc(&q, state_bytes));
    HIP_OK(hipMalloc((void **)&pose_dev, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames));
    HIP_OK(hipHostMalloc((void **)&pose_host, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames, hipHostMallocDefault));
    for (int k = 0; k < N_WAYS; k++) {
        SVGF_OKAY(svgf_restir_create(scene, W, H, &state[k]));
        SVGF_OKAY(svgf_create(0, W, H, &ctx[k]));
        SVGF_OKAY(svgf_set_object_motion(ctx[k], motion, N_OBJECTS));
        HIP_OK(hipMalloc((void **)&D[k], N * 12)); HIP_OK(hipMalloc((void **)&noisy[k], N * 12)); HIP_OK(hipMalloc((void **)&out[k], N * 12));
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
    const float y_axis[3] = { 0, 1, 0 }, zero[3] = { 0, 0, 0 }, light[3] = { 0.0f, 9.5f, 0.0f }, PI = 3.14159265f;

    printf("%d frames of %dx%d, the block %s; %d lamps, one final shadow ray per pixel, against svgf_lights_draw_all with %d samples per lamp\n",
           frames, W, H, moving ? "turning and sliding" : "at rest", N_LAMPS, SVGF_SCENE_MAX_SHADOW_SAMPLES);
    for (int f = 0; f < frames; f++) {
        SvgfScenePose *pose = pose_host + (size_t)f * N_OBJECTS;
        for (int k = 0; k < N_OBJECTS; k++) SVGF_OKAY(svgf_pose_rigid(y_axis, 0.0f, zero, zero, &pose[k]));
        const float slide[3] = { moving ? 0.25f * (float)f : 0.0f, 0, 0 };
        SVGF_OKAY(svgf_pose_rigid(y_axis, moving ? 9.0f * PI / 180.0f * (float)f : 0.0f, block_at, slide, &pose[BLOCK]));
        HIP_OK(hipMemcpyAsync(pose_dev + (size_t)f * N_OBJECTS, pose, sizeof(SvgfScenePose) * N_OBJECTS, hipMemcpyHostToDevice, s));
        const SvgfSynthParams sp = { f, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
        SVGF_OKAY(svgf_scene_pose(scene, pose_dev + (size_t)f * N_OBJECTS, N_OBJECTS, motion, s));
        SVGF_OKAY(svgf_scene_draw(scene, rgb, gb, W, H, &cam, &sp, light, s));                  // the G-buffer; its colour is not used
        SVGF_OKAY(svgf_motion_reproject(0, coord, SVGF_MOTION_PREV_COORD_F32, gb, nullptr, nullptr, W, H, &cam, p.reproj_scale, motion, N_OBJECTS, s));
        for (int k = 0; k < N_WAYS; k++) {
            SVGF_OKAY(svgf_restir_frame(state[k], table, gb, nullptr, coord, &ways[k], &sp, ambient, D[k], s));
            SVGF_OKAY(svgf_trace_compose(0, noisy[k], D[k], zero_term, &guide, W, H, s));
            SVGF_OKAY(svgf_denoise(ctx[k], out[k], D[k], gb, &cam, &p, s));
            SVGF_OKAY(svgf_trace_compose(0, out[k], out[k], zero_term, &guide, W, H, s));
        }
        if (f != 0 && f != 1 && f != 3 && f != 7 && f != frames - 1) continue;
        SVGF_OKAY(svgf_lights_draw_all(scene, table, gb, nullptr, W, H, SVGF_SCENE_MAX_SHADOW_SAMPLES, &sp, ambient, ref, s));
        SVGF_OKAY(svgf_trace_compose(0, ref, ref, zero_term, &guide, W, H, s));
        printf("frame %2d:", f);
        for (int k = 0; k < N_WAYS; k++) {
            SvgfQualityResult r[2];
            const float *scored[2] = { noisy[k], out[k] };
            for (int i = 0; i < 2; i++) {
                SVGF_OKAY(svgf_quality_meter(0, q, scored[i], ref, W, H, &qp, nullptr, nullptr, nullptr, s));
                SVGF_OKAY(svgf_quality_read(0, q, &r[i], s));
            }
            printf("   %s noisy %6.2f dB, denoised %6.2f dB / SSIM %.4f", way_name[k], r[0].psnr_db, r[1].psnr_db, r[1].mean_ssim);
        }
        printf("\n");
    }

    HIP_OK(hipStreamSynchronize(s));
    for (int k = 0; k < N_WAYS; k++) { svgf_restir_destroy(state[k]); svgf_destroy(ctx[k]); (void)hipFree(D[k]); (void)hipFree(noisy[k]); (void)hipFree(out[k]); }
    svgf_lights_destroy(table);
    SVGF_OKAY(svgf_scene_destroy(scene));
    (void)hipFree(rgb); (void)hipFree(ref); (void)hipFree(zero_term); (void)hipFree(gb); (void)hipFree(coord); (void)hipFree(motion); (void)hipFree(q);
    (void)hipFree(pose_dev); (void)hipHostFree(pose_host); (void)hipStreamDestroy(s);
    return 0;
}
