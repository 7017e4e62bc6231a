// examples/gloss_scene.cpp — mirror and glass along the paths (include/svgf_gloss.h row f20), through f18's two-context pipeline with
// and without the history clamp on the indirect term.  C++ through the C ABI of three libraries: libsvgf_hip.so (scene, pose, denoiser,
// quality meter), libsvgf_gloss.so (svgf_gloss_table_create, svgf_gloss_draw_split, and svgf_gloss_draw for the converged frame) and
// libsvgf_split.so (svgf_trace_compose).
//
// The room of examples/shadowed_scene.cpp with the block turning 9 degrees about y and sliding in x per frame, and beside it a MIRROR
// sphere (reflect 1, spec 0.95) and a GLASS cube (refract 1, ior 1.5, spec 1).  Per frame, on one stream: svgf_scene_pose with a motion
// table, ONE svgf_gloss_draw_split (1 path of up to 4 bounces, roulette from bounce 2, 1 shadow ray), then the direct term through a
// plain context and the indirect term through two contexts - both with the f8 firefly filter, one also with the f6 history clamp - and
// svgf_trace_compose of each pair.  On frames 0, 1, 3 and 7 (and the last) a converged frame of the same depth is drawn - 8 paths x 64
// shadow rays without roulette, averaged over `seeds` frame seeds on the host - and svgf_quality_meter scores the noisy frame and both
// pipelines against it; the PSNR is then repeated on the host over the mirror's pixels and over all others.
//
// What to look for: the G-buffer of a mirror pixel is the MIRROR's (its position, its normal, its id), so the temporal pass reprojects
// the sphere, which does not move, while what it shows - the turning block - does.  History there is accepted although the radiance
// changed: the reflection ghosts under motion, and the clamp is the only thing that bounds it.  A virtual-hit G-buffer (the position
// and id of what the mirror shows) is the follow-up; it is out of scope here.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/gloss_scene.cpp -L cuda-path-tracer-denoising_amd -lsvgf_gloss -lsvgf_split \
//         -lsvgf_hip -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/gloss_scene
//   examples/gloss_scene [frames=8] [width=640] [height=360] [moving=1] [seeds=8]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "svgf_gloss.h"
#include "svgf_split.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); return 1; } } while (0)
#define SVGF_OKAY(x) do { int rc__ = (x); if (rc__ != SVGF_OK) { fprintf(stderr, "%s failed (%d)\n", #x, rc__); return 1; } } while (0)

// an axis-aligned cube (type 0) or ellipsoid (type 1): centre t, edge lengths / diameters s
static SvgfSceneGeom prim(int type, float tx, float ty, float tz, float sx, float sy, float sz, float r, float g, float b, float emit)
{
    SvgfSceneGeom q = {};
    const float t[3] = { tx, ty, tz }, s[3] = { sx, sy, sz };
    q.type = type; q.albedo[0] = r; q.albedo[1] = g; q.albedo[2] = b; q.emittance = emit;
    for (int k = 0; k < 3; k++) {
        q.xf[4 * k + k] = s[k]; q.xf[4 * k + 3] = t[k];
        q.inv[4 * k + k] = 1.0f / s[k]; q.inv[4 * k + 3] = -t[k] / s[k];
        q.invT[3 * k + k] = 1.0f / s[k];
    }
    return q;
}

// PSNR (peak 1) of a against b over the pixels whose geomId is (inside) / is not (outside) `id`
static void masked_psnr(const std::vector<float> &a, const std::vector<float> &b, const std::vector<SvgfGBufferTexel> &gb, int id, double out[2], size_t count[2])
{
    double se[2] = { 0.0, 0.0 };
    count[0] = count[1] = 0;
    for (size_t i = 0; i < gb.size(); i++) {
        int gid;
        memcpy(&gid, reinterpret_cast<const char *>(&gb[i]) + 48, 4);       // the 13th word of a texel
        const int k = gid == id ? 0 : 1;
        for (int c = 0; c < 3; c++) { const double e = (double)a[3 * i + c] - (double)b[3 * i + c]; se[k] += e * e; }
        count[k]++;
    }
    for (int k = 0; k < 2; k++) out[k] = count[k] && se[k] > 0.0 ? 10.0 * log10(3.0 * (double)count[k] / se[k]) : 0.0;
}

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 8, W = argc > 2 ? atoi(argv[2]) : 640, H = argc > 3 ? atoi(argv[3]) : 360;
    const int moving = argc > 4 ? atoi(argv[4]) : 1, seeds = argc > 5 ? atoi(argv[5]) : 8;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "gloss_scene: no HIP device (the libraries have no CPU path)\n"); return 2; }
    const unsigned long long state_bytes = frames >= 1 && seeds >= 1 ? svgf_quality_state_bytes(W, H) : 0;
    if (state_bytes == 0) { fprintf(stderr, "usage: gloss_scene [frames >= 1] [width] [height] [moving 0/1] [seeds >= 1]\n"); return 2; }
    if (svgf_gloss_version() != svgf_version()) { fprintf(stderr, "gloss_scene: libsvgf_gloss.so and libsvgf_hip.so disagree on the ABI\n"); return 2; }
    static_assert(sizeof(SvgfGBufferTexel) == 52, "13 words per texel");
    HIP_OK(hipSetDevice(0));

    const int BLOCK = 5, MIRROR = 6, GLASS = 7, N_OBJECTS = 8, N_CTX = 3, N_OUT = 2, DEPTH = 4;
    const float block_at[3] = { -2.5f, 1.1f, 0.0f };
    const std::vector<SvgfSceneGeom> geoms = { prim(0, 0, 0, 0, 12, 0.2f, 12, 0.8f, 0.8f, 0.8f, 0), prim(0, 0, 5, -6, 12, 10, 0.2f, 0.8f, 0.8f, 0.7f, 0),
                                               prim(0, -6, 5, 0, 0.2f, 10, 12, 0.8f, 0.3f, 0.3f, 0), prim(0, 6, 5, 0, 0.2f, 10, 12, 0.3f, 0.8f, 0.3f, 0),
                                               prim(0, 0, 9.9f, 0, 3, 0.1f, 3, 1, 1, 1, 5),
                                               prim(0, block_at[0], block_at[1], block_at[2], 2, 2, 2, 0.3f, 0.4f, 0.9f, 0),
                                               prim(1, 0.5f, 1.6f, -2.5f, 3, 3, 3, 1, 1, 1, 0), prim(0, 3.2f, 1.1f, 0.5f, 2, 2, 2, 1, 1, 1, 0) };
    SvgfSurface surf[N_OBJECTS];
    for (int k = 0; k < N_OBJECTS; k++) surf[k] = SvgfSurface{ 0.0f, 0.0f, 1.0f, { 0.0f, 0.0f, 0.0f } };
    surf[MIRROR] = SvgfSurface{ 1.0f, 0.0f, 1.0f, { 0.95f, 0.95f, 0.95f } };
    surf[GLASS] = SvgfSurface{ 0.0f, 1.0f, 1.5f, { 1.0f, 1.0f, 1.0f } };
    SvgfSceneLight light = { { 0.0f, 9.5f, 0.0f }, { 1.5f, 0.0f, 0.0f }, { 0.0f, 0.0f, 1.5f }, 1 }, light_ref = light;
    light_ref.samples = SVGF_SCENE_MAX_SHADOW_SAMPLES;

    svgf_scene *scene = nullptr;
    svgf_gloss_table *table = nullptr;
    SVGF_OKAY(svgf_scene_create(0, geoms.data(), (int)geoms.size(), nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &scene));
    SVGF_OKAY(svgf_scene_enable_pose(scene, N_OBJECTS));
    SVGF_OKAY(svgf_gloss_table_create(0, surf, N_OBJECTS, &table));        // once: allocates and uploads
    const char *out_name[N_OUT] = { "no clamp", "clamp on I" };
    const size_t N = (size_t)W * H;
    float *noisy, *direct, *indirect, *ref, *out[N_CTX], *composed[N_OUT], *motion;
    void *gb, *gb_ref, *q;
    SvgfScenePose *pose_dev, *pose_host;
    HIP_OK(hipMalloc((void **)&noisy, N * 12)); HIP_OK(hipMalloc((void **)&ref, N * 12));
    HIP_OK(hipMalloc((void **)&direct, N * 12)); HIP_OK(hipMalloc((void **)&indirect, N * 12));
    HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel))); HIP_OK(hipMalloc(&gb_ref, N * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc((void **)&motion, sizeof(float) * 12 * N_OBJECTS)); HIP_OK(hipMalloc(&q, state_bytes));
    HIP_OK(hipMalloc((void **)&pose_dev, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames));
    HIP_OK(hipHostMalloc((void **)&pose_host, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames, hipHostMallocDefault));
    for (int k = 0; k < N_CTX; k++) HIP_OK(hipMalloc((void **)&out[k], N * 12));
    for (int k = 0; k < N_OUT; k++) HIP_OK(hipMalloc((void **)&composed[k], N * 12));
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1; p.sepcolor = 1; p.addcolor = 0;
    const SvgfGuide guide = { gb, nullptr, nullptr, nullptr, nullptr };
    SvgfCamera cam;
    float pixel_length[2];
    SVGF_OKAY(svgf_synth_camera(0, /*moving=*/0, W, H, &cam, pixel_length));
    p.reproj_scale[0] = pixel_length[0] * (float)W / 2.0f; p.reproj_scale[1] = pixel_length[1] * (float)H / 2.0f;
    const SvgfQualityParams qp = { 1.0f, 1.0f, 0 };
    const float y_axis[3] = { 0, 1, 0 }, zero[3] = { 0, 0, 0 }, PI = 3.14159265f;
    std::vector<float> h_one(3 * N), h_ref(3 * N);
    std::vector<double> h_sum(3 * N);
    std::vector<SvgfGBufferTexel> h_gb(N);

    const SvgfPathParams pp = { 1, DEPTH, 2, 0.15f, 1 }, pp_ref = { SVGF_PATH_MAX_PATHS, DEPTH, 0, 0.15f, 1 };
    // contexts: 0 the direct term; 1 the indirect term, firefly filter only; 2 the indirect term, firefly filter and history clamp
    svgf_ctx *ctx[N_CTX] = { nullptr, nullptr, nullptr };
    for (int k = 0; k < N_CTX; k++) {
        SVGF_OKAY(svgf_create(0, W, H, &ctx[k]));
        SVGF_OKAY(svgf_set_object_motion(ctx[k], motion, N_OBJECTS));
    }
    SVGF_OKAY(svgf_set_firefly_filter(ctx[1], 2, 1.0f));
    SVGF_OKAY(svgf_set_firefly_filter(ctx[2], 2, 1.0f));
    SVGF_OKAY(svgf_set_history_clamp(ctx[2], 1, 1.5f));
    printf("max_depth %d: %d frames of %dx%d, the block %s; a mirror sphere (id %d) and a glass cube (id %d, ior 1.5); 1 path (roulette from "
           "bounce %d) and 1 shadow ray per pixel against %d x (%d paths, %d shadow rays, no roulette); firefly filter rank 2, scale 1; clamp "
           "radius 1, 1.5 sigma\n", DEPTH, frames, W, H, moving ? "turning and sliding" : "at rest", MIRROR, GLASS, pp.rr_depth, seeds, pp_ref.paths,
           light_ref.samples);
    for (int f = 0; f < frames; f++) {
        SvgfScenePose *poses = pose_host + (size_t)f * N_OBJECTS;
        for (int k = 0; k < N_OBJECTS; k++) SVGF_OKAY(svgf_pose_rigid(y_axis, 0.0f, zero, zero, &poses[k]));
        const float slide[3] = { moving ? 0.25f * (float)f : 0.0f, 0, 0 };
        SVGF_OKAY(svgf_pose_rigid(y_axis, moving ? 9.0f * PI / 180.0f * (float)f : 0.0f, block_at, slide, &poses[BLOCK]));
        HIP_OK(hipMemcpyAsync(pose_dev + (size_t)f * N_OBJECTS, poses, sizeof(SvgfScenePose) * N_OBJECTS, hipMemcpyHostToDevice, s));
        const SvgfSynthParams sp = { f, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
        SVGF_OKAY(svgf_scene_pose(scene, pose_dev + (size_t)f * N_OBJECTS, N_OBJECTS, motion, s));
        SVGF_OKAY(svgf_gloss_draw_split(scene, table, direct, indirect, noisy, gb, nullptr, W, H, &cam, &sp, &light, &pp, s));
        SVGF_OKAY(svgf_denoise(ctx[0], out[0], direct, gb, &cam, &p, s));
        SVGF_OKAY(svgf_denoise(ctx[1], out[1], indirect, gb, &cam, &p, s));
        SVGF_OKAY(svgf_denoise(ctx[2], out[2], indirect, gb, &cam, &p, s));
        SVGF_OKAY(svgf_trace_compose(0, composed[0], out[0], out[1], &guide, W, H, s));
        SVGF_OKAY(svgf_trace_compose(0, composed[1], out[0], out[2], &guide, W, H, s));
        if (f != 0 && f != 1 && f != 3 && f != 7 && f != frames - 1) continue;
        // the converged frame: the same pose under `seeds` other frame seeds, averaged in double on the host
        for (size_t i = 0; i < 3 * N; i++) h_sum[i] = 0.0;
        for (int k = 0; k < seeds; k++) {
            const SvgfSynthParams sp_ref = { 1000 + f * seeds + k, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
            SVGF_OKAY(svgf_gloss_draw(scene, table, ref, gb_ref, nullptr, W, H, &cam, &sp_ref, &light_ref, &pp_ref, s));
            HIP_OK(hipMemcpyAsync(h_one.data(), ref, N * 12, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            for (size_t i = 0; i < 3 * N; i++) h_sum[i] += h_one[i];
        }
        for (size_t i = 0; i < 3 * N; i++) h_ref[i] = (float)(h_sum[i] / seeds);
        HIP_OK(hipMemcpyAsync(ref, h_ref.data(), N * 12, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(h_gb.data(), gb, N * sizeof(SvgfGBufferTexel), hipMemcpyDeviceToHost, s));
        SvgfQualityResult r[1 + N_OUT];
        const float *scored[1 + N_OUT] = { noisy, composed[0], composed[1] };
        double in_out[1 + N_OUT][2];
        size_t count[2] = { 0, 0 };
        for (int k = 0; k < 1 + N_OUT; k++) {
            SVGF_OKAY(svgf_quality_meter(0, q, scored[k], ref, W, H, &qp, nullptr, nullptr, nullptr, s));
            SVGF_OKAY(svgf_quality_read(0, q, &r[k], s));
            HIP_OK(hipMemcpyAsync(h_one.data(), scored[k], N * 12, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            masked_psnr(h_one, h_ref, h_gb, MIRROR, in_out[k], count);
        }
        printf("frame %2d (%zu mirror pixels): noisy %6.2f dB / SSIM %.4f [mirror %6.2f dB, elsewhere %6.2f dB]", f, count[0], r[0].psnr_db, r[0].mean_ssim,
               in_out[0][0], in_out[0][1]);
        for (int k = 0; k < N_OUT; k++)
            printf("   %s %6.2f dB / %.4f [mirror %6.2f dB, elsewhere %6.2f dB]", out_name[k], r[1 + k].psnr_db, r[1 + k].mean_ssim, in_out[1 + k][0], in_out[1 + k][1]);
        printf("\n");
    }
    HIP_OK(hipStreamSynchronize(s));
    for (int k = 0; k < N_CTX; k++) svgf_destroy(ctx[k]);

    svgf_gloss_table_destroy(table);
    SVGF_OKAY(svgf_scene_destroy(scene));
    for (int k = 0; k < N_CTX; k++) (void)hipFree(out[k]);
    for (int k = 0; k < N_OUT; k++) (void)hipFree(composed[k]);
    (void)hipFree(noisy); (void)hipFree(direct); (void)hipFree(indirect); (void)hipFree(ref); (void)hipFree(gb); (void)hipFree(gb_ref); (void)hipFree(motion);
    (void)hipFree(q); (void)hipFree(pose_dev); (void)hipHostFree(pose_host); (void)hipStreamDestroy(s);
    return 0;
}
