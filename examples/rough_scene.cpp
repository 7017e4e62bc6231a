// examples/rough_scene.cpp — a rough glossy floor (include/svgf_rough.h row f22) through f18's two-context pipeline: the case whose
// one-sample reflection is noisy and is neither the first hit's geometry nor a sharp virtual image.  C++ through the C ABI of four
// libraries: libsvgf_hip.so (scene, pose, denoiser, quality meter), libsvgf_gloss.so (svgf_gloss_table_create), libsvgf_rough.so
// (svgf_rough_table_create, svgf_rough_draw_split, and svgf_rough_draw for the converged frame) and libsvgf_split.so
// (svgf_trace_compose).
//
// The room is examples/gloss_scene.cpp's - the block, a MIRROR sphere and a GLASS cube - with the floor a full mirror (reflect 1) of
// GGX roughness alpha, run for alpha 0.1 and 0.4.  Leg 1: everything at rest, the camera moving (svgf_synth_camera's moving path).
// Leg 2: the camera at rest, the block turning 9 degrees about y and sliding in x per frame.  Per frame, on one stream:
// svgf_scene_pose, then TWO svgf_rough_draw_split - guide_alpha 0 (the floor is too rough for the guide: its texels are the first
// hit's) and guide_alpha 1 (the guide follows the floor as if smooth: its texels are the smooth mirror's virtual hit) - which draw the
// same D and I on bits; then for EACH G-buffer the direct term through a plain context and the indirect term through four contexts -
// with and without the f8 firefly filter, with and without the f6 history clamp - and svgf_trace_compose of each pair.  On frames 0,
// 1, 3, 7 and the last a converged frame is drawn (8 paths x 64 shadow rays, no roulette, averaged over `seeds` frame seeds on the
// host); svgf_quality_meter scores every pipeline against it, and the PSNR is repeated on the host inside and outside the floor's
// pixels (those on which the guide of guide_alpha 1 runs).  The numbers are printed whichever way they fall.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/rough_scene.cpp -L cuda-path-tracer-denoising_amd -lsvgf_rough -lsvgf_gloss \
//         -lsvgf_split -lsvgf_hip -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/rough_scene
//   examples/rough_scene [frames=8] [width=640] [height=360] [seeds=8]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "svgf_rough.h"
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

// PSNR (peak 1) of a against b over the pixels whose chain is not 0 (inside: the floor) / is 0 (outside)
static void masked_psnr(const std::vector<float> &a, const std::vector<float> &b, const std::vector<int> &chain, double out[2], size_t count[2])
{
    double se[2] = { 0.0, 0.0 };
    count[0] = count[1] = 0;
    for (size_t i = 0; i < chain.size(); i++) {
        const int k = chain[i] != 0 ? 0 : 1;
        for (int c = 0; c < 3; c++) { const double e = (double)a[3 * i + c] - (double)b[3 * i + c]; se[k] += e * e; }
        count[k]++;
    }
    for (int k = 0; k < 2; k++) out[k] = count[k] && se[k] > 0.0 ? 10.0 * log10(3.0 * (double)count[k] / se[k]) : 0.0;
}

enum { FLOOR = 0, BLOCK = 5, MIRROR = 6, GLASS = 7, N_OBJECTS = 8, N_GB = 2, N_IND = 4, N_CTX = 1 + N_IND, DEPTH = 4 };

// One leg with a floor of roughness `alpha`: `block_moves` leg 2's motion, `camera_moves` leg 1's
static int leg(const char *title, float alpha, int frames, int W, int H, int seeds, bool block_moves, bool camera_moves)
{
    const float block_at[3] = { -2.5f, 1.1f, 0.0f };
    const std::vector<SvgfSceneGeom> geoms = { prim(0, 0, 0, 0, 12, 0.2f, 12, 0.8f, 0.8f, 0.8f, 0), prim(0, 0, 5, -6, 12, 10, 0.2f, 0.8f, 0.8f, 0.7f, 0),
                                               prim(0, -6, 5, 0, 0.2f, 10, 12, 0.8f, 0.3f, 0.3f, 0), prim(0, 6, 5, 0, 0.2f, 10, 12, 0.3f, 0.8f, 0.3f, 0),
                                               prim(0, 0, 9.9f, 0, 3, 0.1f, 3, 1, 1, 1, 5),
                                               prim(0, block_at[0], block_at[1], block_at[2], 2, 2, 2, 0.3f, 0.4f, 0.9f, 0),
                                               prim(1, 0.5f, 1.6f, -2.5f, 3, 3, 3, 1, 1, 1, 0), prim(0, 3.2f, 1.1f, 0.5f, 2, 2, 2, 1, 1, 1, 0) };
    SvgfSceneLight light = { { 0.0f, 9.5f, 0.0f }, { 1.5f, 0.0f, 0.0f }, { 0.0f, 0.0f, 1.5f }, 1 }, light_ref = light;
    light_ref.samples = SVGF_SCENE_MAX_SHADOW_SAMPLES;
    const unsigned long long state_bytes = svgf_quality_state_bytes(W, H);
    SvgfSurface surf[N_OBJECTS];
    float rough_host[N_OBJECTS];
    for (int k = 0; k < N_OBJECTS; k++) { surf[k] = SvgfSurface{ 0.0f, 0.0f, 1.0f, { 0.0f, 0.0f, 0.0f } }; rough_host[k] = 0.0f; }
    surf[FLOOR] = SvgfSurface{ 1.0f, 0.0f, 1.0f, { 0.9f, 0.9f, 0.9f } };
    surf[MIRROR] = SvgfSurface{ 1.0f, 0.0f, 1.0f, { 0.95f, 0.95f, 0.95f } };
    surf[GLASS] = SvgfSurface{ 0.0f, 1.0f, 1.5f, { 1.0f, 1.0f, 1.0f } };
    rough_host[FLOOR] = alpha;

    svgf_scene *scene = nullptr;
    svgf_gloss_table *table = nullptr;
    svgf_rough_table *rough = nullptr;
    SVGF_OKAY(svgf_scene_create(0, geoms.data(), (int)geoms.size(), nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &scene));
    SVGF_OKAY(svgf_scene_enable_pose(scene, N_OBJECTS));
    SVGF_OKAY(svgf_gloss_table_create(0, surf, N_OBJECTS, &table));        // once: allocates and uploads
    SVGF_OKAY(svgf_rough_table_create(0, rough_host, N_OBJECTS, &rough));  // once: allocates and uploads
    const char *gb_name[N_GB] = { "guide_alpha 0 (first-hit texels on the floor) ", "guide_alpha 1 (smooth-mirror guide on the floor)" };
    const char *ind_name[N_IND] = { "plain", "f8", "f6", "f8+f6" };
    const float guide_alpha[N_GB] = { 0.0f, 1.0f };
    const size_t N = (size_t)W * H;
    float *noisy, *direct, *indirect, *ref, *out[N_GB][N_CTX], *composed[N_GB][N_IND], *motion;
    void *gb[N_GB], *gb_ref, *q;
    int *chain[N_GB];
    SvgfScenePose *pose_dev, *pose_host;
    HIP_OK(hipMalloc((void **)&noisy, N * 12)); HIP_OK(hipMalloc((void **)&ref, N * 12));
    HIP_OK(hipMalloc((void **)&direct, N * 12)); HIP_OK(hipMalloc((void **)&indirect, N * 12));
    HIP_OK(hipMalloc(&gb_ref, N * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc((void **)&motion, sizeof(float) * 12 * N_OBJECTS)); HIP_OK(hipMalloc(&q, state_bytes));
    HIP_OK(hipMalloc((void **)&pose_dev, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames));
    HIP_OK(hipHostMalloc((void **)&pose_host, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames, hipHostMallocDefault));
    for (int g = 0; g < N_GB; g++) {
        HIP_OK(hipMalloc(&gb[g], N * sizeof(SvgfGBufferTexel))); HIP_OK(hipMalloc((void **)&chain[g], N * 4));
        for (int k = 0; k < N_CTX; k++) HIP_OK(hipMalloc((void **)&out[g][k], N * 12));
        for (int k = 0; k < N_IND; k++) HIP_OK(hipMalloc((void **)&composed[g][k], N * 12));
    }
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1; p.sepcolor = 1; p.addcolor = 0;
    SvgfCamera cam;
    float pixel_length[2];
    SVGF_OKAY(svgf_synth_camera(0, /*moving=*/0, W, H, &cam, pixel_length));
    p.reproj_scale[0] = pixel_length[0] * (float)W / 2.0f; p.reproj_scale[1] = pixel_length[1] * (float)H / 2.0f;
    const SvgfQualityParams qp = { 1.0f, 1.0f, 0 };
    const float y_axis[3] = { 0, 1, 0 }, zero[3] = { 0, 0, 0 }, PI = 3.14159265f;
    std::vector<float> h_one(3 * N), h_ref(3 * N);
    std::vector<double> h_sum(3 * N);
    std::vector<int> h_chain(N);

    const SvgfPathParams pp = { 1, DEPTH, 2, 0.15f, 1 }, pp_ref = { SVGF_PATH_MAX_PATHS, DEPTH, 0, 0.15f, 1 };
    const SvgfVirtualParams vp = { DEPTH, N_OBJECTS };          // virtual ids behind the motion table's rows: never moved
    // contexts per G-buffer: 0 the direct term; 1..4 the indirect term: plain, firefly filter, history clamp, both
    svgf_ctx *ctx[N_GB][N_CTX] = {};
    for (int g = 0; g < N_GB; g++) {
        for (int k = 0; k < N_CTX; k++) {
            SVGF_OKAY(svgf_create(0, W, H, &ctx[g][k]));
            SVGF_OKAY(svgf_set_object_motion(ctx[g][k], motion, N_OBJECTS));
        }
        SVGF_OKAY(svgf_set_firefly_filter(ctx[g][2], 2, 1.0f));
        SVGF_OKAY(svgf_set_history_clamp(ctx[g][3], 1, 1.5f));
        SVGF_OKAY(svgf_set_firefly_filter(ctx[g][4], 2, 1.0f));
        SVGF_OKAY(svgf_set_history_clamp(ctx[g][4], 1, 1.5f));
    }
    printf("%s, floor alpha %.2f: %d frames of %dx%d, max_depth %d, max_chain %d, id_offset %d; 1 path (roulette from bounce %d) and 1 shadow ray per "
           "pixel against %d x (%d paths, %d shadow rays, no roulette); f8 = firefly filter rank 2, scale 1; f6 = history clamp radius 1, 1.5 sigma, "
           "either on the indirect term\n", title, alpha, frames, W, H, DEPTH, vp.max_chain, vp.id_offset, pp.rr_depth, seeds, pp_ref.paths, light_ref.samples);
    for (int f = 0; f < frames; f++) {
        SvgfScenePose *poses = pose_host + (size_t)f * N_OBJECTS;
        for (int k = 0; k < N_OBJECTS; k++) SVGF_OKAY(svgf_pose_rigid(y_axis, 0.0f, zero, zero, &poses[k]));
        const float slide[3] = { block_moves ? 0.25f * (float)f : 0.0f, 0, 0 };
        SVGF_OKAY(svgf_pose_rigid(y_axis, block_moves ? 9.0f * PI / 180.0f * (float)f : 0.0f, block_at, slide, &poses[BLOCK]));
        HIP_OK(hipMemcpyAsync(pose_dev + (size_t)f * N_OBJECTS, poses, sizeof(SvgfScenePose) * N_OBJECTS, hipMemcpyHostToDevice, s));
        if (camera_moves) SVGF_OKAY(svgf_synth_camera(f, /*moving=*/1, W, H, &cam, pixel_length));
        const SvgfSynthParams sp = { f, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
        SVGF_OKAY(svgf_scene_pose(scene, pose_dev + (size_t)f * N_OBJECTS, N_OBJECTS, motion, s));
        for (int g = 0; g < N_GB; g++) {
            const SvgfRoughParams rp = { guide_alpha[g] };
            SVGF_OKAY(svgf_rough_draw_split(scene, table, direct, indirect, noisy, gb[g], nullptr, W, H, &cam, &sp, &light, &pp, &vp, chain[g], s, rough, &rp));
        }
        for (int g = 0; g < N_GB; g++) {
            const SvgfGuide guide = { gb[g], nullptr, nullptr, nullptr, nullptr };
            SVGF_OKAY(svgf_denoise(ctx[g][0], out[g][0], direct, gb[g], &cam, &p, s));
            for (int k = 0; k < N_IND; k++) {
                SVGF_OKAY(svgf_denoise(ctx[g][1 + k], out[g][1 + k], indirect, gb[g], &cam, &p, s));
                SVGF_OKAY(svgf_trace_compose(0, composed[g][k], out[g][0], out[g][1 + k], &guide, W, H, s));
            }
        }
        if (f != 0 && f != 1 && f != 3 && f != 7 && f != frames - 1) continue;
        // the converged frame: the same pose and camera under `seeds` other frame seeds, averaged in double on the host
        for (size_t i = 0; i < 3 * N; i++) h_sum[i] = 0.0;
        const SvgfRoughParams rp_ref = { 0.0f };
        for (int k = 0; k < seeds; k++) {
            const SvgfSynthParams sp_ref = { 1000 + f * seeds + k, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
            SVGF_OKAY(svgf_rough_draw(scene, table, ref, gb_ref, nullptr, W, H, &cam, &sp_ref, &light_ref, &pp_ref, &vp, nullptr, s, rough, &rp_ref));
            HIP_OK(hipMemcpyAsync(h_one.data(), ref, N * 12, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            for (size_t i = 0; i < 3 * N; i++) h_sum[i] += h_one[i];
        }
        for (size_t i = 0; i < 3 * N; i++) h_ref[i] = (float)(h_sum[i] / seeds);
        HIP_OK(hipMemcpyAsync(ref, h_ref.data(), N * 12, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(h_chain.data(), chain[1], N * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        size_t count[2] = { 0, 0 }, virt = 0;
        for (size_t i = 0; i < N; i++) virt += h_chain[i] > 0;
        SvgfQualityResult r;
        double io[2];
        SVGF_OKAY(svgf_quality_meter(0, q, noisy, ref, W, H, &qp, nullptr, nullptr, nullptr, s));
        SVGF_OKAY(svgf_quality_read(0, q, &r, s));
        HIP_OK(hipMemcpyAsync(h_one.data(), noisy, N * 12, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        masked_psnr(h_one, h_ref, h_chain, io, count);
        printf("frame %2d (%zu floor pixels, %zu of them with a virtual hit under guide_alpha 1): noisy %6.2f dB / SSIM %.4f [floor %6.2f dB, elsewhere %6.2f dB]\n",
               f, count[0], virt, r.psnr_db, r.mean_ssim, io[0], io[1]);
        for (int g = 0; g < N_GB; g++) {
            printf("    %s:\n", gb_name[g]);
            for (int k = 0; k < N_IND; k++) {
                SVGF_OKAY(svgf_quality_meter(0, q, composed[g][k], ref, W, H, &qp, nullptr, nullptr, nullptr, s));
                SVGF_OKAY(svgf_quality_read(0, q, &r, s));
                HIP_OK(hipMemcpyAsync(h_one.data(), composed[g][k], N * 12, hipMemcpyDeviceToHost, s));
                HIP_OK(hipStreamSynchronize(s));
                masked_psnr(h_one, h_ref, h_chain, io, count);
                printf("        %-6s %6.2f dB / %.4f [floor %6.2f dB, elsewhere %6.2f dB]\n", ind_name[k], r.psnr_db, r.mean_ssim, io[0], io[1]);
            }
        }
    }
    HIP_OK(hipStreamSynchronize(s));
    for (int g = 0; g < N_GB; g++) {
        for (int k = 0; k < N_CTX; k++) { svgf_destroy(ctx[g][k]); (void)hipFree(out[g][k]); }
        for (int k = 0; k < N_IND; k++) (void)hipFree(composed[g][k]);
        (void)hipFree(gb[g]); (void)hipFree(chain[g]);
    }
    svgf_rough_table_destroy(rough);
    svgf_gloss_table_destroy(table);
    SVGF_OKAY(svgf_scene_destroy(scene));
    (void)hipFree(noisy); (void)hipFree(direct); (void)hipFree(indirect); (void)hipFree(ref); (void)hipFree(gb_ref); (void)hipFree(motion);
    (void)hipFree(q); (void)hipFree(pose_dev); (void)hipHostFree(pose_host); (void)hipStreamDestroy(s);
    return 0;
}

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 8, W = argc > 2 ? atoi(argv[2]) : 640, H = argc > 3 ? atoi(argv[3]) : 360;
    const int seeds = argc > 4 ? atoi(argv[4]) : 8;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "rough_scene: no HIP device (the libraries have no CPU path)\n"); return 2; }
    if (frames < 1 || seeds < 1 || svgf_quality_state_bytes(W, H) == 0) { fprintf(stderr, "usage: rough_scene [frames >= 1] [width] [height] [seeds >= 1]\n"); return 2; }
    if (svgf_rough_version() != svgf_version() || svgf_gloss_version() != svgf_version()) {
        fprintf(stderr, "rough_scene: the companion libraries and libsvgf_hip.so disagree on the ABI\n");
        return 2;
    }
    static_assert(sizeof(SvgfGBufferTexel) == 52, "13 words per texel");
    HIP_OK(hipSetDevice(0));
    const float alphas[2] = { 0.1f, 0.4f };
    for (int i = 0; i < 2; i++) {
        if (leg("leg 1, everything at rest, the camera moving", alphas[i], frames, W, H, seeds, false, true)) return 1;
        if (leg("leg 2, the camera at rest, the block turning and sliding", alphas[i], frames, W, H, seeds, true, false)) return 1;
    }
    return 0;
}
