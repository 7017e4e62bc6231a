// examples/highlight_scene.cpp — the lamp's highlight on a rough floor (include/svgf_highlight.h row f23) through f18's two-context
// pipeline: a view-dependent, high-contrast highlight that moves with the camera, the hard case for the temporal pass.  C++ through the
// C ABI of five libraries: libsvgf_hip.so (scene, denoiser, quality meter), libsvgf_gloss.so (svgf_gloss_table_create),
// libsvgf_rough.so (svgf_rough_table_create), libsvgf_highlight.so (svgf_highlight_draw_split, and svgf_highlight_draw for the
// converged frame) and libsvgf_split.so (svgf_trace_compose).
//
// The room is examples/rough_scene.cpp's - the block, a MIRROR sphere and a GLASS cube - with the floor a full mirror (reflect 1) of
// GGX roughness alpha under the lamp, run for alpha 0.1 and 0.4, everything at rest and the camera moving (svgf_synth_camera's moving
// path).  Per frame, on one stream, THREE svgf_highlight_draw_split: highlights off (enable 0: row f22's frame), on without a clamp,
// and on with clamp CLAMP; for each the direct and the indirect term through four pairs of contexts - plain, with the f8 firefly
// filter, with the f6 history clamp, with both, on BOTH terms (the first hit's highlight is part of the direct term) - and
// svgf_trace_compose of each pair.  On frames 0, 1, 3, 7 and the last a converged frame is drawn with the highlight on and no clamp
// (8 paths x 64 shadow rays, no roulette, averaged over `seeds` frame seeds on the host); svgf_quality_meter scores every pipeline
// against it, and the PSNR is repeated on the host on and off the floor's pixels.  The numbers are printed whichever way they fall.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/highlight_scene.cpp -L cuda-path-tracer-denoising_amd -lsvgf_highlight \
//         -lsvgf_rough -lsvgf_gloss -lsvgf_split -lsvgf_hip -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/highlight_scene
//   examples/highlight_scene [frames=8] [width=640] [height=360] [seeds=8]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "svgf_highlight.h"
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

// PSNR (peak 1) of a against b over the floor's pixels (out[0]) and over the others (out[1])
static void masked_psnr(const std::vector<float> &a, const std::vector<float> &b, const std::vector<char> &floor, double out[2], size_t count[2])
{
    double se[2] = { 0.0, 0.0 };
    count[0] = count[1] = 0;
    for (size_t i = 0; i < floor.size(); i++) {
        const int k = floor[i] ? 0 : 1;
        for (int c = 0; c < 3; c++) { const double e = (double)a[3 * i + c] - (double)b[3 * i + c]; se[k] += e * e; }
        count[k]++;
    }
    for (int k = 0; k < 2; k++) out[k] = count[k] && se[k] > 0.0 ? 10.0 * log10(3.0 * (double)count[k] / se[k]) : 0.0;
}

enum { FLOOR = 0, BLOCK = 5, MIRROR = 6, GLASS = 7, N_OBJECTS = 8, N_DRAW = 3, N_FILTER = 4, DEPTH = 4 };
static const float CLAMP = 4.0f;

static int leg(float alpha, int frames, int W, int H, int seeds)
{
    const std::vector<SvgfSceneGeom> geoms = { prim(0, 0, 0, 0, 12, 0.2f, 12, 0.8f, 0.8f, 0.8f, 0), prim(0, 0, 5, -6, 12, 10, 0.2f, 0.8f, 0.8f, 0.7f, 0),
                                               prim(0, -6, 5, 0, 0.2f, 10, 12, 0.8f, 0.3f, 0.3f, 0), prim(0, 6, 5, 0, 0.2f, 10, 12, 0.3f, 0.8f, 0.3f, 0),
                                               prim(0, 0, 9.9f, 0, 3, 0.1f, 3, 1, 1, 1, 5), prim(0, -2.5f, 1.1f, 0.0f, 2, 2, 2, 0.3f, 0.4f, 0.9f, 0),
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
    SVGF_OKAY(svgf_gloss_table_create(0, surf, N_OBJECTS, &table));        // once: allocates and uploads
    SVGF_OKAY(svgf_rough_table_create(0, rough_host, N_OBJECTS, &rough));  // once: allocates and uploads
    const char *draw_name[N_DRAW] = { "highlight off (enable 0)", "highlight on, no clamp", "highlight on, clamp 4" };
    const char *filter_name[N_FILTER] = { "plain", "f8", "f6", "f8+f6" };
    const SvgfHighlightParams hp[N_DRAW] = { { 0, 0.0f }, { 1, 0.0f }, { 1, CLAMP } };
    const size_t N = (size_t)W * H;
    float *noisy[N_DRAW], *direct[N_DRAW], *indirect[N_DRAW], *ref, *out_d[N_DRAW][N_FILTER], *out_i[N_DRAW][N_FILTER], *composed[N_DRAW][N_FILTER];
    void *gb, *gb_ref, *q;
    HIP_OK(hipMalloc((void **)&ref, N * 12));
    HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel))); HIP_OK(hipMalloc(&gb_ref, N * sizeof(SvgfGBufferTexel))); HIP_OK(hipMalloc(&q, state_bytes));
    for (int g = 0; g < N_DRAW; g++) {
        HIP_OK(hipMalloc((void **)&noisy[g], N * 12)); HIP_OK(hipMalloc((void **)&direct[g], N * 12)); HIP_OK(hipMalloc((void **)&indirect[g], N * 12));
        for (int k = 0; k < N_FILTER; k++) {
            HIP_OK(hipMalloc((void **)&out_d[g][k], N * 12)); HIP_OK(hipMalloc((void **)&out_i[g][k], N * 12)); HIP_OK(hipMalloc((void **)&composed[g][k], N * 12));
        }
    }
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1; p.sepcolor = 1; p.addcolor = 0;
    SvgfCamera cam;
    float pixel_length[2];
    SVGF_OKAY(svgf_synth_camera(0, /*moving=*/1, W, H, &cam, pixel_length));
    p.reproj_scale[0] = pixel_length[0] * (float)W / 2.0f; p.reproj_scale[1] = pixel_length[1] * (float)H / 2.0f;
    const SvgfQualityParams qp = { 1.0f, 1.0f, 0 };
    std::vector<float> h_one(3 * N), h_ref(3 * N);
    std::vector<double> h_sum(3 * N);
    std::vector<SvgfGBufferTexel> h_gb(N);
    std::vector<char> h_floor(N);

    const SvgfPathParams pp = { 1, DEPTH, 2, 0.15f, 1 }, pp_ref = { SVGF_PATH_MAX_PATHS, DEPTH, 0, 0.15f, 1 };
    const SvgfVirtualParams vp = { DEPTH, N_OBJECTS };
    const SvgfRoughParams rp = { 0.0f };                // the floor is too rough for the guide: its texels are the first hit's
    // per draw and filter setting a context for the direct and one for the indirect term
    svgf_ctx *ctx_d[N_DRAW][N_FILTER] = {}, *ctx_i[N_DRAW][N_FILTER] = {};
    for (int g = 0; g < N_DRAW; g++) {
        for (int k = 0; k < N_FILTER; k++) {
            svgf_ctx **pair[2] = { &ctx_d[g][k], &ctx_i[g][k] };
            for (int t = 0; t < 2; t++) {
                SVGF_OKAY(svgf_create(0, W, H, pair[t]));
                if (k == 1 || k == 3) SVGF_OKAY(svgf_set_firefly_filter(*pair[t], 2, 1.0f));
                if (k == 2 || k == 3) SVGF_OKAY(svgf_set_history_clamp(*pair[t], 1, 1.5f));
            }
        }
    }
    printf("floor alpha %.2f, everything at rest, the camera moving: %d frames of %dx%d, max_depth %d; 1 path (roulette from bounce %d) and 1 shadow ray "
           "per pixel against %d x (%d paths, %d shadow rays, no roulette, highlight on, no clamp); f8 = firefly filter rank 2, scale 1; f6 = history "
           "clamp radius 1, 1.5 sigma, either on both terms\n", alpha, frames, W, H, DEPTH, pp.rr_depth, seeds, pp_ref.paths, light_ref.samples);
    for (int f = 0; f < frames; f++) {
        SVGF_OKAY(svgf_synth_camera(f, /*moving=*/1, W, H, &cam, pixel_length));
        const SvgfSynthParams sp = { f, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
        for (int g = 0; g < N_DRAW; g++)
            SVGF_OKAY(svgf_highlight_draw_split(scene, table, direct[g], indirect[g], noisy[g], gb, nullptr, W, H, &cam, &sp, &light, &pp, &vp, nullptr, s,
                                                rough, &rp, &hp[g]));
        const SvgfGuide guide = { gb, nullptr, nullptr, nullptr, nullptr };
        for (int g = 0; g < N_DRAW; g++) {
            for (int k = 0; k < N_FILTER; k++) {
                SVGF_OKAY(svgf_denoise(ctx_d[g][k], out_d[g][k], direct[g], gb, &cam, &p, s));
                SVGF_OKAY(svgf_denoise(ctx_i[g][k], out_i[g][k], indirect[g], gb, &cam, &p, s));
                SVGF_OKAY(svgf_trace_compose(0, composed[g][k], out_d[g][k], out_i[g][k], &guide, W, H, s));
            }
        }
        if (f != 0 && f != 1 && f != 3 && f != 7 && f != frames - 1) continue;
        // the converged frame: the same camera under `seeds` other frame seeds, averaged in double on the host
        for (size_t i = 0; i < 3 * N; i++) h_sum[i] = 0.0;
        for (int k = 0; k < seeds; k++) {
            const SvgfSynthParams sp_ref = { 1000 + f * seeds + k, 7, 0.0f, 0.0f, { pixel_length[0], pixel_length[1] } };
            SVGF_OKAY(svgf_highlight_draw(scene, table, ref, gb_ref, nullptr, W, H, &cam, &sp_ref, &light_ref, &pp_ref, &vp, nullptr, s, rough, &rp, &hp[1]));
            HIP_OK(hipMemcpyAsync(h_one.data(), ref, N * 12, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            for (size_t i = 0; i < 3 * N; i++) h_sum[i] += h_one[i];
        }
        for (size_t i = 0; i < 3 * N; i++) h_ref[i] = (float)(h_sum[i] / seeds);
        HIP_OK(hipMemcpyAsync(ref, h_ref.data(), N * 12, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(h_gb.data(), gb, N * sizeof(SvgfGBufferTexel), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        for (size_t i = 0; i < N; i++) { int id; memcpy(&id, (const char *)&h_gb[i] + 48, 4); h_floor[i] = id == FLOOR; }
        size_t count[2] = { 0, 0 };
        SvgfQualityResult r;
        double io[2];
        printf("frame %2d\n", f);
        for (int g = 0; g < N_DRAW; g++) {
            SVGF_OKAY(svgf_quality_meter(0, q, noisy[g], ref, W, H, &qp, nullptr, nullptr, nullptr, s));
            SVGF_OKAY(svgf_quality_read(0, q, &r, s));
            HIP_OK(hipMemcpyAsync(h_one.data(), noisy[g], N * 12, hipMemcpyDeviceToHost, s));
            HIP_OK(hipStreamSynchronize(s));
            masked_psnr(h_one, h_ref, h_floor, io, count);
            printf("    %s (%zu floor pixels of %zu): noisy %6.2f dB / SSIM %.4f [floor %6.2f dB, elsewhere %6.2f dB]\n", draw_name[g], count[0], N, r.psnr_db,
                   r.mean_ssim, io[0], io[1]);
            for (int k = 0; k < N_FILTER; k++) {
                SVGF_OKAY(svgf_quality_meter(0, q, composed[g][k], ref, W, H, &qp, nullptr, nullptr, nullptr, s));
                SVGF_OKAY(svgf_quality_read(0, q, &r, s));
                HIP_OK(hipMemcpyAsync(h_one.data(), composed[g][k], N * 12, hipMemcpyDeviceToHost, s));
                HIP_OK(hipStreamSynchronize(s));
                masked_psnr(h_one, h_ref, h_floor, io, count);
                printf("        %-6s %6.2f dB / %.4f [floor %6.2f dB, elsewhere %6.2f dB]\n", filter_name[k], r.psnr_db, r.mean_ssim, io[0], io[1]);
            }
        }
    }
    HIP_OK(hipStreamSynchronize(s));
    for (int g = 0; g < N_DRAW; g++) {
        for (int k = 0; k < N_FILTER; k++) {
            svgf_destroy(ctx_d[g][k]); svgf_destroy(ctx_i[g][k]);
            (void)hipFree(out_d[g][k]); (void)hipFree(out_i[g][k]); (void)hipFree(composed[g][k]);
        }
        (void)hipFree(noisy[g]); (void)hipFree(direct[g]); (void)hipFree(indirect[g]);
    }
    svgf_rough_table_destroy(rough);
    svgf_gloss_table_destroy(table);
    SVGF_OKAY(svgf_scene_destroy(scene));
    (void)hipFree(ref); (void)hipFree(gb); (void)hipFree(gb_ref); (void)hipFree(q); (void)hipStreamDestroy(s);
    return 0;
}

int main(int argc, char **argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 8, W = argc > 2 ? atoi(argv[2]) : 640, H = argc > 3 ? atoi(argv[3]) : 360;
    const int seeds = argc > 4 ? atoi(argv[4]) : 8;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "highlight_scene: no HIP device (the libraries have no CPU path)\n"); return 2; }
    if (frames < 1 || seeds < 1 || svgf_quality_state_bytes(W, H) == 0) { fprintf(stderr, "usage: highlight_scene [frames >= 1] [width] [height] [seeds >= 1]\n"); return 2; }
    if (svgf_highlight_version() != svgf_version() || svgf_rough_version() != svgf_version() || svgf_gloss_version() != svgf_version()) {
        fprintf(stderr, "highlight_scene: the companion libraries and libsvgf_hip.so disagree on the ABI\n");
        return 2;
    }
    static_assert(sizeof(SvgfGBufferTexel) == 52, "13 words per texel");
    HIP_OK(hipSetDevice(0));
    const float alphas[2] = { 0.1f, 0.4f };
    for (int i = 0; i < 2; i++)
        if (leg(alphas[i], frames, W, H, seeds)) return 1;
    return 0;
}
