// examples/resident_scene.cpp — a renderer's loop on a resident scene (include/svgf.h row f14), in C++ through the C ABI.
//
// Once: svgf_scene_create validates the scene (a room of four cubes, a light and a tessellated sphere of 2 * rings * rings
// triangles), builds the BVH over its triangles on the host and uploads everything in one allocation.  Per frame, on one stream and
// without a host wait: svgf_scene_draw (one launch: primary rays, G-buffer, 1-spp colour) and svgf_denoise.  The scene is static;
// the camera moves.  With `compare` != 0 the same loop runs again through svgf_scene_render_mesh, which uploads the scene and tests
// every triangle on every call, and both times per frame are printed.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/resident_scene.cpp -L cuda-path-tracer-denoising_amd -lsvgf_hip \
//         -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/resident_scene
//   examples/resident_scene [frames=60] [width=1920] [height=1080] [rings=64] [compare=1]
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svgf.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); return 1; } } while (0)
#define SVGF_OKAY(x) do { int rc__ = (x); if (rc__ != SVGF_OK) { fprintf(stderr, "%s failed (%d): %s\n", #x, rc__, svgf_last_error(ctx)); return 1; } } while (0)

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
    const int frames = argc > 1 ? atoi(argv[1]) : 60, W = argc > 2 ? atoi(argv[2]) : 1920, H = argc > 3 ? atoi(argv[3]) : 1080;
    const int rings = argc > 4 ? atoi(argv[4]) : 64, compare = argc > 5 ? atoi(argv[5]) : 1;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "resident_scene: no HIP device (the library has no CPU path)\n"); return 2; }
    if (frames < 1 || W <= 0 || H <= 0 || rings < 3 || rings > 700) { fprintf(stderr, "usage: resident_scene [frames >= 1] [width] [height] [rings 3..700] [compare]\n"); return 2; }
    HIP_OK(hipSetDevice(0));

    // the scene: floor, back wall, two side walls, a light under the ceiling; geomIds 0..4, the sphere's triangles get 5
    const std::vector<SvgfSceneGeom> geoms = { box(0, 0, 0, 12, 0.2f, 12, 0.8f, 0.8f, 0.8f, 0), box(0, 5, -6, 12, 10, 0.2f, 0.8f, 0.8f, 0.7f, 0),
                                               box(-6, 5, 0, 0.2f, 10, 12, 0.8f, 0.3f, 0.3f, 0), box(6, 5, 0, 0.2f, 10, 12, 0.3f, 0.8f, 0.3f, 0),
                                               box(0, 9.9f, 0, 3, 0.1f, 3, 1, 1, 1, 5) };
    const float light[3] = { 0.0f, 9.5f, 0.0f }, centre[3] = { 0.0f, 4.0f, 0.0f }, radius = 2.5f, PI = 3.14159265f;
    std::vector<float> tris;        // per triangle 3 x {position, normal, uv}
    auto vertex = [&](int i, int j) {
        const float th = PI * (float)i / (float)rings, ph = 2.0f * PI * (float)j / (float)(2 * rings);
        const float n[3] = { sinf(th) * cosf(ph), cosf(th), sinf(th) * sinf(ph) };
        for (int c = 0; c < 3; c++) tris.push_back(centre[c] + radius * n[c]);
        for (int c = 0; c < 3; c++) tris.push_back(n[c]);
        tris.push_back((float)j / (float)(2 * rings)); tris.push_back((float)i / (float)rings);
    };
    for (int i = 0; i < rings; i++)
        for (int j = 0; j < 2 * rings; j++) {      // counter-clockwise seen from outside: the producer culls back faces
            if (i > 0) { vertex(i, j); vertex(i, j + 1); vertex(i + 1, j); }
            if (i + 1 < rings) { vertex(i + 1, j); vertex(i, j + 1); vertex(i + 1, j + 1); }
        }
    const int n_tris = (int)(tris.size() / 24);
    const std::vector<int> tri_ids((size_t)n_tris, 5);
    std::vector<float> tri_albedo(3 * (size_t)n_tris);
    for (int i = 0; i < n_tris; i++) { tri_albedo[3 * i] = 0.9f; tri_albedo[3 * i + 1] = 0.7f; tri_albedo[3 * i + 2] = 0.2f + 0.6f * (float)(i & 1); }

    svgf_ctx *ctx = nullptr;
    svgf_scene *scene = nullptr;
    const auto b0 = std::chrono::steady_clock::now();
    SVGF_OKAY(svgf_scene_create(0, geoms.data(), (int)geoms.size(), nullptr, tris.data(), tri_ids.data(), tri_albedo.data(), n_tris,
                                nullptr, nullptr, nullptr, 0, /*bp=*/nullptr, &scene));
    const double build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b0).count();
    SvgfSceneInfo info;
    SVGF_OKAY(svgf_scene_info(scene, &info));
    printf("scene: %d primitives, %d triangles, %d textures; BVH %d nodes, %d leaves (<= %d triangles each), depth %d; %.2f MB on the device; "
           "created in %.1f ms\n", info.n_geoms, info.n_tris, info.n_tex, info.n_nodes, info.n_leaves, info.max_leaf_tris, info.depth,
           (double)info.device_bytes / 1e6, build_ms);

    SVGF_OKAY(svgf_create(0, W, H, &ctx));
    const size_t N = (size_t)W * H;
    float *rgb, *out;
    void *gb;
    HIP_OK(hipMalloc((void **)&rgb, N * 12)); HIP_OK(hipMalloc((void **)&out, N * 12)); HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel)));
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1;

    std::vector<float> first(3), last(3);
    for (int pass = 0; pass < (compare ? 2 : 1); pass++) {      // 0: the resident scene; 1: the per-call upload + brute force
        SVGF_OKAY(svgf_reset(ctx));
        const auto t0 = std::chrono::steady_clock::now();
        for (int f = 0; f < frames; f++) {
            SvgfCamera cam;
            SvgfSynthParams sp = { f, 7, 0.6f, 0.02f, { 0.0f, 0.0f } };
            SVGF_OKAY(svgf_synth_camera(f, /*moving=*/1, W, H, &cam, sp.pixel_length));
            if (pass == 0)
                SVGF_OKAY(svgf_scene_draw(scene, rgb, gb, W, H, &cam, &sp, light, s));
            else
                SVGF_OKAY(svgf_scene_render_mesh(0, rgb, gb, W, H, &cam, &sp, geoms.data(), (int)geoms.size(), nullptr, tris.data(), tri_ids.data(),
                                                 tri_albedo.data(), n_tris, nullptr, nullptr, nullptr, 0, light, s));
            SVGF_OKAY(svgf_denoise(ctx, out, rgb, gb, &cam, &p, s));
        }
        SVGF_OKAY(svgf_sync_stream(ctx, s));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::vector<float> &px = pass == 0 ? first : last;
        HIP_OK(hipMemcpy(px.data(), out + 3 * (N / 2 + (size_t)W / 2), 12, hipMemcpyDeviceToHost));
        printf("%s: %d frames of %dx%d, %.3f ms per frame (producer + denoise); centre pixel of the last frame %.6f %.6f %.6f\n",
               pass == 0 ? "svgf_scene_draw       " : "svgf_scene_render_mesh", frames, W, H, ms / frames, px[0], px[1], px[2]);
    }
    // (bit-equal wherever the nearest triangle passes its own gate, include/svgf.h; a filtered pixel mixes a wide neighbourhood)
    for (int c = 0; compare && c < 3; c++)
        if (!(fabsf(first[c] - last[c]) <= 1e-3f * fabsf(last[c]))) { fprintf(stderr, "the two producers disagree\n"); return 1; }

    SVGF_OKAY(svgf_scene_destroy(scene));
    svgf_destroy(ctx);
    hipFree(rgb); hipFree(out); hipFree(gb); hipStreamDestroy(s);
    return 0;
}
