// examples/animated_scene.cpp — a renderer's loop on an ANIMATED resident scene (include/svgf.h row f15), in C++ through the C ABI.
//
// Once: svgf_scene_create (a room of four cubes and a light, a block - a cube primitive, object 5 - and a tessellated sphere,
// object 6), svgf_scene_enable_pose.  Per frame, on one stream and without a host wait: fill the pose table (the block turns 9
// degrees about y and slides in x per frame, the sphere bobs), svgf_scene_pose with a motion table, svgf_scene_draw, svgf_denoise
// with svgf_set_object_motion pointing at that table.  The loop runs twice, with the table set and without, and prints the share of
// the block's pixels that kept their history (length >= 2) after the last frame.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/animated_scene.cpp -L cuda-path-tracer-denoising_amd -lsvgf_hip \
//         -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/animated_scene
//   examples/animated_scene [frames=6] [width=640] [height=360] [rings=32]
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
    const int frames = argc > 1 ? atoi(argv[1]) : 6, W = argc > 2 ? atoi(argv[2]) : 640, H = argc > 3 ? atoi(argv[3]) : 360;
    const int rings = argc > 4 ? atoi(argv[4]) : 32;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "animated_scene: no HIP device (the library has no CPU path)\n"); return 2; }
    if (frames < 2 || W <= 0 || H <= 0 || rings < 3 || rings > 700) { fprintf(stderr, "usage: animated_scene [frames >= 2] [width] [height] [rings 3..700]\n"); return 2; }
    HIP_OK(hipSetDevice(0));

    // objects 0..4: floor, back wall, side walls, light (never posed: identity rows); 5: the block; 6: the sphere's triangles
    const int BLOCK = 5, SPHERE = 6, N_OBJECTS = 7;
    const float block_at[3] = { -2.5f, 1.1f, 0.0f };
    const std::vector<SvgfSceneGeom> geoms = { box(0, 0, 0, 12, 0.2f, 12, 0.8f, 0.8f, 0.8f, 0), box(0, 5, -6, 12, 10, 0.2f, 0.8f, 0.8f, 0.7f, 0),
                                               box(-6, 5, 0, 0.2f, 10, 12, 0.8f, 0.3f, 0.3f, 0), box(6, 5, 0, 0.2f, 10, 12, 0.3f, 0.8f, 0.3f, 0),
                                               box(0, 9.9f, 0, 3, 0.1f, 3, 1, 1, 1, 5),
                                               box(block_at[0], block_at[1], block_at[2], 2, 2, 2, 0.3f, 0.4f, 0.9f, 0) };
    const float light[3] = { 0.0f, 9.5f, 0.0f }, centre[3] = { 2.5f, 4.0f, -1.0f }, radius = 1.5f, PI = 3.14159265f;
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
    const std::vector<int> tri_ids((size_t)n_tris, SPHERE);
    std::vector<float> tri_albedo(3 * (size_t)n_tris);
    for (int i = 0; i < n_tris; i++) { tri_albedo[3 * i] = 0.9f; tri_albedo[3 * i + 1] = 0.7f; tri_albedo[3 * i + 2] = 0.2f + 0.6f * (float)(i & 1); }

    svgf_ctx *ctx = nullptr;
    svgf_scene *scene = nullptr;
    SVGF_OKAY(svgf_scene_create(0, geoms.data(), (int)geoms.size(), nullptr, tris.data(), tri_ids.data(), tri_albedo.data(), n_tris,
                                nullptr, nullptr, nullptr, 0, /*bp=*/nullptr, &scene));
    SVGF_OKAY(svgf_scene_enable_pose(scene, N_OBJECTS));
    SvgfSceneInfo info;
    SVGF_OKAY(svgf_scene_info(scene, &info));
    printf("scene: %d primitives, %d triangles; BVH %d nodes, depth %d; %d posed objects; %.2f MB on the device\n", info.n_geoms, info.n_tris,
           info.n_nodes, info.depth, N_OBJECTS, (double)info.device_bytes / 1e6);

    SVGF_OKAY(svgf_create(0, W, H, &ctx));
    const size_t N = (size_t)W * H;
    float *rgb, *out, *motion;
    void *gb;
    SvgfScenePose *pose_dev, *pose_host;
    HIP_OK(hipMalloc((void **)&rgb, N * 12)); HIP_OK(hipMalloc((void **)&out, N * 12)); HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc((void **)&motion, sizeof(float) * 12 * N_OBJECTS));
    HIP_OK(hipMalloc((void **)&pose_dev, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames));     // one table per frame: none is overwritten in flight
    HIP_OK(hipHostMalloc((void **)&pose_host, sizeof(SvgfScenePose) * N_OBJECTS * (size_t)frames, hipHostMallocDefault));
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1;
    SvgfCamera cam;
    float pixel_length[2];
    SVGF_OKAY(svgf_synth_camera(0, /*moving=*/0, W, H, &cam, pixel_length));
    // the exact reprojection at any aspect (SvgfParams::reproj_scale): without it a frame that is not square loses its history
    p.reproj_scale[0] = pixel_length[0] * (float)W / 2.0f; p.reproj_scale[1] = pixel_length[1] * (float)H / 2.0f;

    const float y_axis[3] = { 0, 1, 0 }, zero[3] = { 0, 0, 0 };
    std::vector<SvgfGBufferTexel> texels(N);
    std::vector<int> hlen(N);
    for (int pass = 0; pass < 2; pass++) {          // 0: with the motion table; 1: without
        SVGF_OKAY(svgf_reset(ctx));
        SVGF_OKAY(svgf_set_object_motion(ctx, pass == 0 ? motion : nullptr, pass == 0 ? N_OBJECTS : 0));
        const auto t0 = std::chrono::steady_clock::now();
        for (int f = 0; f < frames; f++) {
            SvgfScenePose *table = pose_host + (size_t)f * N_OBJECTS;
            for (int k = 0; k < N_OBJECTS; k++) SVGF_OKAY(svgf_pose_rigid(y_axis, 0.0f, zero, zero, &table[k]));        // identity
            const float slide[3] = { 0.25f * (float)f, 0, 0 }, bob[3] = { 0, 0.3f * sinf(0.5f * (float)f), 0 };
            SVGF_OKAY(svgf_pose_rigid(y_axis, 9.0f * PI / 180.0f * (float)f, block_at, slide, &table[BLOCK]));
            SVGF_OKAY(svgf_pose_rigid(y_axis, 0.0f, zero, bob, &table[SPHERE]));
            HIP_OK(hipMemcpyAsync(pose_dev + (size_t)f * N_OBJECTS, table, sizeof(SvgfScenePose) * N_OBJECTS, hipMemcpyHostToDevice, s));
            SvgfSynthParams sp = { f, 7, 0.6f, 0.02f, { pixel_length[0], pixel_length[1] } };
            SVGF_OKAY(svgf_scene_pose(scene, pose_dev + (size_t)f * N_OBJECTS, N_OBJECTS, motion, s));
            SVGF_OKAY(svgf_scene_draw(scene, rgb, gb, W, H, &cam, &sp, light, s));
            SVGF_OKAY(svgf_denoise(ctx, out, rgb, gb, &cam, &p, s));
        }
        SVGF_OKAY(svgf_sync_stream(ctx, s));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        HIP_OK(hipMemcpy(texels.data(), gb, N * sizeof(SvgfGBufferTexel), hipMemcpyDeviceToHost));
        SVGF_OKAY(svgf_read_state(ctx, SVGF_STATE_HISTORY_LENGTH, hlen.data(), N * sizeof(int)));
        size_t on_block = 0, kept = 0;
        for (size_t i = 0; i < N; i++)
            if (texels[i].geomId == BLOCK) { on_block++; kept += hlen[i] >= 2; }
        printf("%s: %d frames of %dx%d, %.3f ms per frame (pose + draw + denoise); %zu pixels on the block, %.1f %% kept their history\n",
               pass == 0 ? "with the motion table   " : "without the motion table", frames, W, H, ms / frames, on_block,
               on_block ? 100.0 * (double)kept / (double)on_block : 0.0);
        // back to the rest pose and an identity `held`, so that the second pass starts where the first did
        SVGF_OKAY(svgf_scene_pose(scene, pose_dev, N_OBJECTS, nullptr, s));
        SVGF_OKAY(svgf_sync_stream(ctx, s));
    }

    SVGF_OKAY(svgf_scene_destroy(scene));
    svgf_destroy(ctx);
    hipFree(rgb); hipFree(out); hipFree(gb); hipFree(motion); hipFree(pose_dev); hipHostFree(pose_host); hipStreamDestroy(s);
    return 0;
}
