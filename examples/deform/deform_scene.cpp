// examples/deform/deform_scene.cpp — a renderer's loop on a DEFORMING resident scene (include/svgf_deform.h, row f26), in C++ through the C ABI.
//
// Once: svgf_scene_create (row f15's room - four cubes, a light and a block - and a tube of triangles, object 6, that stands in it),
// svgf_scene_enable_pose, svgf_deform_create (two bones: the lower third of the tube follows bone 0, the upper third bone 1, the
// weights cross over in between), svgf_sah_create + svgf_sah_attach.  Per frame, on one stream and without a host wait: the pose
// table (identity: the skinned object's id stands outside it), the bone table (bone 1 turns about the tube's middle),
// svgf_scene_pose, svgf_deform_apply, svgf_sah_build, svgf_scene_draw, svgf_deform_prev_positions, svgf_motion_reproject,
// svgf_denoise_motion.  Beside it the same frames run through svgf_denoise, whose camera path looks every pixel's history up where
// the pixel is now.  Both print the share of the tube's pixels that kept their history (length >= 2) after the last frame.
//
//   hipcc --offload-arch=gfx950 -O2 -I include examples/deform/deform_scene.cpp -L cuda-path-tracer-denoising_amd -lsvgf_deform -lsvgf_sah \
//         -lsvgf_hip -Wl,-rpath,$PWD/cuda-path-tracer-denoising_amd -o examples/deform/deform_scene
//   examples/deform/deform_scene [frames=6] [width=640] [height=360] [segments=32] [degrees per frame=4]
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "svgf.h"
#include "svgf_deform.h"
#include "svgf_sah.h"
#include "svgf_scene_write.h"

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
    const int segments = argc > 4 ? atoi(argv[4]) : 32;
    const float step_deg = argc > 5 ? (float)atof(argv[5]) : 4.0f;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { fprintf(stderr, "deform_scene: no HIP device (the library has no CPU path)\n"); return 2; }
    if (frames < 2 || W <= 0 || H <= 0 || segments < 3 || segments > 500) { fprintf(stderr, "usage: deform_scene [frames >= 2] [width] [height] [segments 3..500] [degrees]\n"); return 2; }
    HIP_OK(hipSetDevice(0));

    // objects 0..5: floor, back wall, side walls, light, block (posed by the identity here); 6: the tube - OUTSIDE the pose table
    const int TUBE = 6, N_POSED = 6, N_BONES = 2;
    const std::vector<SvgfSceneGeom> geoms = { box(0, 0, 0, 12, 0.2f, 12, 0.8f, 0.8f, 0.8f, 0), box(0, 5, -6, 12, 10, 0.2f, 0.8f, 0.8f, 0.7f, 0),
                                               box(-6, 5, 0, 0.2f, 10, 12, 0.8f, 0.3f, 0.3f, 0), box(6, 5, 0, 0.2f, 10, 12, 0.3f, 0.8f, 0.3f, 0),
                                               box(0, 9.9f, 0, 3, 0.1f, 3, 1, 1, 1, 5), box(-2.5f, 1.1f, 0, 2, 2, 2, 0.3f, 0.4f, 0.9f, 0) };
    const float light[3] = { 0.0f, 9.5f, 0.0f }, base[3] = { 1.5f, 0.1f, 3.0f }, length = 5.0f, radius = 0.5f, PI = 3.14159265f;
    const int sides = 2 * segments;
    std::vector<float> tris, weight;        // per triangle 3 x {position, normal, uv}; per corner four weights
    std::vector<unsigned short> bone;
    auto vertex = [&](int i, int j) {
        const float a = 2.0f * PI * (float)(i % sides) / (float)sides, h = (float)j / (float)segments, n[3] = { cosf(a), 0.0f, sinf(a) };
        for (int c = 0; c < 3; c++) tris.push_back(base[c] + radius * n[c] + (c == 1 ? length * h : 0.0f));
        for (int c = 0; c < 3; c++) tris.push_back(n[c]);
        tris.push_back((float)i / (float)sides); tris.push_back(h);
        const float w1 = fminf(fmaxf((h - 1.0f / 3.0f) * 3.0f, 0.0f), 1.0f);
        const float w[4] = { 1.0f - w1, w1, 0.0f, 0.0f };
        const unsigned short b[4] = { 0, 1, 0, 0 };
        for (int k = 0; k < 4; k++) { weight.push_back(w[k]); bone.push_back(b[k]); }
    };
    for (int j = 0; j < segments; j++)
        for (int i = 0; i < sides; i++) {         // counter-clockwise seen from outside: the producer culls back faces
            vertex(i, j); vertex(i, j + 1); vertex(i + 1, j);
            vertex(i + 1, j); vertex(i, j + 1); vertex(i + 1, j + 1);
        }
    const int n_tris = (int)(tris.size() / 24);
    const std::vector<int> tri_ids((size_t)n_tris, TUBE);
    std::vector<int> tri_index((size_t)n_tris);
    std::vector<float> tri_albedo(3 * (size_t)n_tris);
    for (int i = 0; i < n_tris; i++) { tri_index[i] = i; tri_albedo[3 * i] = 0.9f; tri_albedo[3 * i + 1] = 0.7f; tri_albedo[3 * i + 2] = 0.2f + 0.6f * (float)((i / 2) & 1); }

    svgf_ctx *ctx = nullptr;
    svgf_scene *scene = nullptr;
    svgf_deform *rig = nullptr;
    svgf_sah *tree = nullptr;
    SVGF_OKAY(svgf_scene_create(0, geoms.data(), (int)geoms.size(), nullptr, tris.data(), tri_ids.data(), tri_albedo.data(), n_tris,
                                nullptr, nullptr, nullptr, 0, /*bp=*/nullptr, &scene));
    SVGF_OKAY(svgf_scene_enable_pose(scene, N_POSED));
    SVGF_OKAY(svgf_deform_create(scene, tri_index.data(), n_tris, bone.data(), weight.data(), N_BONES, &rig));
    SVGF_OKAY(svgf_sah_create(scene, nullptr, &tree));
    SVGF_OKAY(svgf_sah_attach(tree, scene));
    SvgfDeformInfo di;
    SvgfSahInfo si;
    SVGF_OKAY(svgf_deform_info(rig, &di));
    SVGF_OKAY(svgf_sah_info(tree, &si));
    printf("scene: %d primitives, %d triangles, %d of them skinned by %d bones (%.2f MB); SAH build: %d launches per frame\n", (int)geoms.size(), n_tris,
           di.n_skinned, di.n_bones, (double)di.device_bytes / 1e6, si.launches);

    SVGF_OKAY(svgf_create(0, W, H, &ctx));
    const size_t N = (size_t)W * H;
    float *rgb, *out, *prev_pos, *motion;
    int *prev_id;
    void *gb;
    SvgfScenePose *tables_dev, *tables_host;        // per frame: N_POSED pose records, then N_BONES bone records; none is overwritten in flight
    const size_t per_frame = N_POSED + N_BONES;
    HIP_OK(hipMalloc((void **)&rgb, N * 12)); HIP_OK(hipMalloc((void **)&out, N * 12)); HIP_OK(hipMalloc(&gb, N * sizeof(SvgfGBufferTexel)));
    HIP_OK(hipMalloc((void **)&prev_pos, N * 12)); HIP_OK(hipMalloc((void **)&prev_id, N * 4)); HIP_OK(hipMalloc((void **)&motion, N * 8));
    HIP_OK(hipMalloc((void **)&tables_dev, sizeof(SvgfScenePose) * per_frame * (size_t)frames));
    HIP_OK(hipHostMalloc((void **)&tables_host, sizeof(SvgfScenePose) * per_frame * (size_t)frames, hipHostMallocDefault));
    hipStream_t s;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    SvgfParams p;
    svgf_params_default(&p);
    p.temporal_enable = 1; p.spatial_enable = 1;
    SvgfCamera cam;
    float pixel_length[2];
    SVGF_OKAY(svgf_synth_camera(0, /*moving=*/0, W, H, &cam, pixel_length));
    p.reproj_scale[0] = pixel_length[0] * (float)W / 2.0f; p.reproj_scale[1] = pixel_length[1] * (float)H / 2.0f;

    const float y_axis[3] = { 0, 1, 0 }, z_axis[3] = { 0, 0, 1 }, zero[3] = { 0, 0, 0 }, joint[3] = { base[0], base[1] + 0.5f * length, base[2] };
    std::vector<SvgfGBufferTexel> texels(N);
    std::vector<int> hlen(N);
    for (int pass = 0; pass < 2; pass++) {          // 0: with the previous-position plane; 1: svgf_denoise's camera path
        SVGF_OKAY(svgf_reset(ctx));
        const auto t0 = std::chrono::steady_clock::now();
        for (int f = 0; f < frames; f++) {
            SvgfScenePose *table = tables_host + (size_t)f * per_frame, *table_dev = tables_dev + (size_t)f * per_frame;
            for (size_t k = 0; k < per_frame; k++) SVGF_OKAY(svgf_pose_rigid(y_axis, 0.0f, zero, zero, &table[k]));        // identity
            SVGF_OKAY(svgf_pose_rigid(z_axis, step_deg * PI / 180.0f * (float)f, joint, zero, &table[N_POSED + 1]));         // bone 1 bends the tube
            HIP_OK(hipMemcpyAsync(table_dev, table, sizeof(SvgfScenePose) * per_frame, hipMemcpyHostToDevice, s));
            SvgfSynthParams sp = { f, 7, 0.6f, 0.02f, { pixel_length[0], pixel_length[1] } };
            SVGF_OKAY(svgf_scene_pose(scene, table_dev, N_POSED, nullptr, s));
            SVGF_OKAY(svgf_deform_apply(rig, table_dev + N_POSED, N_BONES, s));
            SVGF_OKAY(svgf_sah_build(tree, s));
            SVGF_OKAY(svgf_scene_draw(scene, rgb, gb, W, H, &cam, &sp, light, s));
            if (pass == 0) {
                SVGF_OKAY(svgf_deform_prev_positions(rig, prev_pos, prev_id, W, H, &cam, pixel_length, s));
                SVGF_OKAY(svgf_motion_reproject(0, motion, SVGF_MOTION_PREV_COORD_F32, nullptr, prev_pos, prev_id, W, H, &cam, p.reproj_scale, nullptr, 0, s));
                SVGF_OKAY(svgf_denoise_motion(ctx, out, rgb, gb, motion, SVGF_MOTION_PREV_COORD_F32, &cam, &p, s));
            } else {
                SVGF_OKAY(svgf_denoise(ctx, out, rgb, gb, &cam, &p, s));
            }
        }
        SVGF_OKAY(svgf_sync_stream(ctx, s));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        HIP_OK(hipMemcpy(texels.data(), gb, N * sizeof(SvgfGBufferTexel), hipMemcpyDeviceToHost));
        SVGF_OKAY(svgf_read_state(ctx, SVGF_STATE_HISTORY_LENGTH, hlen.data(), N * sizeof(int)));
        size_t on_tube = 0, kept = 0;
        for (size_t i = 0; i < N; i++)
            if (texels[i].geomId == TUBE) { on_tube++; kept += hlen[i] >= 2; }
        printf("%s: %d frames of %dx%d, %.3f ms per frame; %zu pixels on the tube, %.1f %% kept their history\n",
               pass == 0 ? "svgf_denoise_motion with the previous-position plane" : "svgf_denoise, the camera path                       ", frames, W, H,
               ms / frames, on_tube, on_tube ? 100.0 * (double)kept / (double)on_tube : 0.0);
        // back to the rest pose with prev == cur, so that the second pass starts where the first did
        for (int k = 0; k < 2; k++) SVGF_OKAY(svgf_deform_apply(rig, tables_dev + N_POSED, N_BONES, s));
        SVGF_OKAY(svgf_sync_stream(ctx, s));
    }

    SVGF_OKAY(svgf_scene_adopt_tree(scene, nullptr, nullptr, 0, 0, 0));
    svgf_sah_destroy(tree);
    svgf_deform_destroy(rig);
    SVGF_OKAY(svgf_scene_destroy(scene));
    svgf_destroy(ctx);
    hipFree(rgb); hipFree(out); hipFree(gb); hipFree(prev_pos); hipFree(prev_id); hipFree(motion); hipFree(tables_dev); hipHostFree(tables_host);
    hipStreamDestroy(s);
    return 0;
}
