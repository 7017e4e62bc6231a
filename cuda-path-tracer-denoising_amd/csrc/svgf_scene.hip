// svgf_scene.hip — device-side producer driven by a list of scene primitives (on top of f1).
//
// The reference's scenes are lists of transformed unit cubes / unit spheres (and triangle meshes, which belong to the
// out-of-scope path tracer) read from a text format (src/scene.cpp); its first bounce fills the G-buffer from them
// (src/pathtrace.cu:317-323, intersection conventions of src/intersections.h:50,104: cube [-0.5,0.5]^3 and sphere
// r = 0.5 in object space, t measured in world space).  The host side (cuda-path-tracer-denoising_amd/scene.py) parses
// the text and builds the SvgfSceneGeom records; this kernel casts the primary rays against them and writes the
// denoiser's inputs with the same shading / noise stub as svgf_synth.hip.  Oracle: scene.render_scene (numpy) for the primitives,
// tests/scene_model.py for every branch (geom_ids, triangles, textures, colour), mirrored here operation for operation in fp32
// with contraction off.
#include "svgf_kernels.h"
#include "../../include/svgf.h"

#include <hip/hip_runtime.h>

#include <cstring>

namespace {

#include "svgf_scene_pixel.inc.h"

__global__ __launch_bounds__(256) void k_scene_frame(SceneArgs a)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.W * a.H) return;
    float o[3], d[3];
    scene_ray(a, p % a.W, p / a.W, o, d);
    SceneHit h;
    scene_primitives(a, o, d, h);
    // Triangle meshes: the nearest triangle of the whole scene (the reference walks one BVH over all of them and keeps the hit
    // if it belongs to the mesh being tested, src/pathtrace.cu:241-252)
    int best = -1;
    float bt = h.t_best, bbx = 0.0f, bby = 0.0f;
    for (int i = 0; i < a.n_tris; i++) {
        float bx, by, t;
        if (!scene_tri_test(a.tris + 24 * (size_t)i, o, d, bx, by, t)) continue;
        if (t > 0.0f && t < bt) { bt = t; best = i; bbx = bx; bby = by; }
    }
    scene_finish(a, p, o, d, h, best, bt, bbx, bby);
}

}  // namespace

static int scene_render_impl(int device, void *out_rgb_dev, void *out_gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height,
                             const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneGeom *geoms, int n_geoms,
                             const int *geom_ids, const float *tris, const int *tri_ids, const float *tri_albedo, int n_tris,
                             const int *tri_tex, const int *tex_desc, const unsigned char *tex_data, int n_tex,
                             const float light[3], void *stream)
{
    if (!out_rgb_dev || (!out_gbuffer_dev && !planes) || !cam || !sp || !light || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if (!out_gbuffer_dev && (!planes->normal || !planes->position || !planes->geom_id)) return SVGF_ERR_INVALID_ARG;
    size_t n_texbytes = 0;
    if (scene_check_inputs(geoms, n_geoms, tris, tri_ids, tri_albedo, n_tris, tri_tex, tex_desc, tex_data, n_tex, &n_texbytes) != SVGF_OK) return SVGF_ERR_INVALID_ARG;
    const size_t b_tex = n_texbytes > 16 ? n_texbytes : 16;     // the allocation is padded, the copy is not
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one staging allocation: [geoms | geom_ids | tris | tri_ids | tri_albedo | tri_tex | tex_desc | tex]
    const size_t b_g = sizeof(SvgfSceneGeom) * (size_t)(n_geoms > 0 ? n_geoms : 1), b_gi = sizeof(int) * (size_t)(n_geoms > 0 ? n_geoms : 1);
    const size_t b_t = sizeof(float) * 24 * (size_t)(n_tris > 0 ? n_tris : 1), b_ti = sizeof(int) * (size_t)(n_tris > 0 ? n_tris : 1);
    const size_t b_ta = sizeof(float) * 3 * (size_t)(n_tris > 0 ? n_tris : 1);
    const size_t b_tt = b_ti, b_td = sizeof(int) * 3 * (size_t)(n_tex > 0 ? n_tex : 1);
    const size_t o_tt = b_g + b_gi + b_t + b_ti + b_ta, o_td = o_tt + b_tt, o_tex = (o_td + b_td + 15) & ~(size_t)15;
    // The uploads run on a library-owned stream `up`, not on the caller's: the host waits for THEM (the arrays are the caller's,
    // usually pageable, often temporaries of a binding, and must have been read when this function returns) without waiting for
    // whatever else is queued on `s` — the previous frame's whole denoise, typically — and without a host synchronisation on a
    // stream that may be under capture.  The kernel and the release of the staging memory stay asynchronous on `s`.
    // (one per device, created on first use under a lock and kept for the life of the process; a creation that fails is not
    // remembered — the next call tries again — and a device index outside the table is refused rather than folded onto slot 0,
    // whose stream belongs to another device)
    static hipStream_t up_streams[64];
    static std::mutex up_mutex;
    if (device < 0 || device >= 64) return SVGF_ERR_UNSUPPORTED;
    hipStream_t up = nullptr;
    {
        std::lock_guard<std::mutex> lock(up_mutex);
        if (!up_streams[device] && hipStreamCreateWithFlags(&up_streams[device], hipStreamNonBlocking) != hipSuccess) up_streams[device] = nullptr;
        up = up_streams[device];
    }
    if (!up) return SVGF_ERR_HIP;
    char *d = nullptr;
    if (hipMallocAsync(reinterpret_cast<void **>(&d), o_tex + b_tex, up) != hipSuccess) return SVGF_ERR_OOM;
    bool ok = true;
    if (n_geoms > 0) ok = ok && hipMemcpyAsync(d, geoms, sizeof(SvgfSceneGeom) * (size_t)n_geoms, hipMemcpyHostToDevice, up) == hipSuccess;
    if (n_geoms > 0 && geom_ids) ok = ok && hipMemcpyAsync(d + b_g, geom_ids, sizeof(int) * (size_t)n_geoms, hipMemcpyHostToDevice, up) == hipSuccess;
    if (n_tris > 0) {
        ok = ok && hipMemcpyAsync(d + b_g + b_gi, tris, sizeof(float) * 24 * (size_t)n_tris, hipMemcpyHostToDevice, up) == hipSuccess;
        ok = ok && hipMemcpyAsync(d + b_g + b_gi + b_t, tri_ids, sizeof(int) * (size_t)n_tris, hipMemcpyHostToDevice, up) == hipSuccess;
        ok = ok && hipMemcpyAsync(d + b_g + b_gi + b_t + b_ti, tri_albedo, sizeof(float) * 3 * (size_t)n_tris, hipMemcpyHostToDevice, up) == hipSuccess;
    }
    if (n_tex > 0) {
        ok = ok && hipMemcpyAsync(d + o_tt, tri_tex, sizeof(int) * (size_t)n_tris, hipMemcpyHostToDevice, up) == hipSuccess;
        ok = ok && hipMemcpyAsync(d + o_td, tex_desc, sizeof(int) * 3 * (size_t)n_tex, hipMemcpyHostToDevice, up) == hipSuccess;
        ok = ok && hipMemcpyAsync(d + o_tex, tex_data, n_texbytes, hipMemcpyHostToDevice, up) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(up) == hipSuccess;      // allocation and uploads complete: `s` may use the memory without an event
    if (!ok) { (void)hipFreeAsync(d, up); return SVGF_ERR_HIP; }
    SceneArgs a;
    scene_frame_args(a, width, height, cam, sp, light);
    a.n_geoms = n_geoms;
    a.geoms = reinterpret_cast<const SvgfSceneGeom *>(d);
    a.geom_ids = (n_geoms > 0 && geom_ids) ? reinterpret_cast<const int *>(d + b_g) : nullptr;
    a.n_tris = n_tris;
    a.tris = reinterpret_cast<const float *>(d + b_g + b_gi);
    a.tri_ids = reinterpret_cast<const int *>(d + b_g + b_gi + b_t);
    a.tri_albedo = reinterpret_cast<const float *>(d + b_g + b_gi + b_t + b_ti);
    a.tri_tex = n_tex > 0 ? reinterpret_cast<const int *>(d + o_tt) : nullptr;
    a.tex_desc = reinterpret_cast<const int *>(d + o_td);
    a.tex = reinterpret_cast<const unsigned char *>(d + o_tex);
    a.out_rgb = static_cast<float *>(out_rgb_dev);
    a.out_gbuf = static_cast<float *>(out_gbuffer_dev);
    a.pl_nrm = planes ? planes->normal : nullptr; a.pl_pos = planes ? planes->position : nullptr;
    a.pl_alb = planes ? planes->albedo : nullptr; a.pl_gid = planes ? planes->geom_id : nullptr;
    const int n = width * height;
    hipLaunchKernelGGL(k_scene_frame, dim3((n + 255) / 256), dim3(256), 0, s, a);
    const hipError_t e = hipGetLastError();
    (void)hipFreeAsync(d, s);
    return e == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_scene_render_mesh(int device, void *out_rgb_dev, void *out_gbuffer_dev, int width, int height,
                                      const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneGeom *geoms, int n_geoms,
                                      const int *geom_ids, const float *tris, const int *tri_ids, const float *tri_albedo, int n_tris,
                                      const int *tri_tex, const int *tex_desc, const unsigned char *tex_data, int n_tex,
                                      const float light[3], void *stream)
{
    if (!out_gbuffer_dev) return SVGF_ERR_INVALID_ARG;
    return scene_render_impl(device, out_rgb_dev, out_gbuffer_dev, nullptr, width, height, cam, sp, geoms, n_geoms, geom_ids, tris, tri_ids,
                             tri_albedo, n_tris, tri_tex, tex_desc, tex_data, n_tex, light, stream);
}

// the same frame written into the planes of svgf_planar_gbuffer (the repack fused into the producer)
extern "C" int svgf_scene_render_mesh_planar(int device, void *out_rgb_dev, const SvgfPlanarGBuffer *out_planes, int width, int height,
                                             const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneGeom *geoms, int n_geoms,
                                             const int *geom_ids, const float *tris, const int *tri_ids, const float *tri_albedo, int n_tris,
                                             const int *tri_tex, const int *tex_desc, const unsigned char *tex_data, int n_tex,
                                             const float light[3], void *stream)
{
    if (!out_planes) return SVGF_ERR_INVALID_ARG;
    return scene_render_impl(device, out_rgb_dev, nullptr, out_planes, width, height, cam, sp, geoms, n_geoms, geom_ids, tris, tri_ids,
                             tri_albedo, n_tris, tri_tex, tex_desc, tex_data, n_tex, light, stream);
}

extern "C" int svgf_scene_render(int device, void *out_rgb_dev, void *out_gbuffer_dev, int width, int height,
                                 const SvgfCamera *cam, const SvgfSynthParams *sp, const SvgfSceneGeom *geoms, int n_geoms,
                                 const float light[3], void *stream)
{
    if (!geoms) return SVGF_ERR_INVALID_ARG;
    return svgf_scene_render_mesh(device, out_rgb_dev, out_gbuffer_dev, width, height, cam, sp, geoms, n_geoms, nullptr, nullptr, nullptr,
                                  nullptr, 0, nullptr, nullptr, nullptr, 0, light, stream);
}
