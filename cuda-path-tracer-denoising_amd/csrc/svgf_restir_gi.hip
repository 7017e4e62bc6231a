// svgf_restir_gi.hip — row f28, libsvgf_restir_gi.so: reservoir resampling of the one-bounce indirect term (include/svgf_restir_gi.h
// states the sample, the reservoirs, the hash streams and both launches).  The library reaches the scene through svgf_scene_view alone
// (struct svgf_scene is unknown here) and links against libsvgf_hip.so alone.
//   k_restir_gi_reset          one thread per pixel: H empty, the previous ids -1
//   k_restir_gi_initial        one thread per pixel: the bounce candidates of row f17, the history tap; writes T
//   k_restir_gi_spatial_shade  one thread per pixel: T's neighbours, one visibility ray to a foreign winner, I; writes H and the previous planes
// Workgroups are 256 threads on a 64 x 4 pixel tile, as svgf_restir.hip's.  The sampler (trace_direction, trace_aim) is
// svgf_scene_trace.inc.h's and the walks (scene_nearest, scene_occluded, scene_shadow_sample) svgf_scene_walk.inc.h's, the text the
// draws of rows f16 / f17 compile, on their per-lane stack in LDS (48 KB per block).  A thread writes only its own pixel's records:
// launch 1 reads H and the previous planes and writes T, launch 2 reads T and writes H and the previous planes, so no thread reads what
// another writes in the same launch, nothing passes between workgroups and there are no atomics.  Reservoirs move as four 16-byte words.
// What the pass is apart from its payload - the tile's pixel, the G-buffer reads, the history tap's address, update()'s sums, the state
// behind the handle with its create / read / info / destroy, scene_args - is svgf_reservoir.inc.h, shared with svgf_restir.hip.
// float32, contraction off (build.PATH_RESAMPLERS' row adds -ffp-contract=off; the pragmas say it again where the arithmetic is normative).
#include "svgf_kernels.h"
#include "svgf_temporal.h"      // svgf_lum_strict
#include "../../include/svgf_trace.h"
#include "../../include/svgf_restir_gi.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

namespace {

#include "svgf_scene_trace.inc.h"

#include "svgf_reservoir.inc.h"

struct GiArgs {
    SceneTraceArgs t;           // the scene's arrays, width, height, seed, frame, the light (b.s.light, edge_u, edge_v), ambient, shadow_secondary
    const float *gbuf;          // AoS texels, or null: the planes
    const float *pl_nrm, *pl_pos;
    const int *pl_gid;
    const float *motion;        // or null
    const float *emit;          // geomId -> emittance
    int n_ids;
    float4 *H, *T;
    float *prev_n;
    int *prev_gid;
    int candidates, temporal, neighbours;
    float m_cap, radius, min_dot, jac_max, jac_min;
    float *out_I;
};

struct GiSample { float xs[3], ns[3], L[3], g; };
struct GiReservoir { GiSample s; float M, W, phat, w_sum; bool valid; };

__device__ __forceinline__ GiReservoir gi_empty()
{
    return GiReservoir{ { { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f }, 0.0f }, 0.0f, 0.0f, 0.0f, 0.0f, false };
}

__device__ __forceinline__ GiReservoir gi_load(const float4 *plane, int p)
{
    const float4 a = plane[4 * (size_t)p], b = plane[4 * (size_t)p + 1], c = plane[4 * (size_t)p + 2], d = plane[4 * (size_t)p + 3];
    return GiReservoir{ { { a.x, a.y, a.z }, { b.x, b.y, b.z }, { c.x, c.y, c.z }, d.x }, a.w, b.w, c.w, 0.0f, __float_as_int(d.y) != 0 };
}

__device__ __forceinline__ void gi_store(float4 *plane, int p, const GiReservoir &r)
{
    const bool v = r.valid;
    plane[4 * (size_t)p] = make_float4(v ? r.s.xs[0] : 0.0f, v ? r.s.xs[1] : 0.0f, v ? r.s.xs[2] : 0.0f, r.M);
    plane[4 * (size_t)p + 1] = make_float4(v ? r.s.ns[0] : 0.0f, v ? r.s.ns[1] : 0.0f, v ? r.s.ns[2] : 0.0f, v ? r.W : 0.0f);
    plane[4 * (size_t)p + 2] = make_float4(v ? r.s.L[0] : 0.0f, v ? r.s.L[1] : 0.0f, v ? r.s.L[2] : 0.0f, v ? r.phat : 0.0f);
    plane[4 * (size_t)p + 3] = make_float4(v ? r.s.g : 0.0f, __int_as_float(v ? 1 : 0), 0.0f, 0.0f);
}

// g_p(xs, ns) at the pixel (pos, n)
__device__ __forceinline__ float gi_geometry(const float xs[3], const float ns[3], const float n[3], const float pos[3])
{
#pragma clang fp contract(off)
    float v[3], wd[3];
    for (int c = 0; c < 3; c++) v[c] = xs[c] - pos[c];
    const float dist2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const float dl = sqrtf(dist2);
    for (int c = 0; c < 3; c++) wd[c] = v[c] / dl;
    const float cs = fmaxf((n[0] * wd[0] + n[1] * wd[1]) + n[2] * wd[2], 0.0f);
    const float cphi = fmaxf(-((ns[0] * wd[0] + ns[1] * wd[1]) + ns[2] * wd[2]), 0.0f);
    return (cs * cphi) / dist2;
}

__device__ __forceinline__ bool gi_update(GiReservoir &r, const GiSample &s, float phat, float w, float M_s, float xi)
{
    const bool sel = reservoir_add(r.w_sum, r.M, w, M_s, xi);
    if (sel) { r.s = s; r.phat = phat; r.valid = true; }
    return sel;
}

__device__ __forceinline__ void gi_finish(GiReservoir &r)
{
#pragma clang fp contract(off)
    r.W = (r.valid && r.phat > 0.0f) ? r.w_sum / (r.M * r.phat) : 0.0f;
}

// s = EMPTY; take(s, r, 0), in r's place: M stays, the sample stays iff its weight is > 0
__device__ __forceinline__ void gi_restart(GiReservoir &r)
{
#pragma clang fp contract(off)
    float w = r.valid ? (r.phat * r.W) * r.M : 0.0f;
    w = w > 0.0f ? w : 0.0f;
    r.w_sum = w;
    r.valid = w > 0.0f;
    r.W = 0.0f;
    if (!r.valid) r.phat = 0.0f;
}

// take'(s, r, M', xi): a reservoir of another pixel or frame, its geometry term evaluated at this pixel; true where it was selected
__device__ __forceinline__ bool gi_take_at(const GiArgs &a, GiReservoir &s, const GiReservoir &r, float Mq, float xi, const float n[3], const float pos[3])
{
#pragma clang fp contract(off)
    if (!r.valid) return false;
    const float g = gi_geometry(r.s.xs, r.s.ns, n, pos);
    if (!(r.s.g > 0.0f) || !(g > 0.0f)) return false;
    const float J = g / r.s.g;
    if (!(J >= a.jac_min && J <= a.jac_max)) return false;
    const float phat = svgf_lum_strict(r.s.L[0], r.s.L[1], r.s.L[2]);
    GiSample t = r.s;
    t.g = g;
    return gi_update(s, t, phat, ((phat * r.W) * J) * Mq, Mq, xi);
}

// row f17's bounce sample j = c of pixel p from (pos, n): k_scene_trace's statements between its sampler and its sum, with the hit kept
__device__ __forceinline__ void gi_bounce(const GiArgs &arg, int p, int c, const float n[3], const float pos[3], const float T[3], const float B[3],
                                          float t_lo, int *const stk, GiSample &out)
{
#pragma clang fp contract(off)
    const SceneBvhArgs &b = arg.t.b;
    const SceneArgs &a = b.s;
    const unsigned base = 256u + 16u * (unsigned)c;
    SceneRay r;
    for (int k = 0; k < 3; k++) r.o[k] = pos[k];
    trace_direction(a, p, base, n, T, B, r.d);
    trace_aim(r);
    SceneHit h2;
    scene_primitives_beyond(a, r.o, r.d, t_lo, h2);
    int best2 = -1;
    float bt2 = h2.t_best, bbx2 = 0.0f, bby2 = 0.0f;
    scene_nearest(b, r, stk, t_lo, bt2, best2, bbx2, bby2);
    float pos2[3];
    scene_surface(a, r.o, r.d, h2, best2, bt2, bbx2, bby2, pos2);
    float L = 0.0f;             // per unit of albedo
    if (h2.gid >= 0) {
        if (h2.emit > 0.0f) {
            L = h2.emit;
        } else {
            bool occluded = false;
            if (arg.t.shadow_secondary) {
                for (int k = 0; k < 3; k++) r.o[k] = pos2[k];
                occluded = scene_shadow_sample(b, arg.t.edge_u, arg.t.edge_v, r, pos2, stk, p, base + 8, base + 9);
            }
            L = arg.t.ambient + (occluded ? 0.0f : 1.0f) * scene_direct(a, h2.n, pos2);
        }
    }
    for (int k = 0; k < 3; k++) { out.xs[k] = pos2[k]; out.ns[k] = h2.n[k]; out.L[k] = h2.gid >= 0 ? h2.alb[k] * L : 0.0f; }
    out.g = gi_geometry(out.xs, out.ns, n, pos);
}

// visible(pos, xs): false where an occluder counts between the two
__device__ __forceinline__ bool gi_visible(const SceneBvhArgs &b, const float pos[3], const float xs[3], int *const stk)
{
#pragma clang fp contract(off)
    float q[3];
    for (int c = 0; c < 3; c++) q[c] = xs[c] - pos[c];
    const float dl = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    bool occluded = false;
    if (dl > 0.0f) {
        SceneRay r;
        for (int c = 0; c < 3; c++) { r.o[c] = pos[c]; r.d[c] = q[c] / dl; }
        trace_aim(r);
        const float t_lo = 0x1p-10f * fmaxf(1.0f, fmaxf(fmaxf(fabsf(pos[0]), fabsf(pos[1])), fabsf(pos[2])));
        occluded = scene_occluded(b, r, stk, t_lo, dl - 0x1p-10f * fmaxf(1.0f, dl));
    }
    return !occluded;
}

__global__ __launch_bounds__(256) void k_restir_gi_reset(GiArgs arg)
{
    int x, y;
    const int p = tile_pixel(arg.t.b.s, x, y);
    if (p < 0) return;
    gi_store(arg.H, p, gi_empty());
    arg.prev_gid[p] = -1;
}

__global__ __launch_bounds__(256) void k_restir_gi_initial(GiArgs arg)
{
#pragma clang fp contract(off)
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneArgs &a = arg.t.b.s;
    int x, y;
    const int p = tile_pixel(a, x, y);
    if (p < 0) return;
    int *const stk = stack + threadIdx.x;
    float n[3], pos[3];
    const int gid = read_surface(arg, p, n, pos);
    GiReservoir r = gi_empty();
    if (gid >= 0 && !(id_emittance(arg, gid) > 0.0f)) {
        const unsigned up = (unsigned)p;
        // row f17's frame of n and its t_lo at pos
        const float s = copysignf(1.0f, n[2]), q = -1.0f / (s + n[2]), w = (n[0] * n[1]) * q;
        const float T[3] = { 1.0f + ((s * n[0]) * n[0]) * q, s * w, -(s * n[0]) };
        const float B[3] = { w, s + (n[1] * n[1]) * q, -n[1] };
        const float t_lo = 0x1p-10f * fmaxf(1.0f, fmaxf(fmaxf(fabsf(pos[0]), fabsf(pos[1])), fabsf(pos[2])));
        for (int c = 0; c < arg.candidates; c++) {
            GiSample cand;
            gi_bounce(arg, p, c, n, pos, T, B, t_lo, stk, cand);
            const float phat = svgf_lum_strict(cand.L[0], cand.L[1], cand.L[2]);
            gi_update(r, cand, phat, phat, 1.0f, scene_hash(a.seed, a.frame, up, 8192u + (unsigned)c));
        }
        gi_finish(r);
        gi_restart(r);
        if (arg.temporal && arg.motion) {
            int qp;
            if (history_tap(arg, a, p, gid, n, qp)) {
                const GiReservoir h = gi_load(arg.H, qp);
                gi_take_at(arg, r, h, fminf(h.M, arg.m_cap * r.M), scene_hash(a.seed, a.frame, up, 8224), n, pos);
            }
        }
        gi_finish(r);
    }
    gi_store(arg.T, p, r);
}

__global__ __launch_bounds__(256) void k_restir_gi_spatial_shade(GiArgs arg)
{
#pragma clang fp contract(off)
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneArgs &a = arg.t.b.s;
    int x, y;
    const int p = tile_pixel(a, x, y);
    if (p < 0) return;
    int *const stk = stack + threadIdx.x;
    float n[3], pos[3];
    const int gid = read_surface(arg, p, n, pos);
    GiReservoir s = gi_empty();
    float I[3] = { 0.0f, 0.0f, 0.0f };
    if (gid >= 0 && !(id_emittance(arg, gid) > 0.0f)) {
        const unsigned up = (unsigned)p;
        s = gi_load(arg.T, p);
        gi_restart(s);
        bool foreign = false;
        for (int k = 0; k < arg.neighbours; k++) {
            const unsigned base = 8256u + 4u * (unsigned)k;
            const int ox = (int)floorf(((2.0f * scene_hash(a.seed, a.frame, up, base) - 1.0f) * arg.radius) + 0.5f);
            const int oy = (int)floorf(((2.0f * scene_hash(a.seed, a.frame, up, base + 1) - 1.0f) * arg.radius) + 0.5f);
            const int qx = x + ox, qy = y + oy;
            if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H || (ox == 0 && oy == 0)) continue;
            const int q = qy * a.W + qx;
            float m[3];
            int gq;
            read_normal(arg, q, m, gq);
            if (gq != gid || !((n[0] * m[0] + n[1] * m[1]) + n[2] * m[2] >= arg.min_dot)) continue;
            const GiReservoir t = gi_load(arg.T, q);
            if (gi_take_at(arg, s, t, t.M, scene_hash(a.seed, a.frame, up, base + 2), n, pos)) foreign = true;
        }
        gi_finish(s);
        if (s.valid) {
            float vis = 1.0f;
            if (foreign && s.W > 0.0f && !gi_visible(arg.t.b, pos, s.s.xs, stk)) vis = 0.0f;
            for (int c = 0; c < 3; c++) I[c] = vis * (s.s.L[c] * s.W);
        }
    }
    float *o = arg.out_I + 3 * (size_t)p;
    o[0] = I[0]; o[1] = I[1]; o[2] = I[2];
    gi_store(arg.H, p, s);
    arg.prev_n[3 * (size_t)p] = n[0]; arg.prev_n[3 * (size_t)p + 1] = n[1]; arg.prev_n[3 * (size_t)p + 2] = n[2];
    arg.prev_gid[p] = gid;
}

bool params_ok(const SvgfRestirGIParams *gp)
{
    if (gp->candidates < 1 || gp->candidates > SVGF_RESTIR_GI_MAX_CANDIDATES || (gp->temporal != 0 && gp->temporal != 1)) return false;
    if (!std::isfinite(gp->m_cap) || gp->m_cap < 1.0f || gp->neighbours < 0 || gp->neighbours > SVGF_RESTIR_GI_MAX_NEIGHBOURS) return false;
    if (!std::isfinite(gp->radius) || gp->radius < 1.0f || gp->radius > 65536.0f || !std::isfinite(gp->normal_min_dot)) return false;
    if (!std::isfinite(gp->jacobian_max) || gp->jacobian_max < 1.0f) return false;
    if (!std::isfinite(gp->ambient) || gp->ambient < 0.0f || (gp->shadow_secondary != 0 && gp->shadow_secondary != 1)) return false;
    return true;
}

}  // namespace

struct svgf_restir_gi : ReservoirState {};
static_assert(SVGF_RESTIR_GI_MAX_ID == RESERVOIR_MAX_ID, "the shared create's bound on ids");

extern "C" int svgf_restir_gi_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

extern "C" int svgf_restir_gi_create(const svgf_scene *scene, int width, int height, svgf_restir_gi **out)
{
    return reservoir_state_create(scene, width, height, 64, svgf_restir_gi_reset, out);
}

extern "C" int svgf_restir_gi_reset(svgf_restir_gi *st, void *stream)
{
    if (!st) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(st->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    GiArgs t;
    std::memset(&t, 0, sizeof(t));
    t.t.b.s.W = st->width; t.t.b.s.H = st->height;
    t.H = st->H; t.prev_gid = st->prev_gid;
    hipLaunchKernelGGL(k_restir_gi_reset, tile_grid(st->width, st->height), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_restir_gi_frame(svgf_restir_gi *st, const SvgfSceneLight *light, const void *gbuffer_dev, const SvgfPlanarGBuffer *planes,
                                    const void *motion_prev_coord_dev, const SvgfRestirGIParams *gp, const SvgfSynthParams *sp, void *out_I_dev,
                                    void *stream)
{
    if (!st || !light || !gp || !sp || !out_I_dev) return SVGF_ERR_INVALID_ARG;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(light->centre[c]) || !std::isfinite(light->edge_u[c]) || !std::isfinite(light->edge_v[c])) return SVGF_ERR_INVALID_ARG;
    if ((gbuffer_dev != nullptr) == (planes != nullptr)) return SVGF_ERR_INVALID_ARG;
    if (!gbuffer_dev && (!planes->normal || !planes->position || !planes->geom_id)) return SVGF_ERR_INVALID_ARG;
    if (!params_ok(gp)) return SVGF_ERR_INVALID_ARG;
    GiArgs t;
    std::memset(&t, 0, sizeof(t));
    int device = 0;
    const int rc = scene_args(t.t.b, st->scene, device);
    if (rc != SVGF_OK) return rc;
    if (st->device != device) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    SceneArgs &a = t.t.b.s;
    a.W = st->width; a.H = st->height; a.seed = sp->seed; a.frame = sp->frame;
    for (int c = 0; c < 3; c++) { a.light[c] = light->centre[c]; t.t.edge_u[c] = light->edge_u[c]; t.t.edge_v[c] = light->edge_v[c]; }
    t.t.ambient = gp->ambient; t.t.shadow_secondary = gp->shadow_secondary;
    t.gbuf = static_cast<const float *>(gbuffer_dev);
    t.pl_nrm = planes ? planes->normal : nullptr; t.pl_pos = planes ? planes->position : nullptr; t.pl_gid = planes ? planes->geom_id : nullptr;
    t.motion = static_cast<const float *>(motion_prev_coord_dev);
    t.emit = st->emit; t.n_ids = st->n_ids;
    t.H = st->H; t.T = st->T; t.prev_n = st->prev_n; t.prev_gid = st->prev_gid;
    t.candidates = gp->candidates; t.temporal = gp->temporal; t.neighbours = gp->neighbours;
    t.m_cap = gp->m_cap; t.radius = gp->radius; t.min_dot = gp->normal_min_dot;
    t.jac_max = gp->jacobian_max; t.jac_min = 1.0f / gp->jacobian_max;
    t.out_I = static_cast<float *>(out_I_dev);
    const dim3 grid = tile_grid(st->width, st->height);
    hipLaunchKernelGGL(k_restir_gi_initial, grid, dim3(256), 0, static_cast<hipStream_t>(stream), t);
    hipLaunchKernelGGL(k_restir_gi_spatial_shade, grid, dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_restir_gi_info(const svgf_restir_gi *st, SvgfRestirGIInfo *out) { return reservoir_state_info(st, out); }

extern "C" int svgf_restir_gi_read(const svgf_restir_gi *st, int which, void *host_dst, unsigned long long host_bytes)
{
    return reservoir_state_read(st, which, host_dst, host_bytes);
}

extern "C" void svgf_restir_gi_destroy(svgf_restir_gi *st) { reservoir_state_destroy(st); }
