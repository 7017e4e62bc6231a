// svgf_restir.hip — row f27, libsvgf_restir.so: many-light direct lighting by reservoir resampling (include/svgf_restir.h states the
// light table, the reservoirs, the hash streams and both launches).  The library reaches the scene through svgf_scene_view alone
// (struct svgf_scene is unknown here) and links against libsvgf_hip.so alone.
//   k_restir_reset          one thread per pixel: H empty, the previous ids -1
//   k_restir_initial        one thread per pixel: candidates, one shadow ray to the winner, the history tap; writes T
//   k_restir_spatial_shade  one thread per pixel: T's neighbours, one shadow ray to the winner, D; writes H and the previous planes
//   k_lights_draw_all       one thread per pixel: every light, `samples` shadow rays each
// Workgroups are 256 threads on a 64 x 4 pixel tile (one wave per row, as the clamp, TAA and upsample kernels), so that the spatial
// taps of a wave's neighbours land in rows the same workgroup reads.  The shadow rays are scene_occluded of svgf_scene_walk.inc.h,
// the product's own text, on its per-lane stack in LDS (48 KB per block).  A thread writes only its own pixel's records: launch 1
// reads H and the previous planes and writes T, launch 2 reads T and writes H and the previous planes, so no thread reads what
// another writes in the same launch, nothing passes between workgroups and there are no atomics.  Reservoirs move as two 16-byte words.
// What the pass is apart from its payload - the tile's pixel, the G-buffer reads, the history tap's address, update()'s sums, the state
// behind the handle with its create / read / info / destroy, scene_args - is svgf_reservoir.inc.h, shared with svgf_restir_gi.hip.
// float32, contraction off (build.LIGHT_SAMPLERS' row adds -ffp-contract=off; the pragmas say it again where the arithmetic is normative).
#include "svgf_kernels.h"
#include "svgf_temporal.h"      // svgf_lum_strict
#include "svgf_device_table.h"
#include "../../include/svgf_restir.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

struct svgf_lights {
    int device, n;
    SvgfLight *dev;
};

namespace {

#include "svgf_scene_pixel.inc.h"

#include "svgf_scene_walk.inc.h"

#include "svgf_reservoir.inc.h"

struct RestirArgs {
    SceneBvhArgs b;             // the scene's arrays, width, height, seed, frame; nothing else of SceneArgs is read
    const float4 *lights;       // SvgfLight as three float4
    int n_lights;
    const float *gbuf;          // AoS texels, or null: the planes
    const float *pl_nrm, *pl_pos;
    const int *pl_gid;
    const float *motion;        // or null
    const float *emit;          // geomId -> emittance
    int n_ids;
    float4 *H, *T;
    float *prev_n;
    int *prev_gid;
    int candidates, temporal, neighbours, samples;
    float m_cap, radius, min_dot, ambient;
    float *out_D;
};

struct Light { float centre[3], eu[3], ev[3], power[3]; };
struct Reservoir { int j; float u, v, M, W, phat, w_sum; };

__device__ __forceinline__ Light load_light(const RestirArgs &a, int j)
{
    const float4 q0 = a.lights[3 * (size_t)j], q1 = a.lights[3 * (size_t)j + 1], q2 = a.lights[3 * (size_t)j + 2];
    return Light{ { q0.x, q0.y, q0.z }, { q0.w, q1.x, q1.y }, { q1.z, q1.w, q2.x }, { q2.y, q2.z, q2.w } };
}

__device__ __forceinline__ Reservoir empty_reservoir() { return Reservoir{ -1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }; }

__device__ __forceinline__ Reservoir load_reservoir(const float4 *plane, int p)
{
    const float4 a = plane[2 * (size_t)p], b = plane[2 * (size_t)p + 1];
    return Reservoir{ __float_as_int(a.x), a.y, a.z, a.w, b.x, b.y, 0.0f };
}

__device__ __forceinline__ void store_reservoir(float4 *plane, int p, const Reservoir &r)
{
    const bool e = r.j < 0;
    plane[2 * (size_t)p] = make_float4(__int_as_float(e ? -1 : r.j), e ? 0.0f : r.u, e ? 0.0f : r.v, r.M);
    plane[2 * (size_t)p + 1] = make_float4(e ? 0.0f : r.W, e ? 0.0f : r.phat, 0.0f, 0.0f);
}

// F_j,c(pos, n) and lam: scene_direct's statements with power_c in 30's place
__device__ __forceinline__ float light_term(const Light &L, const float n[3], const float pos[3], float F[3])
{
#pragma clang fp contract(off)
    float tl[3];
    for (int c = 0; c < 3; c++) tl[c] = L.centre[c] - pos[c];
    const float dist2 = (tl[0] * tl[0] + tl[1] * tl[1]) + tl[2] * tl[2];
    const float dl = sqrtf(dist2);
    const float lam = fmaxf(((tl[0] / dl) * n[0] + (tl[1] / dl) * n[1]) + (tl[2] / dl) * n[2], 0.0f);
    for (int c = 0; c < 3; c++) F[c] = (L.power[c] * lam) / (4.0f + dist2);
    return lam;
}

__device__ __forceinline__ float light_phat(const RestirArgs &a, int j, const float n[3], const float pos[3])
{
    float F[3];
    light_term(load_light(a, j), n, pos, F);
    return svgf_lum_strict(F[0], F[1], F[2]);
}

__device__ __forceinline__ void reservoir_update(Reservoir &r, int j, float u, float v, float phat, float w, float M_s, float xi)
{
    if (reservoir_add(r.w_sum, r.M, w, M_s, xi)) { r.j = j; r.u = u; r.v = v; r.phat = phat; }
}

__device__ __forceinline__ void reservoir_finish(Reservoir &r)
{
#pragma clang fp contract(off)
    r.W = (r.j >= 0 && r.phat > 0.0f) ? r.w_sum / (r.M * r.phat) : 0.0f;
}

// take(s, r, xi): a stored reservoir of this pixel
__device__ __forceinline__ void reservoir_take(Reservoir &s, const Reservoir &r, float xi)
{
#pragma clang fp contract(off)
    reservoir_update(s, r.j, r.u, r.v, r.phat, (r.phat * r.W) * r.M, r.M, xi);
}

// take'(s, r, M', xi): a reservoir of another pixel or frame, its target function evaluated at this pixel
__device__ __forceinline__ void reservoir_take_at(const RestirArgs &a, Reservoir &s, const Reservoir &r, float Mq, float xi, const float n[3],
                                                  const float pos[3])
{
#pragma clang fp contract(off)
    const float phat = (r.j >= 0 && r.j < a.n_lights) ? light_phat(a, r.j, n, pos) : 0.0f;
    reservoir_update(s, r.j, r.u, r.v, phat, (phat * r.W) * Mq, Mq, xi);
}

// row f16's shadow sample towards the point (u, v) of light L: scene_shadow_sample's statements with u and v given
__device__ __forceinline__ bool light_occluded(const SceneBvhArgs &b, const Light &L, const float pos[3], int *const stk, float u, float v)
{
#pragma clang fp contract(off)
    const float su = 2.0f * u - 1.0f, sv = 2.0f * v - 1.0f;
    float q[3];
    for (int c = 0; c < 3; c++) q[c] = ((L.centre[c] + su * L.eu[c]) + sv * L.ev[c]) - pos[c];
    const float dl = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    bool occluded = false;
    if (dl > 0.0f) {
        SceneRay r;
        for (int c = 0; c < 3; c++) { r.o[c] = pos[c]; r.d[c] = q[c] / dl; r.flat[c] = fabsf(r.d[c]) < 0x1p-100f; r.inv[c] = 1.0f / r.d[c]; }
        const float t_lo = 0x1p-10f * fmaxf(1.0f, dl);
        occluded = scene_occluded(b, r, stk, t_lo, dl - t_lo);
    }
    return occluded;
}

__global__ __launch_bounds__(256) void k_restir_reset(RestirArgs arg)
{
    int x, y;
    const int p = tile_pixel(arg.b.s, x, y);
    if (p < 0) return;
    store_reservoir(arg.H, p, empty_reservoir());
    arg.prev_gid[p] = -1;
}

__global__ __launch_bounds__(256) void k_restir_initial(RestirArgs arg)
{
#pragma clang fp contract(off)
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneArgs &a = arg.b.s;
    int x, y;
    const int p = tile_pixel(a, x, y);
    if (p < 0) return;
    int *const stk = stack + threadIdx.x;
    float n[3], pos[3];
    const int gid = read_surface(arg, p, n, pos);
    Reservoir s = empty_reservoir();
    if (gid >= 0 && !(id_emittance(arg, gid) > 0.0f)) {
        const unsigned up = (unsigned)p;
        const float u = scene_hash(a.seed, a.frame, up, 8), v = scene_hash(a.seed, a.frame, up, 9);
        const float fN = (float)arg.n_lights;
        Reservoir r = empty_reservoir();
        for (int c = 0; c < arg.candidates; c++) {
            int j = (int)(scene_hash(a.seed, a.frame, up, 4096u + (unsigned)c) * fN);
            j = j < arg.n_lights - 1 ? j : arg.n_lights - 1;
            const float phat = light_phat(arg, j, n, pos);
            reservoir_update(r, j, u, v, phat, phat * fN, 1.0f, scene_hash(a.seed, a.frame, up, 4128u + (unsigned)c));
        }
        reservoir_finish(r);
        if (r.j >= 0 && r.W > 0.0f && light_occluded(arg.b, load_light(arg, r.j), pos, stk, r.u, r.v)) r.W = 0.0f;
        reservoir_take(s, r, 0.0f);
        if (arg.temporal && arg.motion) {
            int q;
            if (history_tap(arg, a, p, gid, n, q)) {
                const Reservoir h = load_reservoir(arg.H, q);
                reservoir_take_at(arg, s, h, fminf(h.M, arg.m_cap * r.M), scene_hash(a.seed, a.frame, up, 4160), n, pos);
            }
        }
        reservoir_finish(s);
    }
    store_reservoir(arg.T, p, s);
}

__global__ __launch_bounds__(256) void k_restir_spatial_shade(RestirArgs arg)
{
#pragma clang fp contract(off)
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneArgs &a = arg.b.s;
    int x, y;
    const int p = tile_pixel(a, x, y);
    if (p < 0) return;
    int *const stk = stack + threadIdx.x;
    float n[3], pos[3];
    const int gid = read_surface(arg, p, n, pos);
    const float emit = id_emittance(arg, gid);
    Reservoir s = empty_reservoir();
    float D[3] = { 0.0f, 0.0f, 0.0f };
    if (gid >= 0 && emit > 0.0f) {
        D[0] = emit; D[1] = emit; D[2] = emit;
    } else if (gid >= 0) {
        const unsigned up = (unsigned)p;
        reservoir_take(s, load_reservoir(arg.T, p), 0.0f);
        for (int k = 0; k < arg.neighbours; k++) {
            const unsigned base = 4192u + 4u * (unsigned)k;
            const int ox = (int)floorf(((2.0f * scene_hash(a.seed, a.frame, up, base) - 1.0f) * arg.radius) + 0.5f);
            const int oy = (int)floorf(((2.0f * scene_hash(a.seed, a.frame, up, base + 1) - 1.0f) * arg.radius) + 0.5f);
            const int qx = x + ox, qy = y + oy;
            if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H || (ox == 0 && oy == 0)) continue;
            const int q = qy * a.W + qx;
            float m[3];
            int gq;
            read_normal(arg, q, m, gq);
            if (gq != gid || !((n[0] * m[0] + n[1] * m[1]) + n[2] * m[2] >= arg.min_dot)) continue;
            const Reservoir t = load_reservoir(arg.T, q);
            reservoir_take_at(arg, s, t, t.M, scene_hash(a.seed, a.frame, up, base + 2), n, pos);
        }
        reservoir_finish(s);
        D[0] = arg.ambient; D[1] = arg.ambient; D[2] = arg.ambient;
        if (s.j >= 0 && s.j < arg.n_lights) {
            const Light L = load_light(arg, s.j);
            float F[3];
            light_term(L, n, pos, F);
            float vis = 1.0f;
            if (s.W > 0.0f && light_occluded(arg.b, L, pos, stk, s.u, s.v)) vis = 0.0f;
            for (int c = 0; c < 3; c++) D[c] = arg.ambient + vis * (F[c] * s.W);
        }
    }
    float *o = arg.out_D + 3 * (size_t)p;
    o[0] = D[0]; o[1] = D[1]; o[2] = D[2];
    store_reservoir(arg.H, p, s);
    arg.prev_n[3 * (size_t)p] = n[0]; arg.prev_n[3 * (size_t)p + 1] = n[1]; arg.prev_n[3 * (size_t)p + 2] = n[2];
    arg.prev_gid[p] = gid;
}

__global__ __launch_bounds__(256) void k_lights_draw_all(RestirArgs arg)
{
#pragma clang fp contract(off)
    __shared__ int stack[SVGF_SCENE_MAX_DEPTH * 256];
    const SceneArgs &a = arg.b.s;
    int x, y;
    const int p = tile_pixel(a, x, y);
    if (p < 0) return;
    int *const stk = stack + threadIdx.x;
    float n[3], pos[3];
    const int gid = read_surface(arg, p, n, pos);
    float emit = 0.0f;
    bool found = false;
    for (int k = 0; k < a.n_geoms; k++) {
        const bool is = !found && (a.geom_ids ? a.geom_ids[k] : k) == gid;
        emit = is ? a.geoms[k].emittance : emit;
        found = found || is;
    }
    float D[3] = { 0.0f, 0.0f, 0.0f };
    if (gid >= 0 && emit > 0.0f) {
        D[0] = emit; D[1] = emit; D[2] = emit;
    } else if (gid >= 0) {
        float acc[3] = { 0.0f, 0.0f, 0.0f };
        for (int j = 0; j < arg.n_lights; j++) {
            const Light L = load_light(arg, j);
            float F[3];
            const float lam = light_term(L, n, pos, F);
            if (!(lam > 0.0f)) continue;
            int unoccluded = 0;
            for (int s = 0; s < arg.samples; s++) {
                const float u = scene_hash(a.seed, a.frame, (unsigned)p, 8u + 2u * (unsigned)s), v = scene_hash(a.seed, a.frame, (unsigned)p, 9u + 2u * (unsigned)s);
                unoccluded += light_occluded(arg.b, L, pos, stk, u, v) ? 0 : 1;
            }
            const float vis = (float)unoccluded / (float)arg.samples;
            for (int c = 0; c < 3; c++) acc[c] = acc[c] + F[c] * vis;
        }
        for (int c = 0; c < 3; c++) D[c] = arg.ambient + acc[c];
    }
    float *o = arg.out_D + 3 * (size_t)p;
    o[0] = D[0]; o[1] = D[1]; o[2] = D[2];
}

// the G-buffer, the synth parameters and the ambient term of a frame or a draw_all: refusals, then the arguments
int surface_args(RestirArgs &t, const void *gbuffer_dev, const SvgfPlanarGBuffer *planes, int width, int height, const SvgfSynthParams *sp,
                 float ambient, void *out_D_dev)
{
    if (!sp || !out_D_dev || (gbuffer_dev != nullptr) == (planes != nullptr)) return SVGF_ERR_INVALID_ARG;
    if (!gbuffer_dev && (!planes->normal || !planes->position || !planes->geom_id)) return SVGF_ERR_INVALID_ARG;
    if (!std::isfinite(ambient) || ambient < 0.0f || width <= 0 || height <= 0) return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    t.gbuf = static_cast<const float *>(gbuffer_dev);
    t.pl_nrm = planes ? planes->normal : nullptr; t.pl_pos = planes ? planes->position : nullptr; t.pl_gid = planes ? planes->geom_id : nullptr;
    t.b.s.W = width; t.b.s.H = height; t.b.s.seed = sp->seed; t.b.s.frame = sp->frame;
    t.ambient = ambient;
    t.out_D = static_cast<float *>(out_D_dev);
    return SVGF_OK;
}

bool light_ok(const SvgfLight &l)
{
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(l.centre[c]) || !std::isfinite(l.edge_u[c]) || !std::isfinite(l.edge_v[c]) || !std::isfinite(l.power[c])) return false;
    return true;
}

}  // namespace

struct svgf_restir : ReservoirState {};
static_assert(SVGF_RESTIR_MAX_ID == RESERVOIR_MAX_ID, "the shared create's bound on ids");

extern "C" int svgf_restir_version(void) { return (SVGF_VERSION_MAJOR << 16) | SVGF_VERSION_MINOR; }

// svgf_device_table.h's create with this table's own bounds on n (1..SVGF_RESTIR_MAX_LIGHTS); destroy and size are the shared ones
extern "C" int svgf_lights_create(int device, const SvgfLight *host_lights, int n, svgf_lights **out)
{
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    if (n < 1 || n > SVGF_RESTIR_MAX_LIGHTS || !host_lights || device < 0) return SVGF_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (!light_ok(host_lights[i])) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) {
        (void)hipGetLastError();        // a device that does not exist must not fail the next launch's check
        return SVGF_ERR_NO_DEVICE;
    }
    svgf_lights *t = new (std::nothrow) svgf_lights{ device, n, nullptr };
    if (!t) return SVGF_ERR_OOM;
    if (hipMalloc(reinterpret_cast<void **>(&t->dev), (size_t)n * sizeof(SvgfLight)) != hipSuccess) {
        (void)hipGetLastError();
        delete t;
        return SVGF_ERR_OOM;
    }
    if (hipMemcpy(t->dev, host_lights, (size_t)n * sizeof(SvgfLight), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(t->dev);
        delete t;
        return SVGF_ERR_HIP;
    }
    *out = t;
    return SVGF_OK;
}

extern "C" void svgf_lights_destroy(svgf_lights *table) { svgf_device_table_destroy(table); }

extern "C" int svgf_lights_size(const svgf_lights *table) { return svgf_device_table_size(table); }

extern "C" int svgf_restir_create(const svgf_scene *scene, int width, int height, svgf_restir **out)
{
    return reservoir_state_create(scene, width, height, 32, svgf_restir_reset, out);
}

extern "C" int svgf_restir_reset(svgf_restir *st, void *stream)
{
    if (!st) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(st->device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    RestirArgs t;
    std::memset(&t, 0, sizeof(t));
    t.b.s.W = st->width; t.b.s.H = st->height;
    t.H = st->H; t.prev_gid = st->prev_gid;
    hipLaunchKernelGGL(k_restir_reset, tile_grid(st->width, st->height), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_restir_frame(svgf_restir *st, const svgf_lights *table, const void *gbuffer_dev, const SvgfPlanarGBuffer *planes,
                                 const void *motion_prev_coord_dev, const SvgfRestirParams *rp, const SvgfSynthParams *sp, float ambient,
                                 void *out_D_dev, void *stream)
{
    if (!st || !table || !rp) return SVGF_ERR_INVALID_ARG;
    RestirArgs t;
    std::memset(&t, 0, sizeof(t));
    int rc = surface_args(t, gbuffer_dev, planes, st->width, st->height, sp, ambient, out_D_dev);
    if (rc != SVGF_OK) return rc;
    if (rp->candidates < 1 || rp->candidates > SVGF_RESTIR_MAX_CANDIDATES || (rp->temporal != 0 && rp->temporal != 1)) return SVGF_ERR_INVALID_ARG;
    if (!std::isfinite(rp->m_cap) || rp->m_cap < 1.0f || rp->neighbours < 0 || rp->neighbours > SVGF_RESTIR_MAX_NEIGHBOURS) return SVGF_ERR_INVALID_ARG;
    if (!std::isfinite(rp->radius) || rp->radius < 1.0f || rp->radius > 65536.0f || !std::isfinite(rp->normal_min_dot)) return SVGF_ERR_INVALID_ARG;
    int device = 0;
    rc = scene_args(t.b, st->scene, device);
    if (rc != SVGF_OK) return rc;
    if (table->device != device || st->device != device) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    t.lights = reinterpret_cast<const float4 *>(table->dev); t.n_lights = table->n;
    t.motion = static_cast<const float *>(motion_prev_coord_dev);
    t.emit = st->emit; t.n_ids = st->n_ids;
    t.H = st->H; t.T = st->T; t.prev_n = st->prev_n; t.prev_gid = st->prev_gid;
    t.candidates = rp->candidates; t.temporal = rp->temporal; t.neighbours = rp->neighbours;
    t.m_cap = rp->m_cap; t.radius = rp->radius; t.min_dot = rp->normal_min_dot;
    const dim3 grid = tile_grid(st->width, st->height);
    hipLaunchKernelGGL(k_restir_initial, grid, dim3(256), 0, static_cast<hipStream_t>(stream), t);
    hipLaunchKernelGGL(k_restir_spatial_shade, grid, dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_lights_draw_all(const svgf_scene *scene, const svgf_lights *table, const void *gbuffer_dev, const SvgfPlanarGBuffer *planes,
                                    int width, int height, int samples, const SvgfSynthParams *sp, float ambient, void *out_D_dev, void *stream)
{
    if (!scene || !table || samples < 1 || samples > SVGF_SCENE_MAX_SHADOW_SAMPLES) return SVGF_ERR_INVALID_ARG;
    RestirArgs t;
    std::memset(&t, 0, sizeof(t));
    int rc = surface_args(t, gbuffer_dev, planes, width, height, sp, ambient, out_D_dev);
    if (rc != SVGF_OK) return rc;
    int device = 0;
    rc = scene_args(t.b, scene, device);
    if (rc != SVGF_OK) return rc;
    if (table->device != device) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) return SVGF_ERR_NO_DEVICE;
    t.lights = reinterpret_cast<const float4 *>(table->dev); t.n_lights = table->n;
    t.samples = samples;
    hipLaunchKernelGGL(k_lights_draw_all, tile_grid(width, height), dim3(256), 0, static_cast<hipStream_t>(stream), t);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}

extern "C" int svgf_restir_info(const svgf_restir *st, SvgfRestirInfo *out) { return reservoir_state_info(st, out); }

extern "C" int svgf_restir_read(const svgf_restir *st, int which, void *host_dst, unsigned long long host_bytes)
{
    return reservoir_state_read(st, which, host_dst, host_bytes);
}

extern "C" void svgf_restir_destroy(svgf_restir *st) { reservoir_state_destroy(st); }
