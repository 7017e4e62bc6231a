// svgf_trace_compose.hip — libsvgf_split.so, row f18: svgf_trace_compose, the modulation for two terms.  include/svgf_split.h states
// the semantics: out_c = a_c * (D_c + I_c), one add then one multiply, float32, nothing contracted, plain IEEE.
//
// k_compose<AOS>: a streaming kernel, 24 B/px in and 12 out for the images and 12 (an albedo plane) or 24 of a 52-byte texel (AoS)
// for the albedo.  A thread owns FOUR pixels: twelve floats of each image, which are three 16-byte pieces when the image's base plus
// the pixels in front of them falls on 16 bytes.  The host finds that place: `head` pixels (0..3) are taken one by one, `n_groups`
// groups of four follow, the remaining 0..3 pixels are taken one by one again.  That needs every image (and the albedo plane) to sit
// at the SAME offset from a 16-byte boundary; where they do not, n_groups is 0 and every pixel is taken alone, by dwords.  The AoS
// texel's albedo and ialbedo are six dwords at byte 24 of a 52-byte texel: 4-byte aligned only, read by dwords in either path.
// A thread reads all it needs of its own pixels before it writes them and no two threads share a pixel, so `out` may be `direct` or
// `indirect`.  The grid is not capped: one thread per group (at most 2^27 / 4 of them) or per lone pixel, no loop.
#include "svgf_kernels.h"
#include "../../include/svgf_split.h"

#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

namespace {

struct ComposeArgs {
    float *out;
    const float *direct, *indirect;
    const float *albedo;        // the plane, or the AoS texels (13 floats each)
    int n_px, head, n_groups;
};

template <bool AOS>
__device__ __forceinline__ void compose_albedo(const float *albedo, size_t p, float a[3])
{
#pragma clang fp contract(off)
    if (AOS) {
        const float *t = albedo + 13 * p;
        a[0] = t[6] * t[9]; a[1] = t[7] * t[10]; a[2] = t[8] * t[11];
    } else {
        a[0] = albedo[3 * p]; a[1] = albedo[3 * p + 1]; a[2] = albedo[3 * p + 2];
    }
}

template <bool AOS>
__global__ __launch_bounds__(256) void k_compose(ComposeArgs q)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < q.n_groups) {       // pixels head + 4t .. head + 4t + 3: floats 3 * head + 12t .., on 16 bytes in every image
        const size_t p = (size_t)q.head + 4 * (size_t)t;
        const float4 *pd = reinterpret_cast<const float4 *>(q.direct + 3 * p), *pi = reinterpret_cast<const float4 *>(q.indirect + 3 * p);
        const float4 d0 = pd[0], d1 = pd[1], d2 = pd[2], i0 = pi[0], i1 = pi[1], i2 = pi[2];
        float a[12];
        if (AOS) {
#pragma unroll
            for (int k = 0; k < 4; k++) compose_albedo<true>(q.albedo, p + k, a + 3 * k);
        } else {
            const float4 *pa = reinterpret_cast<const float4 *>(q.albedo + 3 * p);
            const float4 a0 = pa[0], a1 = pa[1], a2 = pa[2];
            a[0] = a0.x; a[1] = a0.y; a[2] = a0.z; a[3] = a0.w; a[4] = a1.x; a[5] = a1.y; a[6] = a1.z; a[7] = a1.w;
            a[8] = a2.x; a[9] = a2.y; a[10] = a2.z; a[11] = a2.w;
        }
        float4 *po = reinterpret_cast<float4 *>(q.out + 3 * p);
        po[0] = make_float4(a[0] * (d0.x + i0.x), a[1] * (d0.y + i0.y), a[2] * (d0.z + i0.z), a[3] * (d0.w + i0.w));
        po[1] = make_float4(a[4] * (d1.x + i1.x), a[5] * (d1.y + i1.y), a[6] * (d1.z + i1.z), a[7] * (d1.w + i1.w));
        po[2] = make_float4(a[8] * (d2.x + i2.x), a[9] * (d2.y + i2.y), a[10] * (d2.z + i2.z), a[11] * (d2.w + i2.w));
    }
    // the lone pixels: the head's [0, head), then those behind the groups
    const int n_lone = q.n_px - 4 * q.n_groups;
    if (t < n_lone) {
        const size_t p = t < q.head ? (size_t)t : (size_t)t + 4 * (size_t)q.n_groups;
        float a[3];
        compose_albedo<AOS>(q.albedo, p, a);
        const float d0 = q.direct[3 * p], d1 = q.direct[3 * p + 1], d2 = q.direct[3 * p + 2];
        const float i0 = q.indirect[3 * p], i1 = q.indirect[3 * p + 1], i2 = q.indirect[3 * p + 2];
        q.out[3 * p] = a[0] * (d0 + i0); q.out[3 * p + 1] = a[1] * (d1 + i1); q.out[3 * p + 2] = a[2] * (d2 + i2);
    }
}

}  // namespace

extern "C" int svgf_trace_compose(int device, void *out_rgb_dev, const void *direct_dev, const void *indirect_dev, const SvgfGuide *guide, int width,
                                  int height, void *stream)
{
    if (!out_rgb_dev || !direct_dev || !indirect_dev || !guide || (!guide->gbuffer && !guide->albedo) || width <= 0 || height <= 0)
        return SVGF_ERR_INVALID_ARG;
    if ((long long)width * height >= (1LL << 31) / 16) return SVGF_ERR_UNSUPPORTED;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) {
        (void)hipGetLastError();        // a device that does not exist must not fail the next launch's check
        return SVGF_ERR_NO_DEVICE;
    }
    const bool aos = guide->gbuffer != nullptr;
    ComposeArgs q;
    q.out = static_cast<float *>(out_rgb_dev);
    q.direct = static_cast<const float *>(direct_dev); q.indirect = static_cast<const float *>(indirect_dev);
    q.albedo = aos ? static_cast<const float *>(guide->gbuffer) : guide->albedo;
    q.n_px = width * height;
    // 12 head + (base & 15) = 0 (mod 16) for head = (base & 15) / 4; images off a 4-byte boundary (not allowed) take the dword path
    const uintptr_t off = reinterpret_cast<uintptr_t>(out_rgb_dev) & 15;
    bool vec = (off & 3) == 0 && (reinterpret_cast<uintptr_t>(direct_dev) & 15) == off && (reinterpret_cast<uintptr_t>(indirect_dev) & 15) == off;
    if (!aos) vec = vec && (reinterpret_cast<uintptr_t>(guide->albedo) & 15) == off;
    q.head = vec ? (int)(off / 4) : 0;
    if (q.head > q.n_px) q.head = q.n_px;
    q.n_groups = vec ? (q.n_px - q.head) / 4 : 0;
    const int n_lone = q.n_px - 4 * q.n_groups;
    const int n_threads = q.n_groups > n_lone ? q.n_groups : n_lone;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (aos) hipLaunchKernelGGL(k_compose<true>, dim3((n_threads + 255) / 256), dim3(256), 0, s, q);
    else hipLaunchKernelGGL(k_compose<false>, dim3((n_threads + 255) / 256), dim3(256), 0, s, q);
    return hipGetLastError() == hipSuccess ? SVGF_OK : SVGF_ERR_HIP;
}
