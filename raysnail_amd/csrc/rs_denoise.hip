// rs_denoise.hip — the edge-avoiding a-trous denoiser over the first-hit feature frames (rs_denoise_device; the
// contract, operation by operation, is in include/raysnail_hip.h). One prepare launch and one launch per level, all
// f32, every operation rounded once (the unit is built with -ffp-contract=off like the others), no transcendental.
// Needs nothing of the scene: no rs_device.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_frame_dev.h"

namespace rs {
namespace {

// Level 0's colour plane: (demodulated linear colour, usable flag as 1.0 / 0.0). One thread per pixel.
__global__ __launch_bounds__(kBlock) void k_dn_prepare(const float4* beauty, const float4* __restrict__ albedo,
                                                       const float4* __restrict__ guide, uint32_t n, int gamma,
                                                       float4* __restrict__ plane) {
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (p >= n) return;
    const float4 b = beauty[p];
    bool usable = b.w != 0.f && finite3(b);
    float4 c = b;
    decode(c, gamma);
    if (albedo) {
        const float4 a = albedo[p];
        usable = usable && finite3(a) && finite(a.w);
        const float4 m = modulation(a);
        c.x = c.x / m.x; c.y = c.y / m.y; c.z = c.z / m.z;
    }
    if (guide) {
        const float4 g = guide[p];
        usable = usable && finite3(g) && finite(g.w);
    }
    usable = usable && finite3(c);
    c.w = usable ? 1.0f : 0.0f;
    plane[p] = c;
}

struct DnLevel {
    const float4* in;      // this level's colour plane (a half of d_work)
    const float4* guide;   // the normal frame, read in place (GUIDE only)
    float4* out;           // the next level's plane, or (LAST) the caller's frame
    const float4* beauty;  // LAST: alpha, and the bits of the pixels that are not usable (may alias out)
    const float4* albedo;  // LAST: remodulation (may be null)
    int W, H, s;
    float ic, inv_n, inv_d;
    int gamma;
};

// The level's new colour of the usable pixel (x, y) with colour cp and guide gp. src.color / src.guide fetch the
// plane / guide value of an in-frame pixel; the taps run dy outer, dx inner, and a tap that is outside the frame or
// not usable leaves the four sums as they are (the loads of such a tap go to a clamped address and are dropped).
template <bool GUIDE, class Src>
__device__ __forceinline__ float4 dn_filter(const Src src, const int x, const int y, const int W, const int H, const int s,
                                            const float ic, const float inv_n, const float inv_d, const float4 cp,
                                            const float4 gp) {
    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const Tap qy = tap_at(y + s * dy, H);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float h = b3_tap(dx + 2) * b3_tap(dy + 2);
            if (dx == 0 && dy == 0) {
                sr = sr + h * cp.x; sg = sg + h * cp.y; sb = sb + h * cp.z; sw = sw + h;
                continue;
            }
            const Tap qx = tap_at(x + s * dx, W);
            const float4 cq = src.color(qx.c, qy.c);
            const float dr = cq.x - cp.x, dg = cq.y - cp.y, db = cq.z - cp.z;
            const float dc2 = (dr * dr + dg * dg) + db * db;
            const float A = 1.0f + dc2 * ic;
            float w;
            if (GUIDE) w = guide_weight(A, gp, src.guide(qx.c, qy.c), inv_n, inv_d, h);
            else w = h * (1.0f / A);
            const bool take = qy.in && qx.in && cq.w != 0.f;
            sr = take ? sr + w * cq.x : sr;
            sg = take ? sg + w * cq.y : sg;
            sb = take ? sb + w * cq.z : sb;
            sw = take ? sw + w : sw;
        }
    }
    return make_float4(sr / sw, sg / sw, sb / sw, cp.w);
}

// The level's store of pixel p: the next plane, or (LAST) the finish step into the caller's frame.
template <bool LAST>
__device__ __forceinline__ void dn_store(float4* out, const float4* beauty, const float4* albedo, const int gamma,
                                         const uint32_t p, const bool usable, const float4 c, const float4 cp) {
    if (!LAST) {
        out[p] = select(usable, c, cp);  // a pixel that is not usable is carried through untouched
        return;
    }
    const float4 b = beauty[p];
    float4 o = c;
    if (albedo) {
        const float4 m = modulation(albedo[p]);
        o.x = o.x * m.x; o.y = o.y * m.y; o.z = o.z * m.z;
    }
    if (gamma) { o.x = sqrtf(o.x); o.y = sqrtf(o.y); o.z = sqrtf(o.z); }
    o.w = b.w;
    out[p] = select(usable, o, b);
}

struct DnGlobalSrc {
    const float4* __restrict__ in;
    const float4* __restrict__ g;
    int W;
    __device__ __forceinline__ float4 color(int x, int y) const { return in[(uint32_t)y * (uint32_t)W + (uint32_t)x]; }
    __device__ __forceinline__ float4 guide(int x, int y) const { return g[(uint32_t)y * (uint32_t)W + (uint32_t)x]; }
};

// One thread per pixel of a 64 x 4 tile (rs_frame_dev.h).
template <bool GUIDE, bool LAST>
__global__ __launch_bounds__(kBlock) void k_dn_atrous(DnLevel L, uint32_t tiles_x) {
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x = (int)(tx * kTileW + (threadIdx.x & (kTileW - 1)));
    const int y = (int)(ty * kTileH + (threadIdx.x / kTileW));
    if (x >= L.W || y >= L.H) return;
    const uint32_t p = (uint32_t)y * (uint32_t)L.W + (uint32_t)x;
    const DnGlobalSrc src{L.in, L.guide, L.W};
    const float4 cp = L.in[p];
    const float4 gp = GUIDE ? L.guide[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 c = dn_filter<GUIDE>(src, x, y, L.W, L.H, L.s, L.ic, L.inv_n, L.inv_d, cp, gp);
    dn_store<LAST>(L.out, L.beauty, L.albedo, L.gamma, p, cp.w != 0.f, c, cp);
}

}  // namespace

hipError_t launch_denoise(const float* beauty, const float* albedo, const float* normal, uint32_t width, uint32_t height,
                          uint32_t levels, const float* ic, float inv_n, float inv_d, int gamma, float* out, float* work,
                          hipStream_t st) {
    const uint32_t n = width * height;
    float4* plane[2] = {reinterpret_cast<float4*>(work), reinterpret_cast<float4*>(work) + n};
    const float4* b4 = reinterpret_cast<const float4*>(beauty);
    const float4* a4 = reinterpret_cast<const float4*>(albedo);
    const float4* g4 = reinterpret_cast<const float4*>(normal);
    k_dn_prepare<<<dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st>>>(b4, a4, g4, n, gamma, plane[0]);
    hipError_t e = hipGetLastError();
    for (uint32_t i = 0; i < levels && e == hipSuccess; ++i) {
        const bool last = i + 1 == levels;
        DnLevel L;
        L.in = plane[i & 1];
        L.guide = g4;
        L.out = last ? reinterpret_cast<float4*>(out) : plane[(i + 1) & 1];
        L.beauty = b4;
        L.albedo = a4;
        L.W = (int)width; L.H = (int)height; L.s = 1 << i;
        L.ic = ic[i]; L.inv_n = inv_n; L.inv_d = inv_d;
        L.gamma = gamma;
        if (g4) e = launch_level(last ? k_dn_atrous<true, true> : k_dn_atrous<true, false>, L, st);
        else e = launch_level(last ? k_dn_atrous<false, true> : k_dn_atrous<false, false>, L, st);
    }
    return e;
}

}  // namespace rs
