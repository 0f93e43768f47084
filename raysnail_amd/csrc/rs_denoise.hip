// rs_denoise.hip — the edge-avoiding a-trous denoiser over the first-hit feature frames (rs_denoise_device; the
// contract, operation by operation, is in include/raysnail_hip.h). One prepare launch and one launch per level, all
// f32, every operation rounded once (the unit is built with -ffp-contract=off like the others), no transcendental.
// Needs nothing of the scene: no rs_device.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_internal.h"

namespace rs {
namespace {

__device__ __forceinline__ bool dn_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool dn_finite3(const float4& v) { return dn_finite(v.x) && dn_finite(v.y) && dn_finite(v.z); }

// m of the contract's step 3: the albedo the colour is divided by before the levels and multiplied by after them
__device__ __forceinline__ float4 dn_modulation(const float4& alb) {
    const float u = 1.0f - alb.w;  // the un-covered share counts as albedo 1
    return make_float4(fmaxf(alb.x + u, 1e-3f), fmaxf(alb.y + u, 1e-3f), fmaxf(alb.z + u, 1e-3f), 0.f);
}

// Level 0's colour plane: (demodulated linear colour, usable flag as 1.0 / 0.0). One thread per pixel.
__global__ __launch_bounds__(kBlock) void k_dn_prepare(const float4* beauty, const float4* __restrict__ albedo,
                                                       const float4* __restrict__ guide, uint32_t n, int gamma,
                                                       float4* __restrict__ plane) {
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (p >= n) return;
    const float4 b = beauty[p];
    bool usable = b.w != 0.f && dn_finite3(b);
    float4 c = b;
    if (gamma) { c.x = c.x * c.x; c.y = c.y * c.y; c.z = c.z * c.z; }
    if (albedo) {
        const float4 a = albedo[p];
        usable = usable && dn_finite3(a) && dn_finite(a.w);
        const float4 m = dn_modulation(a);
        c.x = c.x / m.x; c.y = c.y / m.y; c.z = c.z / m.z;
    }
    if (guide) {
        const float4 g = guide[p];
        usable = usable && dn_finite3(g) && dn_finite(g.w);
    }
    usable = usable && dn_finite3(c);
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
    const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + s * dy;
        const bool in_y = (unsigned)qy < (unsigned)H;
        const int cy = min(max(qy, 0), H - 1);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float h = k[dx + 2] * k[dy + 2];
            if (dx == 0 && dy == 0) {
                sr = sr + h * cp.x; sg = sg + h * cp.y; sb = sb + h * cp.z; sw = sw + h;
                continue;
            }
            const int qx = x + s * dx;
            const bool in_x = (unsigned)qx < (unsigned)W;
            const int cx = min(max(qx, 0), W - 1);
            const float4 cq = src.color(cx, cy);
            const float dr = cq.x - cp.x, dg = cq.y - cp.y, db = cq.z - cp.z;
            const float dc2 = (dr * dr + dg * dg) + db * db;
            const float A = 1.0f + dc2 * ic;
            float w;
            if (GUIDE) {
                const float4 gq = src.guide(cx, cy);
                const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
                const float dn2 = (nx * nx + ny * ny) + nz * nz;
                const float dd = gq.w - gp.w;
                const float M = fmaxf(fmaxf(fabsf(gp.w), fabsf(gq.w)), 1e-6f);
                const float M2 = M * M;
                const float B = 1.0f + dn2 * inv_n;
                const float D = M2 + (dd * dd) * inv_d;
                w = h * (M2 / ((A * B) * D));
            } else {
                w = h * (1.0f / A);
            }
            const bool take = in_y && in_x && cq.w != 0.f;
            sr = take ? sr + w * cq.x : sr;
            sg = take ? sg + w * cq.y : sg;
            sb = take ? sb + w * cq.z : sb;
            sw = take ? sw + w : sw;
        }
    }
    return make_float4(sr / sw, sg / sw, sb / sw, cp.w);
}

// (a ?: on two float4 objects selects between their addresses: both go to scratch)
__device__ __forceinline__ float4 dn_select(const bool t, const float4 a, const float4 b) {
    return make_float4(t ? a.x : b.x, t ? a.y : b.y, t ? a.z : b.z, t ? a.w : b.w);
}

// The level's store of pixel p: the next plane, or (LAST) the finish step into the caller's frame.
template <bool LAST>
__device__ __forceinline__ void dn_store(float4* out, const float4* beauty, const float4* albedo, const int gamma,
                                         const uint32_t p, const bool usable, const float4 c, const float4 cp) {
    if (!LAST) {
        out[p] = dn_select(usable, c, cp);  // a pixel that is not usable is carried through untouched
        return;
    }
    const float4 b = beauty[p];
    float4 o = c;
    if (albedo) {
        const float4 m = dn_modulation(albedo[p]);
        o.x = o.x * m.x; o.y = o.y * m.y; o.z = o.z * m.z;
    }
    if (gamma) { o.x = sqrtf(o.x); o.y = sqrtf(o.y); o.z = sqrtf(o.z); }
    o.w = b.w;
    out[p] = dn_select(usable, o, b);
}

struct DnGlobalSrc {
    const float4* __restrict__ in;
    const float4* __restrict__ g;
    int W;
    __device__ __forceinline__ float4 color(int x, int y) const { return in[(uint32_t)y * (uint32_t)W + (uint32_t)x]; }
    __device__ __forceinline__ float4 guide(int x, int y) const { return g[(uint32_t)y * (uint32_t)W + (uint32_t)x]; }
};

// One thread per pixel, every tap from global memory (L1 / L2 / Infinity Cache). Block = a 64 x 4 tile: a wave is 64
// consecutive pixels of one row, so each of its loads is one contiguous 1 KiB run of float4s (shifted by the tap).
// (A variant that staged a 32 x 8 tile and its halo in LDS for the steps 1 and 2 was measured and not kept:
// DESIGN.md section 12.)
constexpr int kDnTileW = 64, kDnTileH = 4;
static_assert(kDnTileW * kDnTileH == kBlock, "one thread per tile pixel");

template <bool GUIDE, bool LAST>
__global__ __launch_bounds__(kBlock) void k_dn_atrous(DnLevel L, uint32_t tiles_x) {
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x = (int)(tx * kDnTileW + (threadIdx.x & (kDnTileW - 1)));
    const int y = (int)(ty * kDnTileH + (threadIdx.x / kDnTileW));
    if (x >= L.W || y >= L.H) return;
    const uint32_t p = (uint32_t)y * (uint32_t)L.W + (uint32_t)x;
    const DnGlobalSrc src{L.in, L.guide, L.W};
    const float4 cp = L.in[p];
    const float4 gp = GUIDE ? L.guide[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 c = dn_filter<GUIDE>(src, x, y, L.W, L.H, L.s, L.ic, L.inv_n, L.inv_d, cp, gp);
    dn_store<LAST>(L.out, L.beauty, L.albedo, L.gamma, p, cp.w != 0.f, c, cp);
}

template <bool GUIDE, bool LAST>
hipError_t dn_level(const DnLevel& L, hipStream_t st) {
    const uint32_t tiles_x = ((uint32_t)L.W + kDnTileW - 1) / kDnTileW, tiles_y = ((uint32_t)L.H + kDnTileH - 1) / kDnTileH;
    // W H <= 2^31 - 1 (checked by the caller), so tiles_x tiles_y < W H / 256 + W / 64 + H / 4 + 1 < 2^31
    k_dn_atrous<GUIDE, LAST><<<dim3(tiles_x * tiles_y), dim3(kBlock), 0, st>>>(L, tiles_x);
    return hipGetLastError();
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
        if (g4) e = last ? dn_level<true, true>(L, st) : dn_level<true, false>(L, st);
        else e = last ? dn_level<false, true>(L, st) : dn_level<false, false>(L, st);
    }
    return e;
}

}  // namespace rs
