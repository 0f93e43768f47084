// rs_frame_dev.h — what the kernels of the frame operators share (rs_denoise.hip, rs_denoise_var.hip, rs_adaptive.hip,
// rs_robust.hip, rs_matte.hip): pixel tests and arithmetic, the frame list in the argument block, the mean / variance stores, and the
// tap geometry, weight and launch of the two a-trous kernels. All f32, every operation rounded once; nothing of the
// scene (no rs_device.h). Everything here is inlined: each kernel's machine code is what it was with its own copy
// (tools/kernel_isa.sh, profiles/frame_ops).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_internal.h"

namespace rs {

__device__ __forceinline__ bool finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool finite3(const float4& v) { return finite(v.x) && finite(v.y) && finite(v.z); }

// (a ?: on two float4 objects selects between their addresses: both go to scratch)
__device__ __forceinline__ float4 select(const bool t, const float4 a, const float4 b) {
    return make_float4(t ? a.x : b.x, t ? a.y : b.y, t ? a.z : b.z, t ? a.w : b.w);
}

// m of rs_denoise's step 3: the albedo the colour is divided by before the levels and multiplied by after them
__device__ __forceinline__ float4 modulation(const float4& alb) {
    const float u = 1.0f - alb.w;  // the un-covered share counts as albedo 1
    return make_float4(fmaxf(alb.x + u, 1e-3f), fmaxf(alb.y + u, 1e-3f), fmaxf(alb.z + u, 1e-3f), 0.f);
}

// a loaded pixel's colour as the operators compute with it: gamma-2 frames are squared (the alpha is left as loaded)
__device__ __forceinline__ void decode(float4& x, const int gamma) {
    if (gamma) { x.x = x.x * x.x; x.y = x.y * x.y; x.z = x.z * x.z; }
}

// The frames of a pass operator, in the kernel's argument block: read with scalar loads, k is wave-uniform.
struct Frames {
    const float4* f[kMaxFrames];
};
inline Frames frame_list(const float* const* frames, uint32_t n_frames) {
    Frames fr;
    for (uint32_t k = 0; k < (uint32_t)kMaxFrames; ++k)  // (the unused slots repeat frame 0: never read)
        fr.f[k] = reinterpret_cast<const float4*>(frames[k < n_frames ? k : 0]);
    return fr;
}

// A pass operator's outputs of a pixel: the mean (x, y, z) re-encoded, all zero where no frame contributed; the
// variance q / den, zero below two frames, with the frame count n in w. (One stores and the other returns its pixel:
// of the forms tried, the pair that leaves every kernel's instructions in the order they had.)
__device__ __forceinline__ void store_mean(float4* mean, const uint32_t p, const int gamma, const bool any, const float x,
                                           const float y, const float z) {
    float ox = x, oy = y, oz = z;
    if (gamma) { ox = sqrtf(ox); oy = sqrtf(oy); oz = sqrtf(oz); }
    mean[p] = make_float4(any ? ox : 0.f, any ? oy : 0.f, any ? oz : 0.f, any ? 1.0f : 0.f);
}
__device__ __forceinline__ float4 var_pixel(const bool two, const float qx, const float qy, const float qz, const float den,
                                            const float n) {
    const float vx = qx / den, vy = qy / den, vz = qz / den;
    return make_float4(two ? vx : 0.f, two ? vy : 0.f, two ? vz : 0.f, n);
}

// ---- the a-trous kernels (k_dn_atrous, k_dv_atrous) ----
// One thread per pixel, every tap from global memory (L1 / L2 / Infinity Cache). Block = a 64 x 4 tile: a wave is 64
// consecutive pixels of one row, so each of its loads is one contiguous 1 KiB run of float4s per plane (shifted by the
// tap). (A variant that staged a 32 x 8 tile and its halo in LDS was measured and not kept: DESIGN.md section 12.)
constexpr int kTileW = 64, kTileH = 4;
static_assert(kTileW * kTileH == kBlock, "one thread per tile pixel");

__device__ __forceinline__ float b3_tap(const int i) {  // i = 0 .. 4: offsets -2 .. 2
    const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    return k[i];
}

// A tap's coordinate q along an axis of n pixels: whether it is in the frame, and the coordinate its loads go to (a
// tap off the frame loads from a clamped address and is dropped).
struct Tap {
    bool in;
    int c;
};
__device__ __forceinline__ Tap tap_at(const int q, const int n) { return Tap{(unsigned)q < (unsigned)n, min(max(q, 0), n - 1)}; }

// A guided tap's weight: its B3 weight h over the colour term A and the normal and relative-depth terms of the guide
// pixels gp (centre) and gq (tap). An unguided tap's is h * (1.0f / A), written at the call: as a branch of this
// function it made the unguided k_dv_atrous load its taps unconditionally.
__device__ __forceinline__ float guide_weight(const float A, const float4& gp, const float4& gq, const float inv_n,
                                              const float inv_d, const float h) {
    const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
    const float dn2 = (nx * nx + ny * ny) + nz * nz;
    const float dd = gq.w - gp.w;
    const float M = fmaxf(fmaxf(fabsf(gp.w), fabsf(gq.w)), 1e-6f);
    const float M2 = M * M;
    const float B = 1.0f + dn2 * inv_n;
    const float D = M2 + (dd * dd) * inv_d;
    return h * (M2 / ((A * B) * D));
}

// One level: a block per tile of the level's W x H frame. kernel(L, tiles_x) is an instance of the a-trous kernel.
template <class Level>
hipError_t launch_level(void (*kernel)(Level, uint32_t), const Level& L, hipStream_t st) {
    const uint32_t tiles_x = ((uint32_t)L.W + kTileW - 1) / kTileW, tiles_y = ((uint32_t)L.H + kTileH - 1) / kTileH;
    // W H <= 2^31 - 1 (checked by the caller), so tiles_x tiles_y < W H / 256 + W / 64 + H / 4 + 1 < 2^31
    kernel<<<dim3(tiles_x * tiles_y), dim3(kBlock), 0, st>>>(L, tiles_x);
    return hipGetLastError();
}

}  // namespace rs
