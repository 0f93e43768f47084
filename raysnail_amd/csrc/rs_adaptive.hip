// rs_adaptive.hip — the running per-pixel moments (rs_moments_update_device, rs_moments_resolve_device) and the
// variance-driven sample mask (rs_adaptive_mask_device); the contracts, operation by operation, are in
// include/raysnail_adaptive.h. All f32, every operation rounded once (the unit is built with -ffp-contract=off like the
// others), no transcendental. Needs nothing of the scene: no rs_device.h. All three kernels stream: they are judged by
// the bytes they move (update: 32 B of state read and written + 16 B per frame and pixel; resolve: 32 B read, 16 B per
// output; mask: 32 B read per tile cell, halo included, 1 B of base read and 1 B of mask written).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_frame_dev.h"

namespace rs {
namespace {

// ------------------------------------------------------------------------------------ Welford update ----
// One thread per pixel: its state in registers over the frames, stored once, and only when a frame contributed.
__global__ __launch_bounds__(kBlock) void k_moments_update(float4* __restrict__ acc, float4* __restrict__ m2,
                                                           const Frames fr, const int n_frames, const uint32_t n_pix,
                                                           const int gamma) {
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (p >= n_pix) return;
    float4 a = acc[p];
    float4 q = m2[p];
    bool any = false;
    for (int k = 0; k < n_frames; ++k) {
        float4 x = fr.f[k][p];
        const bool take = x.w != 0.f && finite3(x);
        decode(x, gamma);
        const float n1 = a.w + 1.0f;
        const float dx = x.x - a.x, dy = x.y - a.y, dz = x.z - a.z;
        const float mx = a.x + dx / n1, my = a.y + dy / n1, mz = a.z + dz / n1;
        const float ex = x.x - mx, ey = x.y - my, ez = x.z - mz;
        const float qx = q.x + dx * ex, qy = q.y + dy * ey, qz = q.z + dz * ez;
        a.x = take ? mx : a.x; a.y = take ? my : a.y; a.z = take ? mz : a.z; a.w = take ? n1 : a.w;
        q.x = take ? qx : q.x; q.y = take ? qy : q.y; q.z = take ? qz : q.z;
        any = any || take;
    }
    if (any) {
        q.w = 0.f;
        acc[p] = a;
        m2[p] = q;
    }
}

// --------------------------------------------------------------------------------------------- resolve ----
__global__ __launch_bounds__(kBlock) void k_moments_resolve(const float4* __restrict__ acc, const float4* __restrict__ m2,
                                                            const uint32_t n_pix, const int gamma,
                                                            float4* __restrict__ mean, float4* __restrict__ var) {
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (p >= n_pix) return;
    const float4 a = acc[p];
    const float n = a.w;
    if (mean) store_mean(mean, p, gamma, n >= 1.0f, a.x, a.y, a.z);
    if (var) {
        const float4 q = m2[p];
        var[p] = var_pixel(n >= 2.0f, q.x, q.y, q.z, n * (n - 1.0f), n);
    }
}

// ------------------------------------------------------------------------------------------------ mask ----
// Block = a 32 x 8 tile of pixels. Its (32 + 2 r) x (8 + 2 r) cells (the tile and its radius-r halo) are classified
// once each, strided over the threads, into one LDS byte per cell: bit 0 hot(q), bit 1 base(q) != 0 and n_q < max_n.
// A cell off the frame is 0. Then every thread scans the (2 r + 1)^2 bytes around its own pixel. The statistics count
// interior cells only (every pixel is interior to exactly one tile): LDS atomics within the block, then one global
// atomic per block and statistic that is not zero.
constexpr int kAdTileW = 32, kAdTileH = 8, kAdMaxRadius = 4;
static_assert(kAdTileW * kAdTileH == kBlock, "one thread per tile pixel");
constexpr int kAdCellsMax = (kAdTileW + 2 * kAdMaxRadius) * (kAdTileH + 2 * kAdMaxRadius);

struct AdMask {
    const float4* acc;
    const float4* m2;
    const uint8_t* base;   // or null: all ones
    uint8_t* mask;
    unsigned int* counters;  // [0] active, [1] hot, [2] nonfinite (each <= W H < 2^31), [3] max_err2's bits; or null
    int W, H, r;
    int row_begin, row_end, row_step;  // the rows that count as base (the loop's render lattice); all rows: 0, H, 1
    float min_n, max_n, tol2, floor;
};

__global__ __launch_bounds__(kBlock) void k_adaptive_mask(const AdMask A, const uint32_t tiles_x) {
    __shared__ uint8_t cell[kAdCellsMax];
    __shared__ unsigned int s_stat[4];  // active, hot, nonfinite, max_err2 bits
    const int W = A.W, H = A.H, r = A.r;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = (int)(tx * kAdTileW), y0 = (int)(ty * kAdTileH);
    const int cw = kAdTileW + 2 * r, ch = kAdTileH + 2 * r;
    if (threadIdx.x < 4) s_stat[threadIdx.x] = 0u;
    __syncthreads();

    for (int c = (int)threadIdx.x; c < cw * ch; c += kBlock) {
        const int cy = c / cw, cx = c - cy * cw;
        const int gx = x0 - r + cx, gy = y0 - r + cy;
        uint8_t flags = 0;
        if ((unsigned)gx < (unsigned)W && (unsigned)gy < (unsigned)H) {
            const uint32_t q = (uint32_t)gy * (uint32_t)W + (uint32_t)gx;
            const float4 a = A.acc[q];
            const float4 m = A.m2[q];
            const bool on_rows = gy >= A.row_begin && gy < A.row_end && (gy - A.row_begin) % A.row_step == 0;
            const bool based = on_rows && (A.base ? A.base[q] != 0 : true);
            const float n = a.w;
            const bool fin = finite3(a) && finite3(m);
            const float t = (m.x + m.y) + m.z;
            const float v = t / (n * (n - 1.0f));
            const float L = (a.x + a.y) + a.z;
            const float Dn = fmaxf(L, A.floor);
            const float err2 = v / (Dn * Dn);
            const bool open = based && n < A.max_n;
            const bool hot = open && (n < A.min_n || (fin && err2 > A.tol2));
            flags = (uint8_t)((hot ? 1 : 0) | (open ? 2 : 0));
            const bool interior = cx >= r && cx < r + kAdTileW && cy >= r && cy < r + kAdTileH;
            if (A.counters && interior) {
                if (hot) atomicAdd(&s_stat[1], 1u);
                if (based && !fin) atomicAdd(&s_stat[2], 1u);
                // (a non-negative float orders like its bit pattern; NaN, zero and negative values take no part)
                if (based && fin && n >= 2.0f && err2 > 0.f) atomicMax(&s_stat[3], __float_as_uint(err2));
            }
        }
        cell[c] = flags;
    }
    __syncthreads();

    const int lx = (int)(threadIdx.x & (kAdTileW - 1)), ly = (int)(threadIdx.x / kAdTileW);
    const int x = x0 + lx, y = y0 + ly;
    if (x < W && y < H) {
        const bool open = (cell[(ly + r) * cw + (lx + r)] & 2) != 0;
        bool near_hot = false;
        for (int dy = 0; dy <= 2 * r; ++dy)
            for (int dx = 0; dx <= 2 * r; ++dx) near_hot = near_hot || (cell[(ly + dy) * cw + (lx + dx)] & 1) != 0;
        const bool on = open && near_hot;
        A.mask[(uint32_t)y * (uint32_t)W + (uint32_t)x] = on ? 1 : 0;
        if (A.counters && on) atomicAdd(&s_stat[0], 1u);
    }
    if (!A.counters) return;
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned int v = s_stat[threadIdx.x];
        if (v) atomicAdd(&A.counters[threadIdx.x], v);
    } else if (threadIdx.x == 3) {
        const unsigned int v = s_stat[3];
        if (v) atomicMax(&A.counters[3], v);
    }
}

}  // namespace

hipError_t launch_moments_update(float* acc, float* m2, const float* const* frames, uint32_t n_frames, uint32_t n_pix,
                                 int gamma, hipStream_t st) {
    k_moments_update<<<dim3((n_pix + kBlock - 1) / kBlock), dim3(kBlock), 0, st>>>(
        reinterpret_cast<float4*>(acc), reinterpret_cast<float4*>(m2), frame_list(frames, n_frames), (int)n_frames, n_pix,
        gamma);
    return hipGetLastError();
}

hipError_t launch_moments_resolve(const float* acc, const float* m2, uint32_t n_pix, int gamma, float* mean, float* var,
                                  hipStream_t st) {
    k_moments_resolve<<<dim3((n_pix + kBlock - 1) / kBlock), dim3(kBlock), 0, st>>>(
        reinterpret_cast<const float4*>(acc), reinterpret_cast<const float4*>(m2), n_pix, gamma,
        reinterpret_cast<float4*>(mean), reinterpret_cast<float4*>(var));
    return hipGetLastError();
}

hipError_t launch_adaptive_mask(const float* acc, const float* m2, const uint8_t* base, uint32_t width, uint32_t height,
                                uint32_t min_n, uint32_t max_n, float tol2, float floor, uint32_t radius, uint8_t* mask,
                                unsigned int* counters, hipStream_t st, uint32_t row_begin, uint32_t row_end,
                                uint32_t row_step) {
    AdMask A;
    A.acc = reinterpret_cast<const float4*>(acc);
    A.m2 = reinterpret_cast<const float4*>(m2);
    A.base = base;
    A.mask = mask;
    A.counters = counters;
    A.W = (int)width; A.H = (int)height; A.r = (int)radius;
    // (rows at or beyond the height do not exist: the clamp keeps the three in int range)
    A.row_end = (int)(row_end < height ? row_end : height);
    A.row_begin = (int)(row_begin < height ? row_begin : height);
    A.row_step = (int)(row_step < 1 ? 1 : (row_step < height ? row_step : height));
    A.min_n = (float)min_n; A.max_n = (float)max_n;  // (exact: both <= 4096)
    A.tol2 = tol2; A.floor = floor;
    const uint32_t tiles_x = (width + kAdTileW - 1) / kAdTileW, tiles_y = (height + kAdTileH - 1) / kAdTileH;
    // W H <= 2^31 - 1 (checked by the caller), so tiles_x tiles_y < W H / 256 + W / 32 + H / 8 + 1 < 2^31
    k_adaptive_mask<<<dim3(tiles_x * tiles_y), dim3(kBlock), 0, st>>>(A, tiles_x);
    return hipGetLastError();
}

}  // namespace rs
