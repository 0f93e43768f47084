// rs_robust.hip — the rank-trimmed mean of K pass frames and its Winsorised variance (rs_pass_robust_device); the
// contract, operation by operation, is in include/raysnail_hip.h. All f32, every operation rounded once (the unit is
// built with -ffp-contract=off like the others), no transcendental. Scene-free: no rs_device.h.
//
// The frame count is a run-time value, so a per-thread array of keys would be indexed by a run-time k and go to
// scratch. The keys live in LDS instead, one column per thread ([k][thread]: a wave's 64 lanes read 64 consecutive
// dwords, conflict-free), and so do the ranks, four one-byte ranks to a dword ([k / 4][thread]). A thread reads and
// writes only its own column, so the kernel has no barrier, and the LDS is sized at launch to the frame count rounded up to
// four: 5 bytes per frame and thread, 40 KB for 64 frames of a 128-thread block (4 blocks to a CU), 5 KB for 8.
// The ranks are found by counting, four frames of the outer loop held in registers against one LDS read of the inner
// (n^2 / 4 reads, n^2 compare-and-add pairs). The rgb triples are not kept: the S, w and Q sweeps re-read the frames.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_frame_dev.h"

namespace rs {
namespace {

constexpr int kRbBlock = 128;  // 2 waves; 64 frames: 40 KB of LDS per block

// frame k's x of the contract (the alpha is left as loaded)
__device__ __forceinline__ float4 rb_value(const Frames& fr, const int k, const uint32_t p, const int gamma) {
    float4 x = fr.f[k][p];
    // (not decode(), here and in the key loop: it reorders this kernel's registers)
    if (gamma) { x.x = x.x * x.x; x.y = x.y * x.y; x.z = x.z * x.z; }
    return x;
}
__device__ __forceinline__ int rb_rank(const uint32_t* ranks, const int k) {
    return (int)((ranks[(k >> 2) * kRbBlock] >> ((k & 3) * 8)) & 0xFFu);
}

// One thread per pixel. Every load of a thread comes before its stores, and it stores only its own pixel: mean may
// alias a frame (no __restrict__ here).
__global__ __launch_bounds__(kRbBlock) void k_pass_robust(const Frames fr, const int n_frames, const uint32_t n_pix,
                                                          const int gamma, const float trim, float4* mean, float4* var,
                                                          uint8_t* trimmed) {
    extern __shared__ float rb_lds[];
    const uint32_t p = blockIdx.x * (uint32_t)kRbBlock + threadIdx.x;
    if (p >= n_pix) return;  // (no barrier below)
    const int n4 = (n_frames + 3) & ~3;
    float* keys = rb_lds + threadIdx.x;                                                  // keys[k * kRbBlock]
    uint32_t* ranks = reinterpret_cast<uint32_t*>(rb_lds + n4 * kRbBlock) + threadIdx.x;  // ranks[(k / 4) * kRbBlock]
    const float inf = __uint_as_float(0x7F800000u);

    // the keys; a frame that does not contribute gets +inf, which is before no finite key
    int n = 0;
    for (int k = 0; k < n_frames; ++k) {
        const float4 f = fr.f[k][p];
        float4 x = f;
        if (gamma) { x.x = x.x * x.x; x.y = x.y * x.y; x.z = x.z * x.z; }
        const float s = (x.x + x.y) + x.z;
        const bool take = f.w != 0.f && finite3(f) && finite(s);
        keys[k * kRbBlock] = take ? s : inf;
        n += take ? 1 : 0;
    }
    for (int k = n_frames; k < n4; ++k) keys[k * kRbBlock] = inf;
    const float fn = (float)n;
    const bool automatic = trim < 0.f;
    // a fixed trim that cuts nothing even where all frames contribute needs no ranks (floorf(trim n) is monotone in n)
    const bool need_ranks = automatic || floorf(trim * (float)n_frames) >= 1.0f;

    // the ranks by counting, and the Gini sums in frame order
    float ss = 0.f, ng = 0.f;
    if (need_ranks) {
        for (int kk = 0; kk < n4; kk += 4) {
            const float a0 = keys[kk * kRbBlock], a1 = keys[(kk + 1) * kRbBlock];
            const float a2 = keys[(kk + 2) * kRbBlock], a3 = keys[(kk + 3) * kRbBlock];
            int r0 = 0, r1 = 0, r2 = 0, r3 = 0;
            for (int j = 0; j < kk; ++j) {  // earlier frames win ties
                const float s = keys[j * kRbBlock];
                r0 += s <= a0 ? 1 : 0; r1 += s <= a1 ? 1 : 0; r2 += s <= a2 ? 1 : 0; r3 += s <= a3 ? 1 : 0;
            }
            r1 += a0 <= a1 ? 1 : 0; r2 += a0 <= a2 ? 1 : 0; r3 += a0 <= a3 ? 1 : 0;
            r0 += a1 < a0 ? 1 : 0;  r2 += a1 <= a2 ? 1 : 0; r3 += a1 <= a3 ? 1 : 0;
            r0 += a2 < a0 ? 1 : 0;  r1 += a2 < a1 ? 1 : 0;  r3 += a2 <= a3 ? 1 : 0;
            r0 += a3 < a0 ? 1 : 0;  r1 += a3 < a1 ? 1 : 0;  r2 += a3 < a2 ? 1 : 0;
            for (int j = kk + 4; j < n_frames; ++j) {  // later frames lose them
                const float s = keys[j * kRbBlock];
                r0 += s < a0 ? 1 : 0; r1 += s < a1 ? 1 : 0; r2 += s < a2 ? 1 : 0; r3 += s < a3 ? 1 : 0;
            }
            ranks[(kk >> 2) * kRbBlock] = (uint32_t)r0 | ((uint32_t)r1 << 8) | ((uint32_t)r2 << 16) | ((uint32_t)r3 << 24);
            if (automatic) {
                const int nm1 = n - 1;
                const bool c0 = finite(a0), c1 = finite(a1), c2 = finite(a2), c3 = finite(a3);
                const float g0 = (float)(2 * r0 - nm1) * a0, g1 = (float)(2 * r1 - nm1) * a1;
                const float g2 = (float)(2 * r2 - nm1) * a2, g3 = (float)(2 * r3 - nm1) * a3;
                ss = c0 ? ss + a0 : ss; ng = c0 ? ng + g0 : ng;
                ss = c1 ? ss + a1 : ss; ng = c1 ? ng + g1 : ng;
                ss = c2 ? ss + a2 : ss; ng = c2 ? ng + g2 : ng;
                ss = c3 ? ss + a3 : ss; ng = c3 ? ng + g3 : ng;
            }
        }
    } else {
        for (int kk = 0; kk < n4; kk += 4) ranks[(kk >> 2) * kRbBlock] = 0u;  // t = 0: every rank passes
    }

    const int t_max = n >= 2 ? (n - 2) / 2 : 0;
    float cut;
    if (automatic) {
        float G = ss > 0.f ? ng / (fn * ss) : 0.f;
        G = fminf(fmaxf(G, 0.f), 1.0f);
        cut = floorf((G * fn) * 0.5f);
    } else {
        cut = floorf(trim * fn);
    }
    const int t = min(t_max, (int)cut);
    const int top = n - 1 - t;  // the rank of hi
    const int h = n - 2 * t;

    // S over the kept frames, and the triples of lo and hi
    float sx = 0.f, sy = 0.f, sz = 0.f;
    float4 xlo = make_float4(0.f, 0.f, 0.f, 0.f), xhi = xlo;
    for (int k = 0; k < n_frames; ++k) {
        const float4 x = rb_value(fr, k, p, gamma);
        const bool c = finite(keys[k * kRbBlock]);
        const int r = rb_rank(ranks, k);
        const bool kept = c && r >= t && r <= top;
        sx = kept ? sx + x.x : sx;
        sy = kept ? sy + x.y : sy;
        sz = kept ? sz + x.z : sz;
        xlo = select(c && r == t, x, xlo);
        xhi = select(c && r == top, x, xhi);
    }
    const float fh = (float)h;
    const float mx = sx / fh, my = sy / fh, mz = sz / fh;  // (n = 0: 0 / 0, dropped below)

    // the Winsorised mean; where no lane of the wave trims, it is S / n as computed
    float wx = sx, wy = sy, wz = sz;
    if (__ballot(t > 0) != 0ull) {
        wx = 0.f; wy = 0.f; wz = 0.f;
        for (int k = 0; k < n_frames; ++k) {
            const float4 x = rb_value(fr, k, p, gamma);
            const bool c = finite(keys[k * kRbBlock]);
            const int r = rb_rank(ranks, k);
            const float4 w = select(r < t, xlo, select(r > top, xhi, x));
            wx = c ? wx + w.x : wx;
            wy = c ? wy + w.y : wy;
            wz = c ? wz + w.z : wz;
        }
    }
    const float mwx = wx / fn, mwy = wy / fn, mwz = wz / fn;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    for (int k = 0; k < n_frames; ++k) {
        const float4 x = rb_value(fr, k, p, gamma);
        const bool c = finite(keys[k * kRbBlock]);
        const int r = rb_rank(ranks, k);
        const float4 w = select(r < t, xlo, select(r > top, xhi, x));
        const float dx = w.x - mwx, dy = w.y - mwy, dz = w.z - mwz;
        qx = c ? qx + dx * dx : qx;
        qy = c ? qy + dy * dy : qy;
        qz = c ? qz + dz * dz : qz;
    }

    if (mean) {  // (not store_mean(): it reorders this kernel's registers)
        const bool any = n >= 1;
        float ox = mx, oy = my, oz = mz;
        if (gamma) { ox = sqrtf(ox); oy = sqrtf(oy); oz = sqrtf(oz); }
        mean[p] = make_float4(any ? ox : 0.f, any ? oy : 0.f, any ? oz : 0.f, any ? 1.0f : 0.f);
    }
    if (var) var[p] = var_pixel(n >= 2, qx, qy, qz, fh * (float)(h - 1), fn);
    if (trimmed) trimmed[p] = (uint8_t)t;
}

}  // namespace

hipError_t launch_pass_robust(const float* const* frames, uint32_t n_frames, uint32_t n_pix, int gamma, float trim,
                              float* mean, float* var, uint8_t* trimmed, hipStream_t st) {
    const uint32_t n4 = (n_frames + 3u) & ~3u;
    const size_t lds = (size_t)n4 * kRbBlock * 5;  // 4 bytes of key and 1 of rank per frame and thread: at most 40 KB
    k_pass_robust<<<dim3((n_pix + kRbBlock - 1) / kRbBlock), dim3(kRbBlock), lds, st>>>(
        frame_list(frames, n_frames), (int)n_frames, n_pix, gamma, trim, reinterpret_cast<float4*>(mean), reinterpret_cast<float4*>(var), trimmed);
    return hipGetLastError();
}

}  // namespace rs
