// rs_denoise_var.hip — the pass moments (rs_pass_moments_device) and the variance-guided a-trous denoiser
// (rs_denoise_var_device); the contracts, operation by operation, are in include/raysnail_hip.h. All f32, every
// operation rounded once (the unit is built with -ffp-contract=off like the others), no transcendental. Needs nothing
// of the scene: no rs_device.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs_frame_dev.h"

namespace rs {
namespace {

// ------------------------------------------------------------------------------------ pass moments ----
// One thread per pixel, two sweeps over the frames (the second finds its lines in L2 / Infinity Cache). Every load of
// a thread comes before its stores, and it stores only its own pixel: mean may alias a frame (no __restrict__ here).
__global__ __launch_bounds__(kBlock) void k_pass_moments(const Frames fr, const int n_frames, const uint32_t n_pix,
                                                         const int gamma, float4* mean, float4* var) {
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (p >= n_pix) return;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int n = 0;
    for (int k = 0; k < n_frames; ++k) {
        float4 x = fr.f[k][p];
        const bool take = x.w != 0.f && finite3(x);
        decode(x, gamma);
        sx = take ? sx + x.x : sx;
        sy = take ? sy + x.y : sy;
        sz = take ? sz + x.z : sz;
        n += take ? 1 : 0;
    }
    const float fn = (float)n;
    const float mx = sx / fn, my = sy / fn, mz = sz / fn;  // (n = 0: 0 / 0, dropped below)
    float qx = 0.f, qy = 0.f, qz = 0.f;
    for (int k = 0; k < n_frames; ++k) {
        float4 x = fr.f[k][p];
        const bool take = x.w != 0.f && finite3(x);
        decode(x, gamma);
        const float dx = x.x - mx, dy = x.y - my, dz = x.z - mz;
        qx = take ? qx + dx * dx : qx;
        qy = take ? qy + dy * dy : qy;
        qz = take ? qz + dz * dz : qz;
    }
    if (mean) store_mean(mean, p, gamma, n >= 1, mx, my, mz);
    if (var) var[p] = var_pixel(n >= 2, qx, qy, qz, fn * (float)(n - 1), fn);
}

// --------------------------------------------------------------------- variance-guided a-trous filter ----
// Level planes: colour = (demodulated linear colour, usable flag as 1.0 / 0.0), as rs_denoise's; variance = (demodulated
// variance v, t) with t = (v.r + v.g) + v.b of a usable pixel (never negative: v >= 0 on entry, and the levels add
// squares times variances) and -1.0 of a pixel that is not usable, whose plane values nobody reads: the 3 x 3 variance
// mean needs one dword per tap and no second plane for the flag.
__global__ __launch_bounds__(kBlock) void k_dv_prepare(const float4* beauty, const float4* var,
                                                       const float4* __restrict__ albedo,
                                                       const float4* __restrict__ guide, uint32_t n, int gamma,
                                                       float4* __restrict__ cplane, float4* __restrict__ vplane) {
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (p >= n) return;
    const float4 b = beauty[p];
    const float4 V = var[p];
    bool usable = b.w != 0.f && finite3(b);
    usable = usable && finite3(V) && V.x >= 0.f && V.y >= 0.f && V.z >= 0.f;
    float4 c = b, v = V;
    decode(c, gamma);
    if (albedo) {
        const float4 a = albedo[p];
        usable = usable && finite3(a) && finite(a.w);
        const float4 m = modulation(a);
        c.x = c.x / m.x; c.y = c.y / m.y; c.z = c.z / m.z;
        const float mmx = m.x * m.x, mmy = m.y * m.y, mmz = m.z * m.z;
        v.x = v.x / mmx; v.y = v.y / mmy; v.z = v.z / mmz;
    }
    if (guide) {
        const float4 g = guide[p];
        usable = usable && finite3(g) && finite(g.w);
    }
    usable = usable && finite3(c) && finite3(v);
    c.w = usable ? 1.0f : 0.0f;
    const float t = (v.x + v.y) + v.z;
    v.w = usable ? t : -1.0f;
    cplane[p] = c;
    vplane[p] = v;
}

struct DvLevel {
    const float4* cin;     // this level's colour plane
    const float4* vin;     // this level's variance plane
    const float4* guide;   // the normal frame, read in place (GUIDE only)
    float4* cout;          // the next level's colour plane, or (LAST) the caller's frame
    float4* vout;          // the next level's variance plane, or (LAST) the caller's variance frame (may be null)
    const float4* beauty;  // LAST: alpha, and the bits of the pixels that are not usable (may alias cout)
    const float4* var;     // LAST: V.w, and the bits of the pixels that are not usable (may alias vout)
    const float4* albedo;  // LAST: remodulation (may be null)
    int W, H, s;
    float kc, inv_n, inv_d;
    int gamma;
};

// 1 / (k_color vs_p + eps) of the usable pixel (x, y): the 3 x 3 Gaussian mean of the variance plane's t at spacing
// 1; a tap off the frame loads from a clamped address and is dropped, like one whose t says "not usable".
__device__ __forceinline__ float dv_inv_variance(const float4* __restrict__ vin, const int x, const int y, const int W,
                                                 const int H, const float kc, const float tp) {
    const float g[3] = {0.25f, 0.5f, 0.25f};
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const Tap qy = tap_at(y + dy, H);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float gw = g[dx + 1] * g[dy + 1];
            if (dx == 0 && dy == 0) {
                num = num + gw * tp; den = den + gw;
                continue;
            }
            const Tap qx = tap_at(x + dx, W);
            const float t = vin[(uint32_t)qy.c * (uint32_t)W + (uint32_t)qx.c].w;
            const bool take = qy.in && qx.in && !(t < 0.f);
            num = take ? num + gw * t : num;
            den = take ? den + gw : den;
        }
    }
    const float vs = num / den;
    return 1.0f / (kc * vs + 1e-6f);  // RS_DENOISE_VAR_EPS
}

// One thread per pixel of a 64 x 4 tile (rs_frame_dev.h), as rs_denoise's k_dn_atrous.
template <bool GUIDE, bool LAST>
__global__ __launch_bounds__(kBlock) void k_dv_atrous(const DvLevel L, const uint32_t tiles_x) {
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x = (int)(tx * kTileW + (threadIdx.x & (kTileW - 1)));
    const int y = (int)(ty * kTileH + (threadIdx.x / kTileW));
    const int W = L.W, H = L.H, s = L.s;
    if (x >= W || y >= H) return;
    const uint32_t p = (uint32_t)y * (uint32_t)W + (uint32_t)x;
    const float4* __restrict__ cin = L.cin;
    const float4* __restrict__ vin = L.vin;
    const float4* __restrict__ gin = L.guide;
    const float4 cp = cin[p];
    const float4 vp = vin[p];
    const float4 gp = GUIDE ? gin[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool usable = cp.w != 0.f;
    const float iv = dv_inv_variance(vin, x, y, W, H, L.kc, vp.w);
    const float inv_n = L.inv_n, inv_d = L.inv_d;

    float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f, vr = 0.f, vg = 0.f, vb = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const Tap qy = tap_at(y + s * dy, H);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float h = b3_tap(dx + 2) * b3_tap(dy + 2);
            if (dx == 0 && dy == 0) {
                const float hh = h * h;
                sr = sr + h * cp.x; sg = sg + h * cp.y; sb = sb + h * cp.z; sw = sw + h;
                vr = vr + hh * vp.x; vg = vg + hh * vp.y; vb = vb + hh * vp.z;
                continue;
            }
            const Tap qx = tap_at(x + s * dx, W);
            const uint32_t q = (uint32_t)qy.c * (uint32_t)W + (uint32_t)qx.c;
            const float4 cq = cin[q];
            const float4 vq = vin[q];
            const float dr = cq.x - cp.x, dg = cq.y - cp.y, db = cq.z - cp.z;
            const float dc2 = (dr * dr + dg * dg) + db * db;
            const float A = 1.0f + dc2 * iv;
            float w;
            if (GUIDE) w = guide_weight(A, gp, gin[q], inv_n, inv_d, h);
            else w = h * (1.0f / A);
            const float ww = w * w;
            const bool take = qy.in && qx.in && cq.w != 0.f;
            sr = take ? sr + w * cq.x : sr;
            sg = take ? sg + w * cq.y : sg;
            sb = take ? sb + w * cq.z : sb;
            sw = take ? sw + w : sw;
            vr = take ? vr + ww * vq.x : vr;
            vg = take ? vg + ww * vq.y : vg;
            vb = take ? vb + ww * vq.z : vb;
        }
    }
    const float ss = sw * sw;
    float4 c = make_float4(sr / sw, sg / sw, sb / sw, cp.w);
    float4 v = make_float4(vr / ss, vg / ss, vb / ss, 0.f);

    if (!LAST) {
        v.w = (v.x + v.y) + v.z;
        L.cout[p] = select(usable, c, cp);  // a pixel that is not usable is carried through untouched
        L.vout[p] = select(usable, v, vp);
        return;
    }
    const float4 b = L.beauty[p];
    if (L.albedo) {
        const float4 m = modulation(L.albedo[p]);
        c.x = c.x * m.x; c.y = c.y * m.y; c.z = c.z * m.z;
        const float mmx = m.x * m.x, mmy = m.y * m.y, mmz = m.z * m.z;
        v.x = v.x * mmx; v.y = v.y * mmy; v.z = v.z * mmz;
    }
    if (L.gamma) { c.x = sqrtf(c.x); c.y = sqrtf(c.y); c.z = sqrtf(c.z); }
    c.w = b.w;
    if (L.vout) {  // (read before the colour store: out may be beauty, and out_var may be var)
        const float4 V = L.var[p];
        v.w = V.w;
        L.vout[p] = select(usable, v, V);
    }
    L.cout[p] = select(usable, c, b);
}

}  // namespace

hipError_t launch_pass_moments(const float* const* frames, uint32_t n_frames, uint32_t n_pix, int gamma, float* mean,
                               float* var, hipStream_t st) {
    k_pass_moments<<<dim3((n_pix + kBlock - 1) / kBlock), dim3(kBlock), 0, st>>>(
        frame_list(frames, n_frames), (int)n_frames, n_pix, gamma, reinterpret_cast<float4*>(mean),
        reinterpret_cast<float4*>(var));
    return hipGetLastError();
}

hipError_t launch_denoise_var(const float* beauty, const float* var, const float* albedo, const float* normal,
                              uint32_t width, uint32_t height, uint32_t levels, float k_color, float inv_n, float inv_d,
                              int gamma, float* out, float* out_var, float* work, hipStream_t st) {
    const uint32_t n = width * height;
    float4* w4 = reinterpret_cast<float4*>(work);
    float4* cplane[2] = {w4, w4 + n};
    float4* vplane[2] = {w4 + 2 * (size_t)n, w4 + 3 * (size_t)n};
    const float4* b4 = reinterpret_cast<const float4*>(beauty);
    const float4* v4 = reinterpret_cast<const float4*>(var);
    const float4* a4 = reinterpret_cast<const float4*>(albedo);
    const float4* g4 = reinterpret_cast<const float4*>(normal);
    k_dv_prepare<<<dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st>>>(b4, v4, a4, g4, n, gamma, cplane[0], vplane[0]);
    hipError_t e = hipGetLastError();
    for (uint32_t i = 0; i < levels && e == hipSuccess; ++i) {
        const bool last = i + 1 == levels;
        DvLevel L;
        L.cin = cplane[i & 1];
        L.vin = vplane[i & 1];
        L.guide = g4;
        L.cout = last ? reinterpret_cast<float4*>(out) : cplane[(i + 1) & 1];
        L.vout = last ? reinterpret_cast<float4*>(out_var) : vplane[(i + 1) & 1];
        L.beauty = b4;
        L.var = v4;
        L.albedo = a4;
        L.W = (int)width; L.H = (int)height; L.s = 1 << i;
        L.kc = k_color; L.inv_n = inv_n; L.inv_d = inv_d;
        L.gamma = gamma;
        if (g4) e = launch_level(last ? k_dv_atrous<true, true> : k_dv_atrous<true, false>, L, st);
        else e = launch_level(last ? k_dv_atrous<false, true> : k_dv_atrous<false, false>, L, st);
    }
    return e;
}

}  // namespace rs
