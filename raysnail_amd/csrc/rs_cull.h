// rs_cull.h — the box tests of World::hit's tree walks: the exact f64 slab test of a leaf's own box (slab64) and the
// conservative f32 cull of the inner nodes' boxes (make_rayf / slab32 for one box, make_rayf4 / slab4 for the four
// children of a 4-wide node), with the outward f64 -> f32 rounding the host gives the node planes (rs_host.cpp
// to_device, to_device4) and the walks give their range ends.
// Plain C++ (host and device): tests/cpp/test_cull.cpp checks the cull against slab64 on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_CULL_HD __host__ __device__ __forceinline__
#define RS_CULL_UNROLL _Pragma("unroll")
#else
#define RS_CULL_HD inline
#define RS_CULL_UNROLL
#endif
#define RS_CULL_FLT_MAX 0x1.fffffep+127f

namespace rs {

struct V3 { double x, y, z; };

// aabb.rs:20-38 with inv = 1/d[i] precomputed per ray (the reference recomputes the same value
// per node). Branch-free form: max/min over the three axes is equivalent to the early-exit loop
// because t_min only grows and t_max only shrinks. This exact f64 test is applied to every
// object's own bbox before the object is intersected.
RS_CULL_HD bool slab64(const double lo[3], const double hi[3], const V3& o, const V3& inv, double tmin, double tmax) {
    double t0x = (lo[0] - o.x) * inv.x, t1x = (hi[0] - o.x) * inv.x;
    double t0y = (lo[1] - o.y) * inv.y, t1y = (hi[1] - o.y) * inv.y;
    double t0z = (lo[2] - o.z) * inv.z, t1z = (hi[2] - o.z) * inv.z;
    if (inv.x < 0.0) { double t = t0x; t0x = t1x; t1x = t; }
    if (inv.y < 0.0) { double t = t0y; t0y = t1y; t1y = t; }
    if (inv.z < 0.0) { double t = t0z; t0z = t1z; t1z = t; }
    const double a = fmax(fmax(fmax(tmin, t0x), t0y), t0z);
    const double b = fmin(fmin(fmin(tmax, t1x), t1y), t1z);
    return !(b <= a);
}

// The next float above f (f not NaN, not +inf; the largest float gives +inf, -inf the most negative float).
RS_CULL_HD float nextup_f(float f) {
    if (f == 0.0f) return 0x1p-149f;
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned u = __float_as_uint(f);
    return __uint_as_float(f > 0.0f ? u + 1u : u - 1u);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    u = f > 0.0f ? u + 1u : u - 1u;
    memcpy(&f, &u, 4);
    return f;
#endif
}
// f64 -> f32 rounded up / down: the outward rounding of a box's hi / lo planes and of a range's end / start (a
// value beyond the largest float gives an infinity on its own side, and the largest float on the other; NaN stays)
RS_CULL_HD float round_up_f(double x) {
    const float f = (float)x;
    return ((double)f < x) ? nextup_f(f) : f;
}
RS_CULL_HD float round_down_f(double x) {
    if (x != x) return (float)x;
    return -round_up_f(-x);
}

// Conservative f32 slab test for inner nodes: for every f64 ray, box and range, finite or not, it never rejects a
// box that the exact f64 test of any descendant leaf would accept (tests/cpp/test_cull.cpp). Boxes are rounded
// outward on the host. The ray origin is shifted per axis by d = |o|*2^-20 + 2^-100 (an expanded box
// [lo-d, hi+d] in effect), which absorbs the f32 rounding of o and of the precomputed products o'*inv (each
// <= |o| 2^-24, or 2^-150 where they underflow); t at a plane is then one FMA, t = lo*inv - (o+d)*inv. The remaining
// roundings (inv, fma) are relative and covered by a 2^-18 slack on the interval.
// That argument needs the axis's f32 quantities to stand for the f64 ones. An axis where they cannot is dropped: its
// inv becomes NaN, which slab32's and slab4's min / max ignore, as the exact test's f64 min / max ignore a NaN
// direction component (aabb.rs:20-38), so the axis culls nothing. These are the axes
//   * with a NaN inv (a NaN direction component);
//   * whose origin is not finite in f32, or whose product (|o| + d) * |inv| is not (an infinite or huge inv: a
//     direction component that is +-0 or tiny. The exact test constrains such an axis through the origin alone, and
//     with |o| * |inv| beyond f32 the products were +-inf and the axis rejected every box, from |o| = 2^29 on for an
//     axis-parallel ray. A clamp of |inv| to 1e30, as before, shrinks the far plane's t instead and rejected boxes
//     the ray reaches on that axis at a larger t);
//   * with |inv| < 2^-40 (a direction component beyond 2^40): a subnormal or zero inv has no relative precision, and
//     below 2^-40 the shift d * |inv| no longer exceeds the absolute error 2^-149 of results that underflow.
// Dropping costs the culling by that one axis, for rays exactly parallel to a coordinate plane or with components
// outside 2^-128 .. 2^40 times the others' scale. slab32 and slab4 clamp the entry to the largest float before the
// slack: an entry beyond f32 (inf) would turn NaN there and fail every comparison, the walks' `entry > -inf` too.
// slab4 returns what slab32 returns for every ray and every box with lo <= hi.
struct RayF {
    float inv[3], opi[3], omi[3];   // inv, (o+d)*inv, (o-d)*inv
};
RS_CULL_HD RayF make_rayf(const V3& o, const V3& inv) {
    RayF r;
    const double oo[3] = {o.x, o.y, o.z}, ii[3] = {inv.x, inv.y, inv.z};
    RS_CULL_UNROLL
    for (int k = 0; k < 3; ++k) {
        const float of = (float)oo[k];
        const float fi = (float)ii[k];
        const float d = fabsf(of) * 0x1p-20f + 0x1p-100f;
        // (false for a NaN or infinite of or fi: the product is then NaN or inf, as d > 0)
        const bool keep = fabsf(fi) >= 0x1p-40f && (fabsf(of) + d) * fabsf(fi) <= RS_CULL_FLT_MAX;
        const float iv = keep ? fi : __builtin_nanf("");
        r.inv[k] = iv;
        r.opi[k] = (of + d) * iv;
        r.omi[k] = (of - d) * iv;
    }
    return r;
}
RS_CULL_HD bool slab32(const float lo[3], const float hi[3], const RayF& r, float tmin, float tmax, float& entry) {
    const float ax = fmaf(lo[0], r.inv[0], -r.opi[0]), bx = fmaf(hi[0], r.inv[0], -r.omi[0]);
    const float ay = fmaf(lo[1], r.inv[1], -r.opi[1]), by = fmaf(hi[1], r.inv[1], -r.omi[1]);
    const float az = fmaf(lo[2], r.inv[2], -r.opi[2]), bz = fmaf(hi[2], r.inv[2], -r.omi[2]);
    float a = fminf(fmaxf(fmaxf(fmaxf(tmin, fminf(ax, bx)), fminf(ay, by)), fminf(az, bz)), RS_CULL_FLT_MAX);
    float b = fminf(fminf(fminf(tmax, fmaxf(ax, bx)), fmaxf(ay, by)), fmaxf(az, bz));
    a = fmaf(-fabsf(a), 0x1p-18f, a);
    b = fmaf(fabsf(b), 0x1p-18f, b);
    entry = a;
    return a <= b;
}

// 4-wide nodes: the ray's direction signs pick, per axis, which of the node's lo / hi planes is
// the entry plane -- for inv >= 0 min(ax, bx) is ax (lo with o+d), else bx (hi with o-d), exactly
// (fma is monotone in each operand) -- so a child costs 6 FMAs and four min / max instead of the
// pairwise min / max of slab32. The plane arrays are fetched at per-ray byte offsets in DNode4.
struct RayF4 {
    float inv[3], nsub[3], fsub[3];   // entry / exit plane offsets ((o+d)*inv or (o-d)*inv)
    uint32_t noff[3];                 // byte offset of the entry-plane array (lo_* or hi_*)
};
RS_CULL_HD RayF4 make_rayf4(const RayF& r) {
    RayF4 q;
    constexpr uint32_t lo_off[3] = {0, 16, 32}, hi_off[3] = {48, 64, 80};
    RS_CULL_UNROLL
    for (int k = 0; k < 3; ++k) {
        const bool pos = r.inv[k] >= 0.0f;
        q.inv[k] = r.inv[k];
        q.nsub[k] = pos ? r.opi[k] : r.omi[k];
        q.fsub[k] = pos ? r.omi[k] : r.opi[k];
        q.noff[k] = pos ? lo_off[k] : hi_off[k];
    }
    return q;
}
// the exit-plane array is the other one of the axis: lo_off ^ hi_off = 48, 80, 112
RS_CULL_HD uint32_t far_off(uint32_t noff, int k) { return noff ^ (k == 0 ? 48u : k == 1 ? 80u : 112u); }
RS_CULL_HD bool slab4(float nx, float ny, float nz, float fx, float fy, float fz, const RayF4& r, float tmin, float tmax,
                      float& entry) {
    const float ax = fmaf(nx, r.inv[0], -r.nsub[0]), bx = fmaf(fx, r.inv[0], -r.fsub[0]);
    const float ay = fmaf(ny, r.inv[1], -r.nsub[1]), by = fmaf(fy, r.inv[1], -r.fsub[1]);
    const float az = fmaf(nz, r.inv[2], -r.nsub[2]), bz = fmaf(fz, r.inv[2], -r.fsub[2]);
    float a = fminf(fmaxf(fmaxf(fmaxf(tmin, ax), ay), az), RS_CULL_FLT_MAX);
    float b = fminf(fminf(fminf(tmax, bx), by), bz);
    a = fmaf(-fabsf(a), 0x1p-18f, a);
    b = fmaf(fabsf(b), 0x1p-18f, b);
    entry = a;
    return a <= b;
}

}  // namespace rs
