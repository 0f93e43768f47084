// rs_raymarch.h — RayMarcher, raysnail's Mandelbulb distance-estimator object
// (src/hittable/geometry/raymarching.rs), restated operation by operation on plain doubles.
//
// Shared bit for bit by the gfx950 kernels (rs_device.h, PK_RAYMARCH) and by host code: it depends on
// rs_crmath.h alone, so a plain C++ compiler builds it too (tests/cpp/raymarch_shim.cpp). Build with
// -ffp-contract=off: every + - * / below is one IEEE-754 double operation in the order the reference
// writes it, fma() exactly where the reference calls mul_add (Vec3::length_squared), sqrt is the IEEE
// one, and atan2 / pow / sin / cos / ln are the correctly rounded rs_cr:: functions.
//
// What a reader should not "fix":
//  * a point that escapes in iteration 0 leaves r = 0 (the power of the zero start value), so
//    distance_est is ln(0) * 0 = NaN; hit() turns a NaN estimate into 0.1 (:130-133). This is the common
//    case for camera rays, whose march therefore advances by 0.1 * 0.05 per step;
//  * hit() accepts on `length > unit_limit.start` (:141): a length along the unit direction is compared
//    with a ray parameter, and the range end is never read;
//  * dr's pow reads r after r was replaced by its eighth power (:217-220).
#pragma once
#include "../../include/rs_crmath.h"

#define RS_RM_HD RS_CR_HD
// iterate() is one real function per device unit: its callers reach it from 11 sites (the searches, the march,
// six distance estimates per normal), and each inlined copy would carry the whole of rs_crmath.h
// RS_RM_CALL marks the marcher's out-of-line device functions (iterate and rs_device.h's one per query). A kernel
// is given the registers of the hungriest function it can call, whether a scene has a marcher or not, and these
// take all 256 VGPRs; so only the kernels of the scenes that hold a marcher can call them (rs_internal.h kSmMarch).
#if defined(__HIPCC__)
#define RS_RM_CALL __noinline__
#define RS_RM_ITER __host__ __device__ RS_RM_CALL
#else
#define RS_RM_ITER
#endif

namespace rs_rm {

constexpr int kIterations = 100;   // RayMarcher::new (:33-38); is_inside / normal pass 100 as a literal
constexpr int kMarchLimit = 1000;  // hit(): `limit` (:120)
constexpr int kSearchSteps = 200;  // search_surface (:61)
constexpr int kBisectDepth = 8;    // search_surface -> binary_search_surface(.., 8) (:66)
constexpr double kRadius = 1.3;    // bbox (:167-176): +-1.3 about the origin

struct P3 { double x, y, z; };
struct Iter { double r, dr; bool inside; };

// Vec3::length (vec3.rs:152-161): sqrt(z.mul_add(z, x.mul_add(x, y * y)))
RS_RM_HD inline double length(P3 a) { return sqrt(fma(a.z, a.z, fma(a.x, a.x, a.y * a.y))); }

// iterate (:202-241)
RS_RM_ITER inline Iter iterate(P3 p, int iterations) {
    double x = 0.0, y = 0.0, z = 0.0;
    const double power = 8.0;
    double r = 0.0, dr = 0.0;
    for (int i = 0; i < iterations; ++i) {
        // to spherical coordinates
        r = sqrt(x * x + y * y + z * z);
        double theta = rs_cr::atan2_cr(sqrt(x * x + y * y), z);
        double phi = rs_cr::atan2_cr(y, x);
        // scale and rotate; dr reads the new r (:217-220)
        r = rs_cr::pow_cr(r, power);
        theta *= power;
        phi *= power;
        dr = rs_cr::pow_cr(r, power - 1.0) * power * dr + 1.0;
        // back to cartesian coordinates: (r * sin theta) * cos phi, (r * sin theta) * sin phi, r * cos theta
        double st, ct, sp, cp;
        rs_cr::sincos_cr(theta, &st, &ct);
        rs_cr::sincos_cr(phi, &sp, &cp);
        x = r * st * cp;
        y = r * st * sp;
        z = r * ct;
        // add c (iteration 0: 0.0 + p.x, so a negative zero of p becomes +0.0 as in the reference)
        x += p.x;
        y += p.y;
        z += p.z;
        if (x * x + y * y + z * z > 8.0) return Iter{r, dr, false};
    }
    return Iter{r, dr, true};
}

// is_inside (:189-192)
RS_RM_HD inline bool is_inside(P3 p, int iterations) { return iterate(p, iterations).inside; }

// distance_est (:195-199): ((0.5 * ln r) * r) / dr
RS_RM_HD inline double distance_est(P3 p, int iterations) {
    const Iter it = iterate(p, iterations);
    return 0.5 * rs_cr::log_cr(it.r) * it.r / it.dr;
}

// search_surface (:56-73) with binary_search_surface (:40-54) as a loop: the recursion only replaces
// one of its two end points per level and returns the outside one at depth 0
RS_RM_HD inline bool search_surface(P3 p, P3 direction, P3* out) {
    const P3 df{direction.x * 0.05, direction.y * 0.05, direction.z * 0.05};
    P3 v = p;
    for (int i = 0; i < kSearchSteps; ++i) {
        if (is_inside(v, kIterations)) {
            P3 outside{v.x - df.x, v.y - df.y, v.z - df.z}, inside = v;
            for (int depth = kBisectDepth; depth > 0; --depth) {
                const P3 mid{(outside.x + inside.x) * 0.5, (outside.y + inside.y) * 0.5, (outside.z + inside.z) * 0.5};
                if (is_inside(mid, 100)) inside = mid;
                else outside = mid;
            }
            *out = outside;
            return true;
        }
        v.x += df.x; v.y += df.y; v.z += df.z;
    }
    return false;
}

// hit (:108-160) up to the record: true and t1 (= t2) when the ray hits. tmin is unit_limit.start; the
// range end is not a parameter because the reference never reads it.
RS_RM_HD inline bool hit_t(P3 origin, P3 dir, double tmin, double* t1) {
    const double len = length(dir);
    const double inv = 1.0 / len;
    const P3 direction{dir.x * inv, dir.y * inv, dir.z * inv};
    P3 current = origin;
    int steps = 0;
    double best_distance = 1000000.0;
    double est_distance = 0.0;
    while (steps < kMarchLimit && est_distance < best_distance + 1.0) {
        steps += 1;
        est_distance = distance_est(current, kIterations);
        if (est_distance != est_distance) est_distance = 0.1;  // NaN check (:130-133)
        if (est_distance < 1.3) {
            P3 p;
            if (search_surface(current, direction, &p)) {
                const double length_ = length(P3{p.x - origin.x, p.y - origin.y, p.z - origin.z});
                if (length_ > tmin) {
                    *t1 = length_ / len;
                    return true;
                }
            }
            return false;
        }
        if (est_distance < best_distance) best_distance = est_distance;
        // current += &direction * est_distance * 0.05
        current.x += direction.x * est_distance * 0.05;
        current.y += direction.y * est_distance * 0.05;
        current.z += direction.z * est_distance * 0.05;
    }
    return false;
}

// normal (:78-91): central differences of distance_est at d = 0.01 (pos + (d, 0, 0) adds 0.0 to the
// other two components, pos - (d, 0, 0) subtracts it), then unit() = v * (1 / length) (vec3.rs:192-194)
RS_RM_HD inline P3 normal(P3 pos) {
    const double d = 0.01;
    const double gx = distance_est(P3{pos.x + d, pos.y + 0.0, pos.z + 0.0}, 100) -
                      distance_est(P3{pos.x - d, pos.y - 0.0, pos.z - 0.0}, 100);
    const double gy = distance_est(P3{pos.x + 0.0, pos.y + d, pos.z + 0.0}, 100) -
                      distance_est(P3{pos.x - 0.0, pos.y - d, pos.z - 0.0}, 100);
    const double gz = distance_est(P3{pos.x + 0.0, pos.y + 0.0, pos.z + d}, 100) -
                      distance_est(P3{pos.x - 0.0, pos.y - 0.0, pos.z - d}, 100);
    const double inv = 1.0 / length(P3{gx, gy, gz});
    return P3{gx * inv, gy * inv, gz * inv};
}

}  // namespace rs_rm
