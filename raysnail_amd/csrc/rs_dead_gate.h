// rs_dead_gate.h — may a streaming frame end the paths whose throughput is exactly zero? (host only)
//
// The rule (rs_kernels.hip, WfState::end_dead): a path whose throughput T is == 0.0 in all three channels after a
// scatter is not carried on; it ends with close_path(0, T) = +0.0. The reference's recursion goes on below such a
// level and multiplies what it finds by the level's zero factor, so the two agree exactly when every term the path
// can still meet is finite: x * 0 is +-0 then, and 0.0 + (+-0) is +0.0, the value written. dead_gate() is true only
// for scenes where that is provable from the scene alone; dead_gate_camera() adds the frame's camera. DESIGN.md
// section 5 ("Ending zero-throughput paths") has the argument line by line; the conditions:
//
//   * the spheres mode (every hittable a sphere, materials of the shading classes) and no moving sphere;
//   * every number a path kernel reads from a material is finite and at most 2^100 in magnitude: the texture
//     colours (even, odd), multiplier, phong_factor, both refractive indices, mix_p; exponent is in [0, 2^100]
//     (ReflectionPdf's pow(u, 1 / (exponent + 1)) must stay in [0, 1]); no material has phong_factor > 0
//     (phong_highlight raises a dot product with the incoming direction, whose length the scene does not bound, to an
//     integer power: it can overflow to inf, and a negative exponent divides by zero);
//   * both background colours are finite and at most 2^100;
//   * every sphere's centre and radius are finite, 2^-100 <= rho <= |radius|, |centre| + |radius| <= M with M <= 2^20 rho
//     (rho: the smallest radius, M: the scene's reach): a hit point computed in f64 from an origin within 2 M per
//     axis then lies within rho / 16 of the sphere's surface (the root of the quadratic errs by a few
//     2^-52 |o - c|^2 / r <= 2^-50 (5 M)^2 / rho < 2^-5 rho), and its normal (p - c) / r is finite;
//   * no sphere's surface comes within a light's ball: for each light l and each other sphere s, with
//     d = |c_s - c_l| as computed in f64, either d > (r_s + r_l) (1 + 2^-20) -- apart -- or
//     (d + r_l) (1 + 2^-20) < r_s -- the light strictly inside s. A scatter point on s (within rho / 16 of its
//     surface, above) is then farther than r_l - rho / 8 >= 7/8 r_l from the light's centre F, so sphere_random's
//     onb_from(F - p) normalises a vector of length >= 7/8 rho, and the direction it returns is finite and not zero.
//     The margin 2^-20 covers d's own rounding (a few 2^-53 relative) a million times over.
//
// The camera (per frame): its origin is finite and within 2 M of the world's origin per axis, so the bound on the hit
// point's error holds for camera rays too (a path can reach T == 0 at its first hit: a black albedo).
#pragma once
#include <math.h>
#include <stdint.h>

#include "rs_layout.h"

namespace rs {

constexpr double kDeadBig = 0x1p100;       // the largest magnitude of a material or background number
constexpr double kDeadReach = 0x1p20;      // the scene's reach over its smallest radius, at most
constexpr double kDeadMargin = 0x1p-20;    // the relative margin of the light-ball tests

inline bool dead_num(double x) { return fabs(x) <= kDeadBig; }  // false for NaN and the infinities

// What the gate reads: the scene mode's answer, DScene::moving, the materials as the kernels get them, every sphere
// (lights included) and the lights as indices into `spheres`, the background.
struct DeadGateIn {
    bool spheres_mode = false;
    bool moving = false;
    const DMaterial* mats = nullptr; uint32_t n_mats = 0;
    const DSphere* spheres = nullptr; uint32_t n_spheres = 0;
    const uint32_t* lights = nullptr; uint32_t n_lights = 0;
    const float* bg_lo = nullptr; const float* bg_hi = nullptr;  // 3 channels each
};

// The scene's reach M (header comment) when zero-throughput paths may be ended, else 0.
inline double dead_gate_reach(const DeadGateIn& g) {
    if (!g.spheres_mode || g.moving) return 0.0;
    for (int k = 0; k < 3; ++k)
        if (!dead_num((double)g.bg_lo[k]) || !dead_num((double)g.bg_hi[k])) return 0.0;
    for (uint32_t i = 0; i < g.n_mats; ++i) {
        const DMaterial& m = g.mats[i];
        for (int k = 0; k < 3; ++k)
            if (!dead_num((double)m.even[k]) || !dead_num((double)m.odd[k])) return 0.0;
        if (!dead_num(m.multiplier) || !dead_num(m.enter_refractive) || !dead_num(m.outer_refractive) ||
            !dead_num(m.mix_p) || !dead_num(m.phong_factor) || !dead_num(m.exponent))
            return 0.0;
        if (!(m.exponent >= 0.0) || m.phong_factor > 0.0) return 0.0;
    }
    if (g.n_spheres == 0) return 0.0;
    double rho = INFINITY, M = 0.0;
    for (uint32_t i = 0; i < g.n_spheres; ++i) {
        const DSphere& s = g.spheres[i];
        const double r = fabs(s.r);
        if (!dead_num(r) || !(r > 0.0)) return 0.0;
        if (s.v[0] != 0.0 || s.v[1] != 0.0 || s.v[2] != 0.0) return 0.0;  // (moving, whatever the caller said)
        if (r < rho) rho = r;
        for (int k = 0; k < 3; ++k) {
            if (!dead_num(s.c[k])) return 0.0;
            if (fabs(s.c[k]) + r > M) M = fabs(s.c[k]) + r;
        }
    }
    if (!(rho >= 1.0 / kDeadBig) || !(M <= kDeadReach * rho)) return 0.0;  // (unit() squares lengths of about rho)
    for (uint32_t a = 0; a < g.n_lights; ++a) {
        if (g.lights[a] >= g.n_spheres) return 0.0;
        const DSphere& l = g.spheres[g.lights[a]];
        const double rl = fabs(l.r);
        for (uint32_t i = 0; i < g.n_spheres; ++i) {
            if (i == g.lights[a]) continue;
            const DSphere& s = g.spheres[i];
            const double rs = fabs(s.r);
            const double dx = s.c[0] - l.c[0], dy = s.c[1] - l.c[1], dz = s.c[2] - l.c[2];
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            const bool apart = d > (rs + rl) * (1.0 + kDeadMargin);
            const bool inside = (d + rl) * (1.0 + kDeadMargin) < rs;
            if (!apart && !inside) return 0.0;
        }
    }
    return M;
}

inline bool dead_gate(const DeadGateIn& g) { return dead_gate_reach(g) > 0.0; }

// The frame's part: the scene's gate (its reach, DScene::dead_reach) and a camera origin within 2 M per axis.
inline bool dead_gate_camera(double reach, const double origin[3]) {
    if (!(reach > 0.0)) return false;
    for (int k = 0; k < 3; ++k)
        if (!(fabs(origin[k]) <= 2.0 * reach)) return false;
    return true;
}

}  // namespace rs
