// C entry points around raysnail_amd/csrc/rs_raymarch.h for tests/test_raymarch_cpu.py, which compiles this file
// with g++ -O2 -ffp-contract=off -shared -fPIC and compares it bit for bit with tests/golden/raymarch_kat.json.
#include "../../raysnail_amd/csrc/rs_raymarch.h"

namespace {
// AABB::hit (prelude/aabb.rs:20-38) of the marcher's bbox over [tmin, inf): the BVH leaf's test (bvh.rs:173-177)
bool leaf_box(const double o[3], const double d[3], double tmin) {
    double t_min = tmin, t_max = INFINITY;
    for (int i = 0; i < 3; ++i) {
        const double inv = 1.0 / d[i];
        double t0 = (-rs_rm::kRadius - o[i]) * inv, t1 = (rs_rm::kRadius - o[i]) * inv;
        if (inv < 0.0) { const double t = t0; t0 = t1; t1 = t; }
        t_min = std::fmax(t_min, t0);
        t_max = std::fmin(t_max, t1);
        if (t_max <= t_min) return false;
    }
    return true;
}
}  // namespace

extern "C" {

// RayMarcher::hit alone: 1 and *t1, or 0
int rm_hit_t(const double ray[7], double tmin, double* t1) {
    return rs_rm::hit_t(rs_rm::P3{ray[0], ray[1], ray[2]}, rs_rm::P3{ray[3], ray[4], ray[5]}, tmin, t1) ? 1 : 0;
}

// World::hit of a world holding the marcher alone (material id mat), in rs_probe_world_hit's layout:
// hit t1 t2 p(3) n(3) u v outside mat; a miss is 13 zeros
int rm_hit(const double ray[7], double tmin, int mat, double out[13]) {
    for (int k = 0; k < 13; ++k) out[k] = 0.0;
    double t1;
    if (!leaf_box(ray, ray + 3, tmin)) return 0;
    if (!rm_hit_t(ray, tmin, &t1)) return 0;
    const rs_rm::P3 p{std::fma(ray[3], t1, ray[0]), std::fma(ray[4], t1, ray[1]), std::fma(ray[5], t1, ray[2])};
    rs_rm::P3 n = rs_rm::normal(p);
    const bool outside = std::fma(ray[5], n.z, std::fma(ray[3], n.x, ray[4] * n.y)) < 0.0;  // HitRecord::new (hit.rs:32-53)
    if (!outside) n = rs_rm::P3{-n.x, -n.y, -n.z};
    out[0] = 1.0; out[1] = t1; out[2] = t1;
    out[3] = p.x; out[4] = p.y; out[5] = p.z; out[6] = n.x; out[7] = n.y; out[8] = n.z;
    out[11] = outside ? 1.0 : 0.0; out[12] = (double)mat;
    return 1;
}

int rm_contains(const double p[3]) { return rs_rm::is_inside(rs_rm::P3{p[0], p[1], p[2]}, rs_rm::kIterations) ? 1 : 0; }

double rm_distance_est(const double p[3]) { return rs_rm::distance_est(rs_rm::P3{p[0], p[1], p[2]}, rs_rm::kIterations); }

}  // extern "C"
