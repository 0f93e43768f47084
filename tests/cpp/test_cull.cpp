// The f32 cull of the tree walks (raysnail_amd/csrc/rs_cull.h) against the exact f64 box test, on the CPU.
// Build as the kernels are built: g++ -O2 -std=c++17 -ffp-contract=off.
//
// Property, for every case (a box [lo, hi], a ray (o, d), a range [tmin, best)): if slab64(lo, hi, o, 1 / d, tmin,
// best) accepts, then slab32 and slab4 accept the outward-rounded f32 box of that box and of a strictly larger one,
// with tmin32 = -round_up_f(-tmin) and best32 = round_up_f(best), and the entry they report is not NaN (the
// near-first walk orders and counts a node's children by it). slab4 equals slab32 on every case (the header's
// guarantee; counted apart for the rays whose f32 quantities are all finite).
// Every family is seeded, prints its count of exact accepts and must have at least 10 % of them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../raysnail_amd/csrc/rs_cull.h"

using namespace rs;

namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }
    double u01() { return (double)(next() >> 11) * 0x1p-53; }   // [0, 1)
    double sym() { return 2.0 * u01() - 1.0; }                  // [-1, 1)
    int below(int n) { return (int)(next() % (uint64_t)n); }
    int range(int a, int b) { return a + below(b - a + 1); }    // [a, b]
    bool coin() { return (next() >> 40) & 1; }
};

struct Fam {
    const char* name;
    uint64_t n = 0, acc = 0, miss32 = 0, miss4 = 0, nan_entry = 0, diff = 0, finite = 0, diff_finite = 0;
    int shown = 0;
    explicit Fam(const char* nm) : name(nm) {}
};

int g_failed = 0;

bool ray_finite(const RayF& r) {
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(r.inv[k]) || !std::isfinite(r.opi[k]) || !std::isfinite(r.omi[k])) return false;
    return true;
}

// slab4 as the walks call it: the entry / exit planes picked by the ray's byte offsets
bool slab4_box(const float lo[3], const float hi[3], const RayF4& q, float tmin, float tmax, float& e) {
    const uint32_t lo_off[3] = {0, 16, 32};
    float n[3], f[3];
    for (int k = 0; k < 3; ++k) {
        const bool near_lo = q.noff[k] == lo_off[k];
        if (far_off(q.noff[k], k) != (near_lo ? lo_off[k] + 48u : lo_off[k])) { std::printf("far_off is wrong\n"); g_failed = 1; }
        n[k] = near_lo ? lo[k] : hi[k];
        f[k] = near_lo ? hi[k] : lo[k];
    }
    return slab4(n[0], n[1], n[2], f[0], f[1], f[2], q, tmin, tmax, e);
}

struct Verdict { bool exact, s32, s4; };

Verdict check(Fam& F, const double lo[3], const double hi[3], const V3& o, const V3& d, double tmin, double best) {
    const V3 inv = {1.0 / d.x, 1.0 / d.y, 1.0 / d.z};
    const bool e = slab64(lo, hi, o, inv, tmin, best);
    const RayF rf = make_rayf(o, inv);
    const RayF4 rq = make_rayf4(rf);
    const float tmin32 = -round_up_f(-tmin), best32 = round_up_f(best);
    const bool fin = ray_finite(rf);
    ++F.n;
    F.acc += e;
    F.finite += fin;
    Verdict v{e, true, true};
    // the box itself, then a strictly larger one (a parent's)
    for (int pass = 0; pass < 2; ++pass) {
        double l[3], h[3];
        for (int k = 0; k < 3; ++k) {
            l[k] = lo[k]; h[k] = hi[k];
            if (pass == 1) {
                const double g = (h[k] - l[k]) * 0.25 + std::fabs(l[k]) * 0x1p-30;
                l[k] = std::fmin(l[k] - g, std::nextafter(l[k], -INFINITY));
                h[k] = std::fmax(h[k] + g, std::nextafter(h[k], INFINITY));
                if (lo[k] != lo[k]) l[k] = lo[k];
                if (hi[k] != hi[k]) h[k] = hi[k];
            }
        }
        const float lf[3] = {round_down_f(l[0]), round_down_f(l[1]), round_down_f(l[2])};
        const float hf[3] = {round_up_f(h[0]), round_up_f(h[1]), round_up_f(h[2])};
        for (int k = 0; k < 3; ++k)
            if ((double)lf[k] > l[k] || (double)hf[k] < h[k]) { std::printf("outward rounding is wrong\n"); g_failed = 1; }
        float e32 = 0.0f, e4 = 0.0f;
        const bool a = slab32(lf, hf, rf, tmin32, best32, e32), b = slab4_box(lf, hf, rq, tmin32, best32, e4);
        if (pass == 0) { v.s32 = a; v.s4 = b; }
        const bool m32 = e && !a, m4 = e && !b;
        const bool ne = (a && e32 != e32) || (b && e4 != e4);
        F.miss32 += m32; F.miss4 += m4; F.nan_entry += ne;
        F.diff += a != b;
        F.diff_finite += fin && a != b;
        if ((m32 || m4 || ne || a != b) && F.shown < 4) {
            ++F.shown;
            std::printf("  %s: exact %d slab32 %d slab4 %d (entries %a %a)%s lo %a %a %a hi %a %a %a o %a %a %a d %a %a %a tmin %g best %a\n",
                        F.name, (int)e, (int)a, (int)b, e32, e4, pass ? " [parent box]" : "", l[0], l[1], l[2], h[0], h[1],
                        h[2], o.x, o.y, o.z, d.x, d.y, d.z, tmin, best);
        }
    }
    return v;
}

void report(const Fam& F) {
    const bool ok = F.miss32 == 0 && F.miss4 == 0 && F.nan_entry == 0 && F.diff == 0 && F.acc * 10 >= F.n;
    std::printf("%-12s %9llu cases, %9llu exact accepts (%4.1f %%), missed by slab32 %llu, by slab4 %llu, NaN entries %llu, "
                "slab4 != slab32 %llu (%llu of the %llu with a finite f32 ray)%s\n",
                F.name, (unsigned long long)F.n, (unsigned long long)F.acc, 100.0 * (double)F.acc / (double)(F.n ? F.n : 1),
                (unsigned long long)F.miss32, (unsigned long long)F.miss4, (unsigned long long)F.nan_entry,
                (unsigned long long)F.diff, (unsigned long long)F.diff_finite, (unsigned long long)F.finite,
                ok ? "" : "  FAILED");
    if (!ok) g_failed = 1;
}

const double kTmin[3] = {0.0, 1e-4, 0.5};

// A box with centre, half sizes at scale 2^ec / 2^eh (shape: 0 plain, 1 one axis of zero thickness, 2 one axis
// 2^-5k thinner) and a point of it: per axis a plane or an interior coordinate (3 planes: a corner, 2: an edge,
// 1: a face point, 0: an interior point).
void make_box(Rng& g, int ec, int eh, int shape, double lo[3], double hi[3], double p[3]) {
    const double sc = std::ldexp(1.0, ec), sh = std::ldexp(1.0, eh);
    const int ax = g.below(3);
    for (int k = 0; k < 3; ++k) {
        const double c = g.sym() * sc;
        double h = (0.05 + g.u01()) * sh;
        if (k == ax && shape == 1) h = 0.0;
        if (k == ax && shape == 2) h = std::ldexp(h, -5 * g.range(1, 12));
        lo[k] = c - h; hi[k] = c + h;
        const int w = g.below(10);
        p[k] = w < 4 ? lo[k] : w < 8 ? hi[k] : lo[k] + (hi[k] - lo[k]) * g.u01();
        if (p[k] < lo[k]) p[k] = lo[k];
        if (p[k] > hi[k]) p[k] = hi[k];
    }
}

// the direction from o to p as subtracted (t = 1 at p), normalised (t = the distance) or scaled by 2^e (t = 2^-e);
// returns the aimed point's t
double aim(Rng& g, const double o[3], const double p[3], int emax, double d[3]) {
    for (int k = 0; k < 3; ++k) d[k] = p[k] - o[k];
    const int mode = g.below(3);
    if (mode == 1) {
        const double l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (l > 0.0 && std::isfinite(l)) { for (int k = 0; k < 3; ++k) d[k] /= l; return l; }
    } else if (mode == 2) {
        const int e = g.range(-emax, emax);
        for (int k = 0; k < 3; ++k) d[k] = std::ldexp(d[k], e);
        return std::ldexp(1.0, -e);
    }
    return 1.0;
}

// the range end: +inf, or a finite one on either side of the aimed point's t
double range_end(Rng& g, double tp) {
    switch (g.below(10)) {
    case 0: return tp * 0.5;
    case 1: return tp * (1.0 - 0x1p-30);
    case 2: return tp * (1.0 + 0x1p-30);
    case 3: return tp * 2.0;
    case 4: return tp * 4.0 * g.u01();
    default: return INFINITY;
    }
}

V3 v(const double a[3]) { return V3{a[0], a[1], a[2]}; }

// scales 2^e, e independent in [-emax, emax] for the centre, the half size and the origin; shape as make_box;
// plane: the origin lies exactly on one of the box's planes
void family_scales(Fam& F, uint64_t seed, uint64_t n, int emax, int shape, bool plane) {
    Rng g{seed};
    for (uint64_t i = 0; i < n; ++i) {
        double lo[3], hi[3], p[3], o[3], d[3];
        make_box(g, g.range(-emax, emax), g.range(-emax, emax), shape < 0 ? g.below(3) : shape, lo, hi, p);
        const double so = std::ldexp(1.0, g.range(-emax, emax));
        for (int k = 0; k < 3; ++k) o[k] = g.sym() * so;
        if (plane) { const int k = g.below(3); o[k] = g.coin() ? lo[k] : hi[k]; }
        // (the exact test accepts a box of zero thickness only for a ray that lies in its plane: t0 = t1 otherwise)
        if (shape == 1 && g.below(10) < 7)
            for (int k = 0; k < 3; ++k) if (lo[k] == hi[k]) o[k] = lo[k];
        const double tp = aim(g, o, p, emax, d);
        check(F, lo, hi, v(o), v(d), kTmin[g.below(3)], range_end(g, tp));
    }
}

// one direction component replaced: kind 0 exactly +-0, 1: +-2^-100 .. 2^-136, 2: in (1e-38, 1e-30) (1 / d beyond the
// cull's own range: the clamp band), 3: NaN. The origin lies in the box's slab of that axis (or on its planes) in
// most cases, as the exact test needs to accept; with a finite tiny component the slab is in part one the ray
// crosses about where it reaches the aimed point. far: origins and boxes up to 2^40 from the coordinate origin.
void family_component(Fam& F, uint64_t seed, uint64_t n, int kind, bool far) {
    Rng g{seed};
    for (uint64_t i = 0; i < n; ++i) {
        double lo[3], hi[3], p[3], o[3], d[3];
        const int emax = far ? 40 : 8;
        make_box(g, g.range(-emax, emax), g.range(-8, 8), g.below(3), lo, hi, p);
        const double so = std::ldexp(1.0, g.range(-emax, emax));
        for (int k = 0; k < 3; ++k) o[k] = far && g.coin() ? p[k] + g.sym() * std::ldexp(1.0, g.range(-8, 8)) : g.sym() * so;
        const int k = g.below(3);
        double dk = 0.0;
        if (kind == 0) dk = g.coin() ? 0.0 : -0.0;
        if (kind == 1) dk = (g.coin() ? 1.0 : -1.0) * std::ldexp(1.0 + g.u01(), -g.range(100, 136));
        if (kind == 2) dk = (g.coin() ? 1.0 : -1.0) * std::exp(std::log(1e-38) + g.u01() * (std::log(1e-30) - std::log(1e-38)));
        if (kind == 3) dk = NAN;
        const int w = g.below(10);
        if ((kind == 1 || kind == 2) && w < 4) {
            // a slab about the coordinate origin as thin as the ray's travel on this axis
            const double h = std::fabs(dk) * std::ldexp(1.0, g.range(-3, 6));
            lo[k] = -h * g.u01(); hi[k] = h * g.u01();
            o[k] = lo[k] + (hi[k] - lo[k]) * g.u01() - dk * g.u01();
        } else if (w < 8) {
            o[k] = lo[k] + (hi[k] - lo[k]) * g.u01();
        } else if (w < 9) {
            o[k] = g.coin() ? lo[k] : hi[k];
        }
        const double tp = aim(g, o, p, 30, d);
        d[k] = dk;
        const double tmin = kTmin[g.below(3)], best = range_end(g, tp);
        const Verdict a = check(F, lo, hi, v(o), v(d), tmin, best);
        if (kind == 3) {
            // the NaN axis is ignored: the verdicts do not depend on the box's extent there
            lo[k] += 1e10; hi[k] += 2e10;
            Fam scratch("nan moved");
            const Verdict b = check(scratch, lo, hi, v(o), v(d), tmin, best);
            if (a.exact != b.exact || a.s32 != b.s32 || a.s4 != b.s4) { ++F.diff; }
        }
    }
}

bool hand(const char* name, double l0, double l1, double l2, double h0, double h1, double h2, V3 o, V3 d) {
    const double lo[3] = {l0, l1, l2}, hi[3] = {h0, h1, h2};
    Fam F(name);
    const Verdict r = check(F, lo, hi, o, d, 1e-4, INFINITY);
    const bool ok = r.exact && F.miss32 == 0 && F.miss4 == 0 && F.nan_entry == 0 && F.diff == 0;
    std::printf("hand case %-28s exact %d slab32 %d slab4 %d%s\n", name, (int)r.exact, (int)r.s32, (int)r.s4, ok ? "" : "  FAILED");
    if (!ok) g_failed = 1;
    return ok;
}

}  // namespace

int main() {
    {
        Fam a("wide +-140"), b("mid +-30"), c("zero-thick"), d("thin axis"), e("on a plane");
        family_scales(a, 1, 2500000, 140, -1, false); report(a);
        family_scales(b, 2, 2500000, 30, -1, false); report(b);
        family_scales(c, 3, 500000, 30, 1, false); report(c);
        family_scales(d, 4, 500000, 30, 2, false); report(d);
        family_scales(e, 5, 1000000, 30, -1, true); report(e);
    }
    {
        Fam a("d = +-0"), b("d = +-0 far"), c("d tiny"), d("d tiny far"), e("clamp band"), f("band far"), n("d = NaN");
        family_component(a, 6, 500000, 0, false); report(a);
        family_component(b, 7, 500000, 0, true); report(b);
        family_component(c, 8, 400000, 1, false); report(c);
        family_component(d, 9, 300000, 1, true); report(d);
        family_component(e, 10, 400000, 2, false); report(e);
        family_component(f, 11, 300000, 2, true); report(f);
        family_component(n, 12, 300000, 3, false); report(n);
    }
    // the three classes of misses this test was written for (profiles/cull/README.md), by name
    for (int e = 30; e >= 28; --e) {
        const double T = std::ldexp(1.0, e);
        char name[64];
        std::snprintf(name, sizeof name, "A, product overflows, 2^%d", e);
        hand(name, T - 1, -1, 4, T + 1, 1, 6, V3{T, 0, 0}, V3{0, 0, 1});
    }
    const double B = std::ldexp(1.0, 130), w = std::ldexp(1.0, 90), back = std::ldexp(1.0, 100);
    hand("B, origin beyond FLT_MAX, +", B - w, -B, -B, B + w, B, B, V3{B - back, 0, 0}, V3{1, 0, 0});
    hand("B, origin beyond FLT_MAX, -", -B - w, -B, -B, -B + w, B, B, V3{-B - back, 0, 0}, V3{1, 0, 0});
    hand("C, clamp band", 4, -1, -1, 6, 1, 1e-32, V3{0, 0, 0}, V3{1, 0, 1e-33});
    std::printf(g_failed ? "FAILED\n" : "ok\n");
    return g_failed;
}
