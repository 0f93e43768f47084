// The gate of the zero-throughput rule (raysnail_amd/csrc/rs_dead_gate.h) on the CPU: which scenes may end the paths
// whose throughput is exactly zero, and which cameras.
//
// Each case is a scene as the commit hands it to dead_gate_reach() -- materials, spheres, the lights as sphere indices,
// the background -- built from the RTIOW-shaped bench scene (a ground sphere of radius 1000, 22 x 22 balls of radius
// 0.2, three spheres of radius 1, a light of radius 12 at (300, 400, 100); Lambertian, Metal, Dielectric and
// DiffuseLight materials) by one change, and prints "case NAME want W got G". The last line is "ok".
//
// Stand-alone (no library): g++ -O2 -std=c++17 -ffp-contract=off tests/cpp/test_dead_gate.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../raysnail_amd/csrc/rs_dead_gate.h"

using namespace rs;

namespace {

struct Scene {
    std::vector<DMaterial> mats;
    std::vector<DSphere> sph;
    std::vector<uint32_t> lights;
    float bg_lo[3] = {0.3f, 0.4f, 0.5f}, bg_hi[3] = {0.7f, 0.89f, 1.0f};
    bool spheres_mode = true, moving = false;
    DeadGateIn in() const {
        DeadGateIn g;
        g.spheres_mode = spheres_mode; g.moving = moving;
        g.mats = mats.data(); g.n_mats = (uint32_t)mats.size();
        g.spheres = sph.data(); g.n_spheres = (uint32_t)sph.size();
        g.lights = lights.data(); g.n_lights = (uint32_t)lights.size();
        g.bg_lo = bg_lo; g.bg_hi = bg_hi;
        return g;
    }
};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
double rnd() {  // [0, 1)
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (double)(g_rng >> 11) * 0x1p-53;
}

DMaterial material(float r, float g, float b, double refractive = 1.0, double multiplier = 1.0) {
    DMaterial m;
    std::memset(&m, 0, sizeof(m));
    m.even[0] = m.odd[0] = r; m.even[1] = m.odd[1] = g; m.even[2] = m.odd[2] = b; m.even[3] = m.odd[3] = 1.0f;
    m.tex_scale = 1.0;
    m.enter_refractive = 1.0 / refractive; m.outer_refractive = refractive;
    m.multiplier = multiplier; m.mix_p = 0.5; m.phong_exponent = 1;
    return m;
}

DSphere sphere(double x, double y, double z, double r) {
    DSphere s;
    std::memset(&s, 0, sizeof(s));
    s.c[0] = x; s.c[1] = y; s.c[2] = z; s.r = r; s.r2 = r * r;
    return s;
}

Scene bench() {
    Scene sc;
    sc.mats = {material(0.5f, 0.5f, 0.5f), material(0.7f, 0.6f, 0.5f), material(1.0f, 1.0f, 1.0f, 1.5),
               material(1.0f, 0.9f, 0.7f, 1.0, 1.5), material(0.0f, 0.0f, 0.0f)};
    sc.sph.push_back(sphere(0.0, -1000.0, 0.0, 1000.0));
    for (int a = -11; a < 11; ++a)
        for (int b = -11; b < 11; ++b) {
            const DSphere q = sphere(a + 0.9 * rnd(), 0.2, b + 0.9 * rnd(), 0.2);
            const double dx = q.c[0] - 4.0, dz = q.c[2];
            if (std::sqrt(dx * dx + dz * dz) > 0.9) sc.sph.push_back(q);
        }
    sc.sph.push_back(sphere(0.0, 1.0, 0.0, 1.0));
    sc.sph.push_back(sphere(-4.0, 1.0, 0.0, 1.0));
    sc.sph.push_back(sphere(4.0, 1.0, 0.0, 1.0));
    sc.sph.push_back(sphere(300.0, 400.0, 100.0, 12.0));
    sc.lights = {(uint32_t)sc.sph.size() - 1};
    return sc;
}

int g_failed = 0;

void expect(const char* name, const Scene& sc, bool want) {
    const bool got = dead_gate(sc.in());
    std::printf("case %-52s want %d got %d%s\n", name, (int)want, (int)got, want == got ? "" : "  FAILED");
    if (want != got) g_failed = 1;
    if ((dead_gate_reach(sc.in()) > 0.0) != got) { std::printf("dead_gate != (reach > 0)  FAILED\n"); g_failed = 1; }
}

void expect_camera(const char* name, double reach, double x, double y, double z, bool want) {
    const double o[3] = {x, y, z};
    const bool got = dead_gate_camera(reach, o);
    std::printf("camera %-50s want %d got %d%s\n", name, (int)want, (int)got, want == got ? "" : "  FAILED");
    if (want != got) g_failed = 1;
}

}  // namespace

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const float nanf = std::numeric_limits<float>::quiet_NaN(), inff = std::numeric_limits<float>::infinity();
    const Scene base = bench();
    const uint32_t light = base.lights[0];

    expect("bench scene", base, true);
    const double M = dead_gate_reach(base.in());
    std::printf("bench scene reach %.17g\n", M);
    if (!(M >= 2000.0 && M <= 2000.0 * (1.0 + 1e-12))) { std::printf("reach is not |c| + r of the ground  FAILED\n"); g_failed = 1; }

    {   // the light (radius 12) strictly inside a glass sphere of radius 40 around it, off centre
        Scene sc = base;
        sc.sph.push_back(sphere(310.0, 395.0, 105.0, 40.0));
        expect("light strictly inside a large glass sphere", sc, true);
    }
    {   // a sphere whose surface cuts the light's ball
        Scene sc = base;
        sc.sph.push_back(sphere(300.0, 400.0, 120.0, 10.0));
        expect("sphere cutting the light's ball", sc, false);
    }
    {   // a sphere inside the light
        Scene sc = base;
        sc.sph.push_back(sphere(301.0, 402.0, 99.0, 3.0));
        expect("sphere inside the light", sc, false);
    }
    {   // the light at the centre of a sphere of its own size
        Scene sc = base;
        sc.sph.push_back(sphere(300.0, 400.0, 100.0, 12.0));
        expect("sphere coincident with the light", sc, false);
    }
    {   // tangent from outside: |c_s - c_l| = r_s + r_l exactly, then just inside the margin, then outside it
        Scene sc = base;
        sc.sph.push_back(sphere(300.0, 400.0, 100.0 + 12.0 + 5.0, 5.0));
        expect("sphere tangent to the light (outside)", sc, false);
        sc.sph.back() = sphere(300.0, 400.0, 100.0 + 17.0 * (1.0 + 0.5 * kDeadMargin), 5.0);
        expect("sphere apart by half the margin", sc, false);
        sc.sph.back() = sphere(300.0, 400.0, 100.0 + 17.0 * (1.0 + 2.0 * kDeadMargin), 5.0);
        expect("sphere apart by twice the margin", sc, true);
    }
    {   // tangent from inside: the light touches the enclosing sphere's surface
        Scene sc = base;
        sc.sph.push_back(sphere(300.0, 400.0, 100.0 + 28.0, 40.0));
        expect("light tangent to its enclosing sphere (inside)", sc, false);
        sc.sph.back() = sphere(300.0, 400.0, 100.0 + 28.0 * (1.0 - 0.5 * kDeadMargin), 40.0);
        expect("light inside by half the margin", sc, false);
        sc.sph.back() = sphere(300.0, 400.0, 100.0 + 27.0, 40.0);
        expect("light inside by one unit", sc, true);
    }
    {
        Scene sc = base;
        sc.sph[5].v[1] = 0.25;
        expect("moving sphere (speed set)", sc, false);
        Scene sd = base;
        sd.moving = true;
        expect("moving scene (DScene::moving)", sd, false);
    }
    {
        Scene sc = base;
        sc.spheres_mode = false;
        expect("not the spheres mode", sc, false);
    }
    {   // material numbers
        struct { const char* name; void (*set)(DMaterial&, double, float); } fields[] = {
            {"colour (even)", [](DMaterial& m, double, float f) { m.even[1] = f; }},
            {"colour (odd)", [](DMaterial& m, double, float f) { m.odd[2] = f; }},
            {"multiplier", [](DMaterial& m, double d, float) { m.multiplier = d; }},
            {"phong_factor", [](DMaterial& m, double d, float) { m.phong_factor = d; }},
            {"enter_refractive", [](DMaterial& m, double d, float) { m.enter_refractive = d; }},
            {"outer_refractive", [](DMaterial& m, double d, float) { m.outer_refractive = d; }},
            {"mix_p", [](DMaterial& m, double d, float) { m.mix_p = d; }},
            {"exponent", [](DMaterial& m, double d, float) { m.exponent = d; }},
        };
        for (const auto& f : fields) {
            char name[96];
            Scene sc = base;
            f.set(sc.mats[3], nan, nanf);
            std::snprintf(name, sizeof name, "NaN %s", f.name);
            expect(name, sc, false);
            sc = base;
            f.set(sc.mats[1], inf, inff);
            std::snprintf(name, sizeof name, "+inf %s", f.name);
            expect(name, sc, false);
            sc = base;
            f.set(sc.mats[0], -inf, -inff);
            std::snprintf(name, sizeof name, "-inf %s", f.name);
            expect(name, sc, false);
        }
        Scene sc = base;
        sc.mats[0].phong_factor = 4.0; sc.mats[0].phong_exponent = 2;
        expect("a Phong highlight (phong_factor > 0)", sc, false);
        sc = base;
        sc.mats[0].exponent = -0.5;
        expect("negative ReflectionPdf exponent", sc, false);
        sc = base;
        sc.mats[0].exponent = 800.0; sc.mats[0].phong_factor = -1.0;
        expect("exponent 800, phong_factor -1 (never read)", sc, true);
        sc = base;
        sc.mats[4].even[0] = -0.0f;
        expect("black and negative-zero colours", sc, true);
    }
    for (int k = 0; k < 3; ++k) {
        Scene sc = base;
        sc.bg_lo[k] = nanf;
        expect("NaN background (low)", sc, false);
        sc = base;
        sc.bg_hi[k] = inff;
        expect("infinite background (high)", sc, false);
    }
    {   // geometry numbers
        Scene sc = base;
        sc.sph[7].c[0] = nan;
        expect("NaN centre", sc, false);
        sc = base;
        sc.sph[7].r = inf;
        expect("infinite radius", sc, false);
        sc = base;
        sc.sph[7].r = 0.0; sc.sph[7].r2 = 0.0;
        expect("zero radius", sc, false);
        sc = base;
        sc.sph[7].r = -0.2;
        expect("negative radius (as |r|)", sc, true);
        sc = base;
        sc.sph[7].r = 1e-4; sc.sph[7].r2 = 1e-8;   // reach 2000 > 2^20 x 1e-4
        expect("a sphere 2^-20 of the scene's reach", sc, false);
        sc = base;   // the whole scene scaled by 2^-110: every ratio as before, the smallest radius below 2^-100
        for (DSphere& q : sc.sph) { for (int k = 0; k < 3; ++k) q.c[k] *= 0x1p-110; q.r *= 0x1p-110; q.r2 = q.r * q.r; }
        expect("scene scaled by 2^-110", sc, false);
        sc = base;
        for (DSphere& q : sc.sph) { for (int k = 0; k < 3; ++k) q.c[k] *= 0x1p-60; q.r *= 0x1p-60; q.r2 = q.r * q.r; }
        expect("scene scaled by 2^-60", sc, true);
        sc = base;
        sc.lights[0] = (uint32_t)sc.sph.size();
        expect("light index out of range", sc, false);
        sc = base;
        sc.sph.clear(); sc.lights.clear();
        expect("no spheres", sc, false);
    }
    {   // two lights, each clear of everything; then the second one cutting a ball
        Scene sc = base;
        sc.sph.push_back(sphere(-200.0, 300.0, 50.0, 8.0));
        sc.lights.push_back((uint32_t)sc.sph.size() - 1);
        expect("two lights, both clear", sc, true);
        sc.sph.back() = sphere(0.0, 1.0, 0.9, 0.5);
        expect("second light cutting a ball", sc, false);
    }
    (void)light;

    expect_camera("bench camera", M, 13.0, 2.0, 3.0, true);
    expect_camera("at twice the reach", M, 2.0 * M, 0.0, 0.0, true);
    expect_camera("beyond twice the reach", M, 0.0, -2.0 * M * (1.0 + 1e-12), 0.0, false);
    expect_camera("NaN origin", M, 0.0, nan, 0.0, false);
    expect_camera("infinite origin", M, 0.0, 0.0, inf, false);
    expect_camera("gate false (reach 0)", 0.0, 13.0, 2.0, 3.0, false);

    std::printf(g_failed ? "FAILED\n" : "ok\n");
    return g_failed;
}
