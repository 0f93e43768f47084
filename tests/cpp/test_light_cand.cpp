// The per-cell candidate lists of the spheres mode's light-sample rays (raysnail_amd/csrc/rs_light_cand.h, the
// criterion cand_beam_ball / cand_sphere of rs_cam_cand.h) on the CPU.
//
// A restatement of the list build by brute force, every sphere against every tested cell (a superset of what the
// GPU's tree walk finds: the walk only culls with the same function on node boxes), checked against rays drawn from
// the exact family: 4,096 rays per tested cell with origins at the cell's corners, face centres, edges and interior
// and just across its faces, aimed at points on and inside the light's ball, the rim at the membership check's limit
// included, and 64 more aimed at each of the scene's marked spheres. A ray counts as from the cell the shared
// light_cell() maps its origin to, and as of the family when the shared light_member() says so (the kernel sends
// every other ray to the tree walk); such a ray is intersected with every sphere by the renderer's sphere_t
// arithmetic over [0.0001, inf), and every sphere it hits -- the closest one, which the kernel's list loop must
// find, among them -- must be in the cell's packed record unless the record is marked overflow.
// Scenes: the RTIOW-shaped bench scene (and the spheres of a file given as argv[1], "cx cy cz r" per line, the light's
// line number as argv[2]); a huge light one cell away from a small grid (every beam `wide`: every cell overflows); a
// light inside the grid; a 0.01-radius sphere 1,000 units along a beam, off its axis by 0.9 of the beam's radius
// there; two identical spheres. light_cell() must map non-finite and out-of-box origins to "outside".
// Teeth: with the lists built for 0.7 rho, or for 0.7 of the cell ball's radius, the same rays must find spheres that
// are not listed. Measured with this program (g++ -O2 -ffp-contract=off, x86-64; printed on every run): 0.7 of the
// cell ball on the bench scene, 764 hits not listed (695 of them the ray's closest); 0.7 rho on the far small sphere's
// scene, 778 (774 the closest). (0.7 rho finds nothing on the bench scene itself: its light is 510 units away, so near the balls the beam's
// radius is the cell ball's and rho adds a few hundredths to it.)
//
// --lists FILE LIGHT [HITS [MAX_CELLS]]: the gate's figures for a scene file instead of the checks -- the grid, the
// histogram of list lengths over the cells that a sphere's surface passes through, their overflow share, and for the
// points of HITS ("x y z" per line: first hits) the share outside the grid or in overflow cells.
//
// Stand-alone (no library): g++ -O2 -std=c++17 -ffp-contract=off tests/cpp/test_light_cand.cpp; prints "ok" last and exits 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "../../raysnail_amd/csrc/rs_light_cand.h"

using namespace rs;

struct Sph { double c[3], r; };
struct Scene {
    std::vector<Sph> s;
    uint32_t light = 0;
    std::vector<uint32_t> marked;   // spheres that get rays aimed at them
};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double rnd() {  // [0, 1)
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (double)(g_rng >> 11) * 0x1p-53;
}
static void rnd_unit(double u[3]) {
    for (;;) {
        double l2 = 0.0;
        for (int k = 0; k < 3; ++k) { u[k] = 2.0 * rnd() - 1.0; l2 += u[k] * u[k]; }
        if (l2 > 1e-4 && l2 <= 1.0) { const double inv = 1.0 / std::sqrt(l2); for (int k = 0; k < 3; ++k) u[k] *= inv; return; }
    }
}

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++g_fail;                                        \
        }                                                    \
    } while (0)

static LightGrid grid_of(const Scene& sc, uint32_t max_cells = 0) {
    std::vector<double> c, r;
    for (const Sph& q : sc.s) { c.push_back(q.c[0]); c.push_back(q.c[1]); c.push_back(q.c[2]); r.push_back(q.r); }
    return light_grid_make(c.data(), r.data(), (uint32_t)sc.s.size(), sc.light, max_cells);
}

// Sphere::hit over [tmin, inf) with sphere_t's arithmetic (sphere.rs:83-109): the root it would return, or -1
static double sphere_root(const Sph& s, const double o[3], const double d[3], double tmin) {
    const double l[3] = {o[0] - s.c[0], o[1] - s.c[1], o[2] - s.c[2]};
    const double half_b = d[0] * l[0] + d[1] * l[1] + d[2] * l[2];
    const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const double c = l[0] * l[0] + l[1] * l[1] + l[2] * l[2] - s.r * s.r;
    const double delta = half_b * half_b - a * c;
    if (delta < 0.0) return -1.0;
    const double sq = std::sqrt(delta);
    const double t1 = (-half_b - sq) / a, t2 = (-half_b + sq) / a;
    if (t1 >= tmin) return t1;
    if (t2 >= tmin) return t2;
    return -1.0;
}

// the cell's record by brute force; k_rho / k_ball scale the light's radius / the cell ball's (1: the product's)
struct Record { uint32_t e[kCandMax]; uint32_t n; bool overflow; };
static Record build_record(const LightGrid& g, const std::vector<Sph>& sph, uint32_t cell, double k_rho = 1.0, double k_ball = 1.0) {
    double O[3], R;
    light_cell_ball(g, cell, O, &R);
    const CandBeam b = cand_beam_ball(O, R * k_ball, g.f, g.rho * k_rho);
    CandList l;
    cand_list_init(l);
    if (!b.ok) l.n = kCandMax + 1;
    for (size_t i = 0; i < sph.size() && !cand_list_overflow(l); ++i) {
        double along;
        if (cand_sphere(b, sph[i].c, sph[i].r, &along)) cand_list_add(l, (uint32_t)i, along);
    }
    uint32_t w[4];
    cand_list_pack(l, w);
    Record r;
    r.n = 0;
    r.overflow = (w[0] & 0xFFFFu) == kCandOverflow;
    for (uint32_t k = 0; k < kCandMax && !r.overflow; ++k) {
        const uint32_t e = (w[k / 2] >> (16 * (k & 1))) & 0xFFFFu;
        if (e == kCandEmpty) break;
        r.e[r.n++] = e;
    }
    return r;
}

// does a sphere's surface pass through the cell's cube?
static bool surface_in_cell(const LightGrid& g, uint32_t cell, const Sph& s) {
    const uint32_t idx[3] = {cell % g.n[0], (cell / g.n[0]) % g.n[1], cell / (g.n[0] * g.n[1])};
    double near2 = 0.0, far2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double lo = g.lo[k] + idx[k] * g.h, hi = lo + g.h;
        const double dn = s.c[k] < lo ? lo - s.c[k] : s.c[k] > hi ? s.c[k] - hi : 0.0;
        const double df = std::fmax(std::fabs(s.c[k] - lo), std::fabs(s.c[k] - hi));
        near2 += dn * dn; far2 += df * df;
    }
    return near2 <= s.r * s.r && s.r * s.r <= far2;
}

// the cells to test: those of about n_cells random surface points of the scene's spheres that lie in the grid, and
// the grid's eight corner cells
static std::vector<uint32_t> pick_cells(const Scene& sc, const LightGrid& g, uint32_t n_cells) {
    std::vector<uint32_t> cells;
    for (uint32_t c = 0; c < 8; ++c)
        cells.push_back((((c & 4) ? g.n[2] - 1 : 0) * g.n[1] + ((c & 2) ? g.n[1] - 1 : 0)) * g.n[0] + ((c & 1) ? g.n[0] - 1 : 0));
    for (uint32_t tries = 0; cells.size() < n_cells + 8 && tries < 100 * n_cells; ++tries) {
        const Sph& q = sc.s[(size_t)(rnd() * sc.s.size()) % sc.s.size()];
        double u[3];
        rnd_unit(u);
        const double p[3] = {q.c[0] + q.r * u[0], q.c[1] + q.r * u[1], q.c[2] + q.r * u[2]};
        const uint32_t cell = light_cell(g, p);
        if (cell != kLightOutside) cells.push_back(cell);
    }
    return cells;
}

struct Tally { uint64_t rays = 0, not_member = 0, outside = 0, over = 0, hits = 0, missed = 0, winner_missed = 0; };

// One ray against the record of the cell its origin maps to.
static void check_ray(const char* name, const Scene& sc, const LightGrid& g, std::map<uint32_t, Record>& recs, const double o[3],
                      const double d[3], double k_rho, double k_ball, bool report, Tally& t) {
    const uint32_t cell = light_cell(g, o);
    if (cell == kLightOutside) { ++t.outside; return; }
    if (!light_member(g, o, d)) { ++t.not_member; return; }
    auto it = recs.find(cell);
    if (it == recs.end()) it = recs.emplace(cell, build_record(g, sc.s, cell, k_rho, k_ball)).first;
    const Record& r = it->second;
    if (r.overflow) { ++t.over; return; }
    ++t.rays;
    double best = std::numeric_limits<double>::infinity();
    bool best_in = true;
    for (size_t i = 0; i < sc.s.size(); ++i) {
        const double root = sphere_root(sc.s[i], o, d, 0.0001);
        if (root < 0.0) continue;
        ++t.hits;
        bool in = false;
        for (uint32_t q = 0; q < r.n; ++q) in = in || r.e[q] == (uint32_t)i;
        if (!in) ++t.missed;
        if (root < best) { best = root; best_in = in; } else if (root == best) best_in = best_in && in;
        if (report)
            CHECK(in, "%s: cell %u ray o %.17g %.17g %.17g d %.17g %.17g %.17g hits sphere %zu (c %.17g %.17g %.17g r %.17g) at t %.17g, not in its record of %u",
                  name, cell, o[0], o[1], o[2], d[0], d[1], d[2], i, sc.s[i].c[0], sc.s[i].c[1], sc.s[i].c[2], sc.s[i].r, root, r.n);
    }
    if (!best_in) ++t.winner_missed;
}

// The family of the picked cells against their records. k_rho, k_ball != 1: the teeth (nothing is reported, the
// tally is returned).
static Tally check_scene(const char* name, const Scene& sc, uint32_t n_cells, double k_rho = 1.0, double k_ball = 1.0) {
    const LightGrid g = grid_of(sc);
    Tally t;
    const bool report = k_rho == 1.0 && k_ball == 1.0;
    CHECK(g.cells > 0, "%s: no grid", name);
    if (!g.cells) return t;
    std::map<uint32_t, Record> recs;
    const double rho_m = std::sqrt(g.rho2m);
    for (const uint32_t cell : pick_cells(sc, g, n_cells)) {
        const uint32_t idx[3] = {cell % g.n[0], (cell / g.n[0]) % g.n[1], cell / (g.n[0] * g.n[1])};
        for (int k = 0; k < 4096 + 64 * (int)sc.marked.size(); ++k) {
            double o[3], d[3], q[3];
            // origins: 0-7 the corners, 8-13 the face centres, then by k & 3: a point on an edge or a face (each
            // coordinate at an end or inside), a point just across a face (the neighbour's, or outside the grid), two interior
            for (int a = 0; a < 3; ++a) {
                double f;
                if (k < 8) f = (k >> a) & 1;
                else if (k < 14) f = (k - 8) / 2 == a ? (double)((k - 8) & 1) : 0.5;
                else if ((k & 3) == 0) { const double e = rnd(); f = e < 0.3 ? 0.0 : e < 0.6 ? 1.0 : rnd(); }
                else f = rnd();
                o[a] = g.lo[a] + ((double)idx[a] + f) * g.h;
                if (k >= 14 && (k & 3) == 1 && a == (k >> 2) % 3) o[a] = std::nextafter(g.lo[a] + (double)(idx[a] + (k & 16 ? 1 : 0)) * g.h, k & 32 ? 1e300 : -1e300);
            }
            // targets: the first 4096 at the light's ball -- a quarter on the rim at the membership check's limit (the
            // ray's distance from F is rho sqrt(1 - 2^-20), just inside it or just beyond), a quarter on the sphere
            // |Fq - F| = rho, the rest inside; then 64 per marked sphere, at it
            const double w[3] = {g.f[0] - o[0], g.f[1] - o[1], g.f[2] - o[2]};
            const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            double u[3];
            rnd_unit(u);
            if (k >= 4096) {
                const Sph& m = sc.s[sc.marked[(k - 4096) / 64]];
                const double rr = (k & 1) ? m.r * (1.0 - 0x1p-30) : m.r * rnd();
                for (int a = 0; a < 3; ++a) q[a] = m.c[a] + rr * u[a];
            } else if ((k & 3) == 0 && wl > g.rho) {
                // u := its part perpendicular to w, unit; the target F + rr u has the ray pass F at rr |w| / sqrt(|w|^2 + rr^2)
                const double p = (u[0] * w[0] + u[1] * w[1] + u[2] * w[2]) / (wl * wl);
                double l2 = 0.0;
                for (int a = 0; a < 3; ++a) { u[a] -= p * w[a]; l2 += u[a] * u[a]; }
                if (l2 < 1e-12) continue;
                const double lim = rho_m * ((k & 12) == 0 ? 1.0 : (k & 12) == 4 ? 1.0 - 0x1p-30 : (k & 12) == 8 ? 1.0 - 0x1p-48 : 1.0 + 0x1p-48);
                const double rr = lim * wl / std::sqrt(wl * wl - lim * lim);
                for (int a = 0; a < 3; ++a) q[a] = g.f[a] + rr * u[a] / std::sqrt(l2);
            } else {
                const double rr = (k & 3) == 1 ? g.rho : g.rho * std::cbrt(rnd());
                for (int a = 0; a < 3; ++a) q[a] = g.f[a] + rr * u[a];
            }
            double dl = 0.0;
            for (int a = 0; a < 3; ++a) { d[a] = q[a] - o[a]; dl += d[a] * d[a]; }
            if (!(dl > 0.0)) continue;
            if (k & 64) { dl = 1.0 / std::sqrt(dl); for (int a = 0; a < 3; ++a) d[a] *= dl; }  // the shading's unit directions
            check_ray(name, sc, g, recs, o, d, k_rho, k_ball, report, t);
        }
    }
    uint64_t over = 0;
    for (const auto& r : recs) over += r.second.overflow ? 1 : 0;
    std::printf("%-16s %ux%ux%u cells of %.4f, %zu spheres; rho x %.1f ball x %.1f: %llu rays, %llu sphere hits, %llu not listed (%llu of them the closest); "
                "%llu rays not of the family, %llu from outside the grid, %llu from overflow cells (%llu of %zu cells)\n",
                name, g.n[0], g.n[1], g.n[2], g.h, sc.s.size(), k_rho, k_ball, (unsigned long long)t.rays, (unsigned long long)t.hits,
                (unsigned long long)t.missed, (unsigned long long)t.winner_missed, (unsigned long long)t.not_member,
                (unsigned long long)t.outside, (unsigned long long)t.over, (unsigned long long)over, recs.size());
    return t;
}

// the layout of RTIOW-13.1 (examples/common/scene.rs): ground, a 22 x 22 field of small spheres, three large ones, the light
static Scene rtiow_like() {
    Scene sc;
    sc.s.push_back({{0.0, -1000.0, 0.0}, 1000.0});
    for (int a = -11; a < 11; ++a)
        for (int b = -11; b < 11; ++b) {
            const Sph q = {{a + 0.9 * rnd(), 0.2, b + 0.9 * rnd()}, 0.2};
            const double dx = q.c[0] - 4.0, dz = q.c[2];
            if (std::sqrt(dx * dx + dz * dz) > 0.9) sc.s.push_back(q);
        }
    sc.s.push_back({{0.0, 1.0, 0.0}, 1.0});
    sc.s.push_back({{-4.0, 1.0, 0.0}, 1.0});
    sc.s.push_back({{4.0, 1.0, 0.0}, 1.0});
    sc.s.push_back({{300.0, 400.0, 100.0}, 12.0});
    sc.light = (uint32_t)sc.s.size() - 1;
    return sc;
}

// a 6 x 6 field of balls on a ground sphere, three larger ones; the light is added by the caller
static Scene small_field() {
    Scene sc;
    sc.s.push_back({{0.0, -1000.0, 0.0}, 1000.0});
    for (int a = -3; a < 3; ++a)
        for (int b = -3; b < 3; ++b) sc.s.push_back({{a + 0.9 * rnd(), 0.2, b + 0.9 * rnd()}, 0.2});
    sc.s.push_back({{0.0, 1.0, 0.0}, 1.0});
    sc.s.push_back({{-2.0, 0.6, 1.0}, 0.6});
    return sc;
}

static bool read_scene(const char* path, const char* light, Scene& sc) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) { std::printf("cannot open %s\n", path); return false; }
    Sph q;
    while (std::fscanf(f, "%lf %lf %lf %lf", &q.c[0], &q.c[1], &q.c[2], &q.r) == 4) sc.s.push_back(q);
    std::fclose(f);
    sc.light = (uint32_t)std::atoi(light);
    return !sc.s.empty() && sc.light < sc.s.size();
}

// --lists: the gate's figures
static int lists_main(int argc, char** argv) {
    Scene sc;
    if (argc < 4 || !read_scene(argv[2], argv[3], sc)) { std::printf("usage: --lists FILE LIGHT [HITS [MAX_CELLS]]\n"); return 2; }
    const LightGrid g = grid_of(sc, argc > 5 ? (uint32_t)std::atoi(argv[5]) : 0);
    if (!g.cells) { std::printf("no grid\n"); return 1; }
    double O[3], R;
    light_cell_ball(g, 0, O, &R);
    std::printf("grid: box low corner (%.4f, %.4f, %.4f), %u x %u x %u = %u cells of side %.5f, cell ball radius %.5f; light (%.1f, %.1f, %.1f) radius %.1f\n",
                g.lo[0], g.lo[1], g.lo[2], g.n[0], g.n[1], g.n[2], g.cells, g.h, R, g.f[0], g.f[1], g.f[2], g.rho);
    std::vector<uint8_t> len(g.cells), surf(g.cells, 0);
    for (uint32_t c = 0; c < g.cells; ++c) {
        const Record r = build_record(g, sc.s, c);
        len[c] = r.overflow ? 255 : (uint8_t)r.n;
    }
    for (const Sph& s : sc.s) {   // the cells of the sphere's own box
        int lo[3], hi[3];
        bool any = true;
        for (int k = 0; k < 3; ++k) {
            lo[k] = (int)std::floor((s.c[k] - s.r - g.lo[k]) * g.inv); hi[k] = (int)std::floor((s.c[k] + s.r - g.lo[k]) * g.inv);
            if (lo[k] < 0) lo[k] = 0;
            if (hi[k] >= (int)g.n[k]) hi[k] = (int)g.n[k] - 1;
            any = any && lo[k] <= hi[k];
        }
        if (!any) continue;
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int x = lo[0]; x <= hi[0]; ++x) {
                    const uint32_t c = ((uint32_t)z * g.n[1] + (uint32_t)y) * g.n[0] + (uint32_t)x;
                    if (!surf[c] && surface_in_cell(g, c, s)) surf[c] = 1;
                }
    }
    uint64_t hist[kCandMax + 2] = {0}, ns = 0, all_over = 0, sum = 0;
    for (uint32_t c = 0; c < g.cells; ++c) {
        all_over += len[c] == 255;
        if (!surf[c]) continue;
        ++ns;
        ++hist[len[c] == 255 ? kCandMax + 1 : len[c]];
        if (len[c] != 255) sum += len[c];
    }
    std::printf("cells a sphere's surface passes through: %llu of %u\nlist length : cells (share)\n", (unsigned long long)ns, g.cells);
    for (uint32_t k = 0; k <= kCandMax; ++k)
        std::printf("%11u : %llu (%.2f %%)\n", k, (unsigned long long)hist[k], 100.0 * hist[k] / (double)(ns ? ns : 1));
    std::printf("   overflow : %llu (%.2f %%)\n", (unsigned long long)hist[kCandMax + 1], 100.0 * hist[kCandMax + 1] / (double)(ns ? ns : 1));
    std::printf("mean length without overflow cells %.3f; overflow cells among all cells %llu (%.2f %%)\n",
                (double)sum / (double)(ns - hist[kCandMax + 1] ? ns - hist[kCandMax + 1] : 1), (unsigned long long)all_over, 100.0 * all_over / g.cells);
    if (argc > 4) {
        std::FILE* f = std::fopen(argv[4], "r");
        if (!f) { std::printf("cannot open %s\n", argv[4]); return 2; }
        double p[3];
        uint64_t n = 0, out = 0, over = 0, lsum = 0;
        while (std::fscanf(f, "%lf %lf %lf", &p[0], &p[1], &p[2]) == 3) {
            ++n;
            const uint32_t c = light_cell(g, p);
            if (c == kLightOutside) ++out;
            else if (len[c] == 255) ++over;
            else lsum += len[c];
        }
        std::fclose(f);
        std::printf("first-hit points: %llu; outside the grid %llu (%.2f %%), in overflow cells %llu (%.2f %%), both %.2f %%; mean list length of the rest %.3f\n",
                    (unsigned long long)n, (unsigned long long)out, 100.0 * out / (double)(n ? n : 1), (unsigned long long)over,
                    100.0 * over / (double)(n ? n : 1), 100.0 * (out + over) / (double)(n ? n : 1), (double)lsum / (double)(n - out - over ? n - out - over : 1));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--lists")) return lists_main(argc, argv);
    if (argc > 2) {  // the scene's own spheres
        Scene sc;
        CHECK(read_scene(argv[1], argv[2], sc), "no scene in %s", argv[1]);
        if (!sc.s.empty()) {
            const Tally t = check_scene("bench (file)", sc, 150);
            CHECK(t.rays > 300000 && t.over * 4 < t.rays, "bench (file): %llu rays checked, %llu from overflow cells", (unsigned long long)t.rays, (unsigned long long)t.over);
        }
    }
    {
        const Scene sc = rtiow_like();
        const Tally t = check_scene("bench", sc, 150);
        CHECK(t.rays > 300000 && t.over * 4 < t.rays, "bench: %llu rays checked, %llu from overflow cells", (unsigned long long)t.rays, (unsigned long long)t.over);
        // teeth
        const Tally b = check_scene("bench", sc, 150, 1.0, 0.7);
        CHECK(b.missed > 0 && b.winner_missed > 0, "lists built for 0.7 of the cell ball miss nothing");
    }
    {
        // a huge light whose surface is one cell away from a small grid: (R + rho) / |d| > 0.99 for every cell, every
        // beam is wide, every sphere a candidate of every cell, and with 14 spheres every cell overflows
        Scene sc;
        for (int i = 0; i < 13; ++i) sc.s.push_back({{1.5 * rnd(), 1.5 * rnd(), 1.5 * rnd()}, 0.2});
        sc.s.push_back({{0.0, 0.0, 0.0}, 1000.0});
        sc.light = 13;
        LightGrid g = grid_of(sc);
        CHECK(g.cells > 0, "huge light: no grid");
        sc.s[13].c[0] = g.lo[0] + g.n[0] * g.h + g.h + 1000.0;   // its surface one cell beyond the box's high x face
        sc.s[13].c[1] = sc.s[13].c[2] = 0.75;
        g = grid_of(sc);
        CHECK(g.cells > 0, "huge light: no grid");
        uint32_t wide = 0, over = 0;
        for (uint32_t c = 0; c < g.cells; ++c) {
            wide += light_cell_beam(g, c).wide ? 1u : 0u;
            over += build_record(g, sc.s, c).overflow ? 1u : 0u;
        }
        std::printf("%-16s %u cells, %u wide, %u overflow\n", "huge light", g.cells, wide, over);
        CHECK(wide == g.cells && over == g.cells, "huge light: %u of %u beams wide, %u records overflow", wide, g.cells, over);
        const Tally t = check_scene("huge light", sc, 20);
        CHECK(t.rays == 0 && t.over > 0, "huge light: %llu rays met a list", (unsigned long long)t.rays);
    }
    {
        // a light inside the grid, among the balls: the cells around it have wide beams, the light's own cell F near O
        Scene sc = small_field();
        sc.s.push_back({{0.3, 0.9, -1.2}, 0.3});
        sc.light = (uint32_t)sc.s.size() - 1;
        sc.marked.push_back(sc.light);
        const LightGrid g = grid_of(sc);
        CHECK(light_cell(g, sc.s[sc.light].c) != kLightOutside, "light inside: the light is outside the grid");
        const Tally t = check_scene("light inside", sc, 150);
        CHECK(t.rays > 100000, "light inside: %llu rays checked", (unsigned long long)t.rays);
    }
    {
        // a 0.01-radius sphere 1,000 units along the beam of one cell (a light of radius 40, 2,000 units away), off the
        // axis by 0.9 of the beam's radius there: a candidate that only the light's radius brings in
        Scene sc = small_field();
        sc.s.push_back({{1200.0, 1600.0, 0.0}, 40.0});
        sc.light = (uint32_t)sc.s.size() - 1;
        LightGrid g = grid_of(sc);
        CHECK(g.cells > 0, "far small sphere: no grid");
        const double p0[3] = {0.35, 0.41, 0.2};
        const uint32_t cell = light_cell(g, p0);
        CHECK(cell != kLightOutside, "far small sphere: the chosen point is outside the grid");
        double O[3], R;
        light_cell_ball(g, cell, O, &R);
        const double dd[3] = {g.f[0] - O[0], g.f[1] - O[1], g.f[2] - O[2]};
        const double len = std::sqrt(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]), s = 1000.0 / len;
        const double off = 0.9 * ((1.0 - s) * R + s * 40.0);
        // off the axis along z (the axis lies nearly in the x-y plane)
        sc.s.push_back({{O[0] + s * dd[0], O[1] + s * dd[1], O[2] + s * dd[2] + off}, 0.01});
        sc.marked.push_back((uint32_t)sc.s.size() - 1);
        g = grid_of(sc);
        const Record r = build_record(g, sc.s, light_cell(g, p0));
        bool in = false;
        for (uint32_t q = 0; q < r.n; ++q) in = in || r.e[q] == sc.marked[0];
        CHECK(r.overflow || in, "far small sphere: not in the record of the cell it was placed for");
        const Tally t = check_scene("far small sphere", sc, 150);
        CHECK(t.rays > 100000, "far small sphere: %llu rays checked", (unsigned long long)t.rays);
        const Tally a = check_scene("far small sphere", sc, 150, 0.7, 1.0);
        CHECK(a.missed > 0, "far small sphere: lists built for 0.7 rho miss nothing");
    }
    {
        // two identical spheres: both are listed wherever one is (the kernel's list loop then meets the tie and walks)
        Scene sc = small_field();
        sc.s.push_back({{0.0, 1.0, 0.0}, 1.0});
        sc.s.push_back({{1.4, 0.5, 1.3}, 0.5});
        sc.s.push_back({{1.4, 0.5, 1.3}, 0.5});
        sc.s.push_back({{30.0, 40.0, 10.0}, 3.0});
        sc.light = (uint32_t)sc.s.size() - 1;
        const Tally t = check_scene("twins", sc, 150);
        CHECK(t.rays > 100000, "twins: %llu rays checked", (unsigned long long)t.rays);
    }
    {
        // the index function: non-finite and out-of-box origins are outside; the box's low faces are inside, its high
        // faces are not
        const Scene sc = rtiow_like();
        const LightGrid g = grid_of(sc);
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        const double in[3] = {0.3, 0.2, -0.4};
        CHECK(light_cell(g, in) != kLightOutside, "a point among the balls is outside");
        for (int k = 0; k < 3; ++k)
            for (const double v : {nan, inf, -inf, 1e300, -1e300, g.lo[k] + g.n[k] * g.h, std::nextafter(g.lo[k], -1e300), g.lo[k] - 1.0, g.lo[k] + (g.n[k] + 1) * g.h}) {
                double o[3] = {in[0], in[1], in[2]};
                o[k] = v;
                CHECK(light_cell(g, o) == kLightOutside, "axis %d value %g is inside", k, v);
                const double d[3] = {nan, 1.0, 0.0};
                CHECK(!light_member(g, in, d), "a NaN direction is of the family");
                const double on[3] = {nan, in[1], in[2]};
                const double d1[3] = {g.f[0] - in[0], g.f[1] - in[1], g.f[2] - in[2]};
                CHECK(!light_member(g, on, d1), "a NaN origin is of the family");
                CHECK(light_member(g, in, d1), "the ray at the light's centre is not of the family");
                const double d2[3] = {-d1[0], -d1[1], -d1[2]};
                CHECK(!light_member(g, in, d2), "the ray away from the light is of the family");
            }
        for (int k = 0; k < 3; ++k) {
            double o[3] = {in[0], in[1], in[2]};
            o[k] = g.lo[k];
            CHECK(light_cell(g, o) != kLightOutside, "the low face of axis %d is outside", k);
            o[k] = g.lo[k] + ((double)g.n[k] - 0x1p-20) * g.h;   // (an ulp below the face may round onto it: outside, the safe side)
            const uint32_t c = light_cell(g, o);
            CHECK(c != kLightOutside, "2^-20 of a cell below the high face of axis %d is outside", k);
            if (c != kLightOutside) {   // ... and inside that cell's ball
                double O[3], R;
                light_cell_ball(g, c, O, &R);
                const double dist = std::sqrt((o[0] - O[0]) * (o[0] - O[0]) + (o[1] - O[1]) * (o[1] - O[1]) + (o[2] - O[2]) * (o[2] - O[2]));
                CHECK(dist <= R, "an origin of cell %u is %g from its centre, the ball's radius is %g", c, dist, R);
            }
        }
        // no grid: one sphere, a NaN, a light too small for its distance (the membership check's rounding)
        Scene one; one.s.push_back({{0.0, 0.0, 0.0}, 1.0});
        CHECK(grid_of(one).cells == 0, "a scene of one sphere has a grid");
        Scene bad = sc; bad.s[5].c[1] = nan;
        CHECK(grid_of(bad).cells == 0, "a NaN centre gives a grid");
        Scene tiny = sc; tiny.s[tiny.light].r = 0.1;
        CHECK(grid_of(tiny).cells == 0, "a light of radius 0.1 at 510 units gives a grid");
        CHECK(light_cell(grid_of(one), in) == kLightOutside, "no grid, and a point is inside");
    }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
