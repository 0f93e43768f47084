// rs_light_cand.h — which spheres a light-sample ray that starts in a cell of space can touch (the spheres mode's
// per-cell candidate lists: k_light_cand_build writes them, the front run of the carried part of k_wfs_extend reads
// them instead of walking the tree).
//
// The family. A scene with exactly one light, a sphere (centre F, radius rho). A ray (o, d) belongs to the family of
// the cell that light_cell() maps o to when it passes the membership check light_member(): F lies ahead of it,
// (F - o) . d > 0, and its line passes within rho sqrt(1 - 2^-20) of F, |(F - o) x d|^2 <= rho^2 (1 - 2^-20) |d|^2.
// Then the ray's point nearest to F, Fq = o + t* d with t* = (F - o) . d / |d|^2 > 0, has |Fq - F| <= rho, and every
// point o + t d, t >= 0, of the ray is (1 - s) o + s Fq with s = t / t* >= 0: exactly a ray of rs_cam_cand.h's family
// with L = o inside the cell's ball (centre O, radius R) and Fq inside the light's ball. cand_beam_ball(O, R, F, rho)
// (rs_cam_cand.h) is that beam, and cand_sphere() with it is the criterion, rounding bounds included. Nothing depends
// on what produced the ray: whatever passes the check is covered.
//
// The check's own rounding. In f64, (F - o) x d squared and summed errs by a few 2^-53 |F - o|^2 |d|^2, the right side
// by a few 2^-53 of itself; the factor 1 - 2^-20 leaves rho^2 2^-20 |d|^2 of room, which covers the former while
// |F - o| <= 2^14 rho (2^-53 2^28 = 2^-25 per unit, a few of them < 2^-20). light_grid_make() gives no grid to a scene
// whose box reaches farther than 2^12 rho from the light, so every origin inside the grid is within that range.
//
// The grid. A box [lo, lo + n h) of n[0] n[1] n[2] cubic cells of side h = 1 / inv. light_cell() maps an f64 origin to
// its cell by idx_k = floor((o_k - lo_k) inv), or to kLightOutside when some (o_k - lo_k) inv is not in [0, n_k) --
// which every NaN and infinity fails. The list build, the kernel and the CPU test (tests/cpp/test_light_cand.cpp) all
// use this one function, so a ray is "from" the cell this function says.
// The cell's ball. light_cell_ball() gives cell idx the centre O_k = lo_k + (idx_k + 1/2) h and the radius
// R = (sqrt(3) / 2) h (1 + 2^-20) + 2^-20 M, M the largest |coordinate| of the box. An origin mapped to the cell has
// a computed (o_k - lo_k) inv in [idx_k, idx_k + 1); the subtraction, the product and inv itself each err by a relative
// 2^-53, so the exact (o_k - lo_k) / h lies in [idx_k - e, idx_k + 1 + e] with e <= 2^-51 (M / h + n_k), that is
// |o_k - O_k| <= h / 2 + 2^-50 M for the exact centre (n_k h <= 2 M); the computed centre errs by a few 2^-53 M more.
// Over three axes the distance exceeds (sqrt(3) / 2) h by less than 2^-48 M, far inside the 2^-20 M added.
#pragma once
#include "rs_cam_cand.h"

namespace rs {

constexpr uint32_t kLightOutside = 0xFFFFFFFFu;   // light_cell(): not in the grid
constexpr uint32_t kLightCellsMax = 1u << 17;     // cells of a grid (2 MiB of 16-byte records)

struct LightGrid {
    double lo[3];       // the box's low corner
    double inv;         // 1 / h
    double h;           // the cells' side
    double f[3];        // the light's centre
    double rho;         // its radius
    double rho2m;       // rho^2 (1 - 2^-20): the membership check's right side per |d|^2
    double grow;        // 2^-20 M, the absolute part of a cell ball's radius
    uint32_t n[3];      // cells per axis
    uint32_t cells;     // n[0] n[1] n[2]; 0: no grid
};

// origin -> cell index, or kLightOutside (beyond the box, NaN, infinite, or no grid)
RS_CC_HD inline uint32_t light_cell(const LightGrid& g, const double o[3]) {
    if (g.cells == 0) return kLightOutside;
    uint32_t idx[3];
    for (int k = 0; k < 3; ++k) {
        const double q = (o[k] - g.lo[k]) * g.inv;
        if (!(q >= 0.0 && q < (double)g.n[k])) return kLightOutside;
        idx[k] = (uint32_t)q;
    }
    return (idx[2] * g.n[1] + idx[1]) * g.n[0] + idx[0];
}

// the ball that holds every origin light_cell() maps to `cell` (the argument is in the header comment)
RS_CC_HD inline void light_cell_ball(const LightGrid& g, uint32_t cell, double O[3], double* R) {
    const uint32_t idx[3] = {cell % g.n[0], (cell / g.n[0]) % g.n[1], cell / (g.n[0] * g.n[1])};
    for (int k = 0; k < 3; ++k) O[k] = g.lo[k] + ((double)idx[k] + 0.5) * g.h;
    *R = 0.8660254037844387 * g.h * (1.0 + 0x1p-20) + g.grow;
}

RS_CC_HD inline CandBeam light_cell_beam(const LightGrid& g, uint32_t cell) {
    double O[3], R;
    light_cell_ball(g, cell, O, &R);
    return cand_beam_ball(O, R, g.f, g.rho);
}

// Does the ray (o, d) belong to the family (header comment)? False for every NaN.
RS_CC_HD inline bool light_member(const LightGrid& g, const double o[3], const double d[3]) {
    const double w[3] = {g.f[0] - o[0], g.f[1] - o[1], g.f[2] - o[2]};
    const double ahead = w[0] * d[0] + w[1] * d[1] + w[2] * d[2];
    const double cx = w[1] * d[2] - w[2] * d[1], cy = w[2] * d[0] - w[0] * d[2], cz = w[0] * d[1] - w[1] * d[0];
    const double d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    return ahead > 0.0 && cx * cx + cy * cy + cz * cz <= g.rho2m * d2;
}

// The grid of a scene of n spheres (centres c[3 i ..], radii r[i]) whose one light is sphere `light`.
// Box: the own boxes of all spheres whose radius is at most 16 x the median radius (that leaves out a ground sphere and
// a far light; scatter points lie on surfaces, and these are the surfaces there are many of), grown by one cell.
// Side: the smallest h >= half the median radius with at most kLightCellsMax cells. On the bench scene (RTIOW: 22 x 22
// balls of radius 0.2 one unit apart, three spheres of radius 1) that is h = 0.219, 104 x 12 x 104 cells with balls of
// radius 0.19, smaller than a scene ball: a list holds the ground, the light and the zero to three balls the thin beam
// passes on its way out of the 0.4-high layer -- 2.45 entries on average over the cells a surface passes through, none
// over 6, and 2.29 at the first hits of a frame, 1 % of which lie outside the grid (profiles/light_cand/lists.txt;
// 2^16 cells: 2.41 entries there, 2^15: 2.56, so the largest grid the record budget allows). No grid (cells = 0): fewer
// than two spheres, anything not finite, a degenerate box, or a box that reaches beyond 2^12 rho from the light (the
// membership check's rounding).
// (max_cells: the tuning runs' other sizes; the product passes none)
inline LightGrid light_grid_make(const double* c, const double* r, uint32_t n, uint32_t light,
                                 uint32_t max_cells = kLightCellsMax) {
    LightGrid g;
    g.cells = 0; g.inv = g.h = g.rho = g.rho2m = g.grow = 0.0;
    for (int k = 0; k < 3; ++k) { g.lo[k] = g.f[k] = 0.0; g.n[k] = 0; }
    if (n < 2 || light >= n) return g;
    // the median radius, by selection on a copy (n is small: commit time)
    double med;
    {
        double* t = new double[n];
        for (uint32_t i = 0; i < n; ++i) t[i] = fabs(r[i]);
        for (uint32_t i = 0; i <= n / 2; ++i) {
            uint32_t m = i;
            for (uint32_t j = i + 1; j < n; ++j) if (t[j] < t[m]) m = j;
            const double x = t[i]; t[i] = t[m]; t[m] = x;
        }
        med = t[n / 2];
        delete[] t;
    }
    if (!(med > 0.0) || !cand_finite(med)) return g;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < n; ++i) {
        const double ri = fabs(r[i]);
        if (!cand_finite(ri) || !cand_finite(c[3 * i]) || !cand_finite(c[3 * i + 1]) || !cand_finite(c[3 * i + 2])) return g;
        if (!(ri <= 16.0 * med)) continue;
        for (int k = 0; k < 3; ++k) {
            if (c[3 * i + k] - ri < lo[k]) lo[k] = c[3 * i + k] - ri;
            if (c[3 * i + k] + ri > hi[k]) hi[k] = c[3 * i + k] + ri;
        }
    }
    double ext[3], vol = 1.0;
    for (int k = 0; k < 3; ++k) {
        ext[k] = hi[k] - lo[k];
        if (!(ext[k] > 0.0) || !cand_finite(ext[k]) || !cand_finite(lo[k])) return g;
        vol *= ext[k];
    }
    if (max_cells == 0 || max_cells > kLightCellsMax) max_cells = kLightCellsMax;
    double h = cbrt(vol / (double)max_cells);
    if (h < 0.5 * med) h = 0.5 * med;
    for (int it = 0; it < 400; ++it, h *= 1.01) {   // the one-cell margin and the round-up: grow h until it fits
        double cells = 1.0;
        for (int k = 0; k < 3; ++k) cells *= ceil(ext[k] / h) + 2.0;
        if (cells <= (double)max_cells) break;
    }
    double cells = 1.0, M = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double nk = ceil(ext[k] / h) + 2.0;
        cells *= nk;
        if (!(nk >= 1.0 && nk <= (double)kLightCellsMax)) return g;
        g.n[k] = (uint32_t)nk;
        g.lo[k] = lo[k] - h;
        const double a = fabs(g.lo[k]), b = fabs(g.lo[k] + nk * h);
        if (a > M) M = a;
        if (b > M) M = b;
    }
    if (!(cells <= (double)kLightCellsMax) || !cand_finite(h) || !cand_finite(M)) return g;
    g.h = h;
    g.inv = 1.0 / h;
    g.grow = 0x1p-20 * M;
    g.rho = fabs(r[light]);
    g.rho2m = g.rho * g.rho * (1.0 - 0x1p-20);
    double far2 = 0.0;   // the box's farthest corner from the light
    for (int k = 0; k < 3; ++k) {
        g.f[k] = c[3 * light + k];
        const double a = fabs(g.f[k] - g.lo[k]), b = fabs(g.f[k] - (g.lo[k] + (double)g.n[k] * h));
        far2 += (a > b ? a : b) * (a > b ? a : b);
    }
    if (!(g.rho > 0.0) || !cand_finite(g.rho) || !cand_finite(far2) || !(far2 <= 0x1p24 * g.rho * g.rho)) return g;
    if (!cand_finite(g.inv)) return g;
    g.cells = g.n[0] * g.n[1] * g.n[2];
    return g;
}

}  // namespace rs
