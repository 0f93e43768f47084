// rs_cam_cand.h — which spheres a lattice pixel's camera rays can touch (the spheres mode's per-pixel candidate
// lists: k_cam_cand_build writes them, the camera part of k_wfs_extend reads them instead of walking the tree).
//
// camera_ray (rs_device.h) starts a pixel's rays at L = origin + hu rd.x + vu rd.y, |rd| < aperture / 2, and aims
// them at Fq = lb + u hf + v vf, where camera_sample_xy keeps (u, v) inside the pixel's footprint
// u in [x / W, (x + 1) / W], v in [(H - 2 - y) / H, (H - 1 - y) / H] (both ends included). With O the camera origin,
// F the footprint's centre, R >= |L - O| and rho >= |Fq - F|, every point of every such ray is (1 - s) L + s Fq for
// some s >= 0 and lies within |1 - s| R + s rho of the axis point A(s) = O + s (F - O). So a sphere (c, r) can be
// hit only if
//     g(s) = |c - A(s)| - (r + |1 - s| R + s rho) <= 0   for some s >= 0.
// g is convex on [0, 1] and on [1, inf) (a distance to a line minus a linear term), so each piece's minimum is at
// its stationary point clamped to the piece. Plain C++ (host and device): tests/cpp/test_cam_cand.cpp runs it on
// the CPU against rays drawn from the family itself.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RS_CC_HD __host__ __device__
#else
#define RS_CC_HD
#endif

namespace rs {

constexpr uint32_t kCandMax = 8;           // entries of a pixel's record (16 bytes of uint16)
constexpr uint32_t kCandEmpty = 0xFFFFu;   // an unused entry (the list ends at the first one)
constexpr uint32_t kCandOverflow = 0xFFFEu;  // in entry 0: more than kCandMax candidates, the pixel's rays walk the tree
constexpr uint32_t kCandMaxEntries = 65534u;  // leaf entries a scene with lists may have (entries 0 .. 0xFFFD)
constexpr int kCandStack = 32;             // k_cam_cand_build's stack entries (scenes with stack_need above it: no lists)

// What the criterion needs of a camera and a frame size: no lists (ok = 0) for anything non-finite or degenerate.
struct CandCam {
    double o[3];        // camera origin
    double lb[3], hf[3], vf[3];
    double R;           // bound on |L - O| over the lens disk
    double rho;         // bound on |Fq - F| over a pixel's footprint
    double inv_w, inv_h, h;
    int ok;
};

// One pixel's beam: the axis from O towards the footprint's centre, and what the test needs of it per piece
// (piece 0: s in [0, 1], the right side is (r + R) + (rho - R) s; piece 1: s >= 1, (r - R) + (R + rho) s).
struct CandBeam {
    double o[3], d[3];  // O, F - O
    double len;         // |F - O|
    double inv_len, inv_len2;
    double R, rho;
    double b[2];        // the right side's slope on each piece
    double kf[2];       // k / (|d| sqrt(1 - k^2)), k = b / |d|: the stationary point is s* = p + h kf
    int wide;           // some |k| > 0.99: the beam opens about as fast as its axis advances, every sphere is kept
    int ok;             // 0: F == O or not finite (the caller marks the pixel overflow: its rays walk)
};

RS_CC_HD inline bool cand_finite(double x) { return x - x == 0.0; }  // false for NaN and +-inf

// origin, lb, hf, vf, hu, vu, aperture: DCamera's fields (camera.rs:18-31).
// R: rd.x hu + rd.y vu with rd.x^2 + rd.y^2 < (aperture / 2)^2 is no longer than (aperture / 2) sqrt(lambda), lambda
// the larger eigenvalue of the Gram matrix of (hu, vu), and lambda <= max(|hu|^2, |vu|^2) + |hu . vu|.
// rho: Fq - F = du hf + dv vf with |du| <= 1 / (2 W), |dv| <= 1 / (2 H); its square is at most
// |hf|^2 / (4 W^2) + |vf|^2 / (4 H^2) + |hf . vf| / (2 W H). Both get a relative 2^-40 on top (their own rounding).
RS_CC_HD inline CandCam cand_camera(const double origin[3], const double lb[3], const double hf[3], const double vf[3],
                                    const double hu[3], const double vu[3], double aperture, uint32_t width,
                                    uint32_t height) {
    CandCam c;
    c.ok = 0;
    bool fin = cand_finite(aperture);
    for (int k = 0; k < 3; ++k) {
        c.o[k] = origin[k]; c.lb[k] = lb[k]; c.hf[k] = hf[k]; c.vf[k] = vf[k];
        fin = fin && cand_finite(origin[k]) && cand_finite(lb[k]) && cand_finite(hf[k]) && cand_finite(vf[k]) &&
              cand_finite(hu[k]) && cand_finite(vu[k]);
    }
    c.R = c.rho = c.inv_w = c.inv_h = c.h = 0.0;
    if (!fin || width == 0 || height == 0) return c;
    const double w = (double)width, h = (double)height;
    const double hu2 = hu[0] * hu[0] + hu[1] * hu[1] + hu[2] * hu[2], vu2 = vu[0] * vu[0] + vu[1] * vu[1] + vu[2] * vu[2];
    const double huvu = fabs(hu[0] * vu[0] + hu[1] * vu[1] + hu[2] * vu[2]);
    const double hf2 = hf[0] * hf[0] + hf[1] * hf[1] + hf[2] * hf[2], vf2 = vf[0] * vf[0] + vf[1] * vf[1] + vf[2] * vf[2];
    const double hfvf = fabs(hf[0] * vf[0] + hf[1] * vf[1] + hf[2] * vf[2]);
    const double slack = 1.0 + 0x1p-40;
    c.R = fabs(aperture) * 0.5 * sqrt((hu2 > vu2 ? hu2 : vu2) + huvu) * slack;
    c.rho = sqrt(hf2 / (4.0 * w * w) + vf2 / (4.0 * h * h) + hfvf / (2.0 * w * h)) * slack;
    c.inv_w = 1.0 / w; c.inv_h = 1.0 / h; c.h = h;
    c.ok = cand_finite(c.R) && cand_finite(c.rho);
    return c;
}

// pixel (x, y) of the frame: the footprint's centre is (u, v) = ((x + 1/2) / W, (H - 3/2 - y) / H)
RS_CC_HD inline CandBeam cand_beam(const CandCam& c, uint32_t x, uint32_t y) {
    CandBeam b;
    const double u = ((double)x + 0.5) * c.inv_w, v = (c.h - 1.5 - (double)y) * c.inv_h;
    double l2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        b.o[k] = c.o[k];
        b.d[k] = c.lb[k] + u * c.hf[k] + v * c.vf[k] - c.o[k];
        l2 += b.d[k] * b.d[k];
    }
    b.len = sqrt(l2);
    b.inv_len = 1.0 / b.len;
    b.inv_len2 = 1.0 / l2;
    b.R = c.R; b.rho = c.rho;
    b.ok = c.ok && cand_finite(l2) && l2 > 0.0 && cand_finite(b.inv_len2);
    b.b[0] = c.rho - c.R;
    b.b[1] = c.R + c.rho;
    b.wide = 0;
    for (int piece = 0; piece < 2; ++piece) {
        const double k = b.b[piece] * b.inv_len;
        if (!(fabs(k) <= 0.99)) { b.wide = 1; b.kf[piece] = 0.0; continue; }
        b.kf[piece] = k * b.inv_len / sqrt(1.0 - k * k);
    }
    return b;
}

// The beam of every ray (1 - s) L + s Fq, s >= 0, with L in the ball (O, R) and Fq in the ball (F, rho): cand_beam()'s
// fields for any such pair, with the same ok / wide rules (rs_light_cand.h: a cell of space and the light).
RS_CC_HD inline CandBeam cand_beam_ball(const double O[3], double R, const double F[3], double rho) {
    CandBeam b;
    double l2 = 0.0;
    bool fin = cand_finite(R) && cand_finite(rho);
    for (int k = 0; k < 3; ++k) {
        b.o[k] = O[k];
        b.d[k] = F[k] - O[k];
        l2 += b.d[k] * b.d[k];
        fin = fin && cand_finite(O[k]) && cand_finite(F[k]);
    }
    b.len = sqrt(l2);
    b.inv_len = 1.0 / b.len;
    b.inv_len2 = 1.0 / l2;
    b.R = fabs(R); b.rho = fabs(rho);
    b.ok = fin && cand_finite(l2) && l2 > 0.0 && cand_finite(b.inv_len2);
    b.b[0] = b.rho - b.R;
    b.b[1] = b.R + b.rho;
    b.wide = 0;
    for (int piece = 0; piece < 2; ++piece) {
        const double k = b.b[piece] * b.inv_len;
        if (!(fabs(k) <= 0.99)) { b.wide = 1; b.kf[piece] = 0.0; continue; }
        b.kf[piece] = k * b.inv_len / sqrt(1.0 - k * k);
    }
    return b;
}

// Can a ray of the beam touch the sphere (centre c, radius r)? Never false when g(s) <= 0 for some s >= 0; *along
// (when given) receives the centre's parameter along the axis (the lists' order). A node's box goes through its
// bounding sphere (centre, half diagonal).
//
// Rounding. With w = c - O, p = (w . d) / |d|^2 and h = |w x d| / |d| (a cross product: no cancellation for centres
// near the axis), |c - A(s)| = sqrt(h^2 + |d|^2 (s - p)^2), and on a piece where the right side is a + b s the
// stationary point is s* = p + h k / (|d| sqrt(1 - k^2)), k = b / |d| (the beam's kf). The test evaluates g at s*
// clamped to the piece. g is Lipschitz in s with constant |d| + |b|, so an error ds in s* raises the value found by at
// most that times ds; for |k| <= 0.99 (beyond it the test accepts: CandBeam::wide) the f64 error of s* is below 2^-46
// (|w| + |d|) / |d|, and g's own evaluation errs by a few 2^-53 of the magnitudes it adds. Both are far inside the
// slack 2^-30 (|w|_1 + r + R + s (|d| + R + rho)) the test allows (|w|_1, the sum of |w|'s components, stands for |w|:
// it is no smaller), and so is the 2^-52 relative distance between a computed ray (origin, unit direction, footprint
// point) and its ideal.
// The ray test's own rounding is different in kind: sphere_t_trav's discriminant half_b^2 - a c carries an
// absolute error of a few 2^-53 |o - c|^2, which acts like r^2 grown by that much -- for a small far sphere more
// than any relative slack on r. So r is replaced by sqrt(r^2 + 2^-40 (|w|_1 + R + r)^2) first.
// (Four square roots and no division per call: the build kernel's time is these.)
RS_CC_HD inline bool cand_sphere(const CandBeam& b, const double c[3], double r, double* along = nullptr) {
    const double w[3] = {c[0] - b.o[0], c[1] - b.o[1], c[2] - b.o[2]};
    const double w1 = fabs(w[0]) + fabs(w[1]) + fabs(w[2]);
    const double p = (w[0] * b.d[0] + w[1] * b.d[1] + w[2] * b.d[2]) * b.inv_len2;
    if (along) *along = p;
    if (!b.ok || b.wide) return true;
    r = fabs(r);
    const double reach = w1 + b.R + r;
    r = sqrt(r * r + 0x1p-40 * reach * reach);
    if (!(r - r == 0.0)) return true;  // NaN / inf (in w too: reach carries it): keep
    const double cx = w[1] * b.d[2] - w[2] * b.d[1], cy = w[2] * b.d[0] - w[0] * b.d[2], cz = w[0] * b.d[1] - w[1] * b.d[0];
    const double h = sqrt(cx * cx + cy * cy + cz * cz) * b.inv_len;
    for (int piece = 0; piece < 2; ++piece) {
        const double bb = b.b[piece];
        const double aa = piece == 0 ? r + b.R : r - b.R;
        double s = p + h * b.kf[piece];
        if (piece == 0) s = s < 0.0 ? 0.0 : s > 1.0 ? 1.0 : s;
        else s = s < 1.0 ? 1.0 : s;
        if (!(s - s == 0.0)) return true;
        const double q[3] = {w[0] - s * b.d[0], w[1] - s * b.d[1], w[2] - s * b.d[2]};
        const double dist = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
        const double g = dist - (aa + bb * s);
        const double slack = 0x1p-30 * (w1 + r + b.R + s * (b.len + b.R + b.rho));
        if (!(g > slack)) return true;
    }
    return false;
}

// A pixel's record: `n` candidates found (in any order) with their parameters along the axis -> 8 uint16,
// nearest first, kCandEmpty after the last; more than kCandMax: kCandOverflow in entry 0.
struct CandList {
    uint32_t e[kCandMax];
    double along[kCandMax];
    uint32_t n;         // candidates met (may exceed kCandMax: overflow)
};
RS_CC_HD inline void cand_list_init(CandList& l) { l.n = 0; }
RS_CC_HD inline void cand_list_add(CandList& l, uint32_t entry, double along) {
    if (l.n >= kCandMax) { l.n = kCandMax + 1; return; }
    uint32_t i = l.n;
    while (i > 0 && l.along[i - 1] > along) { l.e[i] = l.e[i - 1]; l.along[i] = l.along[i - 1]; --i; }
    l.e[i] = entry; l.along[i] = along;
    ++l.n;
}
RS_CC_HD inline bool cand_list_overflow(const CandList& l) { return l.n > kCandMax; }
// the record's four 32-bit words (entry 2 i in the low half of word i)
RS_CC_HD inline void cand_list_pack(const CandList& l, uint32_t out[4]) {
    uint32_t h[kCandMax];
    for (uint32_t i = 0; i < kCandMax; ++i) h[i] = (!cand_list_overflow(l) && i < l.n) ? l.e[i] : kCandEmpty;
    if (cand_list_overflow(l)) h[0] = kCandOverflow;
    for (uint32_t i = 0; i < 4; ++i) out[i] = h[2 * i] | (h[2 * i + 1] << 16);
}

}  // namespace rs
