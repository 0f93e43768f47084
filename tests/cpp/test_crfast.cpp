// rs_crfast.h (host build) against rs_crmath.h, bit for bit.
// usage: test_crfast LOG2_SINCOS LOG2_TRIPLES  -> prints the counts and figures; exit 1 on any failure.
//   sincos: sincos_cr_fast == sincos_cr on 2^LOG2_SINCOS arguments 2 pi u, u drawn as Rng::gen draws it (a 64-bit
//   integer times 2^-64), and on the edge arguments; over the same arguments the largest relative distance of the fast
//   double-double from the full one (at most M / 4) and the share of values whose rounding test fails (at most 2^-12).
//   checker: sin_sign_fast == sin_sign and sin3_negative_fast == sin3_negative on 2^LOG2_TRIPLES triples.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../raysnail_amd/csrc/rs_crfast.h"

using rs_cr::DD;

static inline uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static inline bool same_bits(double a, double b) {
    if (a != a || b != b) return a != a && b != b;
    return std::memcmp(&a, &b, sizeof a) == 0;
}
static const long double PIO2L = 1.57079632679489661923132169163975144L;

struct SincosStats {
    long n = 0, mismatch = 0, wrong_pass = 0, fallback_values = 0, values = 0, restated = 0;
    double max_dev = 0.0;
    void merge(const SincosStats& o) {
        n += o.n; mismatch += o.mismatch; wrong_pass += o.wrong_pass; fallback_values += o.fallback_values;
        values += o.values; restated += o.restated; max_dev = std::max(max_dev, o.max_dev);
    }
};

// one argument: equality of the two functions; inside the fast domain also the deviation and the rounding tests
static void check_sincos(double x, SincosStats& st, bool count_margins) {
    double s0, c0, s1, c1;
    rs_cr::sincos_cr(x, &s0, &c0);
    rs_crfast::sincos_cr_fast(x, &s1, &c1);
    ++st.n;
    if (!same_bits(s0, s1) || !same_bits(c0, c1)) {
        if (st.mismatch++ < 5) std::printf("sincos(%a): %a %a vs %a %a\n", x, s1, c1, s0, c0);
    }
    if (!count_margins || x == 0.0 || !(x == x) || std::isinf(x)) return;
    int64_t k;
    const DD r = rs_cr::reduce_pio2(x, k);
    if (!rs_crfast::fast_domain(x, (double)k)) return;
    const DD z = rs_cr::mul(r, r);
    const DD f[2] = {rs_crfast::sin_fast(r, z), rs_crfast::cos_fast(z)};
    const DD F[2] = {rs_cr::sin_poly(r, z), rs_cr::cos_poly(z)};
    for (int i = 0; i < 2; ++i) {
        const double dev = std::fabs(((f[i].h - F[i].h) + (f[i].l - F[i].l)) / F[i].h);
        st.max_dev = std::max(st.max_dev, dev);
        ++st.values;
        if (!rs_crfast::rounds_alone(f[i])) ++st.fallback_values;
        else if (!same_bits(f[i].h, F[i].h)) ++st.wrong_pass;
    }
    // the full values above are what sincos_cr returned
    const double sr = F[0].h, cr = F[1].h;
    const int q = (int)(k & 3);
    const double es = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
    const double ec = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
    st.restated += !(same_bits(es, s0) && same_bits(ec, c0));
}

struct SignStats {
    long n = 0, bad_sign = 0, bad_triple = 0, fast_decided = 0;
    void merge(const SignStats& o) { n += o.n; bad_sign += o.bad_sign; bad_triple += o.bad_triple; fast_decided += o.fast_decided; }
};
static double sign_arg(uint64_t& g) {
    const uint64_t r = splitmix(g);
    const double u = (double)(splitmix(g) >> 11) * 0x1p-53;
    switch (r & 15) {
    case 0: return (r & 16) ? 0.0 : -0.0;
    case 1: case 2: {  // on and beside a multiple of pi/2, |k| up to 2^22
        const long k = (long)((r >> 8) % (1u << 23)) - (1 << 22);
        double x = (double)((long double)k * PIO2L);
        const int steps = (int)((r >> 40) % 9) - 4;
        for (int i = 0; i < std::abs(steps); ++i) x = std::nextafter(x, steps > 0 ? INFINITY : -INFINITY);
        return x;
    }
    case 3: return (u * 2.0 - 1.0) * 1e8;          // beyond |k| = 2^20
    case 4: return (u * 2.0 - 1.0) * 0x1p21;       // around the bound
    case 5: case 6: case 7: case 8: return (u * 2.0 - 1.0) * 200.0;
    case 9: return std::ldexp(u * 2.0 - 1.0, -(int)((r >> 8) % 1100));
    default: return (u * 2.0 - 1.0) * 2e4;
    }
}
static void check_sign(double x, SignStats& st) {
    if (rs_crfast::sin_sign_fast(x) != rs_cr::sin_sign(x)) {
        if (st.bad_sign++ < 5) std::printf("sin_sign(%a): %d vs %d\n", x, rs_crfast::sin_sign_fast(x), rs_cr::sin_sign(x));
    }
    const double k = std::rint(x * 0x1.45f306dc9c883p-1);
    st.fast_decided += std::fabs(k) < 0x1p20 && std::fabs(x - k * 0x1.921fb54400000p+0) > std::fabs(k) * 0x1p-30;
}

int main(int argc, char** argv) {
    const int lg_s = argc > 1 ? std::atoi(argv[1]) : 22, lg_t = argc > 2 ? std::atoi(argv[2]) : 20;
    const long n_s = 1L << lg_s, n_t = 1L << lg_t;
    const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<SincosStats> ss(T);
    std::vector<SignStats> gs(T);
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) {
        th.emplace_back([&, t] {
            uint64_t g = 0x1234567ULL + 0x1000003ULL * (uint64_t)t;
            for (long i = t; i < n_s; i += T) {
                const double u = (double)splitmix(g) * 0x1p-64;
                check_sincos(2.0 * 3.14159265358979323846 * u, ss[t], true);
            }
            for (long i = t; i < n_t; i += T) {
                const double a = sign_arg(g), b = sign_arg(g), c = sign_arg(g);
                check_sign(a, gs[t]); check_sign(b, gs[t]); check_sign(c, gs[t]);
                ++gs[t].n;
                gs[t].bad_triple += rs_crfast::sin3_negative_fast(a, b, c) != rs_cr::sin3_negative(a, b, c);
            }
        });
    }
    for (auto& x : th) x.join();
    SincosStats S;
    SignStats G;
    for (int t = 0; t < T; ++t) { S.merge(ss[t]); G.merge(gs[t]); }

    // edge arguments: equality only counts here, the margins' figures are the stream's
    SincosStats E;
    std::vector<double> edge = {0.0, -0.0, NAN, INFINITY, -INFINITY, 0x1p-1074, 0x1.8p-1070, 0x1p-1040, 0x1p-1023, 0x1p-1022,
                                0x1.fffffffffffffp-1023, 0x1p-800, 0x1p-600, 0x1p-501, 0x1.fffffffffffffp-501, 0x1p-500,
                                0x1.0000000000001p-500, 0x1p-400, 0x1p-100, 0x1p-30, 1e10, 1e15, 1e22, 1e100, 1e300,
                                0x1.fffffffffffffp+1023};
    for (int k = 0; k <= 8; ++k) {  // the 2,000 doubles around each k pi/2
        double c = (double)((long double)k * PIO2L), lo = c, hi = c;
        edge.push_back(c);
        for (int i = 0; i < 1000; ++i) { lo = std::nextafter(lo, -INFINITY); hi = std::nextafter(hi, INFINITY); edge.push_back(lo); edge.push_back(hi); }
    }
    long beyond = 0, beyond_fast = 0;
    {   // around and beyond |k| = 2^20, where the fast path must fall back
        uint64_t g = 99;
        const double c = (double)((long double)(1 << 20) * PIO2L);
        double lo = c, hi = c;
        for (int i = 0; i < 2000; ++i) { lo = std::nextafter(lo, 0.0); hi = std::nextafter(hi, INFINITY); edge.push_back(lo); edge.push_back(hi); }
        for (int i = 0; i < 200000; ++i) {
            const double u = (double)(splitmix(g) >> 11) * 0x1p-53;
            edge.push_back(c * (0.5 + u));                                  // straddles the bound
            edge.push_back(c * std::ldexp(1.0 + u, (int)(splitmix(g) % 40)));  // beyond it
        }
    }
    for (double x : edge) {
        for (double v : {x, -x}) {
            check_sincos(v, E, true);
            if (v == v && !std::isinf(v) && std::fabs(std::rint(v * 0x1.45f306dc9c883p-1)) >= 0x1p20) {
                ++beyond;
                beyond_fast += rs_crfast::fast_domain(v, std::rint(v * 0x1.45f306dc9c883p-1));
            }
            SignStats dummy;
            check_sign(v, dummy);
            G.bad_sign += dummy.bad_sign;
        }
    }

    const double M = RS_CRFAST_M;
    const double rate = (double)S.fallback_values / (double)std::max(1L, S.values);
    const double dev = std::max(S.max_dev, E.max_dev);
    std::printf("sincos: stream n=%ld mismatches %ld, passed the test with other bits %ld, restated %ld\n", S.n, S.mismatch,
                S.wrong_pass, S.restated);
    std::printf("sincos: edges n=%ld mismatches %ld, passed the test with other bits %ld, restated %ld; beyond 2^20: %ld, fast %ld\n",
                E.n, E.mismatch, E.wrong_pass, E.restated, beyond, beyond_fast);
    std::printf("sincos: deviation 2^%.2f (bound M/4 = 2^%.0f), fallback %ld of %ld values = 2^%.2f (bound 2^-12)\n",
                std::log2(dev), std::log2(M / 4.0), S.fallback_values, S.values, std::log2(rate > 0 ? rate : 1e-300));
    std::printf("checker: triples n=%ld wrong %ld, signs wrong %ld, decided by the fast path %ld of %ld\n", G.n, G.bad_triple,
                G.bad_sign, G.fast_decided, 3 * G.n);
    const bool ok = S.n >= n_s && G.n >= n_t && S.mismatch == 0 && S.wrong_pass == 0 && S.restated == 0 && E.mismatch == 0 &&
                    E.wrong_pass == 0 && E.restated == 0 && beyond > 100000 && beyond_fast == 0 && dev <= M / 4.0 &&
                    rate <= 0x1p-12 && G.bad_triple == 0 && G.bad_sign == 0 && G.fast_decided > G.n;
    std::printf(ok ? "ok\n" : "FAILED\n");
    return ok ? 0 : 1;
}
