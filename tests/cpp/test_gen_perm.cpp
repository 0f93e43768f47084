// The camera samples' trace order (raysnail_amd/csrc/rs_gen_perm.h) on the CPU: i -> gen_perm_item(i) must be a
// bijection of the batch [0, n), whatever the frame's shape -- a frame narrower than a tile, fewer lattice rows than
// a tile has, one column, one row, ragged last tile rows and columns, plane counts that leave groups of every power
// of two, batches that start at a later plane -- or a sample would be traced twice and another never.
//
// Checked for every W in 1 .. 20, lattice rows in 1 .. 12, planes in 1 .. 70, item0 in {0, one plane, 32 planes} and
// row_step in {1, 2, 3, 4, 7, 8, 9} (one of each tile-shape class and its neighbours):
//   - every item of [0, n) is produced exactly once;
//   - the groups are what the header says: full groups of RS_PIX_SAMPLES planes, then decreasing powers of two;
//   - inside a group of SP planes, every run of 64 consecutive i counted from the group's start (what a wave
//     traces when the group starts on a wave boundary) holds exactly 64 / SP distinct lattice pixels, each with SP
//     distinct sample planes of the group: the property the order exists for;
//   - the pixels of such a run lie inside one TW x TH tile wherever the frame has whole tiles;
//   - a batch that is not whole planes (item0 or n no multiple of the lattice) keeps the identity order.
//
// Stand-alone (no library): g++ -O2 -std=c++17 -pthread tests/cpp/test_gen_perm.cpp; prints "ok" last and exits 0.
// The widths are shared among up to 8 threads (285 million items in all).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../raysnail_amd/csrc/rs_gen_perm.h"

using namespace rs;

static std::atomic<int> g_fail{0};
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++g_fail;                                        \
        }                                                    \
    } while (0)

static std::atomic<uint64_t> cases{0}, items{0}, runs{0}, tiled_runs{0};

static void check_width(uint32_t W) {
    const uint32_t steps[7] = {1, 2, 3, 4, 7, 8, 9};
    std::vector<uint32_t> seen, out, sp;
    {
        for (uint32_t R = 1; R <= 12; ++R) {
            const uint32_t npl = W * R;
            for (uint32_t planes = 1; planes <= 70; ++planes) {
                const uint32_t n = planes * npl;
                for (uint32_t si = 0; si < 7; ++si) {
                    const uint32_t step = steps[si];
                    out.assign(n, 0);
                    sp.assign(n, 0);
                    seen.assign(n, 0);
                    for (uint32_t i = 0; i < n; ++i) {
                        out[i] = gen_perm_item(i, 0, n, npl, W, step, &sp[i]);
                        CHECK(out[i] < n, "W %u R %u planes %u step %u: item %u of %u", W, R, planes, step, out[i], n);
                        if (out[i] < n) ++seen[out[i]];
                    }
                    bool bij = true;
                    for (uint32_t i = 0; i < n; ++i) bij = bij && seen[i] == 1;
                    CHECK(bij, "W %u R %u planes %u step %u: not a bijection of %u items", W, R, planes, step, n);
                    // a batch that starts at a later plane gets the same order (item0 enters through item0 % npl only)
                    for (const uint64_t item0 : {(uint64_t)npl, (uint64_t)32 * npl}) {
                        bool same = true;
                        for (uint32_t i = 0; i < n; ++i) same = same && gen_perm_item(i, item0, n, npl, W, step) == out[i];
                        CHECK(same, "W %u R %u planes %u step %u item0 %llu: another order", W, R, planes, step, (unsigned long long)item0);
                    }
                    // the groups and their runs of 64
                    uint32_t g0 = 0, p0 = 0, left = planes;
                    while (left) {
                        uint32_t SP = RS_PIX_SAMPLES;
                        if (left < SP) { SP = 1; while (2 * SP <= left) SP *= 2; }
                        const uint32_t gsz = SP * npl, TP = 64 / SP;
                        const uint32_t TH = gen_perm_tile_rows(TP, step), TW = TP / TH;
                        const uint32_t Wt = W - W % TW, Rt = R - R % TH;
                        for (uint32_t i = g0; i < g0 + gsz; ++i) {
                            CHECK(sp[i] == SP, "W %u R %u planes %u: i %u in a group of %u, expected %u", W, R, planes, i, sp[i], SP);
                            const uint32_t s = out[i] / npl;
                            CHECK(s >= p0 && s < p0 + SP, "W %u R %u planes %u: i %u has plane %u outside [%u, %u)", W, R, planes, i, s, p0, p0 + SP);
                        }
                        for (uint32_t j = 0; 64 * (j + 1) <= gsz; ++j) {
                            uint32_t px[64], cnt[64], npx = 0;
                            uint64_t plane_bits[64];
                            for (uint32_t k = 0; k < 64; ++k) {
                                const uint32_t it = out[g0 + 64 * j + k], pl = it % npl, s = it / npl - p0;
                                uint32_t q = 0;
                                while (q < npx && px[q] != pl) ++q;
                                if (q == npx) { px[npx] = pl; cnt[npx] = 0; plane_bits[npx] = 0; ++npx; }
                                ++cnt[q];
                                plane_bits[q] |= 1ull << s;
                            }
                            bool ok = npx == TP;
                            for (uint32_t q = 0; q < npx; ++q) ok = ok && cnt[q] == SP && plane_bits[q] == (SP == 64 ? ~0ull : (1ull << SP) - 1);
                            CHECK(ok, "W %u R %u planes %u step %u: run %u of group at %u (SP %u) holds %u pixels", W, R, planes, step, j, g0, SP, npx);
                            ++runs;
                            // a run inside the tiled part of the frame is one tile
                            if ((uint64_t)(64 * (j + 1)) / SP <= (uint64_t)Wt * Rt) {
                                uint32_t x0 = W, x1 = 0, y0 = R, y1 = 0;
                                for (uint32_t q = 0; q < npx; ++q) {
                                    const uint32_t x = px[q] % W, y = px[q] / W;
                                    x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
                                }
                                CHECK(x1 - x0 + 1 == TW && y1 - y0 + 1 == TH && x0 % TW == 0 && y0 % TH == 0,
                                      "W %u R %u planes %u step %u: run %u spans %u x %u, tile %u x %u", W, R, planes, step, j, x1 - x0 + 1, y1 - y0 + 1, TW, TH);
                                ++tiled_runs;
                            }
                        }
                        g0 += gsz; p0 += SP; left -= SP;
                    }
                    ++cases;
                    items += n;
                }
                // the identity branch: item0 or n no multiple of the lattice
                if (npl > 1) {
                    for (uint32_t i = 0; i < n; i += 7) {
                        CHECK(gen_perm_item(i, 1, n, npl, W, 1) == i, "W %u R %u: item0 1 is not the identity at %u", W, R, i);
                        CHECK(gen_perm_item(i, (uint64_t)npl - 1, n, npl, W, 2) == i, "W %u R %u: item0 npl - 1 is not the identity at %u", W, R, i);
                    }
                    for (uint32_t i = 0; i + 1 < n; i += 5)
                        CHECK(gen_perm_item(i, 0, n - 1, npl, W, 1) == i, "W %u R %u: n - 1 items is not the identity at %u", W, R, i);
                    for (uint32_t i = 0; i < n + 1; i += 5)
                        CHECK(gen_perm_item(i, (uint64_t)npl, n + 1, npl, W, 8) == i, "W %u R %u: n + 1 items is not the identity at %u", W, R, i);
                }
            }
        }
    }
}

int main() {
    std::atomic<uint32_t> next{20};  // the widest frames first
    std::vector<std::thread> pool;
    const unsigned hw = std::thread::hardware_concurrency();
    for (unsigned t = 0; t < (hw < 1 ? 1 : hw > 8 ? 8 : hw); ++t)
        pool.emplace_back([&] { for (uint32_t W; (W = next.fetch_sub(1)) >= 1 && W <= 20;) check_width(W); });
    for (auto& t : pool) t.join();
    // the tile-shape rule itself (rs_gen_perm.h: 64-pixel tiles: step 1: 8 x 8, 2-3: 16 x 4, 4-7: 32 x 2, >= 8: 16 x 4)
    CHECK(gen_perm_tile_rows(64, 1) == 8 && gen_perm_tile_rows(64, 2) == 4 && gen_perm_tile_rows(64, 3) == 4 &&
          gen_perm_tile_rows(64, 4) == 2 && gen_perm_tile_rows(64, 7) == 2 && gen_perm_tile_rows(64, 8) == 4 &&
          gen_perm_tile_rows(64, 9) == 4, "tile rows of a 64-pixel tile");
    CHECK(gen_perm_tile_rows(2, 1) == 1 && gen_perm_tile_rows(1, 1) == 1 && gen_perm_tile_rows(4, 1) == 2 &&
          gen_perm_tile_rows(8, 1) == 2 && gen_perm_tile_rows(16, 9) == 4 && gen_perm_tile_rows(16, 5) == 2, "tile rows of smaller tiles");
    std::printf("%llu cases, %llu items, %llu runs of 64 (%llu inside whole tiles)\n", (unsigned long long)cases.load(),
                (unsigned long long)items.load(), (unsigned long long)runs.load(), (unsigned long long)tiled_runs.load());
    CHECK(tiled_runs > 0 && runs > tiled_runs, "no run inside whole tiles, or none outside");
    if (g_fail) { std::printf("%d checks failed\n", g_fail.load()); return 1; }
    std::printf("ok\n");
    return 0;
}
