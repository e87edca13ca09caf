// realign_check.cpp - the host arithmetic of vapor_realign_batch (vapor_amd/csrc/vapor_realign_plan.h) held to direct statements
// of its rules, as a program of its own under the address and undefined-behaviour sanitizers (tests/test_realign_cpu.py builds and
// runs it; no HIP, no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc
//       tools/realign_check.cpp -o realign_check && ./realign_check
#include "vapor_realign_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace ra = vapor_realign;

static int g_bad = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            if (++g_bad <= 20) {                            \
                std::printf("FAILED %s: ", #cond);          \
                std::printf(__VA_ARGS__);                   \
                std::printf("\n");                          \
            }                                               \
        }                                                   \
    } while (0)

int main()
{
    // the band of a call
    {
        int n = 0;
        for (int64_t b = -3; b <= VAPOR_MAX_BAND + 3; ++b) {
            CHECK(ra::band_ok(b) == (b >= 1 && b <= 512), "band %lld", (long long)b);
            CHECK((ra::lane_width((int)b) != 0) == ra::band_ok(b), "width of band %lld", (long long)b);
            ++n;
        }
        CHECK(!ra::band_ok((int64_t)1 << 40) && !ra::band_ok(INT64_MIN), "far bands");
        std::printf("bands: %d values\n", n);
    }
    // the slots of a row and their owners: every slot 0 .. 2B has one owner among 64 lanes, the width is a compiled one and the
    // smallest that holds the row
    {
        long long slots = 0;
        for (int b = 1; b <= VAPOR_MAX_BAND; ++b) {
            const int S = ra::lane_width(b), W = ra::row_slots(b);
            bool compiled = false;
            int smallest = 0;
            for (int k = ra::N_WIDTHS - 1; k >= 0; --k) {
                if (ra::WIDTHS[k] == S) compiled = true;
                if (ra::WIDTHS[k] * ra::LANES >= W) smallest = ra::WIDTHS[k];
            }
            CHECK(W == 2 * b + 1 && compiled && S == smallest && S <= ra::MAX_SLOTS, "band %d width %d", b, S);
            CHECK(ra::slots_needed(b) * ra::LANES >= W && (ra::slots_needed(b) - 1) * ra::LANES < W, "band %d needs %d", b, ra::slots_needed(b));
            std::vector<int> owners((size_t)W, 0);
            for (int lane = 0; lane < ra::LANES; ++lane)
                for (int s = 0; s < S; ++s)
                    if (lane * S + s < W) ++owners[(size_t)(lane * S + s)];
            for (int c = 0; c < W; ++c) CHECK(owners[(size_t)c] == 1, "band %d slot %d has %d owners", b, c, owners[(size_t)c]);
            slots += W;
        }
        for (int k = 1; k < ra::N_WIDTHS; ++k) CHECK(ra::WIDTHS[k - 1] < ra::WIDTHS[k], "widths ascend");
        CHECK(ra::WIDTHS[ra::N_WIDTHS - 1] == 17 && ra::MAX_SLOTS == 17, "the widest lane");
        std::printf("owners: %lld slots of 512 bands, one owner each\n", slots);
    }
    // the rows a pair walks: all of them, or as far as the first row whose every cell lies behind the allele's end
    {
        std::mt19937 rng(5);
        int n_cases = 0;
        for (int t = 0; t < 20000; ++t) {
            const int n = (int)(rng() % 65536), m = (int)(rng() % (t % 3 ? 400 : 65536)), b = 1 + (int)(rng() % 512);
            const int rows = ra::rows_walked(n, m, b);
            int first_behind = -1;                    // the first row i whose smallest j, i - b, exceeds m
            for (int i = std::max(0, m + b - 2); i <= m + b + 3; ++i)
                if (i - b > m) { first_behind = i; break; }
            CHECK(rows == std::min(n, first_behind) && rows >= 0 && rows <= n, "rows of n=%d m=%d B=%d: %d", n, m, b, rows);
            ++n_cases;
        }
        CHECK(ra::rows_walked(65535, 65535, 512) == 65535 && ra::rows_walked(0, 0, 1) == 0 && ra::rows_walked(9, 0, 1) == 2, "row edges");
        std::printf("rows: %d cases\n", n_cases);
    }
    // the status and the record of a pair, against the sentences of include/vapor_hip.h
    {
        std::mt19937 rng(11);
        int n_cases = 0, refused = 0;
        for (int t = 0; t < 3000; ++t) {
            const int32_t n_seqs = (int32_t)(rng() % 6);
            std::vector<int32_t> len((size_t)n_seqs);
            std::vector<uint32_t> chunk0((size_t)n_seqs);
            uint32_t at = (t % 7 == 0) ? 0xFFFFF000u : 0u;       // (planes past 2^32 words: the record's offsets are 64 bit)
            for (int32_t s = 0; s < n_seqs; ++s) {
                const uint32_t r = rng() % 10;
                len[(size_t)s] = r == 0 ? 0 : r == 1 ? 65535 : r == 2 ? 65536 + (int32_t)(rng() % 100000) : (int32_t)(rng() % 70000);
                chunk0[(size_t)s] = at;
                at += ((uint32_t)len[(size_t)s] + 31u) / 32u + 3u;
            }
            auto len_of = [&](int32_t s) { return len.at((size_t)s); };
            auto chunk_of = [&](int32_t s) { return chunk0.at((size_t)s); };
            for (int q = 0; q < 8; ++q) {
                vapor_pair a{(int32_t)(rng() % 9) - 2, (int32_t)(rng() % 9) - 2, 0, (int32_t)rng(), (uint32_t)rng()};
                const bool idx_ok = a.seq1 >= 0 && a.seq1 < n_seqs && a.seq2 >= 0 && a.seq2 < n_seqs;
                const int32_t l2 = idx_ok ? len[(size_t)a.seq2] : 0;
                switch (rng() % 5) {
                case 0: a.off2 = l2; break;
                case 1: a.off2 = l2 + 1; break;
                case 2: a.off2 = -1 - (int32_t)(rng() % 3); break;
                case 3: a.off2 = l2 ? (int32_t)(rng() % (uint32_t)l2) : 0; break;
                default: a.off2 = (int32_t)(rng() % 40); break;
                }
                bool ok = idx_ok;
                if (ok) ok = len[(size_t)a.seq1] <= 65535 && l2 <= 65535 && a.off2 >= 0 && a.off2 <= l2;
                const ra::RPair r = ra::pair_record(a, n_seqs, len_of, chunk_of);
                CHECK(ra::pair_status(a, n_seqs, len_of) == (ok ? VAPOR_OK : VAPOR_E_ARG) && r.status == (ok ? VAPOR_OK : VAPOR_E_ARG),
                      "status of (%d, %d, %d) over %d sequences", a.seq1, a.seq2, a.off2, n_seqs);
                if (ok) {
                    CHECK(r.n == len[(size_t)a.seq1] && r.m == l2 - a.off2 && r.off2 == a.off2 && r.m >= 0, "lengths of (%d, %d, %d)", a.seq1,
                          a.seq2, a.off2);
                    CHECK(r.word1 == (uint64_t)chunk0[(size_t)a.seq1] * 4 && r.word2 == (uint64_t)chunk0[(size_t)a.seq2] * 4, "words of (%d, %d)",
                          a.seq1, a.seq2);
                } else {
                    ++refused;
                }
                ++n_cases;
            }
        }
        CHECK(sizeof(ra::RPair) == 32, "the record is 32 bytes");
        std::printf("pairs: %d cases, %s refused\n", n_cases, refused > 1000 ? "many" : "few");
    }
    // the launch: every pair has a wavefront, no workgroup is empty
    {
        int n_cases = 0;
        for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)ra::WAVES, (int64_t)ra::WAVES + 1, (int64_t)300, (int64_t)65537, ra::MAX_PAIRS}) {
            const int64_t g = ra::grid_of(n);
            CHECK(g * ra::WAVES >= n && (g - 1) * ra::WAVES < n && g >= 1 && g < ((int64_t)1 << 31), "grid of %lld", (long long)n);
            ++n_cases;
        }
        CHECK(2 * (int64_t)ra::INF + 2 * VAPOR_MAX_SEQ_LEN + 4 * VAPOR_MAX_BAND < ((int64_t)1 << 31), "two INF and a path stay in 32 bits");
        std::printf("launch: %d sizes\n", n_cases);
    }
    if (g_bad) {
        std::printf("realign_check: %d FAILED\n", g_bad);
        return 1;
    }
    std::printf("realign_check: all equal\n");
    return 0;
}
