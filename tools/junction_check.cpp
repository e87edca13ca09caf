// junction_check.cpp - the host plan of vapor_realign_junction (vapor_amd/csrc/vapor_junction_plan.h) held to direct statements of
// its rules, as a program of its own under the address and undefined-behaviour sanitizers (tests/test_junction_cpu.py builds and
// runs it; no HIP, no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc
//       tools/junction_check.cpp -o junction_check && ./junction_check
#include "vapor_junction_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace ra = vapor_realign;
namespace tr = vapor_trace;
namespace vj = vapor_junction;

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
    // the layouts, the tasks and the key of a row's reduction
    {
        CHECK(vj::OUT == 8 && vj::O_STATUS == 0 && vj::O_COST == 1 && vj::O_I == 2 && vj::O_J1 == 3 && vj::O_J2 == 4 && vj::O_FF == 5 && vj::O_FR == 6,
              "a pair's eight words");
        CHECK(vj::ROW == 4 && vj::R_F_FWD == 0 && vj::R_JF_FWD == 1 && vj::R_F_BWD == 2 && vj::R_JF_BWD == 3, "a row's four words");
        CHECK(sizeof(vj::JPair) == 40, "a pair record");
        CHECK(vj::pair_rows(0) == 1 && vj::pair_rows(65535) == 65536 && vj::pair_bytes(0) == 16 && vj::pair_bytes(9999) == 160000, "16 (ns + 1) bytes");
        CHECK(vj::tasks_of(0) == 0 && vj::tasks_of(5) == 10 && vj::task_pair(7) == 3 && vj::task_backward(7) && !vj::task_backward(6), "the tasks");
        CHECK(vj::rows_grid(1) == 1 && vj::rows_grid(2) == 1 && vj::rows_grid(3) == 2 && vj::pick_grid(4) == 1 && vj::pick_grid(5) == 2, "the grids");
        CHECK(vj::pass_pos(10, false, 3) == 3 && vj::pass_pos(10, true, 0) == 9 && vj::pass_pos(10, true, 9) == 0, "a pass's symbols");
        CHECK(vj::split_j2(100, 30) == 70 && vj::split_valid(5, 5) && !vj::split_valid(6, 5), "a split row");
        int n = 0;
        for (int d = 0; d <= 2 * VAPOR_MAX_SEQ_LEN; d += 977)
            for (int c = 0; c <= 2 * VAPOR_MAX_BAND; c += 31) {
                const int key = vj::row_key(d, c);
                CHECK(key >= 0 && key < vj::NO_CELL && vj::key_d(key) == d && vj::key_c(key) == c, "key of (%d, %d)", d, c);
                // ordered by D first, then by the slot
                CHECK(vj::row_key(d, c) < vj::row_key(d + 1, 0) && (c == 0 || vj::row_key(d, c - 1) < key), "order at (%d, %d)", d, c);
                ++n;
            }
        std::printf("layout and keys: stated, %d keys\n", n);
    }
    std::mt19937 rng(26);
    // a pair's status and record
    {
        int n_cases = 0, refused = 0, why[5] = {0, 0, 0, 0, 0};
        for (int t = 0; t < 24000; ++t) {
            const int32_t n_seqs = 1 + (int32_t)(rng() % 6);
            std::vector<int64_t> len((size_t)n_seqs), chunk((size_t)n_seqs);
            for (int s = 0; s < n_seqs; ++s) {
                const int what = (int)(rng() % 12);
                len[(size_t)s] = what == 0 ? VAPOR_MAX_SEQ_LEN + 1 + (int64_t)(rng() % 9) : what == 1 ? VAPOR_MAX_SEQ_LEN : (int64_t)(rng() % 3000);
                chunk[(size_t)s] = (int64_t)(rng() % 100000);
            }
            vapor_pair a{};
            a.seq1 = (int32_t)(rng() % (n_seqs + 2)) - 1;
            a.seq2 = (int32_t)(rng() % (n_seqs + 2)) - 1;
            a.off2 = rng() % 5 == 0 ? (int32_t)(rng() % 7) - 3 : 0;
            a.k = (int32_t)rng();
            a.flags = (uint32_t)rng();
            auto len_of = [&](int32_t s) { return len[(size_t)s]; };
            auto chunk_of = [&](int32_t s) { return chunk[(size_t)s]; };
            int want = VAPOR_OK, cause = 0;
            if (a.seq1 < 0 || a.seq1 >= n_seqs || a.seq2 < 0 || a.seq2 >= n_seqs) { want = VAPOR_E_ARG; cause = 1; }
            else if (len_of(a.seq1) > VAPOR_MAX_SEQ_LEN || len_of(a.seq2) > VAPOR_MAX_SEQ_LEN) { want = VAPOR_E_ARG; cause = 2; }
            else if (a.off2 != 0) { want = VAPOR_E_ARG; cause = 3; }
            else if (len_of(a.seq1) > len_of(a.seq2)) { want = VAPOR_E_ARG; cause = 4; }
            CHECK(vj::pair_status(a, n_seqs, len_of) == want, "status of case %d", t);
            const vj::JPair r = vj::pair_record(a, n_seqs, len_of, chunk_of);
            if (want) {
                CHECK(r.status == want && r.word1 == 0 && r.word2 == 0 && r.ns == 0 && r.nl == 0 && r.row0 == 0, "a refused pair's record, case %d", t);
            } else {
                CHECK(r.status == 0 && r.word1 == (uint64_t)chunk_of(a.seq1) * 4 && r.word2 == (uint64_t)chunk_of(a.seq2) * 4 &&
                          r.ns == len_of(a.seq1) && r.nl == len_of(a.seq2) && r.ns <= r.nl,
                      "a served pair's record, case %d", t);
            }
            refused += want != 0;
            why[cause]++;
            ++n_cases;
        }
        std::printf("pairs: %d cases, %s\n", n_cases,
                    refused > 5000 && why[0] > 2000 && why[1] > 500 && why[2] > 500 && why[3] > 500 && why[4] > 500 ? "every refusal met" : "a refusal not met");
    }
    // the workspace: the served pairs' tables one behind the other, without overlap, and the budget
    {
        int n_cases = 0, over = 0;
        for (int t = 0; t < 2000; ++t) {
            const int64_t n = (int64_t)(rng() % 200);
            std::vector<vj::JPair> recs((size_t)n);
            int64_t want_rows = 0;
            for (auto& r : recs) {
                r = vj::JPair{0, 0, 0, 0, rng() % 7 == 0 ? VAPOR_E_ARG : 0, 0, -1};
                if (!r.status) r.ns = (int32_t)(rng() % (t % 9 == 0 ? 65536 : 4000)), r.nl = r.ns;
            }
            const int64_t rows = vj::lay_out(recs.data(), n);
            for (const auto& r : recs) {
                CHECK(r.row0 == (r.status ? 0 : want_rows), "row0 of a pair, case %d", t);
                if (!r.status) want_rows += (int64_t)r.ns + 1;
            }
            CHECK(rows == want_rows, "rows of case %d", t);
            const int64_t budget = t % 3 == 0 ? 0 : (int64_t)(rng() % 4) * (tr::BUDGET_FLOOR / 2);
            const bool want_fit = 16 * want_rows <= std::max<int64_t>(budget, tr::BUDGET_FLOOR);
            CHECK(vj::fits(rows, budget) == want_fit, "the budget of case %d", t);
            over += !want_fit;
            ++n_cases;
        }
        CHECK(vj::fits(tr::BUDGET_DEFAULT / 16, tr::BUDGET_DEFAULT) && !vj::fits(tr::BUDGET_DEFAULT / 16 + 1, tr::BUDGET_DEFAULT), "the budget's edge");
        CHECK(vj::fits(2 * 65536, 0), "the command line's two pairs a locus are far below the floor");
        std::printf("workspace: %d calls, %s over the budget\n", n_cases, over > 3 ? "some" : "none");
    }
    // the caller's row table
    {
        int n_cases = 0, refused = 0, small = 0;
        for (int t = 0; t < 2000; ++t) {
            const int64_t n = (int64_t)(rng() % 12);
            std::vector<vj::JPair> recs((size_t)n);
            std::vector<int64_t> off(1, 0);
            for (auto& r : recs) {
                r = vj::JPair{0, 0, (int32_t)(rng() % 50), 0, rng() % 6 == 0 ? VAPOR_E_ARG : 0, 0, 0};
                off.push_back(off.back() + (rng() % 5 == 0 ? (int64_t)(rng() % 50) : (int64_t)r.ns + 1 + (int64_t)(rng() % 3)));
            }
            const int what = (int)(rng() % 5);
            if (what == 1) off[0] = 1;
            if (what == 2 && n > 1) off[(size_t)(1 + rng() % (n - 1))] = off.back() + 1;
            bool want = off[0] == 0;
            for (int64_t k = 0; k < n; ++k) want = want && off[(size_t)k] <= off[(size_t)k + 1];
            CHECK(vj::row_off_ok(n, off.data()) == want, "row_off of case %d", t);
            refused += !want;
            if (want)
                for (int64_t k = 0; k < n; ++k) {
                    const bool holds = recs[(size_t)k].status != 0 || off[(size_t)k + 1] - off[(size_t)k] >= (int64_t)recs[(size_t)k].ns + 1;
                    CHECK(vj::slot_holds(recs[(size_t)k], off.data(), k) == holds, "slot %lld of case %d", (long long)k, t);
                    small += !holds;
                }
            ++n_cases;
        }
        CHECK(!vj::row_off_ok(0, nullptr), "a null table");
        std::printf("row tables: %d calls, %s\n", n_cases, refused > 200 && small > 200 ? "refused ones and short slots among them" : "too few refused");
    }
    if (g_bad) {
        std::printf("junction_check: %d FAILED\n", g_bad);
        return 1;
    }
    std::printf("junction_check: all equal\n");
    return 0;
}
