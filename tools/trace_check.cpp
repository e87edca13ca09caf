// trace_check.cpp - the host arithmetic of vapor_realign_trace (vapor_amd/csrc/vapor_trace_plan.h) held to direct statements of
// its rules, as a program of its own under the address and undefined-behaviour sanitizers (tests/test_trace_cpu.py builds and
// runs it; no HIP, no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc
//       tools/trace_check.cpp -o trace_check && ./trace_check
#include "vapor_trace_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>
#include <vector>

namespace ra = vapor_realign;
namespace tr = vapor_trace;

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
    // the words of a lane and of a pair: two bits a slot, every slot's bits inside the lane's words, the sizes the contract names
    {
        int n = 0;
        for (int k = 0; k < ra::N_WIDTHS; ++k) {
            const int S = ra::WIDTHS[k], words = tr::words_of(S);
            CHECK(words * 32 >= 2 * S && (words - 1) * 32 < 2 * S, "words of S=%d: %d", S, words);
            CHECK(words == (S <= 16 ? 1 : 2), "one dword up to 16 slots, two at 17: S=%d", S);
            for (int s = 0; s < S; ++s) CHECK((s >> 4) < words && (s & 15) * 2 + 2 <= 32, "slot %d of S=%d", s, S);
            CHECK(tr::row_words(S) * 4 == 256 * words, "a row of S=%d is %d lines of 256 bytes", S, words);
            ++n;
        }
        CHECK(tr::pair_bytes(10000, 9) == 2560000, "10 000 rows up to S = 9: 2.56 MB");
        CHECK(tr::pair_bytes(65535, 17) == 33553920 && tr::pair_bytes(65535, 17) <= tr::BUDGET_FLOOR, "the largest pair: 33.5 MB, inside the floor");
        CHECK(tr::pair_bytes(0, 17) == 0, "no rows, no bytes");
        std::printf("words: %d widths\n", n);
    }
    // the run word and the head
    {
        CHECK(tr::OP_EQ == 0 && tr::OP_X == 1 && tr::OP_I == 2 && tr::OP_D == 3, "the op codes");
        CHECK(tr::run_word(1, tr::OP_EQ) == 4u && tr::run_word(131070, tr::OP_D) == (131070u << 2 | 3u), "run words");
        CHECK((tr::run_word(2 * VAPOR_MAX_SEQ_LEN, 3) >> 2) == 2u * VAPOR_MAX_SEQ_LEN, "the longest run keeps its length");
        CHECK(tr::HEAD == 8 && tr::H_D == 0 && tr::H_STATUS == 1 && tr::H_I_END == 2 && tr::H_J_END == 3 && tr::H_N_RUNS == 4, "the head");
        CHECK(!tr::cap_ok(0) && !tr::cap_ok(-1) && tr::cap_ok(1) && tr::cap_ok(INT32_MAX), "cap_runs");
        std::printf("words and head: stated\n");
    }
    // the budget and the groups: consecutive, every pair in one, no group above the budget unless it is one pair, a pair with a
    // status takes nothing, the offsets are the running sums of the group
    {
        CHECK(tr::budget_of(0) == tr::BUDGET_FLOOR && tr::budget_of(-5) == tr::BUDGET_FLOOR && tr::budget_of(tr::BUDGET_FLOOR + 1) == tr::BUDGET_FLOOR + 1,
              "the floor");
        CHECK(tr::BUDGET_DEFAULT == ((int64_t)512 << 20) && tr::BUDGET_FLOOR == ((int64_t)64 << 20), "the default and the floor");
        std::mt19937 rng(7);
        int n_cases = 0, many = 0;
        for (int t = 0; t < 400; ++t) {
            const int band = 1 + (int)(rng() % 512), S = ra::lane_width(band);
            const int64_t n_pairs = (int64_t)(rng() % 200);
            const int64_t budget = t % 4 == 0 ? 0 : tr::BUDGET_FLOOR + (int64_t)(rng() % 4) * tr::BUDGET_FLOOR;
            std::vector<ra::RPair> recs((size_t)n_pairs);
            for (auto& r : recs) {
                r = ra::RPair{0, 0, (int32_t)(rng() % (t % 2 ? 65536 : 3000)), (int32_t)(rng() % 65536), 0, (rng() % 9 == 0) ? VAPOR_E_ARG : 0};
            }
            std::vector<int64_t> first;
            std::vector<uint64_t> off;
            const int64_t most = tr::plan_groups(recs.data(), n_pairs, band, S, budget, first, off);
            CHECK(first.size() >= 2 && first.front() == 0 && first.back() == n_pairs && (int64_t)off.size() == n_pairs, "shape of the groups");
            int64_t seen_most = 0;
            for (size_t g = 0; g + 1 < first.size(); ++g) {
                CHECK(first[g] <= first[g + 1] && (n_pairs == 0 || first[g] < first[g + 1]), "group %zu is empty", g);
                int64_t used = 0;
                for (int64_t p = first[g]; p < first[g + 1]; ++p) {
                    const ra::RPair& r = recs[(size_t)p];
                    const int64_t need = r.status ? 0 : (int64_t)std::min<int64_t>(r.n, (int64_t)r.m + band + 1) * 64 * (S <= 16 ? 1 : 2);
                    CHECK(off[(size_t)p] == (uint64_t)used, "offset of pair %lld", (long long)p);
                    used += need;
                }
                CHECK(used * 4 <= tr::budget_of(budget), "group %zu holds %lld words", g, (long long)used);
                // (greedy: the next group's first pair did not fit)
                if (g + 2 < first.size()) {
                    const ra::RPair& r = recs[(size_t)first[g + 1]];
                    CHECK((used + tr::pair_words(ra::rows_walked(r.n, r.m, band), S)) * 4 > tr::budget_of(budget), "group %zu closed early", g);
                }
                seen_most = std::max(seen_most, used);
            }
            CHECK(most == seen_most, "the largest group");
            many += first.size() > 2;
            ++n_cases;
        }
        std::printf("groups: %d calls, %s in several groups\n", n_cases, many > 20 ? "many" : "few");
    }
    // the end slot: the key prefers what the rule prefers.  Direct statement: every slot of the last row walked that stands for a
    // cell of the last row or of the last column, sorted by (largest i, largest j).
    {
        std::mt19937 rng(13);
        int n_cases = 0;
        for (int t = 0; t < 4000; ++t) {
            const int B = t % 5 == 0 ? 1 + (int)(rng() % 512) : 1 + (int)(rng() % 12);
            const int n = (int)(rng() % (t % 3 ? 40 : 2000)), m = (int)(rng() % (t % 3 ? 40 : 2000));
            const int rows = ra::rows_walked(n, m, B), W = ra::row_slots(B);
            std::vector<std::tuple<int, int, int>> cells;                        // (-i, -j, c): ascending is the rule's preference
            for (int c = 0; c < W; ++c) {
                const int j = rows + c - B;                                      // the slot's column in the last row walked
                if (j < 0) continue;
                if (j <= m) {
                    if (rows == n) cells.emplace_back(-n, -j, c);                // a cell of the last row
                } else {
                    const int i = m - c + B;                                     // where the slot's diagonal meets the last column
                    if (i >= 0 && i <= n && std::abs(i - m) <= B) cells.emplace_back(-i, -m, c);
                }
            }
            std::sort(cells.begin(), cells.end());
            std::vector<std::pair<int, int>> keyed;
            for (int c = -2; c < W + 2; ++c) {
                const int key = tr::end_key(c, n, m, B, rows);
                if (key != tr::NO_SLOT) keyed.emplace_back(key, c);
                CHECK(key == tr::NO_SLOT || (key >= 0 && key < (1 << 19)), "key %d of slot %d packs beside a slot", key, c);
            }
            std::sort(keyed.begin(), keyed.end());
            bool same = keyed.size() == cells.size();
            for (size_t k = 0; same && k < keyed.size(); ++k) {
                int ie = -1, je = -1;
                tr::end_cell(keyed[k].second, n, m, B, rows, ie, je);
                same = keyed[k].second == std::get<2>(cells[k]) && ie == -std::get<0>(cells[k]) && je == -std::get<1>(cells[k]) &&
                       (k == 0 || keyed[k].first != keyed[k - 1].first);
            }
            CHECK(same, "end slots of n=%d m=%d B=%d (%zu against %zu)", n, m, B, keyed.size(), cells.size());
            CHECK(!cells.empty(), "a pair has an end cell: n=%d m=%d B=%d", n, m, B);
            ++n_cases;
        }
        CHECK(tr::slot_of(7, 9, 4) == 6 && ra::row_slots(VAPOR_MAX_BAND) < 2048, "a slot is j - i + B and packs into 11 bits");
        std::printf("end slots: %d pairs\n", n_cases);
    }
    if (g_bad) {
        std::printf("trace_check: %d FAILED\n", g_bad);
        return 1;
    }
    std::printf("trace_check: all equal\n");
    return 0;
}
