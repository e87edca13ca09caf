// polish_check.cpp - the host plan of vapor_realign_polish (vapor_amd/csrc/vapor_polish_plan.h) held to direct statements of its
// rules, and the plan of a whole call that vapor_amd/csrc/vapor_polish_call.h puts together from them (the polish alone; the
// re-vote's share is tools/revote_check.cpp's), as a program of its own under the address and undefined-behaviour sanitizers
// (tests/test_polish_cpu.py builds and runs it; no HIP, no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc
//       tools/polish_check.cpp -o polish_check && ./polish_check
#include "polish_call_world.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace ra = vapor_realign;
namespace tr = vapor_trace;
namespace pp = vapor_polish;

int main()
{
    // the rule's constants, the call codes, the counters, the statistics and the sizes of a locus's tables
    {
        CHECK(pp::MIN_COV == 3 && pp::RMAX == 64 && pp::MAX_SITES == 256, "the rule's constants");
        CHECK(pp::CALL_KEEP == 4 && pp::CALL_DELETE == 5 && pp::SITE_BIT == 8, "the call codes");
        CHECK(pp::COUNTERS == 8 && pp::C_A == 0 && pp::C_T == 3 && pp::C_O == 4 && pp::C_DL == 5 && pp::C_BCOV == 6 && pp::C_INS == 7, "the counters");
        CHECK(pp::STATS == 8 && pp::S_STATUS == 0 && pp::S_PAIRS == 1 && pp::S_PCOV == 2 && pp::S_PSUB == 3 && pp::S_PDEL == 4 && pp::S_SITES == 5 &&
                  pp::S_PINS == 6 && pp::S_DROPPED == 7,
              "the statistics");
        CHECK(pp::SITE_WORDS == 512 && pp::INS_WORDS * 4 == 256 * 64 && pp::INSB_WORDS == 256 * 64 * 4, "a locus's tables");
        CHECK(sizeof(pp::PLocus) == 40, "a locus record");
        CHECK(pp::align4(0) == 0 && pp::align4(1) == 4 && pp::align4(4) == 4 && pp::align4(5) == 8, "16-byte pieces");
        CHECK(pp::calls_words(0) == 0 && pp::calls_words(1) == 1 && pp::calls_words(4) == 1 && pp::calls_words(5) == 2, "a byte a column");
        ra::RPair ok{0, 0, 100, 70, 5, 0}, bad{0, 0, 0, 0, 0, VAPOR_E_ARG};
        CHECK(pp::run_cap(ok) == 171 && pp::run_cap(bad) == 1, "a slot holds n + m steps");
        std::printf("constants and layout: stated\n");
    }
    std::mt19937 rng(11);
    // the call-level checks of the two tables
    {
        int n_cases = 0, refused = 0;
        for (int t = 0; t < 2000; ++t) {
            const int64_t n_loci = (int64_t)(rng() % 12);
            std::vector<int64_t> first(1, 0), col(1, 0);
            for (int64_t g = 0; g < n_loci; ++g) {
                first.push_back(first.back() + (int64_t)(rng() % 5));
                col.push_back(col.back() + (int64_t)(rng() % (t % 7 == 0 ? 70000 : 3000)));
            }
            int64_t n_pairs = first.back();
            const int what = (int)(rng() % 8);
            if (what == 1) n_pairs += 1;
            if (what == 2) first[0] = 1;
            if (what == 3) col[0] = 1;
            if (what == 4 && n_loci > 1) first[(size_t)(1 + rng() % (n_loci - 1))] = first.back() + 1;
            if (what == 5 && n_loci > 1) col[(size_t)(1 + rng() % (n_loci - 1))] = col.back() + 1;
            bool want = first[0] == 0 && col[0] == 0 && first.back() == n_pairs;
            for (int64_t g = 0; g < n_loci; ++g)
                want = want && first[(size_t)g] <= first[(size_t)g + 1] && col[(size_t)g] <= col[(size_t)g + 1] &&
                       col[(size_t)g + 1] - col[(size_t)g] <= VAPOR_MAX_SEQ_LEN;
            CHECK(pp::tables_ok(n_pairs, n_loci, first.data(), col.data()) == want, "tables of case %d", t);
            refused += !want;
            ++n_cases;
        }
        CHECK(!pp::tables_ok(0, 0, nullptr, nullptr) && !pp::tables_ok(0, -1, nullptr, nullptr), "null tables");
        std::printf("tables: %d calls, %s among them\n", n_cases, refused > 200 ? "refused ones" : "few refused");
    }
    // a locus's status
    {
        int n_cases = 0, met[4] = {0, 0, 0, 0};
        for (int t = 0; t < 3000; ++t) {
            const int band = 1 + (int)(rng() % 512), S = ra::lane_width(band);
            const int n = (int)(rng() % (t % 50 == 0 ? 80 : 7));
            const int64_t len2 = 1 + (int64_t)(rng() % 60000);
            std::vector<ra::RPair> recs((size_t)n);
            std::vector<int32_t> seq2((size_t)n, 4);
            const int what = (int)(rng() % 6);
            for (auto& r : recs) {
                const int32_t off2 = (int32_t)(rng() % len2);
                r = ra::RPair{0, 0, (int32_t)(rng() % (t % 50 == 0 ? 65536 : 5000)), (int32_t)(len2 - off2), off2, 0};
            }
            if (what == 1 && n) recs[rng() % n].status = VAPOR_E_ARG;
            if (what == 2 && n > 1) seq2[1 + rng() % (n - 1)] = 5;
            const int64_t span = what == 3 ? len2 + 1 : len2;
            const int64_t budget = t % 3 == 0 ? 0 : tr::BUDGET_DEFAULT;
            int64_t words = -1;
            const int got = pp::locus_status(recs.data(), 0, n, span, band, S, budget, [&](int64_t k) { return seq2[(size_t)k]; },
                                             [&](int64_t) { return len2; }, words);
            int want = VAPOR_OK;
            int64_t want_words = 0;
            for (int k = 0; k < n; ++k) {
                if (recs[(size_t)k].status || seq2[(size_t)k] != seq2[0]) want = VAPOR_E_ARG;
                want_words += (int64_t)std::min<int64_t>(recs[(size_t)k].n, (int64_t)recs[(size_t)k].m + band + 1) * 64 * (S <= 16 ? 1 : 2);
            }
            if (n && span != len2) want = VAPOR_E_ARG;
            if (want == VAPOR_OK && want_words * 4 > tr::budget_of(budget)) want = VAPOR_E_NOMEM;
            CHECK(got == want, "status of case %d: %d, not %d", t, got, want);
            CHECK(words == (want == VAPOR_OK ? want_words : 0), "trace words of case %d", t);
            met[want == VAPOR_OK ? (n ? 0 : 3) : want == VAPOR_E_ARG ? 1 : 2]++;
            ++n_cases;
        }
        std::printf("locus status: %d loci, %s\n", n_cases, met[0] > 100 && met[1] > 100 && met[2] > 3 && met[3] > 10 ? "every status met" : "a status not met");
    }
    // the groups: consecutive whole loci, every locus in one, no group above the budget unless it is one locus, greedy, and the
    // pieces of a group's buffer in order, 16-byte aligned, without overlap
    {
        int n_cases = 0, many = 0;
        for (int t = 0; t < 400; ++t) {
            const int64_t n_loci = (int64_t)(rng() % 150);
            const int64_t budget = t % 4 == 0 ? 0 : tr::BUDGET_FLOOR + (int64_t)(rng() % 4) * tr::BUDGET_FLOOR;
            const int64_t limit = tr::budget_of(budget) / 4;
            std::vector<int64_t> first(1, 0), col(1, 0), words, cap;
            for (int64_t g = 0; g < n_loci; ++g) {
                const int64_t np = (int64_t)(rng() % 9);
                first.push_back(first.back() + np);
                col.push_back(col.back() + (int64_t)(rng() % 5000));
                words.push_back(np ? (int64_t)(rng() % (t % 2 ? 4000000 : 40000)) / 64 * 64 : 0);
                cap.push_back(np ? 1 + (int64_t)(rng() % 9000) : 1);
            }
            std::vector<pp::Group> groups;
            const int64_t most = pp::plan_groups(n_loci, first.data(), col.data(), words.data(), cap.data(), budget, groups);
            CHECK((n_loci == 0) == groups.empty(), "no loci, no groups");
            int64_t next = 0, seen_most = 0;
            for (size_t k = 0; k < groups.size(); ++k) {
                const pp::Group& g = groups[k];
                CHECK(g.locus0 == next && g.locus1 > g.locus0 && g.locus1 <= n_loci, "group %zu is consecutive and not empty", k);
                next = g.locus1;
                const int64_t nl = g.locus1 - g.locus0, np = first[(size_t)g.locus1] - first[(size_t)g.locus0];
                CHECK(g.pair0 == first[(size_t)g.locus0] && g.pair1 == first[(size_t)g.locus1], "pairs of group %zu", k);
                CHECK(g.cols == col[(size_t)g.locus1] - col[(size_t)g.locus0], "columns of group %zu", k);
                int64_t w = 0, c = 0;
                for (int64_t l = g.locus0; l < g.locus1; ++l) {
                    w += words[(size_t)l];
                    c = std::max(c, cap[(size_t)l]);
                }
                CHECK(g.trace_words == w && g.cap_runs == c, "rows and run slots of group %zu", k);
                // the pieces: in this order, each on 16 bytes, each as large as stated
                CHECK(g.runs_off == w && g.zero_off >= g.runs_off + np * c && g.zero_off - (g.runs_off + np * c) < 4, "the run slots");
                CHECK(g.counts_off == g.zero_off && g.slot_off == g.counts_off + 8 * g.cols, "the counters");
                CHECK(g.calls_off >= g.slot_off + g.cols && g.stats_off >= g.calls_off + (g.cols + 3) / 4, "site slots and calls");
                CHECK(g.sites_off == g.stats_off + 8 * nl && g.ins_off == g.sites_off + 512 * nl && g.insb_off == g.ins_off + 4096 * nl &&
                          g.words == g.insb_off + 65536 * nl,
                      "the loci's tables");
                for (int64_t o : {g.zero_off, g.counts_off, g.calls_off, g.stats_off, g.sites_off, g.ins_off, g.insb_off}) CHECK(o % 4 == 0, "alignment");
                CHECK(g.words <= limit || nl == 1, "group %zu holds %lld words", k, (long long)g.words);
                if (k + 1 < groups.size()) {                 // (greedy: the next locus did not fit)
                    pp::Group more = g;
                    more.locus1 += 1;
                    more.pair1 = first[(size_t)more.locus1];
                    more.cols = col[(size_t)more.locus1] - col[(size_t)more.locus0];
                    more.trace_words += words[(size_t)g.locus1];
                    more.cap_runs = std::max(more.cap_runs, cap[(size_t)g.locus1]);
                    pp::lay_out(more);
                    CHECK(more.words > limit, "group %zu closed early", k);
                }
                seen_most = std::max(seen_most, g.words);
            }
            CHECK(next == n_loci && most == seen_most, "every locus in a group; the largest group");
            many += groups.size() > 1;
            ++n_cases;
        }
        std::printf("groups: %d calls, %s in several groups\n", n_cases, many > 20 ? "many" : "few");
    }
    // the plan of a whole call, the polish alone (vapor_polish_call.h): designed loci, then drawn ones at the floor budget - small
    // calls, and calls large enough for several groups - and at the default
    {
        namespace pc = vapor_polish_call;
        using world::pair_of;
        world::Met met;
        {
            world::World w;
            const int32_t allele = w.seq(300), other = w.seq(300), read = w.seq(120), wide = w.seq(65535), wide_read = w.seq(65535);
            w.locus(300, {}, {}, 0);                                                                        // without pairs: served
            w.locus(300, {pair_of(read, allele, 0), pair_of(-1, allele, 0), pair_of(read, allele, 10)}, {}, 0);      // a refused pair inside
            w.locus(300, {pair_of(read, allele, 0), pair_of(read, other, 0)}, {}, 0);                       // two seq2
            w.locus(299, {pair_of(read, allele, 0)}, {}, 0);                                                // columns that are not the allele's length
            // rows alone past the floor: five pairs of 65 535 rows, 64 dwords a row at band 100 - 84 MB
            w.locus(65535, std::vector<vapor_pair>(5, pair_of(wide_read, wide, 0)), {}, 0);
            w.locus(300, {pair_of(read, allele, 0), pair_of(read, allele, 300), pair_of(read, allele, 7)}, {}, 0);
            const int at_floor[6] = {0, VAPOR_E_ARG, VAPOR_E_ARG, VAPOR_E_ARG, VAPOR_E_NOMEM, 0}, n_served[6] = {0, 0, 0, 0, 0, 3};
            for (const int64_t budget : {(int64_t)0, tr::BUDGET_DEFAULT}) {
                const pc::Plan p(w.call(nullptr), w.seqs(), budget);
                for (int g = 0; g < 6; ++g) {
                    const int want = budget && g == 4 ? 0 : at_floor[g];
                    CHECK(p.loci[(size_t)g].status == want && p.loci[(size_t)g].n_pairs == (want ? 0 : g == 4 ? 5 : n_served[g]), "designed locus %d", g);
                    for (int64_t t = w.first[(size_t)g]; t < w.first[(size_t)g + 1]; ++t)
                        CHECK(p.recs[(size_t)t].status == want, "pair %lld of designed locus %d", (long long)t, g);
                }
                CHECK(p.loci[5].word2 == (uint64_t)(5 * allele + 3) * 4 && p.recs[(size_t)w.first[5] + 1].m == 0, "the served locus");
                world::hold(w, nullptr, budget, p, met, "designed loci");
            }
        }
        for (int t = 0; t < 64; ++t) {
            world::World w;
            const int bands[6] = {1, 31, 100, 256, 300, 512};
            w.band = bands[t % 6];
            const bool big = t % 2 == 1;
            if (t == 5) {                                                                                   // loci, and no pair at all
                for (int g = 0; g < 9; ++g) w.locus(100 * g, {}, {}, 0);
            } else
                world::draw(w, rng, big ? 60 + (int64_t)(rng() % 60) : 1 + (int64_t)(rng() % 30), big);
            const int64_t budget = t % 8 == 7 ? tr::BUDGET_DEFAULT : (int64_t)(rng() % 2) * tr::BUDGET_FLOOR;
            const pc::Plan p(w.call(nullptr), w.seqs(), budget);
            world::hold(w, nullptr, budget, p, met, "a drawn call");
        }
        // check_args, the polish's: every way alone, and the earlier of every two
        const auto fresh = [] {
            world::World w;
            const int32_t allele = w.seq(40), read = w.seq(30);
            w.locus(40, {pair_of(read, allele, 0), pair_of(read, allele, 3)}, {}, 0);
            w.locus(40, {pair_of(read, allele, 1)}, {}, 0);
            return w;
        };
        const char *null_or_count = "null argument or a pair count outside 0 .. 2^26", *band = "band outside 1 .. VAPOR_MAX_BAND";
        const char *loci = "a locus count outside 0 .. 2^26", *null_out = "null output";
        const char* tables = "first / col_off must ascend from 0, first must end at n_pairs, a locus has at most VAPOR_MAX_SEQ_LEN columns";
        const std::vector<world::Way> ways = {
            {null_or_count, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.handles = false; }},
            {null_or_count, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.n_pairs = -1; }},
            {null_or_count, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.n_pairs = ra::MAX_PAIRS + 1; }},
            {null_or_count, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.pairs = nullptr; }},
            {band, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.band = 0; }},
            {band, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.band = VAPOR_MAX_BAND + 1; }},
            {loci, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.n_loci = -1; }},
            {loci, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.n_loci = ra::MAX_PAIRS + 1; }},
            {tables, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.first = nullptr; }},
            {tables, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.col_off = nullptr; }},
            {tables, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.first[0] = 1; }},
            {tables, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.col_off[1] = w.col_off[2] + 1; }},
            {tables, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.first[2] = 4; }},
            {tables, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.col_off[2] = 40 + VAPOR_MAX_SEQ_LEN + 1; }},
            {null_out, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.stats = nullptr; }},
            {null_out, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.sites = nullptr; }},
            {null_out, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.ins = nullptr; }},
            {null_out, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.calls = nullptr; }},
        };
        const int n_args = world::hold_check_args(fresh, ways, false);
        {
            bool nothing = false;
            const pc::Call empty{true, 0, nullptr, 100, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            CHECK(!pc::check_args(empty, nothing) && nothing, "a call of nothing is in order and has nothing to run");
            world::World w = fresh();
            pc::Call c = w.call(nullptr);
            c.calls = nullptr;                                   // (no columns: no call bytes to write)
            w.col_off.assign(3, 0);
            CHECK(!pc::check_args(c, nothing) && !nothing, "loci without columns need no calls");
        }
        const bool all_met = met.served > 100 && met.arg > 50 && met.nomem >= 1 && met.no_pairs > 20 && met.several > 10;
        std::printf("call plan: %d calls, %s; check_args: %d cases\n", met.calls, all_met ? "every kind of locus, many in several groups" : "a kind not met", n_args);
    }
    if (g_bad) {
        std::printf("polish_check: %d FAILED\n", g_bad);
        return 1;
    }
    std::printf("polish_check: all equal\n");
    return 0;
}
