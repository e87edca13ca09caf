// revote_check.cpp - the host plan of vapor_realign_revote (vapor_amd/csrc/vapor_revote_plan.h) held to direct statements of its
// rules, as a program of its own under the address and undefined-behaviour sanitizers (tests/test_revote_cpu.py builds and runs
// it; no HIP, no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc
//       tools/revote_check.cpp -o revote_check && ./revote_check
#include "vapor_revote_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace ra = vapor_realign;
namespace tr = vapor_trace;
namespace pp = vapor_polish;
namespace vr = vapor_revote;

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
    // the output layouts, the records and the sizes of a locus's pieces
    {
        CHECK(vr::VOUT == 4 && vr::V_D == 0 && vr::V_STATUS == 1 && vr::V_OFF2 == 2 && vr::V_M == 3, "a vote pair's four words");
        CHECK(vr::LOUT == 4 && vr::L_STATUS == 0 && vr::L_PLEN == 1, "a locus's four words");
        CHECK(sizeof(vr::VPair) == 24 && sizeof(vr::VLocus) == 48, "the records");
        CHECK(vr::spelt_cap(0) == 0 && vr::spelt_cap(1) == 65 && vr::spelt_cap(255) == 255 * 65 && vr::spelt_cap(256) == 256 * 65 &&
                  vr::spelt_cap(257) == 257 + 256 * 64 && vr::spelt_cap(65535) == 65535 + 16384,
              "the most symbols a polished allele has");
        for (int64_t len : {0, 1, 7, 31, 32, 33, 300, 65535}) {
            const int64_t cap = vr::spelt_cap(len), chunks = (cap + 31) / 32;
            CHECK(vr::own_words(len) >= len + 1 && vr::own_words(len) % 4 == 0 && vr::own_words(len) < len + 5, "own[] of %lld", (long long)len);
            CHECK(vr::stage_words(len) == 8 * chunks && vr::plane_words(len) == 4 * chunks, "whole chunks of %lld", (long long)len);
            CHECK(vr::locus_extra(len) == vr::own_words(len) + 12 * chunks && vr::locus_extra(len) % 4 == 0, "the pieces of %lld", (long long)len);
            // RaReader loads word k while 8 k < plen, plen <= cap: the last such word lies inside the plane
            CHECK(cap == 0 || (cap - 1) / 8 < vr::plane_words(len), "the reader stays inside %lld", (long long)len);
            // the pack kernel reads eight staged bytes a plane word
            CHECK(4 * vr::stage_words(len) == 8 * vr::plane_words(len) && 4 * vr::stage_words(len) >= cap, "the staging of %lld", (long long)len);
        }
        CHECK(vr::slot_ok(65, 1) && !vr::slot_ok(64, 1) && vr::slot_ok(0, 0) && !vr::slot_ok(300, 300) && vr::slot_ok(300 + 16384, 300), "a spelt slot");
        std::printf("constants and layout: stated\n");
    }
    std::mt19937 rng(27);
    // the call-level checks of vfirst and spelt_off
    {
        int n_cases = 0, refused = 0;
        for (int t = 0; t < 2000; ++t) {
            const int64_t n_loci = (int64_t)(rng() % 12);
            std::vector<int64_t> vf(1, 0), so(1, 0);
            for (int64_t g = 0; g < n_loci; ++g) {
                vf.push_back(vf.back() + (int64_t)(rng() % 6));
                so.push_back(so.back() + (int64_t)(rng() % 5000));
            }
            int64_t n_votes = vf.back();
            const int what = (int)(rng() % 8);
            if (what == 1) n_votes += 1;
            if (what == 2) vf[0] = 1;
            if (what == 3) so[0] = 1;
            if (what == 4 && n_loci > 1) vf[(size_t)(1 + rng() % (n_loci - 1))] = vf.back() + 1;
            if (what == 5 && n_loci > 1) so[(size_t)(1 + rng() % (n_loci - 1))] = so.back() + 1;
            if (what == 6) n_votes = -1;
            bool want_v = vf[0] == 0 && vf.back() == n_votes && n_votes >= 0, want_s = so[0] == 0;
            for (int64_t g = 0; g < n_loci; ++g) {
                want_v = want_v && vf[(size_t)g] <= vf[(size_t)g + 1];
                want_s = want_s && so[(size_t)g] <= so[(size_t)g + 1];
            }
            CHECK(vr::vfirst_ok(n_votes, n_loci, vf.data()) == want_v, "vfirst of case %d", t);
            CHECK(vr::spelt_off_ok(n_loci, so.data()) == want_s, "spelt_off of case %d", t);
            refused += !want_v || !want_s;
            ++n_cases;
        }
        CHECK(!vr::vfirst_ok(0, 0, nullptr) && !vr::spelt_off_ok(0, nullptr) && !vr::vfirst_ok(ra::MAX_PAIRS + 1, 0, nullptr), "null tables");
        std::printf("tables: %d calls, %s among them\n", n_cases, refused > 200 ? "refused ones" : "few refused");
    }
    // a vote pair's record
    {
        int n_cases = 0, met[2] = {0, 0};
        const int32_t n_seqs = 9;
        std::vector<int64_t> lens(n_seqs);
        for (int t = 0; t < 20000; ++t) {
            for (auto& l : lens) l = (int64_t)(rng() % (t % 40 == 0 ? 70000 : 3000));
            vapor_pair a{};
            a.seq1 = (int32_t)(rng() % 11) - 1;
            a.seq2 = (int32_t)(rng() % 11) - 1;
            a.off2 = (int32_t)(rng() % 3200) - 5;
            const int64_t allele = (int64_t)(rng() % 4 == 0 ? (int64_t)(rng() % 10) - 1 : a.seq2);
            const int32_t locus = (int32_t)(rng() % 100);
            const vr::VPair r = vr::vote_record(a, n_seqs, allele, locus, [&](int32_t s) { return lens[(size_t)s]; }, [&](int32_t s) { return 7 * s; });
            bool ok = a.seq1 >= 0 && a.seq1 < n_seqs && a.seq2 >= 0 && a.seq2 < n_seqs;
            ok = ok && lens[(size_t)a.seq1] <= VAPOR_MAX_SEQ_LEN && lens[(size_t)a.seq2] <= VAPOR_MAX_SEQ_LEN && a.off2 >= 0 && a.off2 <= lens[(size_t)a.seq2];
            ok = ok && allele >= 0 && allele == a.seq2;
            CHECK(r.locus == locus && r.status == (ok ? VAPOR_OK : VAPOR_E_ARG), "status of vote pair %d", t);
            if (ok) CHECK(r.word1 == (uint64_t)(28 * a.seq1) && r.n == lens[(size_t)a.seq1] && r.off2 == a.off2, "record of vote pair %d", t);
            else CHECK(r.word1 == 0 && r.n == 0 && r.off2 == 0, "a refused vote pair is empty (%d)", t);
            met[ok]++;
            ++n_cases;
        }
        std::printf("vote pairs: %d cases, %s\n", n_cases, met[0] > 2000 && met[1] > 2000 ? "served and refused ones" : "one kind only");
    }
    // the groups with the re-vote's pieces charged: polish's groups where nothing is added, never above the budget unless one locus,
    // greedy; and the pieces of every locus in their group's extra stretch, on 16 bytes, without overlap
    {
        int n_cases = 0, many = 0, fewer = 0;
        for (int t = 0; t < 300; ++t) {
            const int64_t n_loci = (int64_t)(rng() % 120);
            const int64_t budget = t % 4 == 0 ? 0 : tr::BUDGET_FLOOR + (int64_t)(rng() % 3) * tr::BUDGET_FLOOR;
            const int64_t limit = tr::budget_of(budget) / 4;
            std::vector<int64_t> first(1, 0), col(1, 0), words, cap, extra, lens;
            for (int64_t g = 0; g < n_loci; ++g) {
                const int64_t np = (int64_t)(rng() % 9), len = (int64_t)(rng() % (t % 3 ? 5000 : 60000));
                first.push_back(first.back() + np);
                col.push_back(col.back() + len);
                lens.push_back(len);
                words.push_back(np ? (int64_t)(rng() % (t % 2 ? 4000000 : 40000)) / 64 * 64 : 0);
                cap.push_back(np ? 1 + (int64_t)(rng() % 9000) : 1);
                extra.push_back(rng() % 7 == 0 ? 0 : vr::locus_extra(len));           // (0: a locus that is not spelt)
            }
            std::vector<pp::Group> plain, groups;
            pp::plan_groups(n_loci, first.data(), col.data(), words.data(), cap.data(), budget, plain);
            const int64_t most = pp::plan_groups(n_loci, first.data(), col.data(), words.data(), cap.data(), budget, groups, extra.data());
            CHECK(groups.size() >= plain.size(), "more to hold, no fewer groups");
            fewer += groups.size() > plain.size();
            int64_t next = 0, seen_most = 0;
            for (size_t k = 0; k < groups.size(); ++k) {
                const pp::Group& g = groups[k];
                CHECK(g.locus0 == next && g.locus1 > g.locus0 && g.locus1 <= n_loci, "group %zu is consecutive and not empty", k);
                next = g.locus1;
                const int64_t nl = g.locus1 - g.locus0;
                int64_t sum = 0;
                for (int64_t l = g.locus0; l < g.locus1; ++l) sum += extra[(size_t)l];
                pp::Group bare = g;
                bare.extra = 0;
                pp::lay_out(bare);
                CHECK(g.extra == sum && g.extra_off == bare.words && g.words == bare.words + sum && g.extra_off % 4 == 0, "the extra stretch of group %zu", k);
                CHECK(g.extra_off >= g.zero_off, "the group's clear reaches the pieces");
                CHECK(g.words <= limit || nl == 1, "group %zu holds %lld words", k, (long long)g.words);
                if (k + 1 < groups.size()) {                 // (greedy: the next locus did not fit)
                    pp::Group more = g;
                    more.locus1 += 1;
                    more.pair1 = first[(size_t)more.locus1];
                    more.cols = col[(size_t)more.locus1] - col[(size_t)more.locus0];
                    more.trace_words += words[(size_t)g.locus1];
                    more.cap_runs = std::max(more.cap_runs, cap[(size_t)g.locus1]);
                    more.extra += extra[(size_t)g.locus1];
                    pp::lay_out(more);
                    CHECK(more.words > limit, "group %zu closed early", k);
                }
                seen_most = std::max(seen_most, g.words);
                // the pieces
                std::vector<vr::VLocus> vl((size_t)nl);
                int64_t stage_base = -1;
                const int64_t used = vr::place(g.extra_off, nl, lens.data() + g.locus0, extra.data() + g.locus0, vl.data(), stage_base);
                CHECK(used == sum, "the pieces of group %zu fill what was charged", k);
                std::vector<std::pair<int64_t, int64_t>> spans;     // (start, words) of every piece
                int64_t stage_end = stage_base;
                for (int64_t l = 0; l < nl; ++l) {
                    const int64_t len = lens[(size_t)(g.locus0 + l)];
                    if (!extra[(size_t)(g.locus0 + l)]) continue;
                    spans.push_back({vl[(size_t)l].own_off, vr::own_words(len)});
                    spans.push_back({vl[(size_t)l].stage_off, vr::stage_words(len)});
                    spans.push_back({vl[(size_t)l].plane_off, vr::plane_words(len)});
                    CHECK(vl[(size_t)l].stage_off == stage_end, "the stagings are one stretch");
                    stage_end += vr::stage_words(len);
                }
                if (nl) CHECK(vl[0].plane_off == stage_end, "the planes follow the stagings");
                std::sort(spans.begin(), spans.end());
                int64_t at = g.extra_off;
                for (const auto& s : spans) {
                    CHECK(s.first % 4 == 0 && s.first >= at, "a piece on 16 bytes behind the one before");
                    at = s.first + s.second;
                }
                CHECK(at <= g.words, "the pieces end inside the group's buffer");
            }
            CHECK(next == n_loci && most == seen_most, "every locus in a group; the largest group");
            many += groups.size() > 1;
            ++n_cases;
        }
        std::printf("groups: %d calls, %s in several groups, %s\n", n_cases, many > 20 ? "many" : "few", fewer > 5 ? "the pieces move some cuts" : "no cut moved");
    }
    if (g_bad) {
        std::printf("revote_check: %d FAILED\n", g_bad);
        return 1;
    }
    std::printf("revote_check: all equal\n");
    return 0;
}
