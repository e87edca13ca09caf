// revote_check.cpp - the host plan of vapor_realign_revote (vapor_amd/csrc/vapor_revote_plan.h) held to direct statements of its
// rules, and what the re-vote adds to the plan of a whole call that vapor_amd/csrc/vapor_polish_call.h puts together - the alleles,
// the vote pairs, the pieces, the image, the dealing of the spelt bytes -, as a program of its own under the address and
// undefined-behaviour sanitizers (tests/test_revote_cpu.py builds and runs it; no HIP, no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc
//       tools/revote_check.cpp -o revote_check && ./revote_check
#include "polish_call_world.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace ra = vapor_realign;
namespace tr = vapor_trace;
namespace pp = vapor_polish;
namespace vr = vapor_revote;
namespace pc = vapor_polish_call;

// deal_spelt on a device that is made up: lout and the stagings filled as spell_kernel would fill them - plen symbols a locus
// that is spelt, now and then a plen past the cap, which no kernel writes and the host must clamp -, the caller's slots exactly
// spelt_off[n_loci] bytes of a canary.  A locus that is spelt and whose slot holds it receives min(plen, cap) bytes of its own
// staging at its offset; every other byte keeps the canary.
struct Dealt {
    int loci = 0, clamped = 0, past_group_0 = 0, untouched = 0;
};
static void hold_deal(const world::World& w, const pc::Plan& p, std::vector<uint8_t>& spelt, std::mt19937& rng, Dealt& met)
{
    const int64_t n_loci = w.n_loci();
    const uint8_t canary = 0xEE;
    const auto symbol = [](int64_t g, int64_t i) { return (uint8_t)(1 + (g * 31 + i) % 200); };
    std::vector<uint32_t> staged((size_t)p.staged_words, 0);
    std::vector<int32_t> lout((size_t)(vr::LOUT * n_loci), 0);
    std::vector<int64_t> given((size_t)n_loci, -1);                 // bytes a locus is due, -1: none
    for (size_t k = 0; k < p.groups.size(); ++k)
        for (int64_t g = p.groups[k].locus0; g < p.groups[k].locus1; ++g) {
            const vr::VLocus& vl = p.vloci[(size_t)g];
            lout[(size_t)(vr::LOUT * g)] = vl.status ? vl.status : vl.short_slot ? VAPOR_E_ARG : 0;
            if (vl.status) continue;
            const int64_t plen = rng() % 5 == 0 ? vl.cap + 1 + (int64_t)(rng() % 50) : (int64_t)(rng() % (vl.cap + 1));
            const int64_t written = std::min<int64_t>(plen, vl.cap);
            lout[(size_t)(vr::LOUT * g + vr::L_PLEN)] = (int32_t)plen;
            uint8_t* at = reinterpret_cast<uint8_t*>(staged.data() + p.stage_host[k] + (vl.stage_off - p.stage_base[k]));
            for (int64_t i = 0; i < written; ++i) at[i] = symbol(g, i);
            if (vl.short_slot) continue;
            given[(size_t)g] = written;
            met.loci += 1;
            met.clamped += plen > vl.cap;
            met.past_group_0 += k > 0 && written > 0;
        }
    std::fill(spelt.begin(), spelt.end(), canary);
    p.deal_spelt(staged.data(), lout.data(), w.spelt_off.data(), spelt.data());
    for (int64_t g = 0; g < n_loci; ++g) {
        const int64_t a = w.spelt_off[(size_t)g], b = w.spelt_off[(size_t)g + 1];
        int64_t wrong = 0;
        for (int64_t i = a; i < b; ++i) wrong += spelt[(size_t)i] != (i - a < given[(size_t)g] ? symbol(g, i - a) : canary);
        CHECK(wrong == 0 && given[(size_t)g] <= b - a, "the slot of locus %lld: %lld bytes wrong", (long long)g, (long long)wrong);
        met.untouched += given[(size_t)g] < 0 && b > a;
    }
}

// what the polish reads of a re-vote call's plan is the plan of the polish alone: the records and the loci everywhere, and what is
// relative to a group - col0, the pairs' loci and workspace offsets - wherever both plans start the locus's group at the same locus
static int hold_same_polish(const world::World& w, const pc::Plan& with, const pc::Plan& alone)
{
    const auto starts = [&](const pc::Plan& p) {
        std::vector<int64_t> s((size_t)w.n_loci());
        for (const pp::Group& gr : p.groups)
            for (int64_t g = gr.locus0; g < gr.locus1; ++g) s[(size_t)g] = gr.locus0;
        return s;
    };
    const std::vector<int64_t> sa = starts(with), sb = starts(alone);
    int agree = 0;
    CHECK(with.recs.size() == alone.recs.size() && (with.recs.empty() || memcmp(with.recs.data(), alone.recs.data(), sizeof(ra::RPair) * with.recs.size()) == 0),
          "the pair records of both plans");
    for (int64_t g = 0; g < w.n_loci(); ++g) {
        const pp::PLocus &x = with.loci[(size_t)g], &y = alone.loci[(size_t)g];
        CHECK(x.status == y.status && x.n_pairs == y.n_pairs && x.len == y.len && x.word2 == y.word2, "locus %lld of both plans", (long long)g);
        if (sa[(size_t)g] != sb[(size_t)g]) continue;
        ++agree;
        CHECK(x.col0 == y.col0, "col0 of locus %lld in both plans", (long long)g);
        for (int64_t t = w.first[(size_t)g]; t < w.first[(size_t)g + 1]; ++t)
            CHECK(with.off[(size_t)t] == alone.off[(size_t)t] && with.pair_locus[(size_t)t] == alone.pair_locus[(size_t)t], "pair %lld in both plans", (long long)t);
    }
    return agree;
}

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
    // the plan of a whole re-vote call (vapor_polish_call.h): designed loci, then drawn ones at the floor budget - small calls, and
    // calls large enough for several groups - and at the default; with and without the spelt output, with and without vote pairs
    {
        using world::pair_of;
        world::Met met;
        Dealt dealt;
        int agree = 0, unasked = 0, no_votes = 0;
        {
            world::World w;
            const int32_t allele = w.seq(300), twin = w.seq(300), longer = w.seq(301), read = w.seq(120), wide = w.seq(65535), wide_read = w.seq(65535);
            const int64_t cap = 300 + 64 * 256;
            // 0: pairs give the allele; a vote pair on another sequence, though as long, is refused.  The slot holds the cap exactly
            w.locus(300, {pair_of(read, allele, 0)}, {pair_of(read, allele, 5), pair_of(read, twin, 5), pair_of(read, allele, 300)}, cap);
            // 1: vote pairs only: a refused one and one whose seq2 has other columns are passed over, the third gives the allele,
            // the fourth names its twin.  The slot is one byte short
            w.locus(300, {}, {pair_of(-1, allele, 0), pair_of(read, longer, 0), pair_of(read, twin, 9), pair_of(read, allele, 9)}, cap - 1);
            w.locus(300, {}, {}, cap + 1);                                                               // 2: neither
            w.locus(300, {}, {pair_of(read, longer, 0), pair_of(read, allele, 301)}, cap);              // 3: vote pairs, none that qualifies
            w.locus(300, {pair_of(read, allele, 0), pair_of(read, twin, 0)}, {pair_of(read, allele, 0)}, cap);      // 4: refused by the polish
            // 5: the rows past the floor; its vote pairs, the refused one too, say so
            w.locus(65535, std::vector<vapor_pair>(5, pair_of(wide_read, wide, 0)), {pair_of(read, wide, 0), pair_of(-1, wide, 0)}, 0);
            uint8_t spelt[1];
            const pc::RevoteArgs rv = w.revote(spelt);
            const pc::Plan p(w.call(&rv), w.seqs(), 0);
            const int want[6] = {0, 0, VAPOR_E_ARG, VAPOR_E_ARG, VAPOR_E_ARG, VAPOR_E_NOMEM};
            for (int g = 0; g < 6; ++g) CHECK(p.vloci[(size_t)g].status == want[g], "designed locus %d", g);
            CHECK(p.vloci[0].word2 == (uint64_t)(5 * allele + 3) * 4 && p.vloci[1].word2 == (uint64_t)(5 * twin + 3) * 4, "the alleles");
            CHECK(p.vloci[0].cap == cap && !p.vloci[0].short_slot && p.vloci[1].short_slot == 1, "cap, and a slot on both sides of it");
            const int votes[12] = {0, VAPOR_E_ARG, 0, VAPOR_E_ARG, VAPOR_E_ARG, 0, VAPOR_E_ARG, VAPOR_E_ARG, VAPOR_E_ARG, VAPOR_E_ARG, VAPOR_E_NOMEM, VAPOR_E_NOMEM};
            for (int t = 0; t < 12; ++t) CHECK(p.vrecs[(size_t)t].status == votes[t], "designed vote pair %d carries %d", t, p.vrecs[(size_t)t].status);
            world::hold(w, &rv, 0, p, met, "designed loci");
        }
        for (int t = 0; t < 64; ++t) {
            world::World w;
            const int bands[6] = {1, 31, 100, 256, 300, 512};
            w.band = bands[t % 6];
            const bool big = t % 2 == 1;
            world::draw(w, rng, big ? 60 + (int64_t)(rng() % 60) : 1 + (int64_t)(rng() % 30), big);
            if (t % 7 == 6) {                                                                            // a re-vote without vote pairs
                w.votes.clear();
                std::fill(w.vfirst.begin(), w.vfirst.end(), 0);
                ++no_votes;
            }
            if (t == 9) {                                                                                // loci, and no pair at all
                w.pairs.clear();
                std::fill(w.first.begin(), w.first.end(), 0);
            }
            const int64_t budget = t % 8 == 7 ? tr::BUDGET_DEFAULT : (int64_t)(rng() % 2) * tr::BUDGET_FLOOR;
            std::vector<uint8_t> spelt((size_t)w.spelt_off.back());
            uint8_t* const asked = t % 5 == 4 ? nullptr : spelt.data();
            const pc::RevoteArgs rv = w.revote(asked);
            const pc::Plan p(w.call(&rv), w.seqs(), budget);
            world::hold(w, &rv, budget, p, met, "a drawn call");
            if (g_bad) break;
            if (asked) hold_deal(w, p, spelt, rng, dealt);
            else {                                                                                       // no spelt output: no host copy, no slot too short
                ++unasked;
                CHECK(p.staged_words == 0 && std::all_of(p.stage_host.begin(), p.stage_host.end(), [](int64_t v) { return v == 0; }), "nothing staged");
                CHECK(std::none_of(p.vloci.begin(), p.vloci.end(), [](const vr::VLocus& v) { return v.short_slot; }), "no slot asked for, none short");
            }
            const pc::Plan alone(w.call(nullptr), w.seqs(), budget);
            agree += hold_same_polish(w, p, alone);
        }
        // check_args, what the re-vote adds: every way alone, and the earlier of every two
        const auto fresh = [] {
            world::World w;
            const int32_t allele = w.seq(40), read = w.seq(30);
            w.locus(40, {pair_of(read, allele, 0), pair_of(read, allele, 3)}, {pair_of(read, allele, 0)}, 3000);
            w.locus(40, {pair_of(read, allele, 1)}, {pair_of(read, allele, 2), pair_of(read, allele, 4)}, 3000);
            return w;
        };
        const char *vote_count = "a vote pair count outside 0 .. 2^26", *vfirst = "vfirst must ascend from 0 to n_votes", *null_out = "null output";
        const char *spelt_off = "spelt_off must ascend from 0", *band = "band outside 1 .. VAPOR_MAX_BAND", *loci = "a locus count outside 0 .. 2^26";
        const char* tables = "first / col_off must ascend from 0, first must end at n_pairs, a locus has at most VAPOR_MAX_SEQ_LEN columns";
        const std::vector<world::Way> ways = {
            {"null argument or a pair count outside 0 .. 2^26", [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.handles = false; }},
            {band, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.band = 0; }},
            {loci, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.n_loci = ra::MAX_PAIRS + 1; }},
            {vote_count, [](world::World&, pc::Call&, pc::RevoteArgs& rv) { rv.n_votes = -1; }},
            {vote_count, [](world::World&, pc::Call&, pc::RevoteArgs& rv) { rv.n_votes = ra::MAX_PAIRS + 1; }},
            {tables, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.first[2] = 4; }},
            {vfirst, [](world::World&, pc::Call&, pc::RevoteArgs& rv) { rv.vfirst = nullptr; }},
            {vfirst, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.vfirst[0] = 1; }},
            {vfirst, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.vfirst[1] = 4; }},
            {vfirst, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.vfirst[2] = 2; }},
            {spelt_off, [](world::World&, pc::Call&, pc::RevoteArgs& rv) { rv.spelt_off = nullptr; }},
            {spelt_off, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.spelt_off[0] = 1; }},
            {spelt_off, [](world::World& w, pc::Call&, pc::RevoteArgs&) { w.spelt_off[1] = 7000; }},
            {null_out, [](world::World&, pc::Call& c, pc::RevoteArgs&) { c.sites = nullptr; }},
            {null_out, [](world::World&, pc::Call&, pc::RevoteArgs& rv) { rv.lout = nullptr; }},
            {null_out, [](world::World&, pc::Call&, pc::RevoteArgs& rv) { rv.votes = nullptr; }},
            {null_out, [](world::World&, pc::Call&, pc::RevoteArgs& rv) { rv.vout = nullptr; }},
        };
        const int n_args = world::hold_check_args(fresh, ways, true);
        {
            bool nothing = false;
            world::World w = fresh();
            pc::RevoteArgs rv = w.revote(nullptr);
            rv.spelt_off = nullptr;                              // (no spelt output: its offsets are not looked at)
            pc::Call c = w.call(&rv);
            CHECK(!pc::check_args(c, nothing) && !nothing, "a re-vote without the spelt output");
            w.votes.clear();
            std::fill(w.vfirst.begin(), w.vfirst.end(), 0);
            rv = w.revote(nullptr);
            rv.votes = nullptr;
            rv.vout = nullptr;                                   // (no vote pairs: nothing to read them from or write them to)
            CHECK(!pc::check_args(c, nothing) && !nothing, "a re-vote without vote pairs");
            const pc::RevoteArgs none{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            const pc::Call empty{true, 0, nullptr, 100, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &none};
            CHECK(!pc::check_args(empty, nothing) && nothing, "a re-vote of nothing is in order and has nothing to run");
        }
        const bool all_met = met.served > 100 && met.arg > 50 && met.nomem >= 1 && met.from_votes > 10 && met.skipped > 5 && met.no_allele > 5 &&
                             met.short_slots > 20 && met.several > 10 && unasked > 5 && no_votes > 5;
        const bool all_dealt = dealt.loci > 200 && dealt.clamped > 20 && dealt.past_group_0 > 50 && dealt.untouched > 50;
        std::printf("call plan: %d calls, %s, %s, %s; check_args: %d cases\n", met.calls, all_met ? "every kind of locus and slot" : "a kind not met",
                    all_dealt ? "spelt bytes dealt past group 0 and clamped" : "few spelt bytes dealt", agree > 500 ? "the polish's share unchanged" : "few cuts agree",
                    n_args);
    }
    if (g_bad) {
        std::printf("revote_check: %d FAILED\n", g_bad);
        return 1;
    }
    std::printf("revote_check: all equal\n");
    return 0;
}
