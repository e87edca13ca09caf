// polish_call_world.h - what tools/polish_check.cpp and tools/revote_check.cpp share to hold the assembled plan of a call
// (vapor_amd/csrc/vapor_polish_call.h) to a direct statement: a call over a set that is only lengths, with loci that are designed
// or drawn, and `hold`, which states every record, offset and table of the plan a second time - per locus and per pair, in plain
// arithmetic, not through the helpers the plan is put together from (vapor_polish::lay_out alone is taken as given where a group's
// size is asked for: both programs hold it to its own statement).  No HIP, no device.
#pragma once

#include "vapor_polish_call.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

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

namespace world {

namespace pc = vapor_polish_call;
namespace ra = vapor_realign;
namespace tr = vapor_trace;
namespace pp = vapor_polish;
namespace vr = vapor_revote;

// A call and the set it runs over.  Sequence s has lens[s] symbols and starts at chunk 5 s + 3.
struct World {
    std::vector<int64_t> lens;
    std::vector<vapor_pair> pairs, votes;
    std::vector<int64_t> first{0}, col_off{0}, vfirst{0}, spelt_off{0};
    int32_t band = 100;
    // the outputs: check_args asks for them, nothing here writes them
    int32_t stats[1] = {0}, sites[1] = {0}, vout[1] = {0}, lout[1] = {0};
    uint8_t calls[1] = {0}, ins[1] = {0};

    int64_t n_loci() const { return (int64_t)first.size() - 1; }
    int32_t seq(int64_t len)
    {
        lens.push_back(len);
        return (int32_t)lens.size() - 1;
    }
    // a locus of `span` columns: its pairs and vote pairs as (seq1, seq2, off2), and the bytes of its spelt slot
    void locus(int64_t span, const std::vector<vapor_pair>& mine, const std::vector<vapor_pair>& voters, int64_t slot)
    {
        pairs.insert(pairs.end(), mine.begin(), mine.end());
        votes.insert(votes.end(), voters.begin(), voters.end());
        first.push_back((int64_t)pairs.size());
        vfirst.push_back((int64_t)votes.size());
        col_off.push_back(col_off.back() + span);
        spelt_off.push_back(spelt_off.back() + slot);
    }
    auto seqs() const
    {
        return pc::seqs((int32_t)lens.size(), [this](int32_t s) { return lens[(size_t)s]; }, [](int32_t s) { return (uint32_t)(5 * s + 3); });
    }
    pc::RevoteArgs revote(uint8_t* spelt)
    {
        return {(int64_t)votes.size(), votes.data(), vfirst.data(), vout, lout, spelt_off.data(), spelt};
    }
    pc::Call call(const pc::RevoteArgs* rv)
    {
        return {true, (int64_t)pairs.size(), pairs.data(), band, n_loci(), first.data(), col_off.data(), stats, calls, sites, ins, nullptr, rv};
    }
};

inline vapor_pair pair_of(int32_t seq1, int32_t seq2, int32_t off2) { return {seq1, seq2, off2, 0, 0}; }
inline int64_t cap_of(int64_t span) { return span + 64 * std::min<int64_t>(span, 256); }

// Loci drawn from `rng` behind whatever the world holds already: about one in five is refused or has no allele, the others are
// served.  big: reads of thousands of rows and alleles of up to 60 000 columns, so that the floor budget cuts several groups.
inline void draw(World& w, std::mt19937& rng, int64_t n_loci, bool big)
{
    const int32_t too_long = w.seq(VAPOR_MAX_SEQ_LEN + 1 + (int64_t)(rng() % 100));
    for (int64_t g = 0; g < n_loci; ++g) {
        const int64_t span = (int64_t)(rng() % (big ? (g % 3 ? 5000 : 60000) : 700));
        const int32_t allele = w.seq(span), other = w.seq(rng() % 2 ? span : span + 1);
        const int what = (int)(rng() % 16);
        std::vector<vapor_pair> mine, voters;
        const int n_mine = what == 0 ? 0 : (int)(rng() % 9), n_voters = (int)(rng() % 7);
        const auto one = [&](bool bad) {
            const int32_t read = w.seq((int64_t)(rng() % (big ? 7000 : 300)));
            vapor_pair p = pair_of(read, allele, (int32_t)(rng() % (span + 1)));
            if (bad) {
                const int how = (int)(rng() % 5);
                if (how == 0) p.seq1 = -1;
                if (how == 1) p.seq2 = 1 << 30;
                if (how == 2) p.off2 = (int32_t)span + 1;
                if (how == 3) p.off2 = -1;
                if (how == 4) p.seq1 = too_long;
            }
            return p;
        };
        for (int k = 0; k < n_mine; ++k) mine.push_back(one(what == 1 && (k == n_mine / 2 || rng() % 4 == 0)));
        if (what == 2 && n_mine > 1) mine[1 + rng() % (n_mine - 1)].seq2 = other;              // (two seq2 in one locus)
        for (int k = 0; k < n_voters; ++k) {
            voters.push_back(one(rng() % 5 == 0));
            if (rng() % 6 == 0) voters.back().seq2 = other;                                     // (not the allele; where span + 1 long, no allele either)
        }
        const int64_t cols = what == 3 ? span + 1 : span;                                       // (columns that are not the allele's length)
        const int64_t cap = cap_of(cols), slot = rng() % 4 == 0 ? (cap ? cap - 1 : 0) : rng() % 4 == 1 ? 0 : cap + (int64_t)(rng() % 3);
        w.locus(cols, mine, voters, slot);
    }
}

// the status of a pair or vote pair by itself
inline int own_status(const World& w, const vapor_pair& p)
{
    const int64_t n = (int64_t)w.lens.size();
    if (p.seq1 < 0 || p.seq1 >= n || p.seq2 < 0 || p.seq2 >= n) return VAPOR_E_ARG;
    if (w.lens[(size_t)p.seq1] > VAPOR_MAX_SEQ_LEN || w.lens[(size_t)p.seq2] > VAPOR_MAX_SEQ_LEN) return VAPOR_E_ARG;
    if (p.off2 < 0 || p.off2 > w.lens[(size_t)p.seq2]) return VAPOR_E_ARG;
    return VAPOR_OK;
}
// dwords of the trace rows of a pair that runs
inline int64_t rows_words(const World& w, const vapor_pair& p)
{
    const int64_t n = w.lens[(size_t)p.seq1], m = w.lens[(size_t)p.seq2] - p.off2;
    const int64_t slots = (2 * (int64_t)w.band + 1 + 63) / 64;                                  // of a lane; the compiled widths: 1 2 3 5 9 17
    return std::min(n, m + w.band + 1) * 64 * (slots > 9 ? 2 : 1);
}

// what `hold` met, for the programs' summary lines
struct Met {
    int calls = 0, served = 0, arg = 0, nomem = 0, no_pairs = 0, several = 0, from_votes = 0, skipped = 0, no_allele = 0, short_slots = 0, kept_own = 0;
};

// The plan of `w`'s call held to the direct statement.  rv: the call's re-vote arguments, null for the polish alone.
inline void hold(World& w, const pc::RevoteArgs* rv, int64_t budget, const pc::Plan& p, Met& met, const char* name)
{
    const int64_t n_loci = w.n_loci(), np = (int64_t)w.pairs.size(), nv = rv ? (int64_t)w.votes.size() : 0;
    const int64_t limit = std::max<int64_t>(budget, (int64_t)64 << 20) / 4;
    CHECK((int64_t)p.recs.size() == np && (int64_t)p.off.size() == np && (int64_t)p.pair_locus.size() == np && (int64_t)p.loci.size() == n_loci,
          "%s: the polish's tables", name);
    CHECK((int64_t)p.vloci.size() == (rv ? n_loci : 0) && (int64_t)p.vrecs.size() == nv, "%s: the re-vote's tables", name);
    if (g_bad) return;
    // the loci and their pairs
    std::vector<int64_t> words((size_t)n_loci, 0), run_cap((size_t)n_loci, 1), extra((size_t)n_loci, 0);
    for (int64_t g = 0; g < n_loci; ++g) {
        const int64_t a = w.first[(size_t)g], b = w.first[(size_t)g + 1], span = w.col_off[(size_t)g + 1] - w.col_off[(size_t)g];
        int status = VAPOR_OK;
        for (int64_t t = a; t < b; ++t)
            if (own_status(w, w.pairs[(size_t)t]) || w.pairs[(size_t)t].seq2 != w.pairs[(size_t)a].seq2) status = VAPOR_E_ARG;
        if (!status && b > a && w.lens[(size_t)w.pairs[(size_t)a].seq2] != span) status = VAPOR_E_ARG;
        int64_t rows = 0;
        for (int64_t t = a; t < b && !status; ++t) rows += rows_words(w, w.pairs[(size_t)t]);
        if (!status && rows > limit) status = VAPOR_E_NOMEM;
        words[(size_t)g] = status ? 0 : rows;
        const pp::PLocus& lc = p.loci[(size_t)g];
        CHECK(lc.status == status && lc.n_pairs == (status ? 0 : b - a) && lc.len == span, "%s: locus %lld is %d with %d pairs of %d columns", name,
              (long long)g, lc.status, lc.n_pairs, lc.len);
        CHECK(lc.word2 == (!status && b > a ? (uint64_t)(5 * w.pairs[(size_t)a].seq2 + 3) * 4 : 0), "%s: the allele of locus %lld", name, (long long)g);
        for (int64_t t = a; t < b; ++t) {
            const vapor_pair& q = w.pairs[(size_t)t];
            const ra::RPair& r = p.recs[(size_t)t];
            const int own = own_status(w, q);
            CHECK(r.status == (own ? own : status), "%s: pair %lld of locus %lld carries %d", name, (long long)t, (long long)g, r.status);
            met.kept_own += own && status && own != status;
            if (own) CHECK(r.n == 0 && r.m == 0 && r.word1 == 0 && r.word2 == 0, "%s: a refused pair is empty", name);
            else {
                CHECK(r.word1 == (uint64_t)(5 * q.seq1 + 3) * 4 && r.word2 == (uint64_t)(5 * q.seq2 + 3) * 4 && r.n == w.lens[(size_t)q.seq1] &&
                          r.m == w.lens[(size_t)q.seq2] - q.off2 && r.off2 == q.off2,
                      "%s: the record of pair %lld", name, (long long)t);
                if (!status) run_cap[(size_t)g] = std::max<int64_t>(run_cap[(size_t)g], w.lens[(size_t)q.seq1] + w.lens[(size_t)q.seq2] - q.off2 + 1);
            }
        }
        met.served += !status && b > a;
        met.no_pairs += !status && b == a;
        met.arg += status == VAPOR_E_ARG;
        met.nomem += status == VAPOR_E_NOMEM;
        if (!rv) continue;
        // the re-vote: the allele, the locus record and the vote pairs
        const int64_t va = w.vfirst[(size_t)g], vb = w.vfirst[(size_t)g + 1];
        int64_t allele = -1;
        int vstatus = status;
        if (!status && b > a) allele = w.pairs[(size_t)a].seq2;
        if (!status && b == a) {
            for (int64_t t = va; t < vb && allele < 0; ++t) {
                const vapor_pair& q = w.votes[(size_t)t];
                if (!own_status(w, q) && w.lens[(size_t)q.seq2] == span) allele = q.seq2;
                else ++met.skipped;
            }
            if (allele < 0) vstatus = VAPOR_E_ARG;
            met.from_votes += allele >= 0;
            met.no_allele += allele < 0;
        }
        const vr::VLocus& vl = p.vloci[(size_t)g];
        const int64_t slot = w.spelt_off[(size_t)g + 1] - w.spelt_off[(size_t)g];
        CHECK(vl.status == vstatus, "%s: the re-vote of locus %lld is %d, not %d", name, (long long)g, vl.status, vstatus);
        if (vstatus) CHECK(vl.word2 == 0 && vl.cap == 0 && vl.short_slot == 0, "%s: a locus that is not spelt is empty", name);
        else {
            CHECK(vl.word2 == (uint64_t)(5 * allele + 3) * 4 && vl.cap == cap_of(span), "%s: allele and cap of locus %lld", name, (long long)g);
            CHECK(vl.short_slot == (rv->spelt && slot < cap_of(span)), "%s: the slot of locus %lld", name, (long long)g);
            met.short_slots += vl.short_slot;
            const int64_t chunks = (cap_of(span) + 31) / 32;
            extra[(size_t)g] = (span + 1 + 3) / 4 * 4 + 8 * chunks + 4 * chunks;
        }
        for (int64_t t = va; t < vb; ++t) {
            const vapor_pair& q = w.votes[(size_t)t];
            const vr::VPair& r = p.vrecs[(size_t)t];
            const int want = vstatus ? vstatus : own_status(w, q) ? VAPOR_E_ARG : q.seq2 != allele ? VAPOR_E_ARG : VAPOR_OK;
            CHECK(r.status == want, "%s: vote pair %lld of locus %lld carries %d, not %d", name, (long long)t, (long long)g, r.status, want);
            if (!want) CHECK(r.word1 == (uint64_t)(5 * q.seq1 + 3) * 4 && r.n == w.lens[(size_t)q.seq1] && r.off2 == q.off2, "%s: the record of vote pair %lld", name, (long long)t);
        }
    }
    // the groups: consecutive whole loci, inside the budget unless one locus, greedy; everything relative to the group
    int64_t next = 0, most = 0, host = 0;
    CHECK(p.stage_base.size() == (rv ? p.groups.size() : 0) && p.stage_words.size() == p.stage_base.size() && p.stage_host.size() == p.stage_base.size(),
          "%s: the stagings' bookkeeping", name);
    for (size_t k = 0; k < p.groups.size() && !g_bad; ++k) {
        const pp::Group& gr = p.groups[k];
        CHECK(gr.locus0 == next && gr.locus1 > gr.locus0 && gr.locus1 <= n_loci, "%s: group %zu is consecutive and not empty", name, k);
        if (g_bad) return;
        next = gr.locus1;
        pp::Group want{};
        want.locus0 = gr.locus0;
        want.locus1 = gr.locus1;
        want.pair0 = w.first[(size_t)gr.locus0];
        want.pair1 = w.first[(size_t)gr.locus1];
        want.cols = w.col_off[(size_t)gr.locus1] - w.col_off[(size_t)gr.locus0];
        for (int64_t g = gr.locus0; g < gr.locus1; ++g) {
            want.trace_words += words[(size_t)g];
            want.cap_runs = std::max(want.cap_runs, run_cap[(size_t)g]);
            want.extra += extra[(size_t)g];
        }
        pp::lay_out(want);
        CHECK(gr.pair0 == want.pair0 && gr.pair1 == want.pair1 && gr.cols == want.cols && gr.trace_words == want.trace_words && gr.cap_runs == want.cap_runs &&
                  gr.extra == want.extra && gr.words == want.words && gr.extra_off == want.extra_off,
              "%s: what group %zu holds", name, k);
        CHECK(gr.words <= limit || gr.locus1 - gr.locus0 == 1, "%s: group %zu holds %lld words", name, k, (long long)gr.words);
        if (gr.locus1 < n_loci) {                              // (greedy: the next locus did not fit)
            pp::Group more = want;
            more.locus1 += 1;
            more.pair1 = w.first[(size_t)more.locus1];
            more.cols = w.col_off[(size_t)more.locus1] - w.col_off[(size_t)more.locus0];
            more.trace_words += words[(size_t)gr.locus1];
            more.cap_runs = std::max(more.cap_runs, run_cap[(size_t)gr.locus1]);
            more.extra += extra[(size_t)gr.locus1];
            pp::lay_out(more);
            CHECK(more.words > limit, "%s: group %zu closed early", name, k);
        }
        most = std::max(most, gr.words);
        uint64_t used = 0;
        for (int64_t g = gr.locus0; g < gr.locus1; ++g) {
            CHECK(p.loci[(size_t)g].col0 == w.col_off[(size_t)g] - w.col_off[(size_t)gr.locus0], "%s: col0 of locus %lld", name, (long long)g);
            for (int64_t t = w.first[(size_t)g]; t < w.first[(size_t)g + 1]; ++t) {
                CHECK(p.pair_locus[(size_t)t] == g - gr.locus0, "%s: the locus of pair %lld", name, (long long)t);
                CHECK(p.off[(size_t)t] == used && (t != gr.pair0 || used == 0), "%s: the rows of pair %lld start at %llu, not %llu", name, (long long)t,
                      (unsigned long long)p.off[(size_t)t], (unsigned long long)used);
                if (!p.recs[(size_t)t].status) used += (uint64_t)rows_words(w, w.pairs[(size_t)t]);
            }
            for (int64_t t = rv ? w.vfirst[(size_t)g] : 0; rv && t < w.vfirst[(size_t)g + 1]; ++t)
                CHECK(p.vrecs[(size_t)t].locus == g - gr.locus0, "%s: the locus of vote pair %lld", name, (long long)t);
        }
        CHECK((int64_t)used == gr.trace_words, "%s: the rows of group %zu", name, k);
        if (!rv) continue;
        // the group's pieces: the own[] tables of its spelt loci, their stagings as one stretch, their planes
        int64_t owns = 0, stagings = 0;
        for (int64_t g = gr.locus0; g < gr.locus1; ++g)
            if (extra[(size_t)g]) {
                const int64_t span = w.col_off[(size_t)g + 1] - w.col_off[(size_t)g];
                owns += (span + 1 + 3) / 4 * 4;
                stagings += 8 * ((cap_of(span) + 31) / 32);
            }
        CHECK(p.stage_base[k] == gr.extra_off + owns && p.stage_words[k] == stagings, "%s: the stagings of group %zu", name, k);
        CHECK(p.stage_host[k] == host, "%s: group %zu's stagings land at %lld, not %lld", name, k, (long long)p.stage_host[k], (long long)host);
        if (rv->spelt) host += stagings;
        int64_t own_at = gr.extra_off, stage_at = gr.extra_off + owns, plane_at = gr.extra_off + owns + stagings;
        for (int64_t g = gr.locus0; g < gr.locus1; ++g) {
            const vr::VLocus& vl = p.vloci[(size_t)g];
            CHECK(vl.own_off == own_at && vl.stage_off == stage_at && vl.plane_off == plane_at, "%s: the pieces of locus %lld", name, (long long)g);
            if (!extra[(size_t)g]) continue;
            const int64_t span = w.col_off[(size_t)g + 1] - w.col_off[(size_t)g], chunks = (cap_of(span) + 31) / 32;
            own_at += (span + 1 + 3) / 4 * 4;
            stage_at += 8 * chunks;
            plane_at += 4 * chunks;
        }
        CHECK(plane_at == gr.words, "%s: the pieces of group %zu fill what was charged", name, k);
    }
    CHECK(next == n_loci && p.most == most && p.staged_words == host, "%s: every locus in a group; the largest group; the host copy", name);
    met.several += p.groups.size() > 1;
    // the image: every table where the order puts it, on 8 bytes, equal to the vector it was filled from; the size is the sum
    const uint8_t* im = p.image.data();
    size_t at = 0;
    const auto table = [&](const auto& t, const auto& from, size_t n, const char* what) {
        using T = typename std::decay_t<decltype(from)>::value_type;
        CHECK(t.off == at && t.off % 8 == 0 && t.n == n && from.size() == n, "%s: %s stand at %zu, not %zu", name, what, t.off, at);
        at += (sizeof(T) * n + 7) / 8 * 8;
        CHECK(at <= p.image.size() && (n == 0 || memcmp(t.in(im), from.data(), sizeof(T) * n) == 0), "%s: %s read back", name, what);
    };
    table(p.t_recs, p.recs, (size_t)np, "the pair records");
    table(p.t_off, p.off, (size_t)np, "the workspace offsets");
    table(p.t_loci, p.loci, (size_t)n_loci, "the loci");
    table(p.t_pair_locus, p.pair_locus, (size_t)np, "the pairs' loci");
    table(p.t_vloci, p.vloci, rv ? (size_t)n_loci : 0, "the vote loci");
    table(p.t_vrecs, p.vrecs, (size_t)nv, "the vote pairs");
    CHECK(p.image.size() == at && at == 32 * (size_t)np + 8 * (size_t)np + 40 * (size_t)n_loci + ((size_t)np * 4 + 7) / 8 * 8 + (rv ? 48 * (size_t)n_loci : 0) + 24 * (size_t)nv,
          "%s: the image is %zu bytes", name, p.image.size());
    ++met.calls;
}

// check_args held to its order.  `ways` are the ways a call in order (made by `fresh`) goes wrong, each with the message it earns,
// listed in the order the checks are made: every one alone gets its code and message, and of two at once the earlier wins.
struct Way {
    const char* msg;
    void (*spoil)(World&, pc::Call&, pc::RevoteArgs&);
};
template <typename Fresh>
inline int hold_check_args(Fresh fresh, const std::vector<Way>& ways, bool revote)
{
    int n = 0;
    uint8_t spelt[1];
    const size_t none = ways.size();
    for (size_t i = 0; i <= none; ++i)
        for (size_t j = i; j <= none; ++j) {               // (j == i: the way alone; both == none: the call in order)
            if ((i == none) != (j == none)) continue;
            World w = fresh();
            pc::RevoteArgs rv = w.revote(spelt);
            pc::Call c = w.call(revote ? &rv : nullptr);
            if (j != none) ways[j].spoil(w, c, rv);
            if (i != j) ways[i].spoil(w, c, rv);
            bool nothing = true;
            const pc::Refusal no = pc::check_args(c, nothing);
            if (i == none) CHECK(!no && no.code == VAPOR_OK && !nothing, "a call in order is refused: %s", no.msg ? no.msg : "");
            else
                CHECK(no && no.code == VAPOR_E_ARG && !nothing && std::string(no.msg ? no.msg : "") == ways[i].msg, "ways %zu and %zu: \"%s\", not \"%s\"",
                      i, j, no.msg ? no.msg : "", ways[i].msg);
            ++n;
        }
    return n;
}

}  // namespace world
