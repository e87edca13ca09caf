// planner_check.cpp - the host planner (vapor_amd/csrc/vapor_planner.h: share_layout, plan_layout, clean_order) on a CPU, against
// direct statements of its rules: the statuses, every pair scored once, the launches and their tasks, the cheapest partition by
// enumeration, the remap tables against the texts the segment lists spell, the clean order.  The inputs come from fixed seeds:
// windows, reads and inserted stretches of 50 to 400 symbols, one to four derived alleles per window (deletions, inversions, tandem
// duplications, insertions, upper-cased twins, random cuts), 1 to 40 pairs a case; the structures the planner declines to share
// are built on purpose.  Nothing here is compared with recorded output of the planner: the tuning constants are free to move.
// Built and run by tests/test_planner_cpu.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc tools/planner_check.cpp
#include "seq_spell.h"
#include "vapor_planner.h"
#include "vapor_seqset_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>

using namespace vapor;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (case %ld)\n", g_case); exit(1); } } while (0)

static std::mt19937_64 rng(20250917);
static long g_case = 0;
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }      // lo .. hi
static bool one_in(int n) { return rng() % (uint64_t)n == 0; }

// ---- texts (what segments spell: tools/seq_spell.h) ----
using seq_spell::revcomp;
using seq_spell::upper;
// `lower`, `odd`: one symbol in that many is lower-case / an N or an X (0: none)
static std::string dna(int n, int lower, int odd)
{
    std::string s((size_t)n, 'A');
    for (char& c : s) {
        c = "ACGT"[rng() & 3];
        if (lower && one_in(lower)) c = (char)(c + 32);
        if (odd && one_in(odd)) c = one_in(2) ? 'N' : 'X';
    }
    return s;
}

// A sequence set as vapor_seqset_create_derived lays it out on the host (vapor_seqset_plan.h's Layout, from the lengths and the
// segments), with the texts its sequences spell.
struct World {
    std::vector<std::string> text;             // per sequence, the hidden ones behind the caller's ("" for the too-long literal)
    std::vector<SeqDesc> h;
    int32_t n = 0, n_lit = 0;
    std::vector<std::vector<HSeg>> derived, hidden;
    std::vector<uint8_t> dflags;
    std::vector<ShareGroup> groups;
    std::vector<int32_t> group_of, slot_of;
    std::vector<int32_t> reads;                // literals meant as first sequences
    std::vector<std::vector<int32_t>> loci;    // per window: the window and its alleles
    std::vector<int32_t> stuffing;             // LONG_HIDDEN: literals as long as the window, all of them inserted into every allele
    int32_t too_long = -1;                     // a literal longer than VAPOR_MAX_SEQ_LEN (a descriptor only), -1: none
    SetView view() const { return SetView{h, n, n_lit, derived, groups, group_of, slot_of}; }
};

// the symbols a text holds outside upper-case ACGT and outside invert_base's alphabet: the counts the kernels would send back
static void count(SeqDesc& d, const std::string& t)
{
    d.n_exc = d.n_invalid = 0;
    for (char c : t) {
        if (!strchr("ACGT", c)) ++d.n_exc;
        if (!strchr("ACGTNacgtn", c)) ++d.n_invalid;
    }
}

static SeqDesc describe(const std::string& t, uint32_t flags)
{
    SeqDesc d;
    memset(&d, 0, sizeof d);
    d.len = (int32_t)t.size();
    d.flags = flags;
    count(d, t);
    return d;
}

static std::string spell(const World& w, const std::vector<HSeg>& segs, bool up)
{
    std::string s, why;
    CHECK(seq_spell::spell(w.text, w.n_lit, segs, up, s, why), "%s", why.c_str());
    return s;
}

static void add_seg(std::vector<HSeg>& a, int32_t parent, int off, int len, bool rc)
{
    if (len <= 0 || a.size() >= VAPOR_MAX_SEGMENTS) return;
    const int32_t dst = a.empty() ? 0 : a.back().dst + a.back().len;
    a.push_back(HSeg{parent, off, len, dst, rc});
}

enum Kind { RANDOM, FOUR_MEMBERS, THIRD_COPY, MANY_INTERVALS, LONG_HIDDEN };
enum Allele { DEL, INV, DUP, INS, TWIN, CUTS, TRIPLE, COMB, STUFFED };

// an allele of window `win` (n symbols); `ins` is the literal that inserted stretches come from
static std::vector<HSeg> allele(const World& w, int32_t win, int32_t ins, Allele what)
{
    const int n = w.h[(size_t)win].len, ni = w.h[(size_t)ins].len;
    std::vector<HSeg> a;
    int x = rnd(1, n - 2), y = rnd(1, n - 2);
    if (x > y) std::swap(x, y);
    ++y;                                                                             // 1 <= x < y <= n - 1
    switch (what) {
    case DEL: add_seg(a, win, 0, x, false); add_seg(a, win, y, n - y, false); break;
    case INV: add_seg(a, win, 0, x, false); add_seg(a, win, x, y - x, true); add_seg(a, win, y, n - y, false); break;
    case DUP: add_seg(a, win, 0, y, false); add_seg(a, win, x, n - x, false); break;                 // [x, y) twice
    case INS: { const int c = rnd(0, ni - 1), l = rnd(1, ni - c);
                add_seg(a, win, 0, x, false); add_seg(a, ins, c, l, one_in(3)); add_seg(a, win, x, n - x, false); break; }
    case TWIN: add_seg(a, win, 0, n, false); break;
    case CUTS:
        for (int s = rnd(1, 6); s > 0; --s) {
            const int32_t par = one_in(4) ? ins : win;
            const int np = w.h[(size_t)par].len, c = rnd(0, np - 1);
            add_seg(a, par, c, rnd(1, np - c), one_in(3));
        }
        break;
    case TRIPLE: add_seg(a, win, 0, y, false); add_seg(a, win, x, y - x, false); add_seg(a, win, x, n - x, false); break;   // [x, y) three times
    case COMB:                                                                        // twelve slices with three symbols missing between them
        for (int s = 0; s < 12; ++s) add_seg(a, win, s * (n / 12), n / 12 - 3, false);
        break;
    case STUFFED:                                                                     // five literals inserted, none longer than the window
        add_seg(a, win, 0, x, false);
        for (int32_t lit : w.stuffing) add_seg(a, lit, 0, w.h[(size_t)lit].len, false);
        add_seg(a, win, x, n - x, false);
        break;
    }
    return a;
}

static World make_world(Kind kind, bool shared_join)
{
    World w;
    auto literal = [&](const std::string& t, uint32_t flags) {
        w.text.push_back(flags & VAPOR_SEQ_UPPER ? upper(t) : t);
        w.h.push_back(describe(w.text.back(), flags));
        return (int32_t)w.h.size() - 1;
    };
    const int n_win = kind == RANDOM ? rnd(1, 2) : 1;
    std::vector<int32_t> wins;
    for (int i = 0; i < n_win; ++i) {
        const bool soft = kind == RANDOM && one_in(3);
        int len = rnd(50, 400);
        if (kind == THIRD_COPY || kind == MANY_INTERVALS) len = rnd(200, 400);       // (room for stretches that hold a k-mer)
        if (kind == LONG_HIDDEN) len = rnd(300, 400);
        wins.push_back(literal(dna(len, soft ? 8 : 0, soft && one_in(2) ? 60 : 0), soft && one_in(4) ? VAPOR_SEQ_UPPER : 0u));
    }
    const int32_t ins = literal(dna(rnd(50, 400), one_in(4) ? 10 : 0, 0), 0);
    if (kind == LONG_HIDDEN)
        for (int s = 0; s < 5; ++s) w.stuffing.push_back(literal(dna(w.h[(size_t)wins[0]].len, 0, 0), 0));
    for (int r = rnd(1, 6); r > 0; --r) {
        const bool tiny = one_in(12);
        w.reads.push_back(literal(dna(tiny ? rnd(5, 39) : rnd(50, 400), one_in(4) ? 12 : 0, one_in(5) ? 40 : 0), one_in(8) ? VAPOR_SEQ_UPPER : 0u));
    }
    if (kind == RANDOM && one_in(6)) {
        SeqDesc d;
        memset(&d, 0, sizeof d);
        d.len = VAPOR_MAX_SEQ_LEN + rnd(1, 5000);
        w.h.push_back(d);
        w.text.push_back("");
        w.too_long = (int32_t)w.h.size() - 1;
    }
    w.n_lit = (int32_t)w.h.size();
    for (int32_t win : wins) {
        std::vector<int32_t> locus{win};
        std::vector<Allele> kinds;
        switch (kind) {
        case RANDOM: for (int a = rnd(1, 4); a > 0; --a) kinds.push_back(one_in(12) ? TRIPLE : (Allele)rnd(DEL, CUTS)); break;
        case FOUR_MEMBERS: kinds = {DEL, INV, DUP, DEL}; break;
        case THIRD_COPY: kinds = {DEL, TRIPLE}; break;
        case MANY_INTERVALS: kinds = {COMB, COMB, COMB}; break;
        case LONG_HIDDEN: kinds = {STUFFED, STUFFED, STUFFED}; break;
        }
        const bool win_upper = w.h[(size_t)win].flags & VAPOR_SEQ_UPPER;
        for (Allele what : kinds) {
            w.derived.push_back(allele(w, win, ins, what));
            // (a derived sequence that is not upper-cased cannot be cut from a literal that was: the library refuses such a set)
            w.dflags.push_back(win_upper || (kind == RANDOM && one_in(3)) ? VAPOR_SEQ_UPPER : 0);
            locus.push_back(w.n_lit + (int32_t)w.derived.size() - 1);
        }
        w.loci.push_back(locus);
    }
    if (kind == MANY_INTERVALS)                                                       // (three combs cut at different places)
        for (size_t d = 0; d < w.derived.size(); ++d)
            for (HSeg& x : w.derived[d]) x.off += (int32_t)d;
    w.n = w.n_lit + (int32_t)w.derived.size();
    // the descriptors of the derived and the hidden sequences and the share groups: as the library lays the set out, from the
    // lengths and the segments (vapor_seqset_plan.h); the counts are the texts'
    std::vector<int32_t> len, seg_first(1, 0);
    std::vector<uint8_t> flags;
    std::vector<vapor_segment> segs;
    for (const SeqDesc& d : w.h) { len.push_back(d.len); flags.push_back((uint8_t)d.flags); }
    for (const auto& v : w.derived) {
        for (const HSeg& x : v) segs.push_back(vapor_segment{x.parent, x.off, x.len, x.rc ? VAPOR_SEG_REVCOMP : 0u});
        seg_first.push_back((int32_t)segs.size());
    }
    vapor_seqset_plan::Layout L;
    const vapor_seqset_plan::Refusal no = L.build(vapor_seqset_plan::Call{vapor_seqset_plan::DERIVED, true, w.n_lit, nullptr, nullptr, nullptr, len.data(), flags.data(), nullptr,
                                                                          nullptr, (int32_t)w.derived.size(), seg_first.data(), segs.data(), w.dflags.data()}, shared_join);
    CHECK(!no && L.n == w.n && L.derived.size() == w.derived.size(), "the set is refused: %s", no.msg ? no.msg : "");
    for (size_t i = 0; i < (size_t)w.n_lit; ++i) { L.h[i].n_exc = w.h[i].n_exc; L.h[i].n_invalid = w.h[i].n_invalid; }
    w.h = L.h;
    w.hidden = L.hidden;
    w.groups = L.groups;
    w.group_of = L.group_of;
    w.slot_of = L.slot_of;
    for (size_t i = (size_t)w.n_lit; i < w.h.size(); ++i) {
        w.text.push_back(spell(w, L.segments(i - (size_t)w.n_lit), w.h[i].flags & VAPOR_SEQ_UPPER));
        count(w.h[i], w.text.back());
    }
    return w;
}

static const int KS[4] = {10, 20, 30, 40};

// 1 to 40 pairs: reads against windows and their alleles, now and then a pair the planner must refuse
static std::vector<vapor_pair> make_pairs(const World& w, Kind kind, int most)
{
    std::vector<vapor_pair> pairs;
    const int want = rnd(1, most);
    while ((int)pairs.size() < want) {
        const int32_t read = w.reads[(size_t)rnd(0, (int)w.reads.size() - 1)];
        const auto& locus = w.loci[(size_t)rnd(0, (int)w.loci.size() - 1)];
        const int k = KS[kind == RANDOM ? rnd(0, 3) : rnd(0, 1)];
        for (int32_t target : locus) {
            if (kind == RANDOM && one_in(5)) continue;
            vapor_pair p;
            p.seq1 = read; p.seq2 = target; p.k = k; p.flags = (uint32_t)rnd(0, 7);
            p.off2 = one_in(6) ? rnd(0, w.h[(size_t)target].len - 1) : 0;
            if (kind == RANDOM && one_in(25)) {
                switch (rnd(0, 5)) {
                case 0: p.seq1 = one_in(2) ? -1 : w.n + rnd(0, 2); break;            // (a hidden sequence is no sequence of the caller's)
                case 1: p.seq2 = one_in(2) ? -1 - rnd(0, 3) : w.n + rnd(0, 2); break;
                case 2: p.off2 = -rnd(1, 100); break;
                case 3: p.k = one_in(2) ? rnd(-5, 9) : rnd(41, 64); break;
                case 4: p.k = rnd(11, 39); if (p.k % 10 == 0) ++p.k; break;
                case 5: if (w.too_long >= 0) (one_in(2) ? p.seq1 : p.seq2) = w.too_long; break;
                }
            }
            if ((int)pairs.size() < want) pairs.push_back(p);
        }
    }
    for (size_t i = pairs.size(); i > 1; --i) if (one_in(3)) std::swap(pairs[i - 1], pairs[(size_t)rnd(0, (int)i - 1)]);
    return pairs;
}

struct Tally {
    long cases = 0, pairs = 0, refused = 0, keyerror = 0;                             // check 1
    long joined = 0, served = 0, shares = 0;                                          // check 2
    long launches = 0, tasks = 0;                                                     // check 3
    long small_launches = 0, partitions = 0;                                          // check 4
    long tables = 0, kmers = 0, flipped = 0, twice = 0;                               // check 5
    long orders = 0;                                                                  // check 6
    long declined[5] = {0, 0, 0, 0, 0};
};
static Tally T;

// ---- check 1 ----
static int status_rule(const World& w, const vapor_pair& a)
{
    if (a.seq1 < 0 || a.seq1 >= w.n || a.seq2 < 0 || a.seq2 >= w.n) return VAPOR_E_ARG;
    if (a.off2 < 0) return VAPOR_E_ARG;
    if (a.k != 10 && a.k != 20 && a.k != 30 && a.k != 40) return VAPOR_E_ARG;
    const SeqDesc &s1 = w.h[(size_t)a.seq1], &s2 = w.h[(size_t)a.seq2];
    if (s1.len > VAPOR_MAX_SEQ_LEN || s2.len > VAPOR_MAX_SEQ_LEN) return VAPOR_E_ARG;
    if (s1.n_invalid > 0 && s1.len >= a.k) return VAPOR_E_KEYERROR;
    return 0;
}
static void check_statuses(const World& w, const std::vector<vapor_pair>& pairs, const PlanLayout& L)
{
    CHECK(L.status.size() == pairs.size(), "%zu statuses", L.status.size());
    for (size_t i = 0; i < pairs.size(); ++i) {
        const int want = status_rule(w, pairs[i]);
        CHECK(L.status[i] == want, "pair %zu (%d, %d, off2 %d, k %d): status %d, the rule says %d", i, pairs[i].seq1, pairs[i].seq2, pairs[i].off2,
              pairs[i].k, L.status[i], want);
        T.refused += want == VAPOR_E_ARG;
        T.keyerror += want == VAPOR_E_KEYERROR;
    }
    T.pairs += (long)pairs.size();
}

// ---- check 2 ----
static bool is_served(const PlanLayout& L, size_t i) { return !L.serve.empty() && L.serve[i].dpair >= 0; }

static void check_scored_once(const World& w, const std::vector<vapor_pair>& pairs, const PlanLayout& L, bool shared_join)
{
    const size_t n_pairs = pairs.size();
    CHECK(L.hp.size() == n_pairs + L.shares.size(), "%zu pairs in hp", L.hp.size());
    CHECK(L.serve.empty() || L.serve.size() == n_pairs, "%zu serve records", L.serve.size());
    std::vector<int> times(L.hp.size(), 0);
    for (int32_t x : L.task_pairs) {
        CHECK(x >= 0 && (size_t)x < L.hp.size(), "pair %d in task_pairs", x);
        ++times[(size_t)x];
    }
    long served = 0;
    for (size_t i = 0; i < n_pairs; ++i) {
        const vapor_pair& a = pairs[i];
        const bool scored = L.status[i] == 0 && w.h[(size_t)a.seq1].len >= a.k && w.h[(size_t)a.seq2].len >= a.k;
        if (!scored) { CHECK(times[i] == 0 && !is_served(L, i), "pair %zu has nothing to join and is joined", i); continue; }
        if (!is_served(L, i)) { CHECK(times[i] == 1, "pair %zu is in task_pairs %d times", i, times[i]); ++T.joined; continue; }
        ++served;
        const DServe& sv = L.serve[i];
        CHECK(times[i] == 0, "pair %zu is served and joined", i);
        CHECK((size_t)sv.dpair >= n_pairs && (size_t)sv.dpair < L.hp.size(), "pair %zu is served by pair %d", i, sv.dpair);
        const DShare& sh = L.shares[(size_t)sv.dpair - n_pairs];
        CHECK(sh.dpair == sv.dpair, "share %zu runs pair %d", (size_t)sv.dpair - n_pairs, sh.dpair);
        CHECK(sv.slot >= 0 && sv.slot < 4 && sh.target[sv.slot] == (int32_t)i, "pair %zu is not target %d of its share", i, sv.slot);
    }
    for (size_t x = n_pairs; x < L.hp.size(); ++x) CHECK(times[x] == 1, "hidden pair %zu is in task_pairs %d times", x, times[x]);
    CHECK(L.n_served == served, "n_served %ld, %ld pairs are served", (long)L.n_served, served);
    for (size_t s = 0; s < L.shares.size(); ++s) {
        const DShare& sh = L.shares[s];
        CHECK(sh.dpair == (int32_t)(n_pairs + s), "share %zu runs pair %d", s, sh.dpair);
        const DPair& hd = L.hp[(size_t)sh.dpair];
        int targets = 0, counting = 0, group = -1;
        for (int t = 0; t < 4; ++t) {
            if (sh.target[t] < 0) continue;
            CHECK((size_t)sh.target[t] < n_pairs && L.serve[(size_t)sh.target[t]].dpair == sh.dpair, "target %d of share %zu", t, s);
            const DPair& d = L.hp[(size_t)sh.target[t]];
            const int g = w.group_of[(size_t)d.seq2];
            CHECK(d.seq1 == hd.seq1 && d.k == hd.k && g >= 0 && (group < 0 || g == group), "share %zu: target %d is of another read, group or k", s, t);
            CHECK(w.slot_of[(size_t)d.seq2] == t && w.groups[(size_t)g].t_seq == hd.seq2, "share %zu: target %d is not slot %d of the group", s, t, t);
            group = g;
            ++targets;
            counting += L.serve[(size_t)sh.target[t]].pad == 1;
        }
        CHECK(targets >= 2 && counting == 1, "share %zu: %d targets, %d count an overflow", s, targets, counting);
    }
    CHECK(shared_join || (served == 0 && L.shares.empty()), "shared joins are off and %ld pairs are served", served);
    T.served += served;
    T.shares += (long)L.shares.size();
}

// ---- checks 3 and 4 ----
struct Mode { int bps, exc; };
static Mode mode_rule(const SeqDesc& read, const SeqDesc& allele)
{
    if (read.n_exc > 0 && allele.n_exc > 0) return Mode{4, 0};
    if (allele.n_exc > 0) return Mode{2, 1};
    if (read.n_exc > 0) return Mode{2, 2};
    return Mode{2, 0};
}

// cost of pairs [a, b) of a launch as one task
static int64_t range_cost(const World& w, const PlanParams& P, const PlanLayout& L, const Launch& la, size_t a, size_t b)
{
    int64_t cost = 0;
    for (size_t t = a; t < b; ++t) {
        const DPair& d = L.hp[(size_t)L.task_pairs[t]];
        const int64_t len1 = w.h[(size_t)d.seq1].len, len2 = w.h[(size_t)d.seq2].len;
        const int64_t tile = la.bps == 4 ? P.tile4 : P.tile2;
        const int64_t tiles = std::max<int64_t>(1, (len2 - la.k + 1 + tile - 1) / tile);
        cost += len1 * tiles + 256;
        if (t == a || d.seq2 != L.hp[(size_t)L.task_pairs[t - 1]].seq2) cost += VAPOR_BUILD_COST_X8 * len2 / 8;
    }
    return cost;
}

static void check_tasks(const World& w, const PlanParams& P, const PlanLayout& L)
{
    size_t next_pair = 0, next_task = 0;
    std::set<std::vector<int>> seen;
    for (const Launch& la : L.launches) {
        CHECK(la.n_tasks >= 1 && (size_t)la.task_begin == next_task && next_task + (size_t)la.n_tasks <= L.tasks.size(), "launch of tasks %d + %d", la.task_begin, la.n_tasks);
        CHECK(seen.insert({la.bps, la.exc, la.k}).second, "two launches of bps %d, exc %d, k %d", la.bps, la.exc, la.k);
        const size_t first = next_pair;
        int64_t dearest = 0;
        for (int t = 0; t < la.n_tasks; ++t) {
            const DTask& tk = L.tasks[next_task++];
            CHECK((size_t)tk.first == next_pair, "task at pair %d, the one before ends at %zu", tk.first, next_pair);
            CHECK(tk.n_reads >= 1 && tk.n_reads <= P.reads_per_task && next_pair + (size_t)tk.n_reads <= L.task_pairs.size(), "task of %d pairs", tk.n_reads);
            CHECK(tk.k == la.k && tk.seq2 == L.hp[(size_t)L.task_pairs[next_pair]].seq2, "task of k %d and allele %d", tk.k, tk.seq2);
            dearest = std::max(dearest, range_cost(w, P, L, la, next_pair, next_pair + (size_t)tk.n_reads));
            next_pair += (size_t)tk.n_reads;
        }
        const size_t n = next_pair - first;
        for (size_t t = first; t < next_pair; ++t) {
            const DPair& d = L.hp[(size_t)L.task_pairs[t]];
            const Mode m = mode_rule(w.h[(size_t)d.seq1], w.h[(size_t)d.seq2]);
            CHECK(d.k == la.k && m.bps == la.bps && m.exc == la.exc, "pair %d (k %d, bps %d, exc %d) in the launch of k %d, bps %d, exc %d", L.task_pairs[t], d.k,
                  m.bps, m.exc, la.k, la.bps, la.exc);
            CHECK(t == first || L.hp[(size_t)L.task_pairs[t - 1]].seq2 <= d.seq2, "pair %d: the alleles of a launch are not sorted", L.task_pairs[t]);
        }
        // join_tasks tasks, or whole rounds of them when reads_per_task asks for more, never more than the pairs
        int64_t want = std::min<int64_t>((int64_t)n, P.join_tasks);
        const int64_t need = ((int64_t)n + P.reads_per_task - 1) / P.reads_per_task;
        if (need > want) want = std::min<int64_t>((int64_t)n, (need + want - 1) / want * want);
        CHECK(la.n_tasks <= want, "%d tasks for %zu pairs, join_tasks %d, reads_per_task %d", la.n_tasks, n, P.join_tasks, P.reads_per_task);
        ++T.launches;
        T.tasks += la.n_tasks;
        // check 4: every contiguous partition (bit t of `cuts`: a task begins at pair t + 1)
        if (n > 10 || P.join_tasks > 4 || P.reads_per_task > 5) continue;
        int64_t best = -1;
        for (unsigned cuts = 0; cuts < (1u << (n - 1)); ++cuts) {
            int64_t worst = 0, ranges = 0;
            bool fits = true;
            for (size_t a = 0; a < n;) {
                size_t b = a + 1;
                while (b < n && !((cuts >> (b - 1)) & 1u)) ++b;
                fits = fits && (int64_t)(b - a) <= P.reads_per_task;
                worst = std::max(worst, range_cost(w, P, L, la, first + a, first + b));
                ++ranges;
                a = b;
            }
            if (!fits || ranges > want) continue;
            if (best < 0 || worst < best) best = worst;
            ++T.partitions;
        }
        CHECK(best == dearest, "the dearest task costs %ld, the best partition's %ld (%zu pairs, join_tasks %d, reads_per_task %d)", (long)dearest, (long)best, n,
              P.join_tasks, P.reads_per_task);
        ++T.small_launches;
    }
    CHECK(next_pair == L.task_pairs.size() && next_task == L.tasks.size(), "%zu pairs and %zu tasks in launches", next_pair, next_task);
}

// ---- check 5 ----
static void check_tables(const World& w, const std::vector<vapor_pair>& pairs, const PlanLayout& L)
{
    std::set<int32_t> done;
    for (const DShare& sh : L.shares) {
        CHECK(sh.n_iv >= 1 && sh.n_iv <= REMAP_MAX_IV, "%d intervals", sh.n_iv);
        CHECK(sh.iv_first >= 0 && (size_t)sh.iv_first + (size_t)sh.n_iv + 1 + (size_t)sh.n_iv * REMAP_OPS <= L.tables.size(), "table at %d of %zu words", sh.iv_first,
              L.tables.size());
        for (int t = 0; t < 4; ++t)
            if (sh.target[t] >= 0) {
                const DServe& sv = L.serve[(size_t)sh.target[t]];
                CHECK(sv.iv_first == sh.iv_first && sv.n_iv == sh.n_iv, "pair %d reads the table at %d + %d, its share the one at %d + %d", sh.target[t], sv.iv_first,
                      sv.n_iv, sh.iv_first, sh.n_iv);
            }
        const int32_t* B = &L.tables[(size_t)sh.iv_first];
        const int32_t* ops = B + sh.n_iv + 1;
        const DPair& hd = L.hp[(size_t)sh.dpair];
        const int k = hd.k;
        const std::string& shared = w.text[(size_t)hd.seq2];
        const int32_t gi = w.group_of[(size_t)L.hp[(size_t)sh.target[sh.target[0] >= 0 ? 0 : sh.target[1] >= 0 ? 1 : 2]].seq2];
        const ShareGroup& g = w.groups[(size_t)gi];
        // what the four slots of the group spell (slot 0 is the window as the group reads it, in the set or not)
        std::string slot_text[4];
        bool have[4] = {true, false, false, false};
        slot_text[0] = g.upper ? upper(w.text[(size_t)g.parent]) : w.text[(size_t)g.parent];
        CHECK(g.identity < 0 || w.text[(size_t)g.identity] == slot_text[0], "sequence %d is not the window of its group", g.identity);
        for (size_t m = 0; m < g.members.size(); ++m) { slot_text[m + 1] = w.text[(size_t)g.members[m]]; have[m + 1] = true; }
        std::vector<char> image[4];
        for (int t = 0; t < 4; ++t) {
            CHECK(sh.target[t] < 0 || (have[t] && pairs[(size_t)sh.target[t]].seq2 == (t == 0 ? g.identity : g.members[(size_t)t - 1])), "target %d is not slot %d", t, t);
            image[t].assign(slot_text[t].size(), 0);
        }
        if (!done.insert(sh.iv_first).second) continue;                              // (a table per group and k: spelled out once)
        CHECK(B[0] == 0, "the boundaries begin at %d", B[0]);
        for (int t = 0; t < sh.n_iv; ++t) CHECK(B[t] < B[t + 1], "boundary %d: %d, then %d", t, B[t], B[t + 1]);
        CHECK(B[sh.n_iv] <= (int32_t)shared.size() - k + 1, "the last boundary %d, the shared sequence has %zu symbols", B[sh.n_iv], shared.size());
        int iv = 0;
        for (int e = 0; e + k <= (int)shared.size() && e < B[sh.n_iv]; ++e) {
            while (e >= B[iv + 1]) ++iv;
            const std::string kmer = shared.substr((size_t)e, (size_t)k);
            for (int t = 0; t < 4; ++t)
                for (int c = 0; c < 2; ++c) {
                    const int32_t op = ops[(size_t)iv * REMAP_OPS + (size_t)t * 2 + (size_t)c];
                    if (!(op & 1)) continue;
                    const bool flip = op & 2;
                    const int delta = op >> 2, j = flip ? delta - e : e + delta;
                    CHECK(have[t], "an op for slot %d, which the group has not", t);
                    CHECK(j >= 0 && j + k <= (int)slot_text[t].size(), "e %d goes to %d of slot %d (%zu symbols, k %d)", e, j, t, slot_text[t].size(), k);
                    const std::string there = slot_text[t].substr((size_t)j, (size_t)k);
                    CHECK(kmer == (flip ? revcomp(there) : there), "e %d, slot %d, j %d%s: %s in the shared sequence, %s in the target", e, t, j, flip ? " flipped" : "",
                          kmer.c_str(), there.c_str());
                    T.twice += c == 1;
                    image[t][(size_t)j] = 1;
                    ++T.kmers;
                    T.flipped += flip;
                }
        }
        for (int t = 0; t < 4; ++t)
            for (int j = 0; have[t] && j + k <= (int)slot_text[t].size(); ++j)
                CHECK(image[t][(size_t)j], "k-mer %d of slot %d (k %d) is the image of nothing in the shared sequence", j, t, k);
        ++T.tables;
    }
}

// ---- check 6 ----
static void check_clean_order(const std::vector<vapor_pair>& pairs, const PlanLayout& L)
{
    const size_t n = pairs.size();
    const std::vector<int32_t> ord = clean_order(L, (int64_t)n);
    CHECK(ord.size() == n, "%zu pairs in the order", ord.size());
    std::vector<char> seen(n, 0);
    bool refused = false;
    for (size_t x = 0; x < n; ++x) {
        const int32_t i = ord[x];
        CHECK(i >= 0 && (size_t)i < n && !seen[(size_t)i], "pair %d at place %zu", i, x);
        seen[(size_t)i] = 1;
        CHECK(clean_cost(L, i) >= 0 && (L.status[(size_t)i] == 0 || clean_cost(L, i) == 0), "pair %d costs %ld", i, (long)clean_cost(L, i));
        // (every pair here has symbols on both sides, so one that is scored costs something and the refused ones come last)
        CHECK(!refused || L.status[(size_t)i] != 0, "pair %d (status 0) behind a refused pair", i);
        refused = L.status[(size_t)i] != 0;
        if (x == 0) continue;
        const int64_t before = clean_cost(L, ord[x - 1]), here = clean_cost(L, i);
        CHECK(before > here || (before == here && ord[x - 1] < i), "pairs %d (cost %ld) and %d (cost %ld) at places %zu and %zu", ord[x - 1], (long)before, i,
              (long)here, x - 1, x);
    }
    ++T.orders;
}

// the structures the planner declines: they are simply not shared
static void check_declined(const World& w, Kind kind, const std::vector<vapor_pair>& pairs, const PlanLayout& L)
{
    for (size_t i = 0; i < pairs.size(); ++i) {
        const bool served = is_served(L, i);
        switch (kind) {
        case RANDOM: break;
        case FOUR_MEMBERS:
            if (pairs[i].seq2 == w.n - 1) { CHECK(!served && w.group_of[(size_t)pairs[i].seq2] < 0, "a fourth member is shared"); ++T.declined[kind]; }
            break;
        case THIRD_COPY:
            // (the stretch must hold a k-mer to lie in a map three times)
            if (w.derived[1][1].len >= pairs[i].k) { CHECK(!served, "a third copy of a stretch is shared"); ++T.declined[kind]; }
            break;
        case MANY_INTERVALS:
            if (w.derived[0][0].len >= pairs[i].k) { CHECK(!served, "more than %d intervals are shared", REMAP_MAX_IV); ++T.declined[kind]; }
            break;
        case LONG_HIDDEN:
            CHECK(!served && w.hidden.empty(), "a hidden sequence longer than twice its window and 4096 symbols is shared");
            ++T.declined[kind];
            break;
        }
    }
}

static void one_case(Kind kind)
{
    ++g_case;
    PlanParams P;
    const bool small = one_in(2);
    P.join_tasks = small ? rnd(1, 4) : rnd(1, 64);
    P.reads_per_task = small ? rnd(1, 5) : rnd(1, MAX_READS_PER_TASK);
    P.max_pair_cap = one_in(4) ? rnd(64, 2000) : (int64_t)1 << 28;
    P.shared_join = kind != RANDOM || !one_in(5);
    static const int tiles[4] = {64, 300, 2048, 24576};
    P.tile2 = tiles[rnd(0, 3)];
    P.tile4 = std::max(32, P.tile2 * 7 / 8);
    if (kind != RANDOM) P.tile2 = P.tile4 = 24576;                                   // (sharing always pays: only the structure declines)
    const World w = make_world(kind, P.shared_join);
    const std::vector<vapor_pair> pairs = make_pairs(w, kind, small ? 14 : 40);
    const PlanLayout L = plan_layout(P, w.view(), (int64_t)pairs.size(), pairs.data());
    check_statuses(w, pairs, L);
    check_scored_once(w, pairs, L, P.shared_join);
    check_tasks(w, P, L);
    check_tables(w, pairs, L);
    check_clean_order(pairs, L);
    check_declined(w, kind, pairs, L);
    for (size_t i = 0; i < pairs.size(); ++i)
        if (L.status[i] == 0) {
            const int64_t n1 = w.h[(size_t)pairs[i].seq1].len, n2 = w.h[(size_t)pairs[i].seq2].len - pairs[i].off2;
            CHECK(L.hp[i].cap == (uint32_t)std::min<int64_t>(std::min(n1, n2) + ((n1 * n2) >> 17) + 1024, P.max_pair_cap), "pair %zu has %u record slots", i, L.hp[i].cap);
        }
    ++T.cases;
}

int main()
{
    for (int c = 0; c < 2600; ++c) one_case(RANDOM);
    for (int c = 0; c < 100; ++c) one_case(FOUR_MEMBERS);
    for (int c = 0; c < 100; ++c) one_case(THIRD_COPY);
    for (int c = 0; c < 100; ++c) one_case(MANY_INTERVALS);
    for (int c = 0; c < 100; ++c) one_case(LONG_HIDDEN);
    CHECK(T.refused > 100 && T.keyerror > 100, "%ld pairs refused, %ld with a key error", T.refused, T.keyerror);
    CHECK(T.served > 1000 && T.joined > 1000, "%ld pairs served, %ld joined on their own", T.served, T.joined);
    CHECK(T.small_launches > 500, "%ld launches enumerated", T.small_launches);
    CHECK(T.tables > 500 && T.flipped > 1000 && T.twice > 1000, "%ld tables, %ld flipped k-mers, %ld k-mers that lie twice in their target", T.tables, T.flipped, T.twice);
    for (int kind = FOUR_MEMBERS; kind <= LONG_HIDDEN; ++kind) CHECK(T.declined[kind] > 50, "structure %d was declined %ld times", kind, T.declined[kind]);
    printf("statuses: %ld cases equal the rule (%ld pairs, %ld refused, %ld with a key error)\n", T.cases, T.pairs, T.refused, T.keyerror);
    printf("scored once: %ld cases (%ld pairs joined on their own, %ld served by %ld shared joins)\n", T.cases, T.joined, T.served, T.shares);
    printf("tasks: %ld cases (%ld launches, %ld tasks)\n", T.cases, T.launches, T.tasks);
    printf("partition: %ld launches as cheap as the best of their partitions (%ld enumerated)\n", T.small_launches, T.partitions);
    printf("tables: %ld cases (%ld tables, %ld k-mers equal their targets', %ld of them flipped, %ld a second copy)\n", T.cases, T.tables, T.kmers, T.flipped, T.twice);
    printf("declined: %ld fourth members, %ld third copies, %ld of more than %d intervals, %ld long hidden sequences are not shared\n", T.declined[FOUR_MEMBERS],
           T.declined[THIRD_COPY], T.declined[MANY_INTERVALS], REMAP_MAX_IV, T.declined[LONG_HIDDEN]);
    printf("clean order: %ld cases\n", T.orders);
    printf("planner_check: all equal\n");
    return 0;
}
