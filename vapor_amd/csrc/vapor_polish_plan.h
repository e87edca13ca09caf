// vapor_polish_plan.h - the host arithmetic of vapor_realign_polish, without HIP: the rule's constants and the call
// codes, the layout of a column's counters, which calls and which loci are refused, how a call's loci fall into consecutive groups
// under the trace budget and where every piece of a group stands in its one device buffer.  The four kernels of vapor_polish.h read
// the same constants and records; tools/polish_check.cpp holds the functions to direct statements on the host under the sanitizers.
#pragma once

#include "vapor_trace_plan.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace vapor_polish {

constexpr int MIN_COV = 3;                 // a column, or a boundary, is judged from this many pairs on
constexpr int RMAX = 64;                   // inserted bases kept per site: one lane each
constexpr int MAX_SITES = 256;             // insertion sites kept per locus, in column order

// the call byte of a column: 0 .. 3 a substituted base, KEEP, DELETE; SITE_BIT when a kept insertion site lies before the column
enum Call : uint8_t { CALL_KEEP = 4, CALL_DELETE = 5, SITE_BIT = 8 };

// a column's counters, eight uint32: reads' bases by code & 3, other read symbols, deletions, pairs that cover the column and its
// predecessor, insertions before the column
constexpr int COUNTERS = 8;
enum Counter { C_A = 0, C_C = 1, C_G = 2, C_T = 3, C_O = 4, C_DL = 5, C_BCOV = 6, C_INS = 7 };

// a locus's statistics, eight int32
constexpr int STATS = 8;
enum Stat { S_STATUS = 0, S_PAIRS = 1, S_PCOV = 2, S_PSUB = 3, S_PDEL = 4, S_SITES = 5, S_PINS = 6, S_DROPPED = 7 };

// A locus as the kernels take it (40 B).  col0 is relative to the locus's group.
struct PLocus {
    uint64_t word2;            // first x4 word of the allele (of its pairs' seq2)
    int64_t col0;              // first column of the locus among the group's columns
    int32_t len;               // columns
    int32_t n_pairs;
    int32_t status;            // 0, VAPOR_E_ARG or VAPOR_E_NOMEM: no pair of such a locus is walked
    int32_t pad[3];
};
static_assert(sizeof(PLocus) == 40, "PLocus layout");

// words of the per-locus tables in a group's buffer: statistics, sites (column, bases), inserted text, inserted-base counters
constexpr int64_t SITE_WORDS = 2 * MAX_SITES;
constexpr int64_t INS_WORDS = (int64_t)MAX_SITES * RMAX / 4;
constexpr int64_t INSB_WORDS = (int64_t)MAX_SITES * RMAX * 4;
constexpr int64_t LOCUS_WORDS = STATS + SITE_WORDS + INS_WORDS + INSB_WORDS;
// words of a column: its counters, the slot of its site (0: none, else slot + 1) and its call byte (rounded up per group)
constexpr int64_t COLUMN_WORDS = COUNTERS + 1;

// the run slot of a pair always holds a path: n + m steps at the most, and one word to spare as vapor_realign_trace's callers ask
inline int64_t run_cap(const vapor_realign::RPair& r) { return r.status ? 1 : (int64_t)r.n + r.m + 1; }

// call-level checks of the two offset tables: ascending from 0, `first` ending at n_pairs, no locus wider than a sequence can be
inline bool tables_ok(int64_t n_pairs, int64_t n_loci, const int64_t* first, const int64_t* col_off)
{
    if (n_loci < 0 || !first || !col_off || first[0] != 0 || col_off[0] != 0) return false;
    for (int64_t g = 0; g < n_loci; ++g) {
        if (first[g + 1] < first[g] || col_off[g + 1] < col_off[g]) return false;
        if (col_off[g + 1] - col_off[g] > VAPOR_MAX_SEQ_LEN) return false;
    }
    return first[n_loci] == n_pairs;
}

// The status of locus g and the trace words of its pairs: VAPOR_E_ARG when a pair is refused, when two pairs name different seq2
// or when the columns are not the allele's length (len2_of(t): the length of pair t's seq2); VAPOR_E_NOMEM when the rows alone
// do not fit the budget.  A locus without pairs is served: every column is KEEP.
template <typename Seq2Of, typename Len2Of>
inline int locus_status(const vapor_realign::RPair* recs, int64_t a, int64_t b, int64_t span, int band, int S, int64_t budget, Seq2Of seq2_of,
                        Len2Of len2_of, int64_t& trace_words)
{
    trace_words = 0;
    for (int64_t t = a; t < b; ++t) {
        if (recs[t].status) return VAPOR_E_ARG;
        if (seq2_of(t) != seq2_of(a)) return VAPOR_E_ARG;
    }
    if (b > a && len2_of(a) != span) return VAPOR_E_ARG;
    for (int64_t t = a; t < b; ++t) trace_words += vapor_trace::pair_words(vapor_realign::rows_walked(recs[t].n, recs[t].m, band), S);
    if (trace_words > vapor_trace::budget_of(budget) / 4) {
        trace_words = 0;
        return VAPOR_E_NOMEM;
    }
    return VAPOR_OK;
}

// A group: consecutive whole loci, and where its pieces stand in the group's buffer, in dwords.  The trace rows come first (the
// pairs' offsets are relative to it), then the run slots - traceback_kernel's slots are one size a launch, so every pair of the
// group gets the group's largest n + m + 1 -, then everything that starts at zero (`zero_off` .. `words`): the columns' counters,
// their site slots and call bytes, and the loci's tables, and behind those `extra` dwords that a caller adds for its own pieces
// (vapor_realign_revote's, vapor_revote_plan.h; none for the polish alone).
struct Group {
    int64_t locus0, locus1;    // loci of the group
    int64_t pair0, pair1;      // their pairs
    int64_t cols;              // their columns
    int64_t cap_runs;          // words of a run slot
    int64_t trace_words;
    int64_t runs_off, zero_off, counts_off, slot_off, calls_off, stats_off, sites_off, ins_off, insb_off, words;
    int64_t extra, extra_off;  // the caller's own dwords (a multiple of four) and where they start
};

inline int64_t calls_words(int64_t cols) { return (cols + 3) / 4; }
// every piece starts on 16 bytes: the kernels read a column's counters and a position's four bases as one load each
inline int64_t align4(int64_t words) { return (words + 3) / 4 * 4; }

inline void lay_out(Group& g)
{
    const int64_t nl = g.locus1 - g.locus0, np = g.pair1 - g.pair0;
    g.runs_off = g.trace_words;
    g.zero_off = align4(g.runs_off + np * g.cap_runs);
    g.counts_off = g.zero_off;
    g.slot_off = g.counts_off + COUNTERS * g.cols;
    g.calls_off = align4(g.slot_off + g.cols);
    g.stats_off = align4(g.calls_off + calls_words(g.cols));
    g.sites_off = g.stats_off + STATS * nl;
    g.ins_off = g.sites_off + SITE_WORDS * nl;
    g.insb_off = g.ins_off + INS_WORDS * nl;
    g.extra_off = g.insb_off + INSB_WORDS * nl;
    g.words = g.extra_off + g.extra;
}

// The groups of a call.  trace_words[g] (0 for a refused locus) and cap[g] (the largest run_cap of the locus's pairs, 1 without
// one that is served) describe locus g; first / col_off are the call's tables.  A locus joins the open group while the group's
// buffer stays inside the budget; a group always takes at least one locus, so a single locus whose tables go past the budget
// (its rows alone do not: locus_status) still runs.  ws_off[t]: the first trace dword of pair t inside its group (the caller
// fills it from the pairs' own words).  extra[g] (may be null: none): the dwords locus g adds to its group's buffer beside the
// polish's own, charged to the budget like them.  Returns the dwords of the largest group.
inline int64_t plan_groups(int64_t n_loci, const int64_t* first, const int64_t* col_off, const int64_t* trace_words, const int64_t* cap,
                           int64_t budget, std::vector<Group>& groups, const int64_t* extra = nullptr)
{
    const int64_t limit = vapor_trace::budget_of(budget) / 4;
    groups.clear();
    int64_t most = 0, g = 0;
    while (g < n_loci) {
        Group cur{};
        cur.locus0 = g;
        cur.pair0 = first[g];
        int64_t h = g;
        while (h < n_loci) {
            Group next = cur;
            next.locus1 = h + 1;
            next.pair1 = first[h + 1];
            next.cols = col_off[h + 1] - col_off[g];
            next.trace_words = cur.trace_words + trace_words[h];
            next.cap_runs = cap[h] > cur.cap_runs ? cap[h] : cur.cap_runs;
            next.extra = cur.extra + (extra ? extra[h] : 0);
            lay_out(next);
            if (next.words > limit && h > g) break;
            cur = next;
            ++h;
        }
        groups.push_back(cur);
        if (cur.words > most) most = cur.words;
        g = h;
    }
    return most;
}

}  // namespace vapor_polish
