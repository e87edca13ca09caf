// vapor_trace_plan.h - the host arithmetic of vapor_realign_trace, without HIP: the codes of a trace's runs, the
// layout of a pair's head, how many dwords a lane packs its 2-bit moves into, what a pair's rows take in the workspace, how a call's
// pairs fall into consecutive groups under the budget, and the preference key that picks the end slot from the last row walked.
// realign_trace_kernel and traceback_kernel (vapor_realign_trace.h) read the same constants and the same functions;
// tools/trace_check.cpp holds them to direct statements on the host under the sanitizers.
#pragma once

#include "vapor_realign_plan.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace vapor_trace {

// a run is len << 2 | op
enum Op : uint32_t { OP_EQ = 0, OP_X = 1, OP_I = 2, OP_D = 3 };
VAPOR_RA_HD inline uint32_t run_word(uint32_t len, uint32_t op) { return len << 2 | op; }

// head[8 t ..] of pair t
constexpr int HEAD = 8;
enum HeadField { H_D = 0, H_STATUS = 1, H_I_END = 2, H_J_END = 3, H_N_RUNS = 4 };

// dwords a lane of S slots packs its moves into (two bits a slot): one up to S = 16, two at 17
VAPOR_RA_HD constexpr int words_of(int S) { return (2 * S + 31) / 32; }
// ... of a row of a pair (64 lanes, lane-contiguous), and the bytes of a pair's rows in the workspace
VAPOR_RA_HD constexpr int64_t row_words(int S) { return (int64_t)vapor_realign::LANES * words_of(S); }
VAPOR_RA_HD inline int64_t pair_words(int rows, int S) { return (int64_t)rows * row_words(S); }
inline int64_t pair_bytes(int rows, int S) { return 4 * pair_words(rows, S); }

// the budget of a call's workspace: the default, and the floor that always holds the largest pair the entry accepts
// (65 535 rows at S = 17: 33.5 MB); a lower value is raised to the floor
constexpr int64_t BUDGET_DEFAULT = (int64_t)512 << 20;
constexpr int64_t BUDGET_FLOOR = (int64_t)64 << 20;
inline int64_t budget_of(int64_t asked) { return asked < BUDGET_FLOOR ? BUDGET_FLOOR : asked; }
static_assert(4 * (int64_t)VAPOR_MAX_SEQ_LEN * 64 * words_of(vapor_realign::MAX_SLOTS) <= BUDGET_FLOOR, "the floor holds one pair");

// Consecutive groups of pairs whose workspaces fit the budget: first[g] .. first[g + 1] are the pairs of group g, off[t] the first
// dword of pair t inside its group's workspace; a pair with a status has no rows.  Returns the dwords of the largest group.
inline int64_t plan_groups(const vapor_realign::RPair* recs, int64_t n_pairs, int band, int S, int64_t budget, std::vector<int64_t>& first,
                           std::vector<uint64_t>& off)
{
    const int64_t cap = budget_of(budget) / 4;
    first.assign(1, 0);
    off.assign((size_t)n_pairs, 0);
    int64_t used = 0, most = 0;
    for (int64_t t = 0; t < n_pairs; ++t) {
        const vapor_realign::RPair& r = recs[t];
        const int64_t need = r.status ? 0 : pair_words(vapor_realign::rows_walked(r.n, r.m, band), S);
        if (used + need > cap && used > 0) {
            first.push_back(t);
            used = 0;
        }
        off[(size_t)t] = (uint64_t)used;
        used += need;
        if (used > most) most = used;
    }
    first.push_back(n_pairs);
    return most;
}

// The end slot.  A slot c of the last row walked is cell (n, n + c - B) of the last row while c <= c* = m - n + B
// (the corner's slot), and stands for cell (m - c + B, m) of the last column behind it.  The rule wants the largest i, then the
// largest j: c*, c* - 1, .., 0, then c* + 1, .., 2B.  The key is smaller for the slot preferred; NO_SLOT for a slot that is no
// cell (outside the row, left of the allele's start, or a diagonal that meets the last column above row 0).
constexpr int NO_SLOT = 1 << 30;
VAPOR_RA_HD inline int end_key(int c, int n, int m, int B, int rows)
{
    if (c < 0 || c >= vapor_realign::row_slots(B) || rows + c - B < 0 || c > m + B) return NO_SLOT;
    const int cs = rows == n ? m - n + B : -1;
    return c <= cs ? cs - c : c;
}
// ... and the end cell of the slot chosen
VAPOR_RA_HD inline void end_cell(int c, int n, int m, int B, int rows, int& i_end, int& j_end)
{
    if (rows == n && c <= m - n + B) { i_end = n; j_end = n + c - B; }
    else { i_end = m - c + B; j_end = m; }
}

// the slot of row i that is cell (i, j), the lane that owns it and where its two bits stand
VAPOR_RA_HD inline int slot_of(int i, int j, int B) { return j - i + B; }

inline bool cap_ok(int64_t cap_runs) { return cap_runs >= 1; }

}  // namespace vapor_trace
