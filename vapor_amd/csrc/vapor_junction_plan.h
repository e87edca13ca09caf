// vapor_junction_plan.h - the host arithmetic of vapor_realign_junction, without HIP: which pairs are refused, the
// record a pair travels as, the tasks of a call (a pair in each direction), what a pair's two row tables take, where they stand in
// the call's one workspace, whether that fits the trace budget, and the layout of a pair's answer and of a row as the caller sees
// it.  junction_rows_kernel and junction_pick_kernel (vapor_junction.h) read the same constants and records;
// tools/junction_check.cpp holds the functions to direct statements on the host under the sanitizers.
#pragma once

#include "vapor_trace_plan.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace vapor_junction {

// out[8 t ..] of pair t
constexpr int OUT = 8;
enum OutField { O_STATUS = 0, O_COST = 1, O_I = 2, O_J1 = 3, O_J2 = 4, O_FF = 5, O_FR = 6 };

// a row of a pair, in the workspace and in the caller's `rows`: four int32, each pass's pair indexed by that pass's own row
constexpr int ROW = 4;
enum RowField { R_F_FWD = 0, R_JF_FWD = 1, R_F_BWD = 2, R_JF_BWD = 3 };

// the row's reduction key is vapor_realign's, of D (at most ns + nl) and the slot; NO_CELL lies above every key
using vapor_realign::KEY_SHIFT;
using vapor_realign::key_c;
using vapor_realign::key_d;
using vapor_realign::row_key;
constexpr int NO_CELL = 0x7FFFFFFF;

// A pair as the kernels take it (40 B): the sequences' first words in the 4-bit plane, ns = len(seq1) <= nl = len(seq2), and the
// first row of its tables in the workspace.
struct JPair {
    uint64_t word1, word2;     // first x4 word of seq1 / of seq2 (chunk0 * 4)
    int32_t ns, nl;
    int32_t status;            // 0, or VAPOR_E_ARG: no row of such a pair is walked, its record is zero behind the status
    int32_t pad;
    int64_t row0;              // its ns + 1 rows are row0 .. row0 + ns of the workspace
};
static_assert(sizeof(JPair) == 40, "JPair layout");

// the tasks of a call: task 2 t is pair t forward, task 2 t + 1 pair t backward (symbol k of either sequence is its symbol
// len - 1 - k); one wavefront a task
VAPOR_RA_HD inline int64_t tasks_of(int64_t n_pairs) { return 2 * n_pairs; }
VAPOR_RA_HD inline int64_t task_pair(int64_t task) { return task >> 1; }
VAPOR_RA_HD inline bool task_backward(int64_t task) { return (task & 1) != 0; }
// the position in its sequence of symbol k of a pass
VAPOR_RA_HD inline int pass_pos(int len, bool backward, int k) { return backward ? len - 1 - k : k; }

// rows and bytes of a pair's two tables
VAPOR_RA_HD inline int64_t pair_rows(int ns) { return (int64_t)ns + 1; }
inline int64_t pair_bytes(int ns) { return 4 * ROW * pair_rows(ns); }

// the status of a pair over a set of n_seqs sequences: vapor_realign_batch's refusals, an off2 that is not 0 and a seq1 longer
// than seq2
template <typename LenOf>
inline int pair_status(const vapor_pair& a, int32_t n_seqs, LenOf len_of)
{
    const int st = vapor_realign::pair_status(a, n_seqs, len_of);
    if (st) return st;
    if (a.off2 != 0 || len_of(a.seq1) > len_of(a.seq2)) return VAPOR_E_ARG;
    return VAPOR_OK;
}

template <typename LenOf, typename ChunkOf>
inline JPair pair_record(const vapor_pair& a, int32_t n_seqs, LenOf len_of, ChunkOf chunk_of)
{
    JPair r{0, 0, 0, 0, pair_status(a, n_seqs, len_of), 0, 0};
    if (r.status) return r;
    r.word1 = (uint64_t)chunk_of(a.seq1) * 4u;
    r.word2 = (uint64_t)chunk_of(a.seq2) * 4u;
    r.ns = (int32_t)len_of(a.seq1);
    r.nl = (int32_t)len_of(a.seq2);
    return r;
}

// The workspace: the served pairs' tables one behind the other, in pair order; sets row0 of every record and returns the rows of
// the call (a refused pair has none and row0 = 0).
inline int64_t lay_out(JPair* recs, int64_t n_pairs)
{
    int64_t rows = 0;
    for (int64_t t = 0; t < n_pairs; ++t) {
        recs[t].row0 = recs[t].status ? 0 : rows;
        if (!recs[t].status) rows += pair_rows(recs[t].ns);
    }
    return rows;
}
// ... which must fit the trace budget (vapor_trace::budget_of: never below its floor), or the call is refused with VAPOR_E_NOMEM
inline bool fits(int64_t rows, int64_t budget) { return 4 * ROW * rows <= vapor_trace::budget_of(budget); }

// the caller's row table (`rows` not NULL): n_pairs + 1 ascending int64 from 0
inline bool row_off_ok(int64_t n_pairs, const int64_t* row_off)
{
    if (!row_off || row_off[0] != 0) return false;
    for (int64_t t = 0; t < n_pairs; ++t)
        if (row_off[t + 1] < row_off[t]) return false;
    return true;
}
// ... in which a served pair's slot must hold its ns + 1 rows: else the pair is refused with VAPOR_E_ARG
inline bool slot_holds(const JPair& r, const int64_t* row_off, int64_t t) { return r.status != 0 || row_off[t + 1] - row_off[t] >= pair_rows(r.ns); }

// the pick of a split row: the jump of row i is l[j1 : j2), valid iff j2 >= j1
VAPOR_RA_HD inline int split_j2(int nl, int jf_bwd) { return nl - jf_bwd; }
VAPOR_RA_HD inline bool split_valid(int j1, int j2) { return j2 >= j1; }

// launch geometry: vapor_realign's four wavefronts a workgroup, a task (rows) or a pair (pick) each
inline int64_t rows_grid(int64_t n_pairs) { return vapor_realign::grid_of(tasks_of(n_pairs)); }
inline int64_t pick_grid(int64_t n_pairs) { return vapor_realign::grid_of(n_pairs); }

}  // namespace vapor_junction
