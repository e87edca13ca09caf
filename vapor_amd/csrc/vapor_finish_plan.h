// vapor_finish_plan.h - the host side of the per-read / per-locus finishing and of the breakpoint grid,
// without HIP: vapor_plan_set_reads, vapor_plan_set_grid, vapor_plan_run_loci, vapor_plan_run_grid, vapor_grid_pick and
// vapor_plan_run_loci_async.  The widths of the records; what a read table and a grid are refused for, in order; the two upload
// images (reads | locus_first, and first_locus | score_off | winner_idx (| read_first)) with each table's place stated once;
// the sizes of the blocks behind them; which path a run takes, when the host's statuses go up again and when a run is repeated.
// Everything finish_kernel and grid_pick_kernel index with is checked here.  tools/finish_plan_check.cpp holds it to direct
// statements on the host under the sanitizers; oracle/cpu_twin.cpp takes the per-read check from here.  The functions in
// vapor_hip.hip are allocations, copies, launches, event records and synchronisations.
#pragma once

#include "vapor_hip.h"
#include "vapor_image.h"

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace vapor {
namespace finish_plan {

using vapor_image::Carve;
using vapor_image::Refusal;
using vapor_image::Table;

// ------------------------------------------------------------------------------------------
// widths
// ------------------------------------------------------------------------------------------
constexpr int LOCUS_DOUBLES = VAPOR_LOCUS_STRIDE;          // a locus record
constexpr int GROUP_DOUBLES = 2 * LOCUS_DOUBLES;           // a group record: the winner's locus record, then candidate 0's
constexpr size_t GT_ENTRIES = (size_t)2 * VAPOR_GT_TABLE_N * VAPOR_GT_TABLE_N;     // doubles of the genotype table
constexpr int STATS_WORDS = VAPOR_STATS_STRIDE;            // a pair's statistics record

// ------------------------------------------------------------------------------------------
// the read table (vapor_plan_set_reads)
// ------------------------------------------------------------------------------------------
// What a read is refused for, the first in this order: its locus below the one before it (`prev`; -1 before the first read) or
// not below n_loci; a pair index of a scorer it uses outside the plan; its scorer kind.  (Reads of locus -1 at the front pass:
// they raise locus_first[0] and so belong to no locus.)
inline Refusal read_refusal(const vapor_read& x, int32_t prev, int64_t n_loci, int64_t n_pairs)
{
    if (x.locus < prev || x.locus >= n_loci) return {VAPOR_E_ARG, "reads must be sorted by locus"};
    const int32_t idx[4] = {x.ref_a, x.alt_a, x.kind == 0 ? x.ref_b : x.ref_a, x.kind == 0 ? x.alt_b : x.alt_a};
    for (int32_t q : idx)
        if (q < 0 || q >= n_pairs) return {VAPOR_E_ARG, "read refers to a pair outside the plan"};
    if (x.kind < 0 || x.kind > 3) return {VAPOR_E_ARG, "unknown scorer kind"};
    return {};
}

// The upload image reads | locus_first (one blocking copy out of caller memory instead of two) and the blocks behind it: a score
// per read and a record per locus, neither smaller than one entry.
struct ReadImage {
    Table<vapor_read> reads;                   // max(n_reads, 1) entries, the first n_reads the caller's
    Table<int32_t> locus_first;                // n_loci + 1: locus l's reads are locus_first[l] .. locus_first[l + 1]
    size_t bytes = 0, score_bytes = 0, loci_bytes = 0;
    ReadImage() = default;
    ReadImage(int64_t n_reads, int64_t n_loci)
    {
        Carve c;
        c.take(reads, (size_t)std::max<int64_t>(n_reads, 1));
        c.take(locus_first, (size_t)n_loci + 1);
        bytes = c.off;
        score_bytes = sizeof(double) * (size_t)std::max<int64_t>(n_reads, 1);
        loci_bytes = sizeof(double) * LOCUS_DOUBLES * (size_t)std::max<int64_t>(n_loci, 1);
    }
};
// the checks, the host's locus_first and the filled image, the reads walked once
inline Refusal read_table(int64_t n_reads, const vapor_read* reads, int64_t n_loci, int64_t n_pairs, std::vector<int32_t>& first,
                          ReadImage& im, std::vector<uint8_t>& image)
{
    first.assign((size_t)n_loci + 1, 0);
    int32_t prev = -1;
    for (int64_t r = 0; r < n_reads; ++r) {
        if (const Refusal no = read_refusal(reads[r], prev, n_loci, n_pairs)) return no;
        prev = reads[r].locus;
        first[(size_t)prev + 1]++;
    }
    for (int64_t l = 0; l < n_loci; ++l) first[(size_t)l + 1] += first[(size_t)l];
    im = ReadImage(n_reads, n_loci);
    image.assign(im.bytes, 0);
    if (n_reads) memcpy(im.reads.in(image.data()), reads, sizeof(vapor_read) * (size_t)n_reads);
    im.locus_first.fill(image, first);
    return {};
}

// ------------------------------------------------------------------------------------------
// the grid (vapor_plan_set_grid, vapor_grid_pick)
// ------------------------------------------------------------------------------------------
// Breakpoint refinement: the loci are the candidates of n_groups refined loci, group g the loci first_locus[g] ..
// first_locus[g + 1].  Every candidate of a group scores the group's reads, so all of them have one read count (lf: the loci's
// read ranges); off[g] .. off[g + 1]: the group's slots among the winners' scores.  Five refusals, the first in this order: the
// cover, then per group its size, a decreasing read range, unequal read counts, a score slot beyond int32.
inline Refusal grid_check(int64_t n_groups, const int32_t* first_locus, int64_t n_loci, const int32_t* lf, std::vector<int32_t>& off)
{
    if (first_locus[0] != 0 || first_locus[n_groups] != n_loci) return {VAPOR_E_ARG, "grid: the groups must cover the loci"};
    off.assign((size_t)n_groups + 1, 0);
    for (int64_t g = 0; g < n_groups; ++g) {
        const int32_t a = first_locus[g], b = first_locus[g + 1];
        if (a < 0 || b <= a || b - a > VAPOR_MAX_CANDIDATES || b > n_loci)
            return {VAPOR_E_ARG, "grid: a group holds 1 .. VAPOR_MAX_CANDIDATES consecutive loci"};
        const int32_t nr = lf[(size_t)a + 1] - lf[a];
        if (nr < 0) return {VAPOR_E_ARG, "grid: read ranges must not decrease"};
        for (int32_t c = a; c < b; ++c)
            if (lf[(size_t)c + 1] - lf[c] != nr) return {VAPOR_E_ARG, "grid: the candidates of a group score the same reads"};
        if ((int64_t)off[(size_t)g] + nr > INT32_MAX) return {VAPOR_E_ARG, "grid: too many reads"};
        off[(size_t)g + 1] = off[(size_t)g] + nr;
    }
    return {};
}

// The upload image first_locus | score_off | winner_idx (| read_first: vapor_grid_pick's, a plan has its read table's) of
// n_groups > 0 groups, and the blocks behind it: a group record per group, and the winners' scores, not smaller than one.
struct GridImage {
    Table<int32_t> first_locus, score_off;     // n_groups + 1 each
    Table<int32_t> winner_idx;                 // n_groups, written by the kernel
    Table<int32_t> read_first;                 // n_loci + 1, or none
    size_t bytes = 0, group_bytes = 0, winner_bytes = 0;
    GridImage() = default;
    GridImage(size_t n_groups, int32_t n_winner_scores, size_t n_read_first)
    {
        Carve c;
        c.take(first_locus, n_groups + 1);
        c.take(score_off, n_groups + 1);
        c.take(winner_idx, n_groups);
        c.take(read_first, n_read_first);
        bytes = c.off;
        group_bytes = sizeof(double) * GROUP_DOUBLES * n_groups;
        winner_bytes = sizeof(double) * (size_t)std::max<int32_t>(n_winner_scores, 1);
    }
    // the image filled: the caller's groups, grid_check's offsets, zeros where the winners go (rf: null without read_first)
    std::vector<uint8_t> filled(const int32_t* fl, const std::vector<int32_t>& off, const int32_t* rf) const
    {
        std::vector<uint8_t> image(bytes, 0);
        memcpy(first_locus.in(image.data()), fl, first_locus.bytes());
        score_off.fill(image, off);
        if (read_first.n) memcpy(read_first.in(image.data()), rf, read_first.bytes());
        return image;
    }
};

// vapor_grid_pick's own range checks in front of grid_check (the loci are first_locus[n_groups] many, read_first their read
// ranges; n_groups >= 0 and the pointers are there) ...
inline Refusal pick_check(int64_t n_groups, const int32_t* first_locus, const int32_t* read_first, std::vector<int32_t>& off)
{
    const int64_t n_loci = first_locus[n_groups];
    if (n_loci < 0 || n_loci > INT32_MAX || read_first[0] != 0) return {VAPOR_E_ARG, "vapor_grid_pick: bad ranges"};
    for (int64_t l = 0; l < n_loci; ++l)
        if (read_first[l + 1] < read_first[l]) return {VAPOR_E_ARG, "vapor_grid_pick: read ranges must not decrease"};
    return grid_check(n_groups, first_locus, n_loci, read_first, off);
}
// ... and the one behind it, once score_off is handed out and a call without groups has returned: reads without their scores
inline Refusal pick_scores_check(size_t n_reads, const double* read_scores)
{
    if (n_reads && !read_scores) return {VAPOR_E_ARG, "vapor_grid_pick: null argument"};
    return {};
}

// ------------------------------------------------------------------------------------------
// the run's decisions (vapor_plan_run_loci, vapor_plan_run_grid, vapor_plan_run_loci_async)
// ------------------------------------------------------------------------------------------
// a pair the host gave a status: at plan creation, or a run did (the targets of a shared dot plot beyond max_pair_cap)
inline bool any_status(const int32_t* status, int64_t n_pairs)
{
    for (int64_t i = 0; i < n_pairs; ++i)
        if (status[i] != 0) return true;
    return false;
}
// The light path leaves the statistics on the device.  The full path (vapor_plan_run: statistics to the host, slots grown) is
// taken by the first run and whenever a pair has a host-side status ...
inline bool light_run(bool ran, bool host_status) { return ran && !host_status; }
// ... and hands the host's records to the device again when one has, before the run or by it (the light path has none to hand)
inline bool reupload_statuses(bool light, bool host_status) { return !light && host_status; }
// A light run that saw a pair outgrow its record slot is repeated through the full path, which resizes - unless an earlier
// repeat has shown that some pair overflows even at max_pair_cap (overflow_final): such a pair keeps VAPOR_E_OVERFLOW in its
// statistics, is scored as a read without a usable plot, and nothing is retried for it again.
inline bool repeat_full(bool light, bool overflow_seen, bool overflow_final) { return light && overflow_seen && !overflow_final; }
// what the repeat's full run says about overflow_final
inline bool still_overflows(const int64_t* stats, int64_t n_pairs)
{
    for (int64_t i = 0; i < n_pairs; ++i)
        if (stats[STATS_WORDS * (size_t)i + VAPOR_ST_STATUS] == VAPOR_E_OVERFLOW) return true;
    return false;
}

// what an asynchronous step is refused for before anything is enqueued, in order
inline Refusal async_refusal(bool has_reads, bool ran, const int32_t* status, int64_t n_pairs)
{
    if (!has_reads) return {VAPOR_E_ARG, "vapor_plan_run_loci_async: call vapor_plan_set_reads first"};
    if (!ran) return {VAPOR_E_ARG, "vapor_plan_run_loci_async: run the plan once with vapor_plan_run_loci first (it sizes the slots)"};
    if (any_status(status, n_pairs)) return {VAPOR_E_ARG, "vapor_plan_run_loci_async: the plan holds pairs the host rejected; use vapor_plan_run_loci"};
    return {};
}

}  // namespace finish_plan
}  // namespace vapor
