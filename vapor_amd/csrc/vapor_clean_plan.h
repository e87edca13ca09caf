// vapor_clean_plan.h - the host side of a clean launch, without HIP: the constants of clean_kernel and
// clean_big_kernel, the carving of their one dynamic LDS allocation, how many records a workgroup stages and how many workgroups a
// CU then holds, which compiled width a value range takes, who cuts a served pair's records, the slots of a plan's records, what a
// blocking run decides from its statistics, and the packing of caller-supplied dot lists.  The kernels (vapor_kernels.h) take their
// LDS pointers and their constants from here, so the host's byte counts and the device's offsets are one piece of arithmetic;
// tools/clean_plan_check.cpp holds it to direct statements on the host under the sanitizers.
#pragma once

#include "vapor_hip.h"
#include "vapor_image.h"
#include "vapor_records.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define VAPOR_CL_HD __host__ __device__
#else
#define VAPOR_CL_HD
#endif

namespace vapor {

// ------------------------------------------------------------------------------------------
// constants
// ------------------------------------------------------------------------------------------
#ifndef VAPOR_CLEAN_THREADS
#define VAPOR_CLEAN_THREADS 256
#endif
constexpr int CLEAN_THREADS = VAPOR_CLEAN_THREADS;
constexpr int CLEAN_WAVES = CLEAN_THREADS / 64;
// words of the clean kernels' value bitmap: values i + j and i - j + len2 stay below 2 * 65536 (positions are 16 bit)
constexpr int CLEAN_RANGE_WORDS_MAX = 4096;
constexpr int CLEAN_PER_MAX = (CLEAN_RANGE_WORDS_MAX + CLEAN_THREADS - 1) / CLEAN_THREADS;   // bitmap words per thread at the largest value range
static_assert((2 * VAPOR_MAX_SEQ_LEN + 2 + 31) / 32 <= CLEAN_RANGE_WORDS_MAX, "cluster_axis sizes its per-thread word list for this");
// clean_kernel is instantiated for these bitmap words per thread: a value range takes the smallest that covers it
constexpr int CLEAN_N_WIDTHS = 3;
constexpr int CLEAN_WIDTHS[CLEAN_N_WIDTHS] = {4, 8, CLEAN_PER_MAX};
// records a pair staged in LDS has at most: the staged format keeps a record's group in 13 bits (rec_decode, vapor_kernels.h)
constexpr int CLEAN_HCAP_MAX = 8192;
constexpr int CLEAN_BIG_GRID = 1024;      // clean_big_kernel walks its list with at most this many workgroups
// A CU's LDS and what of it one workgroup may ask for as dynamic memory (the kernels' attribute); workgroups a CU holds at most
// (32 waves); and the room the residency search leaves beside a workgroup's dynamic allocation - for the kernel's static LDS
// (CleanShared, some 200 bytes) and for the granularity LDS is handed out in.  The search leaves that room on both sides of its
// comparison, as it always has, and every measured residency below rests on it.
constexpr size_t CLEAN_LDS_PER_CU = 160 * 1024;
constexpr size_t CLEAN_LDS_DYNAMIC_MAX = CLEAN_LDS_PER_CU - 4096;
constexpr int CLEAN_PER_CU_MAX = 2048 / CLEAN_THREADS;
constexpr size_t CLEAN_STATIC_LDS_ROOM = 512;

// remap_for_target (a served pair's records cut out of the shared plot by its own clean workgroup) uses the start of the
// dynamic LDS before the cleaning does: words 0..2 counters, from REMAP_BOUNDS_WORD the n_iv + 2 boundaries, from REMAP_OPS_WORD
// two op words per interval, for at most REMAP_MAX_IV intervals.
constexpr int REMAP_BOUNDS_WORD = 4;
constexpr int REMAP_OPS_WORD = 64;
constexpr size_t REMAP_SCRATCH_BYTES = sizeof(uint32_t) * (REMAP_OPS_WORD + 2 * REMAP_MAX_IV);
static_assert(3 <= REMAP_BOUNDS_WORD && REMAP_BOUNDS_WORD + REMAP_MAX_IV + 2 <= REMAP_OPS_WORD, "counters, boundaries and ops do not overlap");

namespace clean_plan {

using vapor_image::Refusal;

// ------------------------------------------------------------------------------------------
// the layout of the dynamic LDS, in 32-bit words from its start - read by clean_pair and by the host's byte counts
// ------------------------------------------------------------------------------------------
// clean_kernel (staged): bitmap and 16-bit ranks of one axis, or of both (`dual`: cluster_dual works on the two axes of C1 at
// once), one region of `groups_cap` 16-bit group counters, then `hcap` staged records, 8 bytes each with their flag byte inside.
// clean_big_kernel: bitmap | ranks | `groups_cap` 32-bit group counters, dual false, no records.
struct Layout {
    int range_words_cap, groups_cap, hcap;
    bool dual;
    VAPOR_CL_HD constexpr int axis_words() const { return range_words_cap + (range_words_cap + 1) / 2; }     // a bitmap and its ranks
    VAPOR_CL_HD constexpr int bitmap() const { return 0; }
    VAPOR_CL_HD constexpr int bitmap2() const { return axis_words(); }
    VAPOR_CL_HD constexpr int ranks_behind_bitmap() const { return range_words_cap; }      // an axis' ranks, from its bitmap's first word
    VAPOR_CL_HD constexpr int ranks() const { return bitmap() + ranks_behind_bitmap(); }
    VAPOR_CL_HD constexpr int ranks2() const { return bitmap2() + ranks_behind_bitmap(); }
    VAPOR_CL_HD constexpr int counters() const { return dual ? 2 * axis_words() : axis_words(); }
    VAPOR_CL_HD constexpr int records() const { return (counters() + (groups_cap + 1) / 2 + 1) & ~1; }   // (8-byte aligned)
    // the allocation of a staged launch, and of clean_big_kernel's (32-bit counters, no records)
    VAPOR_CL_HD constexpr size_t staged_bytes() const { return sizeof(uint32_t) * (size_t)records() + 64 + (size_t)hcap * 8 + 8; }
    VAPOR_CL_HD constexpr size_t big_bytes() const { return sizeof(uint32_t) * ((size_t)axis_words() + (size_t)groups_cap) + 64; }
};

// ------------------------------------------------------------------------------------------
// the geometry of a launch
// ------------------------------------------------------------------------------------------
// groups a value range can hold at most (clean_big_kernel counts that many)
inline int groups_cap(int range_words_cap) { return range_words_cap * 32 / 10 + 8; }

// clean_kernel: 16-bit group sizes.  A pair staged in LDS has at most hcap records and every group holds at least
// one, so hcap counters do; the same region later holds the per-value counters of the median (value span / 100).
inline int groups_lds(int rw, int hcap)
{
    const int g = std::min(groups_cap(rw), std::max(hcap, 1));
    return 2 * std::max((g + 1) / 2, rw * 32 / 100 + 8);
}

inline Layout staged_layout(int rw, int hcap, bool dual) { return Layout{rw, groups_lds(rw, hcap), hcap, dual}; }
inline Layout big_layout(int rw) { return Layout{rw, groups_cap(rw), 0, false}; }

// The scratch floor.  A launch whose workgroups serve pairs (remap_for_target) needs REMAP_SCRATCH_BYTES of dynamic LDS whatever
// the layout asks for: after a measured fit a plan of tiny pairs asks for as little as 152 bytes.  This is the one place where a
// launch asks for more than its layout, and only below 640 bytes - where residency is bounded by the 32 waves of a CU, not by its
// LDS (eight workgroups of 640 bytes), so per_cu and every result are what they were.
inline size_t launch_bytes(const Layout& staged, bool serves) { return serves ? std::max(staged.staged_bytes(), REMAP_SCRATCH_BYTES) : staged.staged_bytes(); }

// The kernel waits for memory and barriers more than it computes, so residency matters: take the largest number
// of workgroups per CU (32 waves at most) whose share of the 160 KB still stages ~90 % of the expected records.
struct Geom { int hcap, per_cu; bool dual; };
inline Geom geom_for(int range_words_cap, int want, bool dual, bool exact = false)
{
    Geom g{0, 1, dual};
    for (int per_cu = CLEAN_PER_CU_MAX; per_cu >= 1; --per_cu) {
        const size_t share = CLEAN_LDS_PER_CU / per_cu - CLEAN_STATIC_LDS_ROOM;
        int cap = std::min(want, CLEAN_HCAP_MAX) & ~3;
        while (cap > 0 && staged_layout(range_words_cap, cap, dual).staged_bytes() + CLEAN_STATIC_LDS_ROOM > share) cap -= 4;
        // (an estimated `want`: nine tenths of it staged is enough; a measured one - the largest record count of the plan's
        // pairs - is staged whole, so that no pair is left to clean_big_kernel for the sake of residency)
        if (cap >= (exact ? want : want * 9 / 10) || per_cu == 1) { g.hcap = std::max(cap, 0); g.per_cu = per_cu; break; }
    }
    return g;
}
// Both axes of C1 in one sweep (cluster_dual) need a second bitmap and rank array per workgroup.  Measured (tools/clean_sweep.py,
// profiles/r03_clean_variants.txt): the sweep wins where the extra LDS costs no residency (30 kb x 40 kb pairs, two workgroups
// per CU either way: clean 1.87 -> 1.70 ms) and loses where it does (10 kb x 20 kb: 7 -> 6 per CU, 0.075 vs 0.078 ms; 15 kb x
// 20 kb: 5 -> 4, 1.32 vs 1.42 ms) - so it is used exactly when it is free.
inline Geom geom(int range_words_cap, int want, bool exact = false)
{
    const Geom seq = geom_for(range_words_cap, want, false, exact), dual = geom_for(range_words_cap, want, true, exact);
    return dual.per_cu >= seq.per_cu ? dual : seq;      // (either stages at least nine tenths of the expected records)
}

// the compiled width (CLEAN_WIDTHS) a value range runs at
inline int width(int range_words_cap)
{
    const int per = (range_words_cap + CLEAN_THREADS - 1) / CLEAN_THREADS;
    for (int k = 0; k < CLEAN_N_WIDTHS - 1; ++k)
        if (per <= CLEAN_WIDTHS[k]) return CLEAN_WIDTHS[k];
    return CLEAN_PER_MAX;
}

// Who cuts the served pairs' records out of the shared dot plots: the clean workgroup of each pair, or remap_kernel before the
// cleaning.  Measured (profiles/r04_remap_experiments.txt): the clean workgroups win when the plan is a couple of rounds of them
// - a resident batch of the 10 kb shape, 4 000 pairs at seven workgroups per CU: such a launch is bound by its start, its tail
// and the chains of loads in between, and a kernel boundary and a trip of the records through HBM is what the kernel of its own
// adds (+3 % loci/s) - and lose when it is many rounds (cfg3, 15 kb reads: 80 000 pairs at five per CU, 62 rounds: a launch bound by
// what its workgroups execute, and every target reads the shared plot and searches the interval table again; -3 %).  Between
// the two measured shapes the rule is a guess: the clean workgroups up to four rounds.
// "remap_in_clean" (`param`): 1 = that rule, 0 = always the kernel, 2 = always the clean workgroups.
constexpr int REMAP_IN_CLEAN_ROUNDS = 4;
inline bool remap_in_clean(int param, int64_t n_plots, int64_t n_pairs, int per_cu, int n_cus)
{
    if (n_plots <= 0 || param == 0) return false;
    if (param == 2) return true;
    return n_pairs <= REMAP_IN_CLEAN_ROUNDS * (int64_t)per_cu * n_cus;
}

// ------------------------------------------------------------------------------------------
// the record slots of a plan
// ------------------------------------------------------------------------------------------
// Lays the slots out from hp[].cap: every slot padded to four records (the kernels store flag bytes four at a time), four records
// of tail; the served pairs see their shared plot's slot.  Returns the records to allocate.
inline int64_t lay_slots(std::vector<DPair>& hp, std::vector<DServe>& serve)
{
    int64_t tot = 0;
    for (auto& d : hp) {
        d.hit_off = tot;
        tot += (int64_t)((d.cap + 3u) & ~3u);
    }
    for (auto& sv : serve)
        if (sv.dpair >= 0) { sv.hit_off = hp[(size_t)sv.dpair].hit_off; sv.cap = hp[(size_t)sv.dpair].cap; }
    return tot + 4;
}

// ------------------------------------------------------------------------------------------
// what a blocking run decides from what it fetched.  `stats`: 16 words per pair; `plots`: the packed counters (records | dots << 32)
// of the shared dot plots, which are hp[n_pairs ..]
// ------------------------------------------------------------------------------------------
// Slots whose pair or plot produced more records than they hold are enlarged to the exact count, up to max_pair_cap; returns how many.
inline int64_t grow_slots(const long long* stats, int64_t n_pairs, const std::vector<unsigned long long>& plots, int64_t max_pair_cap,
                          std::vector<DPair>& hp)
{
    int64_t grow = 0;
    for (int64_t i = 0; i < n_pairs; ++i) {
        const long long* s = stats + 16 * i;
        if (s[15] == VAPOR_E_OVERFLOW && s[14] <= max_pair_cap && (uint32_t)s[14] > hp[(size_t)i].cap) {
            hp[(size_t)i].cap = (uint32_t)s[14];     // records the pair produced
            ++grow;
        }
    }
    for (size_t t = 0; t < plots.size(); ++t) {
        DPair& d = hp[(size_t)n_pairs + t];
        const uint32_t need = (uint32_t)plots[t];   // (a plot's record count is the low half of the join's packed counter)
        if (need > d.cap && (int64_t)need <= max_pair_cap) { d.cap = need; ++grow; }
    }
    return grow;
}

// The clean kernel's geometry from what the pairs really hold: a plan is created with an ESTIMATE of the records a pair
// will have (a tenth of the shorter sequence plus the chance dots), which sizes the LDS copy and with it the workgroups a
// CU holds; the join is deterministic, so after one blocking run the largest record count is known exactly and the copy
// is sized for that.  On the 10 kb x 20 kb shape that is eight workgroups per CU instead of seven - and 4 000 pairs are
// 1.95 rounds of 2 048 workgroups instead of 2.2 rounds of 1 792, i.e. two rounds instead of three.
// `counts`: the pairs' packed counters.  Refused pairs and pairs of more than 65 535 dots (which go to clean_big_kernel whatever is
// staged) do not count.  Returns the measured want, a multiple of four, or 0: keep the estimate.
inline int measured_want(const std::vector<unsigned long long>& counts, const std::vector<int32_t>& status)
{
    uint32_t most = 0;
    for (size_t i = 0; i < counts.size(); ++i)
        if (status[i] == 0 && (uint32_t)(counts[i] >> 32) <= 65535u) most = std::max(most, (uint32_t)counts[i]);
    return most > 0 && most <= (uint32_t)CLEAN_HCAP_MAX ? (int)((most + 3u) & ~3u) : 0;
}

// A shared dot plot that needs more than max_pair_cap cannot grow: the records its targets were cut from are a
// truncated plot, although the targets' own slots did not overflow.  Every pair it serves keeps VAPOR_E_OVERFLOW
// (include/vapor_hip.h, "max_pair_cap") - as a host-side status, so that every later run reports it as well and
// vapor_plan_run_loci takes the path that hands the statuses to the finish kernel.
inline void refuse_truncated_plots(const std::vector<unsigned long long>& plots, const std::vector<DPair>& hp, int64_t n_pairs,
                                   const std::vector<DShare>& shares, std::vector<int32_t>& status)
{
    for (size_t t = 0; t < plots.size(); ++t)
        if ((uint32_t)plots[t] > hp[(size_t)n_pairs + t].cap)
            for (int32_t tg : shares[t].target)
                if (tg >= 0 && status[(size_t)tg] == 0) status[(size_t)tg] = VAPOR_E_OVERFLOW;
}

// the statistics of a refused pair: 0 dots, no first and last j, its status
inline void mask_refused(long long* stats, const std::vector<int32_t>& status, int64_t n_pairs)
{
    for (int64_t i = 0; i < n_pairs; ++i) {
        long long* s = stats + 16 * i;
        if (status[(size_t)i] != 0) {
            for (int t = 0; t < 16; ++t) s[t] = 0;
            s[1] = s[2] = -1;
            s[15] = status[(size_t)i];
        }
    }
}

// ------------------------------------------------------------------------------------------
// caller-supplied dot lists (vapor_clean_hits, vapor_clean_hits_wide)
// ------------------------------------------------------------------------------------------
// The lists: coordinates in 0 .. coord_max.  Only the wide entry point has ever checked the offsets themselves (list_cap >= 0:
// they do not decrease, no list longer than that); the narrow one (list_cap < 0) takes them as given.  Each entry point keeps
// its own set of refusals here; aligning them is a change of behaviour.  (The messages go behind the entry's name.)
inline Refusal lists_check(bool ctx, int64_t n_lists, const int32_t* hits_ji, const int64_t* off, const int64_t* stats, int coord_max,
                           int64_t list_cap)
{
    if (!ctx || n_lists < 0 || (n_lists && (!off || !stats))) return Refusal{VAPOR_E_ARG, "null argument"};
    if (n_lists == 0) return Refusal{};
    if (off[n_lists] && !hits_ji) return Refusal{VAPOR_E_ARG, "null hit list"};
    for (int64_t t = 0; t < n_lists; ++t) {
        if (list_cap >= 0 && (off[t + 1] < off[t] || off[t + 1] - off[t] > list_cap)) return Refusal{VAPOR_E_ARG, "bad list offsets"};
        for (int64_t h = off[t]; h < off[t + 1]; ++h) {
            const int j = hits_ji[2 * h], i = hits_ji[2 * h + 1];
            if (j < 0 || i < 0 || j > coord_max || i > coord_max) return Refusal{VAPOR_E_ARG, "coordinate out of range"};
        }
    }
    return Refusal{};
}

// records the narrow list route stages at most: vapor_clean_hits asks the geometry for this want
constexpr int LISTS_WANT = 4096;

// What vapor_clean_hits uploads: one record of one dot per coordinate pair, every list's slot padded to a multiple of four
// records, the lists as pairs of their own, their packed counts and the value range of the largest list.
struct ListPack {
    std::vector<int64_t> poff;                     // n_lists + 1 padded record offsets
    std::vector<unsigned long long> packed, counts;
    std::vector<DPair> dp;
    int rw = 1;
    ListPack(int64_t n_lists, const int32_t* hits_ji, const int64_t* off, const uint32_t* flags)
        : poff((size_t)n_lists + 1, 0), counts((size_t)n_lists), dp((size_t)n_lists)
    {
        for (int64_t t = 0; t < n_lists; ++t) poff[t + 1] = poff[t] + ((off[t + 1] - off[t] + 3) & ~(int64_t)3);
        packed.assign((size_t)std::max<int64_t>(poff[n_lists], 4), 0ull);
        for (int64_t t = 0; t < n_lists; ++t) {
            int mi = 0, mj = 0;
            for (int64_t h = off[t]; h < off[t + 1]; ++h) {
                int j = hits_ji[2 * h], i = hits_ji[2 * h + 1];
                mi = std::max(mi, i); mj = std::max(mj, j);
                packed[poff[t] + (h - off[t])] = (unsigned long long)(((uint32_t)j << 16) | (uint32_t)i) | (1ull << 32);
            }
            DPair& d = dp[t];
            d.seq1 = (int32_t)(2 * t); d.seq2 = (int32_t)(2 * t + 1); d.off2 = 0; d.k = 10;
            d.len1 = mi + 1; d.len2 = mj + 1;
            d.flags = flags ? flags[t] : 3u;
            d.cap = (uint32_t)(off[t + 1] - off[t]);
            d.hit_off = poff[t];
            counts[t] = (unsigned long long)(off[t + 1] - off[t]) * 0x100000001ull;   // records | dots << 32
            // the largest values, i + j = 131070 and i - j + len2 = 131071, still fall into word 4095
            rw = std::min(std::max(rw, (mi + mj + 4 + 31) / 32), CLEAN_RANGE_WORDS_MAX);
        }
    }
};

}  // namespace clean_plan
}  // namespace vapor
