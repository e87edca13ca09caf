// vapor_dots_plan.h - the host side of the explicit-dot routes, without HIP: the wide route (vapor_wide_batch,
// vapor_clean_hits_wide; vapor_wide.h) and the any-k route (vapor_anyk_batch; vapor_anyk.h).  What a call and a pair are refused
// for, in order; a pair's shape; the sizes and grids of the wide join; the any-k pass with its sort schedule, symbol layout,
// buffers and edit cut; the passes and the scratch of the cleaning; the accumulator the clean kernels fill (WideAcc) and the three
// writers of a statistics record; the capacity protocol of hits_ji / hit_off; the bound on a pair's dots; the slots of the routes'
// device blocks.  vapor_wide.h takes WideAcc from here and vapor_anyk.h its constants, so host and device read one statement;
// tools/dots_plan_check.cpp holds it to direct statements on the host under the sanitizers.  The functions in vapor_hip.hip are
// allocations, memsets, launches, copies and synchronisations.
#pragma once

#include "vapor_clean_plan.h"
#include "vapor_hip.h"
#include "vapor_image.h"
#include "vapor_planner.h"
#include "vapor_records.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace vapor {

// ------------------------------------------------------------------------------------------
// constants of the any-k kernels (vapor_anyk.h) that the host's arithmetic reads as well
// ------------------------------------------------------------------------------------------
constexpr int ANYK_EXACT_MAX_K = 40;            // k up to this: exact matches; above: the edit-distance branch
constexpr int ANYK_TILE = 512;                  // elements sorted in LDS by one 256-thread workgroup
constexpr int ANYK_EDIT_WAVES = 4;              // allele k-mers (one wave each) per workgroup of anyk_edit_kernel
constexpr long long ANYK_EDIT_PAIRS = 1ll << 31;        // (query, key) distances per launch of the edit pass unless "anyk_edit_pairs" says otherwise

// per-pair results of the cleaning (device side; record_folded turns them into the statistics record)
struct WideAcc {
    unsigned long long n_diag, n_lower, c1_kept, c1_sum_abs, c2_kept, c2_count10, c2_kept_diag;
    long long dir_sum2;
    int min_j, max_j, kd_lo, kd_hi;
    int dir_c2x, dir_n, dir_lists, pad;
    uint32_t max_group[4];      // largest group of each clustering pass (0: i - j over all dots, 1: i + j for C1, 2: i + j for C2)
};

namespace dots_plan {

using vapor_image::Refusal;

// ------------------------------------------------------------------------------------------
// the dot bound
// ------------------------------------------------------------------------------------------
// Every kernel of the two routes counts a pair's dots in an int.  "max_pair_cap" may be set above that, so wherever the routes
// compare against it they compare against this: a pair beyond it keeps VAPOR_E_OVERFLOW as one beyond max_pair_cap does, a
// caller's list beyond it is refused ("bad list offsets").
inline int64_t dots_cap(int64_t max_pair_cap) { return std::min<int64_t>(max_pair_cap, INT32_MAX); }

// ------------------------------------------------------------------------------------------
// what a call is refused for (the messages go behind the entry's name)
// ------------------------------------------------------------------------------------------
// BATCH: vapor_wide_batch and vapor_anyk_batch (handles: context and set).  LISTS: vapor_clean_hits_wide (handles: the context),
// clean_plan::lists_check with the wide limits - coordinates up to VAPOR_MAX_WIDE_SEQ_LEN, no list beyond the dot bound.
enum Entry { BATCH, LISTS };
struct Call {
    Entry entry;
    bool handles;
    int64_t n;                     // pairs or lists
    const int64_t* stats;
    const int32_t* hits_ji;        // BATCH: where the dots go, or null; LISTS: the dots
    const int64_t* off;            // BATCH: hit_off; LISTS: the lists' offsets
    const vapor_pair* pairs;       // BATCH
    int64_t hits_capacity;         // BATCH
    int64_t max_pair_cap;          // LISTS
};
inline Refusal call_refusal(const Call& c)
{
    if (c.entry == LISTS) return clean_plan::lists_check(c.handles, c.n, c.hits_ji, c.off, c.stats, VAPOR_MAX_WIDE_SEQ_LEN, dots_cap(c.max_pair_cap));
    if (!c.handles || c.n < 0 || (c.n && (!c.pairs || !c.stats)) || (c.hits_ji && !c.off) || c.hits_capacity < 0) return Refusal{VAPOR_E_ARG, "null argument"};
    return Refusal{};
}

// ------------------------------------------------------------------------------------------
// what a pair is refused for: the status it keeps, before any device work
// ------------------------------------------------------------------------------------------
// the set as the rules read it: the caller's sequences, and where the bytes of those with symbols outside the alphabet are kept
struct SetView {
    int32_t n;
    const SeqDesc* h;
    const int64_t* raw_off;
    size_t n_raw;
};
// a symbol outside the alphabet whose byte was not kept (a derived sequence's)
inline bool no_bytes(const SetView& s, int32_t q) { return s.h[q].n_invalid > 0 && ((size_t)q >= s.n_raw || s.raw_off[q] < 0); }

// The rules, and per route the order they are tried in: the first one broken gives the pair its status.  A rule reads the
// sequences only behind INDICES.  KEY_ERROR: seq1 has k-mers and a symbol outside invert_base's alphabet (the reference raises
// KeyError building its lookup; the any-k route without inversions has no such lookup).  NO_BYTES: the any-k route without
// inversions compares such symbols byte for byte and needs the bytes.
enum Rule { INDICES, OFF2, K_WIDE, K_ANY, LENGTH, KEY_ERROR, NO_BYTES };
struct Step { Rule rule; int code; };
constexpr int N_WIDE_STEPS = 5, N_ANYK_STEPS = 6;
constexpr Step WIDE_STEPS[N_WIDE_STEPS] = {{INDICES, VAPOR_E_ARG}, {OFF2, VAPOR_E_ARG}, {K_WIDE, VAPOR_E_ARG}, {LENGTH, VAPOR_E_ARG}, {KEY_ERROR, VAPOR_E_KEYERROR}};
constexpr Step ANYK_STEPS[N_ANYK_STEPS] = {{INDICES, VAPOR_E_ARG}, {OFF2, VAPOR_E_ARG}, {K_ANY, VAPOR_E_ARG}, {LENGTH, VAPOR_E_ARG}, {KEY_ERROR, VAPOR_E_KEYERROR},
                                           {NO_BYTES, VAPOR_E_ARG}};

inline bool forward_only(const vapor_pair& a) { return (a.flags & VAPOR_PF_FORWARD) != 0; }     // the any-k route: no inversions

inline bool broken(Rule r, const SetView& s, const vapor_pair& a, bool inversions)
{
    switch (r) {
    case INDICES: return a.seq1 < 0 || a.seq1 >= s.n || a.seq2 < 0 || a.seq2 >= s.n;
    case OFF2: return a.off2 < 0;
    case K_WIDE: return !k_supported(a.k);
    case K_ANY: return a.k < 1 || a.k > VAPOR_MAX_ANY_K;
    case LENGTH: return s.h[a.seq1].len > VAPOR_MAX_WIDE_SEQ_LEN || s.h[a.seq2].len > VAPOR_MAX_WIDE_SEQ_LEN;
    case KEY_ERROR: return inversions && s.h[a.seq1].len - a.k + 1 > 0 && s.h[a.seq1].n_invalid > 0;
    case NO_BYTES: return !inversions && (no_bytes(s, a.seq1) || no_bytes(s, a.seq2));
    }
    return false;
}
// the first step of `steps` the pair breaks, or -1
inline int first_broken(const Step* steps, int n_steps, const SetView& s, const vapor_pair& a, bool inversions)
{
    for (int t = 0; t < n_steps; ++t)
        if (broken(steps[t].rule, s, a, inversions)) return t;
    return -1;
}
inline int admit_wide(const SetView& s, const vapor_pair& a)
{
    const int t = first_broken(WIDE_STEPS, N_WIDE_STEPS, s, a, true);
    return t < 0 ? 0 : WIDE_STEPS[t].code;
}
inline int admit_anyk(const SetView& s, const vapor_pair& a)
{
    const int t = first_broken(ANYK_STEPS, N_ANYK_STEPS, s, a, !forward_only(a));
    return t < 0 ? 0 : ANYK_STEPS[t].code;
}

// ------------------------------------------------------------------------------------------
// an admitted pair's shape
// ------------------------------------------------------------------------------------------
struct Shape {
    int nk1, nk2;                  // k-mers of seq1 and of seq2[off2:] (not above zero: none)
    int n2;                        // symbols of seq2[off2:]
    bool kmers() const { return nk1 > 0 && nk2 > 0; }       // otherwise the pair has no dots and nothing is counted
};
inline Shape shape(const SeqDesc& s1, const SeqDesc& s2, const vapor_pair& a)
{
    const int n2 = std::max(0, s2.len - a.off2);
    return Shape{s1.len - a.k + 1, n2 - a.k + 1, n2};
}

// workgroups of 256 threads, one thread an item
constexpr int THREADS = 256;
inline unsigned grid(int64_t n) { return (unsigned)((n + THREADS - 1) / THREADS); }
// a block of the routes is never smaller than this
constexpr size_t BLOCK_FLOOR = 256;

// ------------------------------------------------------------------------------------------
// the slots of the routes' device blocks, one list per owner
// ------------------------------------------------------------------------------------------
// the per-pair loop's (and vapor_clean_hits_wide's): the dots, their flag bytes, the cleaning's scratch, the accumulator
enum SharedSlot { DOTS, FL, SCR, ACC, N_SHARED };
// the wide join's: the table (keys, bucket heads, chain links), dots per allele position and their prefix, the count pass' booking word
enum WideSlot { WIDE_KEYS, WIDE_HEAD, WIDE_NEXT, WIDE_CNT, WIDE_OFF, WIDE_BOOKED, N_WIDE };
// the any-k pass': symbol bytes, sorted entries, dots per allele position, first entry of its run and the prefix; the edit
// branch's first-of-run marks, runs, key ranks and key table
enum AnykSlot { ANYK_SYM, ANYK_IDX, ANYK_CNT, ANYK_FIRST, ANYK_OFF, ANYK_ISF, ANYK_RUN, ANYK_RANK, ANYK_KEYS, N_ANYK };

// ------------------------------------------------------------------------------------------
// the wide join of one pair (nk1, nk2 > 0)
// ------------------------------------------------------------------------------------------
// Entries: every k-mer of the read, forward and reverse complemented.  The chained hash table has the smallest power of two of
// buckets that is at least twice the entries; a key is 4 k bits in whole 32-bit words.
struct WideJoin {
    int64_t ne;
    uint32_t H, mask;
    size_t keys, heads, nexts, counts, offsets;    // bytes
    unsigned table_grid, probe_grid, scan_grid;    // wide_table_kernel, wide_probe_kernel (256 threads), wide_scan_kernel (one workgroup)
};
inline size_t wide_key_bytes(int k) { return sizeof(uint32_t) * (size_t)((4 * k + 31) / 32); }
inline WideJoin wide_join(int k, int nk1, int nk2)
{
    WideJoin w{};
    w.ne = 2 * (int64_t)nk1;
    for (w.H = 1; (int64_t)w.H < 2 * w.ne;) w.H <<= 1;
    w.mask = w.H - 1;
    w.keys = (size_t)w.ne * wide_key_bytes(k);
    w.heads = sizeof(int32_t) * (size_t)w.H;
    w.nexts = sizeof(int32_t) * (size_t)w.ne;
    w.counts = sizeof(uint32_t) * (size_t)nk2;
    w.offsets = sizeof(long long) * ((size_t)nk2 + 1);
    w.table_grid = grid(w.ne);
    w.probe_grid = grid(nk2);
    w.scan_grid = 1;
    return w;
}

// ------------------------------------------------------------------------------------------
// the any-k pass of one pair (nk1, nk2 > 0)
// ------------------------------------------------------------------------------------------
// The symbol bytes: seq1, with inversions its reverse complement, seq2[off2:] - each string on 16 bytes with at least 16 bytes
// behind it (the kernels read whole words past a k-mer's end).
inline size_t anyk_pad(int n) { return ((size_t)n + 16 + 15) & ~(size_t)15; }
struct Symbols { size_t s1, r1, s2, bytes; };      // offsets of the read, its reverse complement (inversions only) and the allele
inline Symbols symbols(int len1, int n2, bool inversions)
{
    Symbols y{0, anyk_pad(len1), 0, 0};
    y.s2 = y.r1 + (inversions ? anyk_pad(len1) : 0);
    y.bytes = y.s2 + anyk_pad(n2);
    return y;
}

// One launch of the bitonic sort of np entries.  local: anyk_sort_local_kernel(full, kk) on np / ANYK_TILE workgroups, every
// stride below ANYK_TILE in LDS; otherwise anyk_sort_global_kernel(np, kk, jj), one stride jj >= ANYK_TILE over np / 2 threads.
struct SortStep { bool local; int full, kk, jj; };
inline int sort_size(int n)
{
    int np = ANYK_TILE;
    while (np < n) np <<= 1;
    return np;
}
// the whole network: tiles sorted in LDS, then for each merge size kk its global strides, widest first, and one local merge
inline std::vector<SortStep> sort_schedule(int np)
{
    std::vector<SortStep> s{SortStep{true, 1, 0, 0}};
    for (int64_t kk = 2 * ANYK_TILE; kk <= np; kk <<= 1) {
        for (int jj = (int)(kk >> 1); jj >= ANYK_TILE; jj >>= 1) s.push_back(SortStep{false, 0, (int)kk, jj});
        s.push_back(SortStep{true, 0, (int)kk, 0});
    }
    return s;
}

// entries (one per k-mer of the read, two with inversions), the sort's size, which branch counts, where the symbols lie, and the
// bytes of every block the pass takes (0: the branch does not use it)
struct AnykPass {
    int n, np;
    bool exact;
    Symbols sym;
    size_t bytes[N_ANYK];
    unsigned iota_grid, tile_grid, stride_grid, entry_grid, allele_grid;       // over np, np / ANYK_TILE, np / 2, n, nk2
};
inline AnykPass anyk_pass(int k, bool inversions, int len1, const Shape& sh)
{
    AnykPass p{};
    const size_t nk2 = (size_t)sh.nk2;
    p.n = inversions ? 2 * sh.nk1 : sh.nk1;
    p.np = sort_size(p.n);
    p.exact = k <= ANYK_EXACT_MAX_K;
    p.sym = symbols(len1, sh.n2, inversions);
    p.bytes[ANYK_SYM] = p.sym.bytes;
    p.bytes[ANYK_IDX] = sizeof(uint32_t) * (size_t)p.np;
    p.bytes[ANYK_CNT] = sizeof(uint32_t) * nk2;
    p.bytes[ANYK_OFF] = sizeof(long long) * (nk2 + 1);
    if (p.exact) {
        p.bytes[ANYK_FIRST] = sizeof(uint32_t) * nk2;
    } else {
        p.bytes[ANYK_ISF] = sizeof(uint32_t) * (size_t)p.n;             // a mark per entry
        p.bytes[ANYK_RUN] = 8 * (size_t)p.n;                            // an int2 per entry
        p.bytes[ANYK_RANK] = sizeof(long long) * ((size_t)p.n + 1);     // the marks' prefix; its last word: the number of keys
        p.bytes[ANYK_KEYS] = 16 * (size_t)p.n;                          // an int4 per key
    }
    p.iota_grid = grid(p.np);
    p.tile_grid = (unsigned)(p.np / ANYK_TILE);
    p.stride_grid = grid(p.np / 2);
    p.entry_grid = grid(p.n);
    p.allele_grid = grid(sh.nk2);
    return p;
}

// The edit pass over allele k-mers 0 .. nk2 - 1 in launches of at most edit_pairs distances ("anyk_edit_pairs"; the n entries
// bound the number of keys): `per` allele k-mers a launch, a multiple of ANYK_EDIT_WAVES and at least that.
struct EditCut {
    long long per;
    int nk2;
    int launches() const { return nk2 <= 0 ? 0 : (int)((nk2 - 1) / per) + 1; }
    int j0(int t) const { return (int)(t * per); }                                             // t < launches(): below nk2
    int j1(int t) const { return nk2 - j0(t) <= per ? nk2 : (int)(j0(t) + per); }
    unsigned grid(int t) const { return (unsigned)((j1(t) - j0(t) + ANYK_EDIT_WAVES - 1) / ANYK_EDIT_WAVES); }   // workgroups of 64 * ANYK_EDIT_WAVES threads
};
inline EditCut edit_cut(int n, int nk2, long long edit_pairs)
{
    return EditCut{std::max<long long>(ANYK_EDIT_WAVES, edit_pairs / std::max(n, 1) / ANYK_EDIT_WAVES * ANYK_EDIT_WAVES), nk2};
}

// ------------------------------------------------------------------------------------------
// the cleaning of n dots with coordinates i <= maxi, j <= maxj
// ------------------------------------------------------------------------------------------
// A cluster pass: the occupancy counts of an axis (0: i - j + shift, 1: i + j) over the dots whose flag byte has none of `skip`,
// the gap clustering with its largest group into WideAcc::max_group[slot], wide_flag_kernel in `mode`.  C1 (flags & 1) and C2
// (flags & 2) share the pass over i - j, which writes every flag byte anew; without either the flag bytes are only zeroed.  The
// directed statistics (wide_dir_kernel) are C1's: flags & 4 without C1 asks for nothing.
struct ClusterPass { int axis; uint32_t skip; int slot, mode; };
constexpr uint32_t SKIP_C2D = 2u;                  // the flag bit of a dot C2 dropped on i - j (HF_C2D)
struct Cleaning {
    int n_passes;
    ClusterPass pass[3];
    bool zero_flags, dir;
};
inline Cleaning cleaning(uint32_t flags)
{
    const bool c1 = flags & 1u, c2 = flags & 2u;
    Cleaning c{0, {}, !(c1 || c2), c1 && (flags & 4u)};
    if (c1 || c2) c.pass[c.n_passes++] = ClusterPass{0, 0u, 0, 0};
    if (c1) c.pass[c.n_passes++] = ClusterPass{1, 0u, 1, 1};
    if (c2) c.pass[c.n_passes++] = ClusterPass{1, SKIP_C2D, 2, 2};
    return c;
}
inline bool wants_dir(uint32_t flags) { return cleaning(flags).dir; }

// the scratch: counts, group ids and group sizes, a 32-bit word each per value of an axis; i - j is shifted to start at 0
struct Scratch {
    int R, shift;
    size_t bytes;
    size_t axis_bytes() const { return sizeof(uint32_t) * (size_t)R; }        // of one of the three arrays
};
inline Scratch scratch(int maxi, int maxj) { return Scratch{maxi + maxj + 1, maxj, sizeof(uint32_t) * 3 * ((size_t)maxi + (size_t)maxj + 1)}; }

// the largest coordinates of a caller's list, dots h0 .. h1 - 1 of (j, i) pairs (an empty list: 0, 0)
struct Extent { int mi, mj; };
inline Extent extent(const int32_t* hits_ji, int64_t h0, int64_t h1)
{
    Extent x{0, 0};
    for (int64_t h = h0; h < h1; ++h) { x.mj = std::max(x.mj, hits_ji[2 * h]); x.mi = std::max(x.mi, hits_ji[2 * h + 1]); }
    return x;
}
constexpr uint32_t LIST_FLAGS = 3u;                // a list without flags is cleaned by C1 and C2

// ------------------------------------------------------------------------------------------
// the accumulator's first value and the three writers of a statistics record (16 words)
// ------------------------------------------------------------------------------------------
inline WideAcc acc_init()
{
    WideAcc a;
    memset(&a, 0, sizeof(a));
    a.min_j = 0x7FFFFFFF; a.max_j = -1; a.kd_lo = 0x7FFFFFFF; a.kd_hi = -0x7FFFFFFF;
    return a;
}
// a refused pair: no dots, no first and last j, its status
inline void record_refused(int code, int64_t* st)
{
    for (int t = 0; t < 16; ++t) st[t] = 0;
    st[1] = st[2] = -1;
    st[15] = code;
}
// a pair with more dots than a pair may hold: VAPOR_E_OVERFLOW with the dots counted (the wide route's count pass stops early:
// more than the bound, not necessarily all of them)
inline void record_overflowed(int64_t total, int64_t* st)
{
    record_refused(VAPOR_E_OVERFLOW, st);
    st[0] = total;
    st[14] = total;
}
// a scored pair or list of n dots
inline void record_folded(const WideAcc& a, int64_t n, uint32_t flags, int64_t* st)
{
    for (int t = 0; t < 16; ++t) st[t] = 0;
    st[0] = n;
    st[1] = n ? a.min_j : -1;
    st[2] = n ? a.max_j : -1;
    if (!n) return;
    st[3] = (int64_t)a.c1_kept; st[4] = (int64_t)a.c1_sum_abs; st[5] = (int64_t)a.c2_kept; st[6] = (int64_t)a.c2_count10;
    st[7] = (int64_t)a.n_diag; st[8] = (int64_t)a.n_lower; st[9] = (int64_t)a.c2_kept_diag;
    if (wants_dir(flags)) { st[10] = a.dir_c2x; st[11] = a.dir_n; st[12] = a.dir_sum2; st[13] = a.dir_lists; }
}

// ------------------------------------------------------------------------------------------
// the capacity protocol of a batch: hits_ji holds hits_capacity dots, hit_off[t + 1] the dots of pairs 0 .. t whether they fit or not
// ------------------------------------------------------------------------------------------
struct Capacity {
    bool wanted;                   // the caller gave hits_ji
    int64_t capacity;
    int64_t* hit_off;              // or null
    int64_t running = 0;           // dots of the pairs closed so far: where the next pair's dots go
    Capacity(bool hits, int64_t cap, int64_t* off) : wanted(hits), capacity(cap), hit_off(off) { if (hit_off) hit_off[0] = 0; }
    bool fits(int64_t n) const { return wanted && n && running + n <= capacity; }      // this pair's dots are copied out
    void close(int64_t t, int64_t n)                                                   // pair t ends with n dots (a refused one: 0)
    {
        running += n;
        if (hit_off) hit_off[t + 1] = running;
    }
    bool overflowed() const { return wanted && running > capacity; }                    // VAPOR_E_OVERFLOW; hit_off[n_pairs] holds the need
};

}  // namespace dots_plan
}  // namespace vapor
