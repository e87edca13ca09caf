// vapor_realign_plan.h - the host arithmetic of vapor_realign_batch, without HIP: which calls and which pairs are
// refused, the record a pair travels as, how the 2 * band + 1 slots of a band row are dealt to the 64 lanes of a wavefront, which
// of the compiled lane widths a band takes, how many rows a pair runs and the launch geometry.  realign_kernel (vapor_realign.h)
// reads the same constants and the same functions; tools/realign_check.cpp holds them to direct statements on the host under the
// sanitizers.
#pragma once

#include "vapor_hip.h"

#include <cstdint>

#if defined(__HIPCC__)
#define VAPOR_RA_HD __host__ __device__
#else
#define VAPOR_RA_HD
#endif

namespace vapor_realign {

constexpr int LANES = 64;                  // one wavefront a pair
constexpr int WAVES = 4;                   // wavefronts (pairs) of a workgroup
constexpr int INF = 1 << 28;               // a cell that does not exist: two of them, and a sequence's length, add up below 2^31
constexpr int MAX_SLOTS = (2 * VAPOR_MAX_BAND + 1 + LANES - 1) / LANES;       // 17: slots of a lane at the widest band
// the lane widths realign_kernel<S> is compiled for: a band takes the smallest that holds its row (a lane's slots live in
// registers, so the width is a template argument; the steps keep the idle slots of a band below a half)
constexpr int N_WIDTHS = 6;
constexpr int WIDTHS[N_WIDTHS] = {1, 2, 3, 5, 9, MAX_SLOTS};

// A pair as the kernel takes it (32 B): the sequences' first words in the 4-bit plane, n = len(seq1), m = len(seq2) - off2.
struct RPair {
    uint64_t word1, word2;     // first x4 word of seq1 / of seq2 (chunk0 * 4)
    int32_t n, m, off2;
    int32_t status;            // 0, or VAPOR_E_ARG: the kernel writes d = -1 and this
};

inline bool band_ok(int64_t band) { return band >= 1 && band <= VAPOR_MAX_BAND; }

// slots of a band row: c = j - i + band, 0 .. 2 * band
VAPOR_RA_HD inline int row_slots(int band) { return 2 * band + 1; }
// slots a lane must own so that 64 lanes hold the row: lane l owns c = l * S + s, s = 0 .. S - 1
VAPOR_RA_HD inline int slots_needed(int band) { return (row_slots(band) + LANES - 1) / LANES; }
// ... and the compiled width the band runs at (0: none, the band is out of range)
inline int lane_width(int band)
{
    if (!band_ok(band)) return 0;
    for (int k = 0; k < N_WIDTHS; ++k)
        if (WIDTHS[k] >= slots_needed(band)) return WIDTHS[k];
    return 0;
}

// The key a wave minimum picks a slot of a row by is rank << KEY_SHIFT | c: a slot is below 2^11 (2 * VAPOR_MAX_BAND + 1 slots); the
// rank is a distance (at most the two sequences' lengths, < 2^17) or vapor_trace::end_key (a slot, or at most m + band)
constexpr int KEY_SHIFT = 11;
static_assert(2 * VAPOR_MAX_BAND + 1 <= (1 << KEY_SHIFT), "a slot fits the key");
static_assert(2 * (int64_t)VAPOR_MAX_SEQ_LEN < ((int64_t)1 << (31 - KEY_SHIFT)), "a distance fits the key");
VAPOR_RA_HD inline int row_key(int d, int c) { return d << KEY_SHIFT | c; }
VAPOR_RA_HD inline int key_d(int key) { return key >> KEY_SHIFT; }
VAPOR_RA_HD inline int key_c(int key) { return key & ((1 << KEY_SHIFT) - 1); }

// Rows the kernel walks: behind row m + band + 1 every cell of the band lies past the allele's end, where the free end makes
// every step along a diagonal cost nothing - the row's minimum is the answer and does not change any more.
VAPOR_RA_HD inline int rows_walked(int n, int m, int band)
{
    const int64_t stop = (int64_t)m + band + 1;
    return (int64_t)n < stop ? n : (int)stop;
}

// the status of a pair over a set of n_seqs sequences; len_of(s) is the length of sequence s
template <typename LenOf>
inline int pair_status(const vapor_pair& a, int32_t n_seqs, LenOf len_of)
{
    if (a.seq1 < 0 || a.seq1 >= n_seqs || a.seq2 < 0 || a.seq2 >= n_seqs) return VAPOR_E_ARG;
    const int64_t l1 = len_of(a.seq1), l2 = len_of(a.seq2);
    if (l1 < 0 || l2 < 0 || l1 > VAPOR_MAX_SEQ_LEN || l2 > VAPOR_MAX_SEQ_LEN) return VAPOR_E_ARG;
    if (a.off2 < 0 || (int64_t)a.off2 > l2) return VAPOR_E_ARG;
    return VAPOR_OK;
}

// the record of a pair: chunk_of(s) is the sequence's first 32-symbol chunk in the planes (4 words of x4 each)
template <typename LenOf, typename ChunkOf>
inline RPair pair_record(const vapor_pair& a, int32_t n_seqs, LenOf len_of, ChunkOf chunk_of)
{
    RPair r{0, 0, 0, 0, 0, pair_status(a, n_seqs, len_of)};
    if (r.status) return r;
    r.word1 = (uint64_t)chunk_of(a.seq1) * 4u;
    r.word2 = (uint64_t)chunk_of(a.seq2) * 4u;
    r.n = (int32_t)len_of(a.seq1);
    r.m = (int32_t)len_of(a.seq2) - a.off2;
    r.off2 = a.off2;
    return r;
}

// workgroups of a launch over n_pairs pairs; a call takes at most MAX_PAIRS (its grid and its 8 bytes a pair stay far below 2^31)
constexpr int64_t MAX_PAIRS = (int64_t)1 << 26;
inline int64_t grid_of(int64_t n_pairs) { return (n_pairs + WAVES - 1) / WAVES; }

}  // namespace vapor_realign
