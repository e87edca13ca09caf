// vapor_band_row.h - the band row that realign_kernel, realign_trace_kernel and junction_rows_kernel walk: the
// banded edit distance of a read against an allele, start anchored, on the sequences' 4-bit plane, a row of the band in the
// registers of one wavefront.
//
// Slot c = j - i + B of row i is cell (i, j); lane l owns the S consecutive slots c = l * S + s.  The row keeps E = D - c:
//   diagonal    D[i-1][j-1] + sub  is the same slot of the row before:   E[c] + sub
//   vertical    D[i-1][j] + 1      is slot c + 1 of the row before:      E[c + 1] + 2   (a one-lane shift at a lane's last slot)
//   horizontal  D[i][j-1] + 1      is slot c - 1 of this row:            E[c - 1]
// so a row is t[c] = min(E[c] + sub, E[c + 1] + 2) and then a prefix minimum of t: serial inside a lane, wave_scan<OpMin> across
// lanes.  A cell left of the allele's start (j < 0) holds INF and keeps it, since all its predecessors do; slot 2B takes no
// vertical step (its addend is INF), and what the slots behind 2B hold feeds nothing in front of them.
// The free end on the last column: the allele is continued behind its end by a symbol that matches everything, at no cost along a
// diagonal.  A path that reaches (i, m) then runs down its slot to the last row for nothing, a path that reaches a cell behind
// column m has crossed the column, so the minimum of the last row over every slot of the band IS min(last row, last column) of
// the rule - no column is tracked and no cell behind the end is masked.
// Symbols: one nibble a slot, one-hot (A C G T = 1 2 4 8 in either case, N / IUPAC / other = 0, behind the end = 15); the read
// symbol of a row is wave-uniform, a bit position p, and slot s mismatches iff bit 4 s + p is clear.  The nibbles of a lane are
// a shift register that moves one slot a row and takes lane l + 1's first nibble; lane 63 takes the allele's next symbol, which is
// wave-uniform too.  RaReader feeds a sequence read forwards a word of eight symbols at a time, one word ahead.
#pragma once

#include "vapor_realign_plan.h"

namespace vapor {

using vapor_realign::RPair;
constexpr int RA_INF = vapor_realign::INF;

// the one-hot nibble of a symbol code: 0 for a code that matches nothing
__device__ __forceinline__ uint32_t ra_onehot(uint32_t code) { return code < 8u ? 1u << (code & 3u) : 0u; }

// the nibble of allele symbol jb (0-based behind off2) of a pair: nothing in front of the start, the wildcard behind the end
__device__ __forceinline__ uint32_t ra_allele_nibble(const uint32_t* __restrict__ x2, int off2, int m, int jb)
{
    if (jb < 0) return 0u;
    if (jb >= m) return 15u;
    const uint32_t q = (uint32_t)(off2 + jb);
    return ra_onehot((x2[q >> 3] >> ((q & 7u) * 4u)) & 15u);
}

// The symbols k0, k0 + 1, .. of the first len symbols of a plane, a word of eight at a time, one word ahead; everything here is
// wave-uniform.  take(k) and nibble(k) must be called with consecutive k from k0 >= 0 on; no word that starts behind the end
// is loaded.
struct RaReader {
    const uint32_t* __restrict__ x;
    int len;
    uint32_t cur, next;

    __device__ __forceinline__ uint32_t word(int k) const { return k * 8 < len ? x[k] : 0u; }
    __device__ __forceinline__ void start(const uint32_t* __restrict__ x_, int len_, int k0)
    {
        x = x_; len = len_;
        cur = word(k0 >> 3);
        next = word((k0 >> 3) + 1);
    }
    __device__ __forceinline__ uint32_t take(int k)
    {
        const uint32_t code = (cur >> ((k & 7) * 4)) & 15u;      // (k < len)
        if ((k & 7) == 7) {
            cur = next;
            next = word((k >> 3) + 2);
        }
        return code;
    }
    // the nibble of symbol k: the wildcard behind the end
    __device__ __forceinline__ uint32_t nibble(int k)
    {
        const uint32_t code = take(k);
        return k < len ? ra_onehot(code) : 15u;
    }
};

// the hooks of a kernel that keeps nothing of a row's steps
struct RaNoHooks {
    __device__ __forceinline__ void slot(int, int, int, int, uint32_t) {}
    __device__ __forceinline__ void carried(int) {}
};

// The row of a lane: E[S], vadd[S] (the vertical step's addend: 2, INF at and behind slot 2B) and the nibble words w[ra_words(S)].
// They are arrays of the kernel, handed to the functions below, which are inlined: the compiler keeps such an array in one run of
// registers and updates it in place, which a member of a struct does not get.
constexpr int ra_words(int S) { return (4 * S + 31) / 32; }

// row 0: D[0][j] = j for 0 <= j <= B, so E = -B at the slots c = B .. 2B; the nibbles of row 1: slot c meets the allele's symbol
// c - B, whose nibble nibble_of(c - B) returns.  c0 is the lane's first slot, lane * S.
template <int S, typename NibbleOf>
__device__ __forceinline__ void ra_row_start(int (&E)[S], int (&vadd)[S], uint32_t (&w)[ra_words(S)], int c0, int B, int W, NibbleOf nibble_of)
{
#pragma unroll
    for (int k = 0; k < ra_words(S); ++k) w[k] = 0u;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int c = c0 + s;
        E[s] = (c >= B && c < W) ? -B : RA_INF;
        vadd[s] = (c + 1 < W) ? 2 : RA_INF;
        w[s >> 3] |= nibble_of(c - B) << ((s & 7) * 4);
    }
}

// One row, for the wave-uniform code ca of the read's symbol.  hooks.slot(s, run, d, v, sub) sees slot s inside the lane: its
// value run, the diagonal's d, the vertical's v and the mismatch bit; hooks.carried(s) is called where what the lanes before
// this one end with is smaller still.
template <int S, typename Hooks>
__device__ __forceinline__ void ra_row_step(int (&E)[S], const int (&vadd)[S], const uint32_t (&w)[ra_words(S)], uint32_t ca, Hooks& hooks)
{
    constexpr int NW = ra_words(S);
    // mismatch bits: bit 4 s of x[s / 8] is set iff slot s does not match (a read symbol outside ACGT matches the wildcard only)
    uint32_t x[NW];
    if (ca < 8u) {
#pragma unroll
        for (int k = 0; k < NW; ++k) x[k] = ~(w[k] >> (ca & 3u));
    } else {
#pragma unroll
        for (int k = 0; k < NW; ++k) x[k] = ~(w[k] & (w[k] >> 1) & (w[k] >> 2) & (w[k] >> 3));
    }
    // t = min(diagonal, vertical) and its prefix minimum inside the lane
    const int vin = dpp_from<0x130, 0xF>(RA_INF, E[0]);              // wave_shl:1 - lane l + 1's first slot (lane 63: none)
    int run = RA_INF;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t sub = (x[s >> 3] >> ((s & 7) * 4)) & 1u;
        const int d = E[s] + (int)sub;
        const int v = (s + 1 < S ? E[s + 1] : vin) + vadd[s];
        run = min(run, min(d, v));
        E[s] = run;
        hooks.slot(s, run, d, v, sub);
    }
    // ... and across the lanes: what the lanes before this one end with
    const int before = dpp_from<0x138, 0xF>(RA_INF, wave_scan<OpMin>(run, RA_INF));     // wave_shr:1 (lane 0: none)
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (before < E[s]) hooks.carried(s);
        E[s] = min(E[s], before);
    }
}

// the nibbles move one slot down; lane 63 takes the nibble nb of the allele's next symbol
template <int S>
__device__ __forceinline__ void ra_row_shift(uint32_t (&w)[ra_words(S)], uint32_t nb)
{
    constexpr int NW = ra_words(S);
    const uint32_t in = (uint32_t)dpp_from<0x130, 0xF>((int)nb, (int)(w[0] & 15u));
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = (w[k] >> 4) | (k + 1 < NW ? w[k + 1] << 28 : 0u);
    w[(S - 1) >> 3] |= in << (((S - 1) & 7) * 4);
}

// this lane's minimum of D = E + c over its slots that are cells of row `rows`: inside the band and at or behind the allele's
// start
template <int S>
__device__ __forceinline__ int ra_row_best(const int (&E)[S], int c0, int rows, int B, int W)
{
    int b = RA_INF;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int c = c0 + s;
        if (c < W && rows + c - B >= 0) b = min(b, E[s] + c);
    }
    return b;
}

}  // namespace vapor
