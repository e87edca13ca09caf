// vapor_realign.h - realign_kernel: the banded edit distance of a read against an allele, start anchored at the
// window start, both ends free, on the sequences' 4-bit plane.  One wavefront a pair, a row of the band in registers.
//
// Slot c = j - i + B of row i is cell (i, j); lane l owns the S consecutive slots c = l * S + s.  The kernel keeps E = D - c:
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
// wave-uniform too.  Both sequences are read a word of eight symbols at a time, one word ahead.
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

template <int S>
__global__ __launch_bounds__(64 * vapor_realign::WAVES) void realign_kernel(const uint32_t* __restrict__ x4, const RPair* __restrict__ pairs,
                                                                            long long n_pairs, int band, int32_t* __restrict__ out)
{
    constexpr int NW = (4 * S + 31) / 32;                  // words of a lane's nibbles
    const int lane = (int)(threadIdx.x & 63u);
    const long long t = (long long)blockIdx.x * vapor_realign::WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (t >= n_pairs) return;                              // (a whole wavefront: the cross-lane steps below need all 64 lanes)
    const RPair p = pairs[t];
    if (p.status != 0) {
        if (lane == 0) { out[2 * t] = -1; out[2 * t + 1] = p.status; }
        return;
    }
    const uint32_t* __restrict__ x1 = x4 + p.word1;
    const uint32_t* __restrict__ x2 = x4 + p.word2;
    const int n = p.n, m = p.m, off2 = p.off2, B = band, W = vapor_realign::row_slots(band);
    const int len2 = off2 + m;
    const int rows = vapor_realign::rows_walked(n, m, B);
    const int c0 = lane * S;

    // row 0: D[0][j] = j for 0 <= j <= B, so E = -B at the slots c = B .. 2B; the nibbles of row 1: slot c meets b[c - B]
    int E[S], vadd[S];
    uint32_t w[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = 0u;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int c = c0 + s;
        E[s] = (c >= B && c < W) ? -B : RA_INF;
        vadd[s] = (c + 1 < W) ? 2 : RA_INF;
        w[s >> 3] |= ra_allele_nibble(x2, off2, m, c - B) << ((s & 7) * 4);
    }

    // the words of the two sequences, one ahead: the read's symbol i - 1 for row i; the allele's symbol that enters at lane 63's
    // last slot for row i + 1, jb = i + 64 S - B - 1 (never negative: 64 S >= 2B + 1)
    uint32_t rw = 0u, rnext = n > 0 ? x1[0] : 0u;
    const int q0 = off2 + 64 * S - B;
    uint32_t bw = (q0 >> 3) * 8 < len2 ? x2[q0 >> 3] : 0u;
    uint32_t bnext = ((q0 >> 3) + 1) * 8 < len2 ? x2[(q0 >> 3) + 1] : 0u;

    for (int i = 1; i <= rows; ++i) {
        const int ia = i - 1;
        if ((ia & 7) == 0) {
            rw = rnext;
            const int nx = (ia >> 3) + 1;
            rnext = nx * 8 < n ? x1[nx] : 0u;
        }
        const uint32_t ca = (rw >> ((ia & 7) * 4)) & 15u;
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
            const int d = E[s] + (int)((x[s >> 3] >> ((s & 7) * 4)) & 1u);
            const int v = (s + 1 < S ? E[s + 1] : vin) + vadd[s];
            run = min(run, min(d, v));
            E[s] = run;
        }
        // ... and across the lanes: what the lanes before this one end with
        const int before = dpp_from<0x138, 0xF>(RA_INF, wave_scan<OpMin>(run, RA_INF));     // wave_shr:1 (lane 0: none)
#pragma unroll
        for (int s = 0; s < S; ++s) E[s] = min(E[s], before);
        // the nibbles move one slot down; lane 63 takes the allele's next symbol
        const int q = q0 + ia;
        const uint32_t nb = q - off2 < m ? ra_onehot((bw >> ((q & 7) * 4)) & 15u) : 15u;
        if ((q & 7) == 7) {
            bw = bnext;
            const int nx = (q >> 3) + 2;
            bnext = nx * 8 < len2 ? x2[nx] : 0u;
        }
        const uint32_t in = (uint32_t)dpp_from<0x130, 0xF>((int)nb, (int)(w[0] & 15u));
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = (w[k] >> 4) | (k + 1 < NW ? w[k + 1] << 28 : 0u);
        w[(S - 1) >> 3] |= in << (((S - 1) & 7) * 4);
    }

    // the minimum of the last row walked, over the slots of the band that lie at or behind the allele's start
    int best = RA_INF;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int c = c0 + s;
        if (c < W && rows + c - B >= 0) best = min(best, E[s] + c);
    }
    best = wave_scan<OpMin>(best, RA_INF);
    if (lane == 63) { out[2 * t] = best; out[2 * t + 1] = 0; }
}

}  // namespace vapor
