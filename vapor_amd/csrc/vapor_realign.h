// vapor_realign.h - realign_kernel: the banded edit distance of a read against an allele, start anchored at the
// window start, both ends free, on the sequences' 4-bit plane.  One wavefront a pair; the row, its E = D - c arithmetic, the free
// end and the one-hot nibbles are vapor_band_row.h's.  Here: which pair, and the minimum of the last row walked.
#pragma once

#include "vapor_band_row.h"

namespace vapor {

template <int S>
__global__ __launch_bounds__(64 * vapor_realign::WAVES) void realign_kernel(const uint32_t* __restrict__ x4, const RPair* __restrict__ pairs,
                                                                            long long n_pairs, int band, int32_t* __restrict__ out)
{
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
    const int rows = vapor_realign::rows_walked(n, m, B);
    const int c0 = lane * S;
    int E[S], vadd[S];
    uint32_t w[ra_words(S)];
    ra_row_start<S>(E, vadd, w, c0, B, W, [&](int jb) { return ra_allele_nibble(x2, off2, m, jb); });
    // the read's symbol i - 1 for row i; the allele's symbol that enters at lane 63's last slot for row i + 1,
    // jb = i + 64 S - B - 1 (never negative: 64 S >= 2B + 1)
    RaReader r1, r2;
    const int q0 = off2 + 64 * S - B;
    r1.start(x1, n, 0);
    r2.start(x2, off2 + m, q0);
    RaNoHooks none;
    for (int ia = 0; ia < rows; ++ia) {
        ra_row_step<S>(E, vadd, w, r1.take(ia), none);
        ra_row_shift<S>(w, r2.nibble(q0 + ia));
    }

    // the minimum of the last row walked, over the slots of the band that lie at or behind the allele's start
    const int best = wave_scan<OpMin>(ra_row_best<S>(E, c0, rows, B, W), RA_INF);
    if (lane == 63) { out[2 * t] = best; out[2 * t + 1] = 0; }
}

}  // namespace vapor
