// vapor_refine.h - breakpoint refinement (`--refine`): the choice among the candidate breakpoints of a locus on the device.
//
//   grid_pick_kernel  one wavefront per refined locus ("group"): the finish kernel's records of its candidates -> the winner
//                     (vapor_amd/refine.py: pick), the winner's and candidate 0's records, the winner's per-read scores
//
// A group's candidates are consecutive "loci" of a plan (vapor_plan_set_grid); finish_kernel has written eight doubles per
// candidate and one score per (candidate, read).  Only what this kernel gathers crosses the link.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vapor {

#define VAPOR_MAX_CANDIDATES 128   // one wavefront holds a group with two candidates per lane

// A double as a key that orders like the number: NaN lowest (it never beats a number: `nan > x` is false in
// vapor_amd/finish.py's tests as well), -0.0 as 0.0, the rest by value.
__device__ __forceinline__ unsigned long long pick_key(double v)
{
    if (v != v) return 0ULL;
    if (v == 0.0) v = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

struct PickCand {
    unsigned long long gs, qs;     // pick_key of GS and QS; 0 for a candidate that is not eligible
    int elig, idx;
};

// eligible first, then the larger GS, then the larger QS, then the lower index
__device__ __forceinline__ bool pick_better(const PickCand& a, const PickCand& b)
{
    if (a.elig != b.elig) return a.elig > b.elig;
    if (a.gs != b.gs) return a.gs > b.gs;
    if (a.qs != b.qs) return a.qs > b.qs;
    return a.idx < b.idx;
}

__device__ __forceinline__ unsigned long long pick_shfl_xor(unsigned long long v, int m)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// loci: the finish kernel's records (8 doubles per candidate); first_locus[g] .. first_locus[g + 1]: the candidates of group g
// (1 .. VAPOR_MAX_CANDIDATES of them, checked by vapor_plan_set_grid); locus_first / read_scores: the finish kernel's read ranges
// and scores; score_off[g] .. score_off[g + 1]: the group's slots of winner_scores (the read count every candidate of the group has).
// Records and scores are moved as 64-bit words, so that a NaN arrives as it was written.
__global__ __launch_bounds__(64) void grid_pick_kernel(const double* __restrict__ loci, const int32_t* __restrict__ first_locus,
                                                       const int32_t* __restrict__ locus_first, const double* __restrict__ read_scores,
                                                       const int32_t* __restrict__ score_off, int32_t* __restrict__ winner_idx,
                                                       double* __restrict__ group_out, double* __restrict__ winner_scores)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    const int c0 = first_locus[g];
    const int n = min(first_locus[g + 1] - c0, VAPOR_MAX_CANDIDATES);
    if (n <= 0) return;
    const double n0 = loci[8LL * c0 + 4];
    PickCand best;
    best.elig = 0; best.gs = 0; best.qs = 0; best.idx = 2 * VAPOR_MAX_CANDIDATES;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = lane + 64 * h;
        if (t < n) {
            const double* r = loci + 8LL * (c0 + t);
            const double ns = r[4];
            PickCand c;
            c.elig = (ns > 0.0 && ns >= n0) ? 1 : 0;
            c.gs = c.elig ? pick_key(r[1]) : 0ULL;
            c.qs = c.elig ? pick_key(r[0]) : 0ULL;
            c.idx = t;
            if (pick_better(c, best)) best = c;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        PickCand o;
        o.gs = pick_shfl_xor(best.gs, m);
        o.qs = pick_shfl_xor(best.qs, m);
        o.elig = __shfl_xor(best.elig, m, 64);
        o.idx = __shfl_xor(best.idx, m, 64);
        if (pick_better(o, best)) best = o;
    }
    const int w = best.idx;                   // (uniform: every lane holds the wavefront's best; candidate 0 when none is eligible)
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(loci);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(group_out) + 16LL * g;
    if (lane < 8) dst[lane] = src[8LL * (c0 + w) + lane];
    else if (lane < 16) dst[lane] = src[8LL * c0 + (lane - 8)];
    if (lane == 0) winner_idx[g] = w;
    const int r0 = locus_first[c0 + w];
    const int cnt = min(locus_first[c0 + w + 1] - r0, score_off[g + 1] - score_off[g]);
    const unsigned long long* sc = reinterpret_cast<const unsigned long long*>(read_scores);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(winner_scores) + score_off[g];
    for (int t = lane; t < cnt; t += 64) out[t] = sc[r0 + t];
}

}  // namespace vapor
