// vapor_polish.h - the four kernels of vapor_realign_polish: the traces of a locus's pairs stacked on the alt
// allele column by column, and the allele the reads carry, by a rule of integer comparisons.
//
// They run behind realign_trace_kernel and traceback_kernel (vapor_realign_trace.h, not edited) on the same stream; the runs stay
// in device memory.  All four index a group's tables by vapor_polish_plan.h's layout.
//   pileup_kernel       one wavefront a pair: walks the pair's runs with (i, j) wave-uniform.  A run of '=' / 'X' or of 'D' is taken
//                       64 columns a step, lane k the column of step k: one atomicAdd on the uint32 counter of the read's base (or
//                       of Dl) and one on bcov, on 64 consecutive column records.  An 'I' run is one add by lane 0.
//   consensus_kernel    one workgroup a locus, 256 columns a round: the column's call, its site flag, the sites numbered in column
//                       order by a block scan (ballots inside a wavefront, four words of LDS across them), the statistics.
//   pileup_ins_kernel   the walk again, 'I' runs only: where the run's column is a kept site, lane r adds for inserted base r.
//   insert_kernel       one wavefront a site slot, lane r position r: emits while 2 * tot > bcov - a ballot, and the count of its
//                       trailing ones.
// Integer adds commute: the counters are exact whatever the order.  A run word is data: every column is checked against the
// locus's length, every read symbol against the read's, before anything is touched.
#pragma once

#include "vapor_polish_plan.h"

namespace vapor {

using vapor_polish::PLocus;

__device__ __forceinline__ uint32_t pl_nibble(const uint32_t* __restrict__ x, int q) { return (x[q >> 3] >> ((q & 7) * 4)) & 15u; }

// what both walks need of a pair: false for a pair that is not walked
struct PolishPair {
    const uint32_t* x1;
    const uint32_t* slot;      // the pair's runs in path order
    int n, off2, n_runs, lead, j_end, len;
    long long col0;
    int locus;
};

__device__ __forceinline__ bool polish_pair(const uint32_t* __restrict__ x4, const RPair* __restrict__ pairs, const int32_t* __restrict__ pair_locus,
                                            const PLocus* __restrict__ loci, const int32_t* __restrict__ head, const uint32_t* __restrict__ runs,
                                            int cap_runs, long long t, PolishPair& q)
{
    const RPair p = pairs[t];
    const int32_t* __restrict__ h = head + vapor_trace::HEAD * t;
    if (p.status != 0 || h[vapor_trace::H_STATUS] != 0) return false;
    q.locus = __builtin_amdgcn_readfirstlane(pair_locus[t]);
    const PLocus lc = loci[q.locus];
    if (lc.status != 0) return false;
    int k = __builtin_amdgcn_readfirstlane(h[vapor_trace::H_N_RUNS]);
    if (k < 0) k = 0;
    if (k > cap_runs) k = cap_runs;
    q.n_runs = k;
    q.slot = runs + (size_t)t * (size_t)cap_runs + (size_t)(cap_runs - k);
    q.x1 = x4 + p.word1;
    q.n = p.n;
    q.off2 = p.off2;
    q.j_end = __builtin_amdgcn_readfirstlane(h[vapor_trace::H_J_END]);
    q.len = lc.len;
    q.col0 = lc.col0;
    q.lead = 0;
    if (k > 0) {
        const uint32_t w = q.slot[0];
        if ((w & 3u) == (uint32_t)vapor_trace::OP_D) q.lead = (int)(w >> 2);
    }
    return true;
}

__global__ __launch_bounds__(64 * vapor_realign::WAVES) void pileup_kernel(const uint32_t* __restrict__ x4, const RPair* __restrict__ pairs,
                                                                           const int32_t* __restrict__ pair_locus, const PLocus* __restrict__ loci,
                                                                           long long count, const int32_t* __restrict__ head,
                                                                           const uint32_t* __restrict__ runs, int cap_runs, uint32_t* __restrict__ counts)
{
    namespace pp = vapor_polish;
    const int lane = (int)(threadIdx.x & 63u);
    const long long t = (long long)blockIdx.x * vapor_realign::WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (t >= count) return;
    PolishPair q;
    if (!polish_pair(x4, pairs, pair_locus, loci, head, runs, cap_runs, t, q)) return;
    uint32_t* __restrict__ cnt = counts + pp::COUNTERS * q.col0;
    const long long first_col = (long long)q.off2 + q.lead, end_col = (long long)q.off2 + q.j_end;
    long long i = 0, j = 0;
    for (int r = 0; r < q.n_runs; ++r) {
        const uint32_t w = q.slot[r];
        const uint32_t op = w & 3u;
        const long long L = (long long)(w >> 2);
        if (op == (uint32_t)vapor_trace::OP_I) {
            const long long c = q.off2 + j;
            if (lane == 0 && c > first_col && c < end_col && c < q.len) atomicAdd(&cnt[pp::COUNTERS * c + pp::C_INS], 1u);
            i += L;
            continue;
        }
        if (op == (uint32_t)vapor_trace::OP_D && r == 0) {       // the leading run: the read starts that far behind the allele's start
            j += L;
            continue;
        }
        for (long long k0 = 0; k0 < L && q.off2 + j + k0 < q.len; k0 += 64) {      // (no step behind the locus's last column)
            const long long k = k0 + lane;
            const long long c = q.off2 + j + k;
            if (k < L && c >= 0 && c < q.len) {
                int which = pp::C_DL;
                if (op != (uint32_t)vapor_trace::OP_D) {
                    const long long s = i + k;
                    const uint32_t code = s < q.n ? pl_nibble(q.x1, (int)s) : 15u;
                    which = code < 8u ? (int)(code & 3u) : pp::C_O;
                }
                atomicAdd(&cnt[pp::COUNTERS * c + which], 1u);
                if (c != first_col) atomicAdd(&cnt[pp::COUNTERS * c + pp::C_BCOV], 1u);
            }
        }
        j += L;
        if (op != (uint32_t)vapor_trace::OP_D) i += L;
    }
}

constexpr int CONSENSUS_THREADS = 256;

__global__ __launch_bounds__(CONSENSUS_THREADS) void consensus_kernel(const uint32_t* __restrict__ x4, const PLocus* __restrict__ loci,
                                                                      const uint32_t* __restrict__ counts, uint32_t* __restrict__ site_slot,
                                                                      uint8_t* __restrict__ calls, int32_t* __restrict__ stats,
                                                                      int32_t* __restrict__ sites)
{
    namespace pp = vapor_polish;
    __shared__ int wave_sites[CONSENSUS_THREADS / 64];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PLocus lc = loci[g];
    int32_t* __restrict__ st = stats + pp::STATS * g;
    if (lc.status != 0) {
        if (tid < pp::STATS) st[tid] = tid == pp::S_STATUS ? lc.status : 0;
        for (int c = tid; c < lc.len; c += CONSENSUS_THREADS) calls[lc.col0 + c] = (uint8_t)pp::CALL_KEEP;
        return;
    }
    const uint32_t* __restrict__ x2 = x4 + lc.word2;
    const uint32_t* __restrict__ cnt = counts + pp::COUNTERS * lc.col0;
    int pcov = 0, psub = 0, pdel = 0;
    int n_sites = 0;                                                  // sites of the columns before this round (uniform)
    for (int c0 = 0; c0 < lc.len; c0 += CONSENSUS_THREADS) {         // (uniform bounds: every thread reaches the barriers)
        const int c = c0 + tid;
        int call = pp::CALL_KEEP;
        bool site = false;
        if (c < lc.len) {
            const uint4 lo = *reinterpret_cast<const uint4*>(cnt + (size_t)pp::COUNTERS * c);
            const uint4 hi = *reinterpret_cast<const uint4*>(cnt + (size_t)pp::COUNTERS * c + 4);
            const uint32_t cov = lo.x + lo.y + lo.z + lo.w + hi.x + hi.y;
            if (cov >= (uint32_t)pp::MIN_COV) {
                ++pcov;
                uint32_t best = lo.x;
                int arg = 0;
                if (lo.y > best) { best = lo.y; arg = 1; }
                if (lo.z > best) { best = lo.z; arg = 2; }
                if (lo.w > best) { best = lo.w; arg = 3; }
                if (hi.y > best) { best = hi.y; arg = pp::CALL_DELETE; }
                if (2u * best > cov) {
                    const uint32_t code = pl_nibble(x2, c);
                    if (arg == pp::CALL_DELETE) { call = pp::CALL_DELETE; ++pdel; }
                    else if (!(code < 8u && (int)(code & 3u) == arg)) { call = arg; ++psub; }
                }
            }
            site = c >= 1 && hi.z >= (uint32_t)pp::MIN_COV && 2u * hi.w > hi.z;
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(site);
        if (lane == 0) wave_sites[wave] = __builtin_popcountll(m);
        __syncthreads();
        int before = n_sites, all = 0;
#pragma unroll
        for (int k = 0; k < CONSENSUS_THREADS / 64; ++k) {
            const int v = wave_sites[k];
            if (k < wave) before += v;
            all += v;
        }
        __syncthreads();
        if (site) {
            const int num = before + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (num < pp::MAX_SITES) {
                call |= pp::SITE_BIT;
                site_slot[lc.col0 + c] = (uint32_t)num + 1u;
                sites[(size_t)2 * pp::MAX_SITES * g + 2 * num] = c;
            }
        }
        if (c < lc.len) calls[lc.col0 + c] = (uint8_t)call;
        n_sites += all;
    }
    pcov = wave_sum_i32(pcov);
    psub = wave_sum_i32(psub);
    pdel = wave_sum_i32(pdel);
    if (lane == 0) {                                                  // (the statistics start at zero: the group's tables are cleared)
        atomicAdd(&st[pp::S_PCOV], pcov);
        atomicAdd(&st[pp::S_PSUB], psub);
        atomicAdd(&st[pp::S_PDEL], pdel);
    }
    if (tid == 0) {
        st[pp::S_STATUS] = 0;
        st[pp::S_PAIRS] = lc.n_pairs;
        st[pp::S_SITES] = n_sites < pp::MAX_SITES ? n_sites : pp::MAX_SITES;
        st[pp::S_DROPPED] = n_sites < pp::MAX_SITES ? 0 : n_sites - pp::MAX_SITES;
    }
}

__global__ __launch_bounds__(64 * vapor_realign::WAVES) void pileup_ins_kernel(const uint32_t* __restrict__ x4, const RPair* __restrict__ pairs,
                                                                               const int32_t* __restrict__ pair_locus,
                                                                               const PLocus* __restrict__ loci, long long count,
                                                                               const int32_t* __restrict__ head, const uint32_t* __restrict__ runs,
                                                                               int cap_runs, const uint32_t* __restrict__ site_slot,
                                                                               uint32_t* __restrict__ insb)
{
    namespace pp = vapor_polish;
    const int lane = (int)(threadIdx.x & 63u);
    const long long t = (long long)blockIdx.x * vapor_realign::WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (t >= count) return;
    PolishPair q;
    if (!polish_pair(x4, pairs, pair_locus, loci, head, runs, cap_runs, t, q)) return;
    uint32_t* __restrict__ mine = insb + (size_t)pp::INSB_WORDS * q.locus;
    const long long first_col = (long long)q.off2 + q.lead, end_col = (long long)q.off2 + q.j_end;
    long long i = 0, j = 0;
    for (int r = 0; r < q.n_runs; ++r) {
        const uint32_t w = q.slot[r];
        const uint32_t op = w & 3u;
        const long long L = (long long)(w >> 2);
        if (op != (uint32_t)vapor_trace::OP_I) {
            j += L;
            if (op != (uint32_t)vapor_trace::OP_D) i += L;
            continue;
        }
        const long long c = q.off2 + j;
        if (c > first_col && c < end_col && c < q.len) {
            const uint32_t s = site_slot[q.col0 + c];                 // (wave-uniform)
            const long long at = i + lane;
            if (s != 0u && lane < pp::RMAX && (long long)lane < L && at < q.n) {
                const uint32_t code = pl_nibble(q.x1, (int)at);
                if (code < 8u) atomicAdd(&mine[((size_t)(s - 1u) * pp::RMAX + lane) * 4 + (code & 3u)], 1u);
            }
        }
        i += L;
    }
}

__global__ __launch_bounds__(64 * vapor_realign::WAVES) void insert_kernel(const PLocus* __restrict__ loci, long long n_slots,
                                                                           const uint32_t* __restrict__ counts, const uint32_t* __restrict__ insb,
                                                                           int32_t* __restrict__ stats, int32_t* __restrict__ sites,
                                                                           uint8_t* __restrict__ ins)
{
    namespace pp = vapor_polish;
    static_assert(pp::RMAX == 64, "one lane an inserted base");
    const int lane = (int)(threadIdx.x & 63u);
    const long long w = (long long)blockIdx.x * vapor_realign::WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= n_slots) return;
    const int g = (int)(w / pp::MAX_SITES), slot = (int)(w % pp::MAX_SITES);
    int32_t* __restrict__ st = stats + pp::STATS * g;
    const PLocus lc = loci[g];
    if (lc.status != 0 || slot >= st[pp::S_SITES]) return;
    int32_t* __restrict__ site = sites + (size_t)2 * pp::MAX_SITES * g + 2 * slot;
    const int c = site[0];
    if (c < 0 || c >= lc.len) return;
    const uint32_t bcov = counts[pp::COUNTERS * (lc.col0 + c) + pp::C_BCOV];
    const uint4 v = *reinterpret_cast<const uint4*>(insb + ((size_t)pp::INSB_WORDS * g + ((size_t)slot * pp::RMAX + lane) * 4));
    const uint32_t tot = v.x + v.y + v.z + v.w;
    uint32_t best = v.x;
    int arg = 0;
    if (v.y > best) { best = v.y; arg = 1; }                          // (the smallest code on a tie)
    if (v.z > best) { best = v.z; arg = 2; }
    if (v.w > best) { best = v.w; arg = 3; }
    const unsigned long long emit = __builtin_amdgcn_ballot_w64(2u * tot > bcov);
    const int nb = ~emit ? __builtin_ctzll(~emit) : 64;               // trailing ones: up to the first position that does not emit
    if (lane < nb) ins[((size_t)pp::MAX_SITES * g + slot) * pp::RMAX + lane] = (uint8_t)((0x54474341u >> (8 * arg)) & 255u);   // "ACGT"[arg]
    if (lane == 0) {
        site[1] = nb;
        atomicAdd(&st[pp::S_PINS], nb);
    }
}

}  // namespace vapor
