// vapor_revote.h - the three kernels of vapor_realign_revote: the polished allele of every locus spelt into a 4-bit
// plane on the device, and every read of the locus aligned against it.
//
// They run behind insert_kernel (vapor_polish.h, not edited) on the same stream: the calls, the sites and the inserted text of a
// locus are read where the polish left them in the group's buffer, and the pieces written here lie behind them (vapor_revote_plan.h).
//   spell_kernel           one workgroup a locus, 256 columns a round, in consensus_kernel's shape: a column emits e = the bases of
//                          the site before it + 1 unless it is deleted.  The rank of a flagged column - which slot holds its text -
//                          is a ballot and mbcnt inside a wavefront, four words of LDS across them and a carry across rounds; e
//                          goes through the same scan to start(q).  own[q], the column's own code and the site's text (lane r base
//                          r) are stored one byte a symbol: every symbol has one writer, nothing is atomic.
//   spell_pack_kernel      one workgroup a locus, a lane an x4 word: eight staged bytes to eight nibbles, whole chunks up to plen;
//                          what lies behind stays as the group's clear left it.
//   realign_onto_kernel    realign_kernel (vapor_realign.h) with x2 the polished plane and off2' = own[off2]; the row is
//                          vapor_band_row.h's, untouched.
// What the polish wrote is data: a site's slot and its length are clamped, every store is held inside the locus's pieces.
#pragma once

#include "vapor_polish.h"
#include "vapor_revote_plan.h"

namespace vapor {

using vapor_revote::VLocus;
using vapor_revote::VPair;

__global__ __launch_bounds__(CONSENSUS_THREADS) void spell_kernel(const uint32_t* __restrict__ x4, const PLocus* __restrict__ loci,
                                                                  const VLocus* __restrict__ vloci, const uint8_t* __restrict__ calls,
                                                                  const int32_t* __restrict__ sites, const uint8_t* __restrict__ ins,
                                                                  uint32_t* __restrict__ buf, int32_t* __restrict__ lout)
{
    namespace pp = vapor_polish;
    namespace rv = vapor_revote;
    __shared__ int wave_flags[CONSENSUS_THREADS / 64], wave_emits[CONSENSUS_THREADS / 64];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PLocus lc = loci[g];
    const VLocus vl = vloci[g];
    int32_t* __restrict__ lo = lout + rv::LOUT * g;
    if (vl.status != 0) {
        if (tid < rv::LOUT) lo[tid] = tid == rv::L_STATUS ? vl.status : 0;
        return;
    }
    const uint32_t* __restrict__ x2 = x4 + vl.word2;
    int32_t* __restrict__ own = reinterpret_cast<int32_t*>(buf + vl.own_off);
    uint8_t* __restrict__ stage = reinterpret_cast<uint8_t*>(buf + vl.stage_off);
    const uint8_t* __restrict__ cl = calls + lc.col0;
    const int32_t* __restrict__ st = sites + (size_t)2 * pp::MAX_SITES * g;
    const uint8_t* __restrict__ tx = ins + (size_t)pp::MAX_SITES * pp::RMAX * g;
    int n_flags = 0, n_emits = 0;                                     // flagged columns / symbols before this round (uniform)
    for (int c0 = 0; c0 < lc.len; c0 += CONSENSUS_THREADS) {         // (uniform bounds: every thread reaches the barriers)
        const int c = c0 + tid;
        int call = pp::CALL_DELETE;
        bool flagged = false;
        if (c < lc.len) {
            const int v = cl[c];
            flagged = (v & pp::SITE_BIT) != 0;
            call = v & 7;
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(flagged);
        if (lane == 0) wave_flags[wave] = __builtin_popcountll(m);
        __syncthreads();
        int k = n_flags + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)), all_flags = 0;
#pragma unroll
        for (int w = 0; w < CONSENSUS_THREADS / 64; ++w) {
            const int v = wave_flags[w];
            if (w < wave) k += v;
            all_flags += v;
        }
        int nb = 0;
        if (flagged && k < pp::MAX_SITES) {
            nb = st[2 * k + 1];
            nb = nb < 0 ? 0 : nb > pp::RMAX ? pp::RMAX : nb;
        }
        const int emits = call <= pp::CALL_KEEP ? 1 : 0;             // (a column behind the end was given DELETE: nothing)
        const int e = nb + emits;
        const int incl = wave_scan<OpAdd>(e, 0);
        if (lane == 63) wave_emits[wave] = incl;
        __syncthreads();
        int start = n_emits + incl - e, all_emits = 0;
#pragma unroll
        for (int w = 0; w < CONSENSUS_THREADS / 64; ++w) {
            const int v = wave_emits[w];
            if (w < wave) start += v;
            all_emits += v;
        }
        if (c < lc.len) {
            const int at = start + nb;
            own[c] = at;
            if (emits && at < vl.cap) stage[at] = (uint8_t)(call == pp::CALL_KEEP ? pl_nibble(x2, c) : (uint32_t)call);
        }
        // the texts of this wavefront's sites, one after the other, lane r base r ("ACGT" to 0 .. 3)
        unsigned long long todo = __builtin_amdgcn_ballot_w64(nb > 0);
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int s0 = __shfl(start, l), n = __shfl(nb, l), slot = __shfl(k, l);
            if (lane < n && s0 + lane < vl.cap) {
                const uint32_t x = ((uint32_t)tx[(size_t)slot * pp::RMAX + lane] >> 1) & 3u;      // A C G T: 0 1 3 2
                stage[s0 + lane] = (uint8_t)(x ^ (x >> 1));
            }
        }
        n_flags += all_flags;
        n_emits += all_emits;
    }
    if (tid == 0) {
        own[lc.len] = n_emits;
        lo[rv::L_STATUS] = (n_emits > VAPOR_MAX_SEQ_LEN || vl.short_slot) ? VAPOR_E_ARG : 0;
        lo[rv::L_PLEN] = n_emits;
        lo[2] = 0;
        lo[3] = 0;
    }
}

__global__ __launch_bounds__(CONSENSUS_THREADS) void spell_pack_kernel(const VLocus* __restrict__ vloci, uint32_t* __restrict__ buf,
                                                                       const int32_t* __restrict__ lout)
{
    namespace rv = vapor_revote;
    const int g = (int)blockIdx.x;
    const VLocus vl = vloci[g];
    if (vl.status != 0) return;
    int plen = lout[rv::LOUT * g + rv::L_PLEN];
    if (plen > vl.cap) plen = vl.cap;
    const uint2* __restrict__ stage = reinterpret_cast<const uint2*>(buf + vl.stage_off);
    uint32_t* __restrict__ plane = buf + vl.plane_off;
    const int n_words = 4 * ((plen + 31) / 32);                       // (whole chunks: inside both pieces, which hold whole chunks of cap)
    for (int w = (int)threadIdx.x; w < n_words; w += CONSENSUS_THREADS) {
        const uint2 v = stage[w];
        const uint32_t lo = (v.x & 15u) | ((v.x >> 4) & 0xF0u) | ((v.x >> 8) & 0xF00u) | ((v.x >> 12) & 0xF000u);
        const uint32_t hi = (v.y & 15u) | ((v.y >> 4) & 0xF0u) | ((v.y >> 8) & 0xF00u) | ((v.y >> 12) & 0xF000u);
        plane[w] = lo | hi << 16;
    }
}

template <int S>
__global__ __launch_bounds__(64 * vapor_realign::WAVES) void realign_onto_kernel(const uint32_t* __restrict__ x4, const VPair* __restrict__ votes,
                                                                                 const VLocus* __restrict__ vloci, const uint32_t* __restrict__ buf,
                                                                                 const int32_t* __restrict__ lout, long long n_votes, int band,
                                                                                 int32_t* __restrict__ out)
{
    namespace rv = vapor_revote;
    const int lane = (int)(threadIdx.x & 63u);
    const long long t = (long long)blockIdx.x * vapor_realign::WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (t >= n_votes) return;                              // (a whole wavefront: the cross-lane steps below need all 64 lanes)
    const VPair p = votes[t];
    int32_t* __restrict__ o = out + rv::VOUT * t;
    const int status = p.status != 0 ? p.status : lout[rv::LOUT * p.locus + rv::L_STATUS];
    if (status != 0) {
        if (lane == 0) { o[rv::V_D] = -1; o[rv::V_STATUS] = status; o[rv::V_OFF2] = 0; o[rv::V_M] = 0; }
        return;
    }
    const VLocus vl = vloci[p.locus];
    const int plen = __builtin_amdgcn_readfirstlane(lout[rv::LOUT * p.locus + rv::L_PLEN]);
    const int off2 = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int32_t*>(buf + vl.own_off)[p.off2]);
    const uint32_t* __restrict__ x1 = x4 + p.word1;
    const uint32_t* __restrict__ x2 = buf + vl.plane_off;
    const int n = p.n, m = plen - off2, B = band, W = vapor_realign::row_slots(band);
    const int rows = vapor_realign::rows_walked(n, m, B);
    const int c0 = lane * S;
    int E[S], vadd[S];
    uint32_t w[ra_words(S)];
    ra_row_start<S>(E, vadd, w, c0, B, W, [&](int jb) { return ra_allele_nibble(x2, off2, m, jb); });
    RaReader r1, r2;
    const int q0 = off2 + 64 * S - B;
    r1.start(x1, n, 0);
    r2.start(x2, off2 + m, q0);
    RaNoHooks none;
    for (int ia = 0; ia < rows; ++ia) {
        ra_row_step<S>(E, vadd, w, r1.take(ia), none);
        ra_row_shift<S>(w, r2.nibble(q0 + ia));
    }
    const int best = wave_scan<OpMin>(ra_row_best<S>(E, c0, rows, B, W), RA_INF);
    if (lane == 63) { o[rv::V_D] = best; o[rv::V_STATUS] = 0; o[rv::V_OFF2] = off2; o[rv::V_M] = m; }
}

}  // namespace vapor
