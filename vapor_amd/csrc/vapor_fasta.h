// vapor_fasta.h - reference windows cut out of a bgzipped FASTA on the device (`samtools faidx ref.fa.gz chrom:start-end`,
// ref_seq_readin SF:1203-1217, for every window of a chunk of loci at once).  The host reads the blocks that hold the windows'
// raw bytes (their ranges come from the .fai and .gzi as virtual offsets), bgzf_inflate_kernel (vapor_bamdev.h) inflates each
// distinct block once and checks its CRC-32, and
//
//   fasta_window_kernel   one wavefront per window: the window's raw bytes in the inflated arena, newlines dropped - a kept
//                         byte's place is the count of kept bytes before it, a 64-bit ballot and the lane's mbcnt rank - and,
//                         by the same pass, the window's traits: what fastpath._window_traits and the isascii checks ask.
//
// A window whose blocks did not inflate or failed their check, or that holds a byte of 0x80 or more, gets a non-zero status
// and the caller reads it on the host (seqio.BgzfFasta), which words the errors.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vapor_readrec.h"      // FastaWin and the WIN_* codes

namespace vapor_fasta {

// traits of a window's text
constexpr uint32_t TR_LOWER = 1, TR_NOT_ACGTN = 2, TR_NOT_ACGTN_ANY_CASE = 4, TR_HIGH = 8;

constexpr int WIN_WAVES = 4;    // windows (wavefronts) a workgroup

__device__ __forceinline__ bool is_acgtn(uint32_t c)
{
    return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N';
}

__device__ __forceinline__ uint32_t trait_bits(uint32_t c)
{
    const bool up = is_acgtn(c);
    const bool low = c >= 'a' && c <= 'z';
    const bool low_acgtn = low && is_acgtn(c - 32u);
    return (low ? TR_LOWER : 0u) | (up ? 0u : TR_NOT_ACGTN) | (up || low_acgtn ? 0u : TR_NOT_ACGTN_ANY_CASE) | (c >= 0x80u ? TR_HIGH : 0u);
}

// status[w] holds the host's verdict on entry (range, room); the kernel leaves a non-zero one as it is and writes no text for it
__global__ __launch_bounds__(64 * WIN_WAVES) void fasta_window_kernel(const uint8_t* __restrict__ arena, const FastaWin* __restrict__ wins, int n_wins,
                                                                      const int32_t* __restrict__ blk_status, uint8_t* __restrict__ text,
                                                                      int64_t* __restrict__ text_len, uint8_t* __restrict__ traits,
                                                                      int32_t* __restrict__ status)
{
    const int w = (int)blockIdx.x * WIN_WAVES + (int)(threadIdx.x >> 6);
    if (w >= n_wins) return;
    const uint32_t lane = threadIdx.x & 63u;
    const FastaWin W = wins[w];
    int st = status[w];
    bool bad = false;
    for (uint32_t b = lane; b < W.blk_n; b += 64u) bad |= blk_status[(size_t)W.blk_first + b] != 0;
    if (st == WIN_OK && __any(bad)) st = WIN_BLOCK;
    uint64_t o = 0;
    uint32_t tr = 0;
    if (st == WIN_OK) {
        uint8_t* out = text + W.t_off;
        for (uint64_t base = W.a_beg; base < W.a_end; base += 64u) {
            const uint64_t p = base + lane;
            const uint32_t c = p < W.a_end ? (uint32_t)arena[p] : (uint32_t)'\n';
            const bool keep = c != '\n' && c != '\r';
            const uint64_t m = __ballot(keep);
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (keep) {
                out[o + rank] = (uint8_t)c;
                tr |= trait_bits(c);
            }
            o += (uint64_t)__popcll(m);
        }
        uint32_t all = 0;
        for (uint32_t bit = 1; bit <= TR_HIGH; bit <<= 1)
            if (__any(tr & bit)) all |= bit;
        tr = all;
        if (tr & TR_HIGH) st = WIN_NON_ASCII;
    }
    if (lane == 0) {
        text_len[w] = st == WIN_OK ? (int64_t)o : 0;
        traits[w] = (uint8_t)tr;
        status[w] = st;
    }
}

}  // namespace vapor_fasta
