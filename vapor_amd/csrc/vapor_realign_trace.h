// vapor_realign_trace.h - the two kernels of vapor_realign_trace: the alignment behind realign_kernel's distance.
//
// realign_trace_kernel<S> walks realign_kernel<S>'s rows (vapor_band_row.h) and keeps two bits per slot and row through the row's
// hooks, the move the rule takes out of that cell:
//   0 '='  1 'X'   the diagonal predecessor, E' == E[c] + sub of the row before (the sub bit tells the two apart)
//   2 'I'          otherwise the vertical predecessor, E' == E[c + 1] + 2 of the row before
//   3 'D'          otherwise the horizontal predecessor: E' came out of the prefix minimum
// E' is the slot's value after the prefix minimum.  Inside the lane the running minimum already is E' unless what the lanes
// before end with is strictly smaller, and then the move is horizontal: the codes are taken in the slot loop and the lanes'
// carry only overwrites them with 3.  A lane packs its S codes into words_of(S) dwords and stores them lane-contiguously, a row
// of a pair one 256-byte line (two at S = 17); plain vector stores.  Behind the last row it picks the end slot by
// vapor_trace::end_key and writes the pair's head.
//
// traceback_kernel<S> runs behind it on the same stream, one wavefront a pair, from the end cell back to (0, 0).  A step of the
// walk fetches three things at once, lane k its own: the codes of rows i - k in the same slot (a diagonal stretch), of rows
// i - k in slots c + k (a vertical stretch) and of slots c - k in row i (a horizontal stretch).  The code at k = 0 says which of
// the three holds, a ballot how far it holds: one round trip for up to 64 cells of the path.  The runs are wave-uniform
// (ballots and scalar arithmetic); lane 0 stores them from the back of the pair's slot, and n_runs counts on past cap_runs.
#pragma once

#include "vapor_band_row.h"
#include "vapor_trace_plan.h"

namespace vapor {

// the hooks of a row that records its moves: TW words of 2-bit codes, slot s at bits 2 (s & 15) of word s / 16
template <int TW>
struct TraceMoves {
    uint32_t mv[TW] = {};
    __device__ __forceinline__ void slot(int s, int run, int d, int v, uint32_t sub)
    {
        const uint32_t code = run == d ? sub : run == v ? (uint32_t)vapor_trace::OP_I : (uint32_t)vapor_trace::OP_D;
        mv[s >> 4] |= code << ((s & 15) * 2);
    }
    __device__ __forceinline__ void carried(int s) { mv[s >> 4] |= 3u << ((s & 15) * 2); }
};

template <int S>
__global__ __launch_bounds__(64 * vapor_realign::WAVES) void realign_trace_kernel(const uint32_t* __restrict__ x4, const RPair* __restrict__ pairs,
                                                                                  const uint64_t* __restrict__ ws_off, long long t0, long long count,
                                                                                  int band, uint32_t* __restrict__ ws, int32_t* __restrict__ head)
{
    constexpr int TW = vapor_trace::words_of(S);           // words of a lane's moves
    const int lane = (int)(threadIdx.x & 63u);
    const long long g = (long long)blockIdx.x * vapor_realign::WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (g >= count) return;                                // (a whole wavefront)
    const long long t = t0 + g;
    const RPair p = pairs[t];
    int32_t* __restrict__ h = head + vapor_trace::HEAD * t;
    if (p.status != 0) {
        if (lane < vapor_trace::HEAD) h[lane] = lane == vapor_trace::H_D ? -1 : lane == vapor_trace::H_STATUS ? p.status : 0;
        return;
    }
    const uint32_t* __restrict__ x1 = x4 + p.word1;
    const uint32_t* __restrict__ x2 = x4 + p.word2;
    const int n = p.n, m = p.m, off2 = p.off2, B = band, W = vapor_realign::row_slots(band);
    const int rows = vapor_realign::rows_walked(n, m, B);
    uint32_t* __restrict__ tr = ws + ws_off[t] + (size_t)lane * TW;      // this lane's words of row 1

    const int c0 = lane * S;
    int E[S], vadd[S];
    uint32_t w[ra_words(S)];
    ra_row_start<S>(E, vadd, w, c0, B, W, [&](int jb) { return ra_allele_nibble(x2, off2, m, jb); });
    RaReader r1, r2;                                       // (as realign_kernel feeds the row)
    const int q0 = off2 + 64 * S - B;
    r1.start(x1, n, 0);
    r2.start(x2, off2 + m, q0);
    for (int ia = 0; ia < rows; ++ia) {
        TraceMoves<TW> moves;
        ra_row_step<S>(E, vadd, w, r1.take(ia), moves);
        if constexpr (TW == 1) tr[0] = moves.mv[0];
        else *reinterpret_cast<uint2*>(tr) = make_uint2(moves.mv[0], moves.mv[1]);
        tr += vapor_trace::row_words(S);
        ra_row_shift<S>(w, r2.nibble(q0 + ia));
    }

    // d as realign_kernel has it, then the slot the rule prefers among those that hold d
    const int best = wave_min_i32(ra_row_best<S>(E, c0, rows, B, W));
    int pick = 0x7FFFFFFF;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int c = c0 + s;
        const int key = vapor_trace::end_key(c, n, m, B, rows);
        if (key != vapor_trace::NO_SLOT && E[s] + c == best) pick = min(pick, vapor_realign::row_key(key, c));
    }
    pick = wave_min_i32(pick);
    int i_end = 0, j_end = 0, status = 0;
    if (pick == 0x7FFFFFFF) status = VAPOR_E_HIP;          // (no slot holds d: cannot be; the traceback leaves such a pair alone)
    else vapor_trace::end_cell(vapor_realign::key_c(pick), n, m, B, rows, i_end, j_end);
    if (lane < vapor_trace::HEAD)
        h[lane] = lane == vapor_trace::H_D ? best : lane == vapor_trace::H_STATUS ? status : lane == vapor_trace::H_I_END ? i_end
                  : lane == vapor_trace::H_J_END ? j_end : 0;
}

template <int S>
__global__ __launch_bounds__(64 * vapor_realign::WAVES) void traceback_kernel(const RPair* __restrict__ pairs, const uint64_t* __restrict__ ws_off,
                                                                              long long t0, long long count, int band, const uint32_t* __restrict__ ws,
                                                                              int cap_runs, int32_t* __restrict__ head, uint32_t* __restrict__ runs)
{
    constexpr int TW = vapor_trace::words_of(S);
    const int lane = (int)(threadIdx.x & 63u);
    const long long g = (long long)blockIdx.x * vapor_realign::WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (g >= count) return;
    const long long t = t0 + g;
    int32_t* __restrict__ h = head + vapor_trace::HEAD * t;
    if (pairs[t].status != 0 || h[vapor_trace::H_STATUS] != 0) return;
    const int B = band, W = vapor_realign::row_slots(band);
    int i = __builtin_amdgcn_readfirstlane(h[vapor_trace::H_I_END]), j = __builtin_amdgcn_readfirstlane(h[vapor_trace::H_J_END]);
    const uint32_t* __restrict__ base = ws + ws_off[t];
    uint32_t* __restrict__ slot = runs + (size_t)t * (size_t)cap_runs;

    // the code of slot c in row `row`, 4 where there is no such slot or row
    auto code_at = [&](int row, int c) -> uint32_t {
        if (row < 1 || c < 0 || c >= W) return 4u;
        const int l = c / S, s = c - l * S;
        return (base[((size_t)(row - 1) * 64 + (size_t)l) * TW + (s >> 4)] >> ((s & 15) * 2)) & 3u;
    };
    int n_runs = 0;
    uint32_t cur_op = 0u, cur_len = 0u;
    auto flush = [&]() {
        if (cur_len == 0u) return;
        if (n_runs < cap_runs && lane == 0) slot[cap_runs - 1 - n_runs] = vapor_trace::run_word(cur_len, cur_op);
        ++n_runs;
    };
    auto append = [&](uint32_t op, uint32_t len) {
        if (len == 0u) return;
        if (cur_len != 0u && op == cur_op) { cur_len += len; return; }
        flush();
        cur_op = op;
        cur_len = len;
    };

    while (i > 0) {
        const int c = j - i + B;
        const uint32_t cd = code_at(i - lane, c);
        const uint32_t cv = code_at(i - lane, c + lane);
        const uint32_t ch = code_at(i, c - lane);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)cd);
        if (first < 2u) {
            const unsigned long long stop = __builtin_amdgcn_ballot_w64(cd >= 2u), xm = __builtin_amdgcn_ballot_w64(cd == 1u);
            const int L = stop ? __builtin_ctzll(stop) : 64;
            int k = 0;
            while (k < L) {                                // the stretch's runs of '=' and 'X'
                const uint32_t op = (uint32_t)((xm >> k) & 1ull);
                const unsigned long long turn = (op ? ~xm : xm) >> k;
                int len = turn ? __builtin_ctzll(turn) : 64;
                if (len > L - k) len = L - k;
                append(op, (uint32_t)len);
                k += len;
            }
            i -= L;
            j -= L;
        } else if (first == 2u) {
            const unsigned long long stop = __builtin_amdgcn_ballot_w64(cv != 2u);
            const int L = stop ? __builtin_ctzll(stop) : 64;
            append((uint32_t)vapor_trace::OP_I, (uint32_t)L);
            i -= L;
        } else if (first == 3u) {
            const unsigned long long stop = __builtin_amdgcn_ballot_w64(ch != 3u);
            const int L = stop ? __builtin_ctzll(stop) : 64;
            append((uint32_t)vapor_trace::OP_D, (uint32_t)L);
            j -= L;
        } else {
            break;                                         // (a path that left the band: cannot be)
        }
    }
    if (i == 0 && j > 0) append((uint32_t)vapor_trace::OP_D, (uint32_t)j);        // row 0 is all horizontal
    flush();
    if (lane == 0) {
        h[vapor_trace::H_N_RUNS] = n_runs;
        if (n_runs > cap_runs) h[vapor_trace::H_STATUS] = VAPOR_E_OVERFLOW;
    }
}

}  // namespace vapor
