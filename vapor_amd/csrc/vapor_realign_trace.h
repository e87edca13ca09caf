// vapor_realign_trace.h - the two kernels of vapor_realign_trace: the alignment behind realign_kernel's distance.
//
// realign_trace_kernel<S> is realign_kernel<S>'s row (vapor_realign.h: the band row in E = D - c, the nibble shift register, the
// scalar sequence loads) with two bits kept per slot and row, the move the rule takes out of that cell:
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

#include "vapor_trace_plan.h"

namespace vapor {

template <int S>
__global__ __launch_bounds__(64 * vapor_realign::WAVES) void realign_trace_kernel(const uint32_t* __restrict__ x4, const RPair* __restrict__ pairs,
                                                                                  const uint64_t* __restrict__ ws_off, long long t0, long long count,
                                                                                  int band, uint32_t* __restrict__ ws, int32_t* __restrict__ head)
{
    constexpr int NW = (4 * S + 31) / 32;                  // words of a lane's nibbles
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
    const int len2 = off2 + m;
    const int rows = vapor_realign::rows_walked(n, m, B);
    const int c0 = lane * S;
    uint32_t* __restrict__ tr = ws + ws_off[t] + (size_t)lane * TW;      // this lane's words of row 1

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
        uint32_t x[NW];
        if (ca < 8u) {
#pragma unroll
            for (int k = 0; k < NW; ++k) x[k] = ~(w[k] >> (ca & 3u));
        } else {
#pragma unroll
            for (int k = 0; k < NW; ++k) x[k] = ~(w[k] & (w[k] >> 1) & (w[k] >> 2) & (w[k] >> 3));
        }
        const int vin = dpp_from<0x130, 0xF>(RA_INF, E[0]);              // wave_shl:1
        int run = RA_INF;
        uint32_t mv[TW];
#pragma unroll
        for (int k = 0; k < TW; ++k) mv[k] = 0u;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const uint32_t sub = (x[s >> 3] >> ((s & 7) * 4)) & 1u;
            const int d = E[s] + (int)sub;
            const int v = (s + 1 < S ? E[s + 1] : vin) + vadd[s];
            run = min(run, min(d, v));
            E[s] = run;
            const uint32_t code = run == d ? sub : run == v ? (uint32_t)vapor_trace::OP_I : (uint32_t)vapor_trace::OP_D;
            mv[s >> 4] |= code << ((s & 15) * 2);
        }
        const int before = dpp_from<0x138, 0xF>(RA_INF, wave_scan<OpMin>(run, RA_INF));     // wave_shr:1
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (before < E[s]) mv[s >> 4] |= 3u << ((s & 15) * 2);
            E[s] = min(E[s], before);
        }
        if constexpr (TW == 1) tr[0] = mv[0];
        else *reinterpret_cast<uint2*>(tr) = make_uint2(mv[0], mv[1]);
        tr += vapor_trace::row_words(S);
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

    // d as realign_kernel has it, then the slot the rule prefers among those that hold d (key << 11 | slot: a slot is below 2048)
    int best = RA_INF;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int c = c0 + s;
        if (c < W && rows + c - B >= 0) best = min(best, E[s] + c);
    }
    best = wave_min_i32(best);
    int pick = 0x7FFFFFFF;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int c = c0 + s;
        const int key = vapor_trace::end_key(c, n, m, B, rows);
        if (key != vapor_trace::NO_SLOT && E[s] + c == best) pick = min(pick, key << 11 | c);
    }
    pick = wave_min_i32(pick);
    int i_end = 0, j_end = 0, status = 0;
    if (pick == 0x7FFFFFFF) status = VAPOR_E_HIP;          // (no slot holds d: cannot be; the traceback leaves such a pair alone)
    else vapor_trace::end_cell(pick & 2047, n, m, B, rows, i_end, j_end);
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
