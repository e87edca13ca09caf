// vapor_junction.h - junction_rows_kernel and junction_pick_kernel: the one jump that turns the longer of two
// sequences into the shorter, from a forward pass anchored at the common start and a backward pass anchored at the common end.
//
// junction_rows_kernel<S>: one wavefront a task, a task a pair in one direction.  It walks the band row of vapor_band_row.h with
// off2 = 0, and behind every row, row 0 included, takes the minimum of D = E + c over the slots that are cells
// (c <= 2B and 0 <= j = i + c - B <= nl) with the smallest slot on a tie: one wave minimum of vapor_realign::row_key(D, c), stored
// by one lane as (f, jf).  The cells behind column nl are the wildcard continuation of the row and are masked here only: they
// feed no cell at or before column nl.  The backward task reads both sequences from their last symbol towards their first: symbol k of a pass is
// symbol len - 1 - k, the words of the 4-bit plane loaded descending, one ahead; no reversed copy exists.
// junction_pick_kernel: one wavefront a pair, 64 split rows a step: cost = f_F(i) + f_R(ns - i), j1 = jf_F(i),
// j2 = nl - jf_R(ns - i), valid iff j2 >= j1, the smallest (cost, i) wins; one lane writes the pair's eight words.
#pragma once

#include "vapor_junction_plan.h"
#include "vapor_band_row.h"

namespace vapor {

using vapor_junction::JPair;

// the symbol code at position pos of a sequence in the 4-bit plane
__device__ __forceinline__ uint32_t jn_code(const uint32_t* __restrict__ x, int pos) { return (x[pos >> 3] >> ((pos & 7) * 4)) & 15u; }

// the nibble of symbol jb of a pass over the longer sequence: nothing in front of the start, the wildcard behind the end
__device__ __forceinline__ uint32_t jn_nibble(const uint32_t* __restrict__ x2, int nl, bool back, int jb)
{
    if (jb < 0) return 0u;
    if (jb >= nl) return 15u;
    return ra_onehot(jn_code(x2, vapor_junction::pass_pos(nl, back, jb)));
}

// The symbols k0, k0 + 1, .. of a pass over a sequence of len symbols, a word of eight at a time, one word ahead; everything here
// is wave-uniform.  take(k) must be called with consecutive k from k0 on; it returns 16 behind the sequence's end, and loads
// nothing there.
struct JnReader {
    const uint32_t* __restrict__ x;
    int len;
    bool back, first;
    uint32_t cur, next;

    __device__ __forceinline__ void start(const uint32_t* __restrict__ x_, int len_, bool back_, int k0)
    {
        x = x_; len = len_; back = back_; first = true; cur = 0u;
        next = k0 < len ? x[vapor_junction::pass_pos(len, back, k0) >> 3] : 0u;
    }
    __device__ __forceinline__ uint32_t take(int k)
    {
        if (k >= len) return 16u;
        const int pos = vapor_junction::pass_pos(len, back, k);
        if (first || (pos & 7) == (back ? 7 : 0)) {
            first = false;
            cur = next;
            const int nx = (pos >> 3) + (back ? -1 : 1);
            next = nx >= 0 && nx * 8 < len ? x[nx] : 0u;
        }
        return (cur >> ((pos & 7) * 4)) & 15u;
    }
};

// (f, jf) of row i from the row's registers: lane 63 holds the wave's minimum and stores it
template <int S>
__device__ __forceinline__ void jn_store_row(const int (&E)[S], int c0, int i, int B, int W, int nl, int lane, int32_t* __restrict__ dst)
{
    // the cells of row i are the slots lo .. lo + span: c <= 2B and 0 <= j = i + c - B <= nl (never empty: i <= ns <= nl)
    const int lo = max(0, B - i);
    const unsigned span = (unsigned)(min(W - 1, nl + B - i) - lo);
    int key = vapor_junction::NO_CELL;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int c = c0 + s;
        if ((unsigned)(c - lo) <= span) key = min(key, vapor_junction::row_key(E[s] + c, c));
    }
    key = wave_scan<OpMin>(key, vapor_junction::NO_CELL);
    if (lane == 63) *reinterpret_cast<int2*>(dst) = make_int2(vapor_junction::key_d(key), i + vapor_junction::key_c(key) - B);
}

template <int S>
__global__ __launch_bounds__(64 * vapor_realign::WAVES) void junction_rows_kernel(const uint32_t* __restrict__ x4, const JPair* __restrict__ pairs,
                                                                                  long long n_tasks, int band, int32_t* __restrict__ ws)
{
    const int lane = (int)(threadIdx.x & 63u);
    const long long task = (long long)blockIdx.x * vapor_realign::WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (task >= n_tasks) return;                           // (a whole wavefront: the cross-lane steps below need all 64 lanes)
    const JPair p = pairs[vapor_junction::task_pair(task)];
    if (p.status != 0) return;                             // (junction_pick_kernel writes the refused pair's record)
    const bool back = vapor_junction::task_backward(task);
    const uint32_t* __restrict__ x1 = x4 + p.word1;
    const uint32_t* __restrict__ x2 = x4 + p.word2;
    const int ns = p.ns, nl = p.nl, B = band, W = vapor_realign::row_slots(band);
    // row i of this pass: words 4 (row0 + i) + (backward ? 2 : 0) and the one behind it
    int32_t* __restrict__ mine = ws + p.row0 * vapor_junction::ROW + (back ? vapor_junction::R_F_BWD : vapor_junction::R_F_FWD);

    const int c0 = lane * S;
    int E[S], vadd[S];
    uint32_t w[ra_words(S)];
    ra_row_start<S>(E, vadd, w, c0, B, W, [&](int jb) { return jn_nibble(x2, nl, back, jb); });
    jn_store_row<S>(E, c0, 0, B, W, nl, lane, mine);

    // the shorter sequence's symbol i - 1 for row i; the longer one's symbol that enters at lane 63's last slot for row i + 1,
    // jb = i + 64 S - B - 1 (never negative: 64 S >= 2B + 1)
    JnReader r1, r2;
    const int q0 = 64 * S - B;
    r1.start(x1, ns, back, 0);
    r2.start(x2, nl, back, q0);
    RaNoHooks none;
    for (int i = 1; i <= ns; ++i) {
        const int ia = i - 1;
        ra_row_step<S>(E, vadd, w, r1.take(ia), none);
        jn_store_row<S>(E, c0, i, B, W, nl, lane, mine + (long long)i * vapor_junction::ROW);
        const uint32_t cb = r2.take(q0 + ia);
        ra_row_shift<S>(w, cb < 16u ? ra_onehot(cb) : 15u);
    }
}

__global__ __launch_bounds__(64 * vapor_realign::WAVES) void junction_pick_kernel(const JPair* __restrict__ pairs, long long n_pairs,
                                                                                  const int32_t* __restrict__ ws, int32_t* __restrict__ out)
{
    const int lane = (int)(threadIdx.x & 63u);
    const long long t = (long long)blockIdx.x * vapor_realign::WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (t >= n_pairs) return;
    const JPair p = pairs[t];
    int32_t* __restrict__ o = out + t * vapor_junction::OUT;
    if (p.status != 0) {
        if (lane < vapor_junction::OUT) o[lane] = lane == vapor_junction::O_STATUS ? p.status : 0;
        return;
    }
    const int4* __restrict__ tab = reinterpret_cast<const int4*>(ws) + p.row0;
    const int ns = p.ns, nl = p.nl;
    int best = vapor_junction::NO_CELL, bi = vapor_junction::NO_CELL, bj1 = 0, bj2 = 0, bff = 0, bfr = 0;
    for (int base = 0; base <= ns; base += 64) {
        const int i = base + lane;
        if (i <= ns) {
            const int4 f = tab[i], r = tab[ns - i];
            const int j1 = f.y, j2 = vapor_junction::split_j2(nl, r.w), cost = f.x + r.z;
            if (vapor_junction::split_valid(j1, j2) && cost < best) {        // (a lane's rows ascend: the leftmost stays)
                best = cost; bi = i; bj1 = j1; bj2 = j2; bff = f.x; bfr = r.z;
            }
        }
    }
    const int cost = wave_min_i32(best);                   // (row 0 is always valid: some lane holds a row)
    const int row = wave_min_i32(best == cost ? bi : vapor_junction::NO_CELL);
    if (best == cost && bi == row) {
        *reinterpret_cast<int4*>(o) = make_int4(0, cost, row, bj1);
        *reinterpret_cast<int4*>(o + 4) = make_int4(bj2, bff, bfr, 0);
    }
}

}  // namespace vapor
