// vapor_wide.h - the wide route: dot plots and cleaning of sequences longer than VAPOR_MAX_SEQ_LEN (up to
// VAPOR_MAX_WIDE_SEQ_LEN), for gfx950.  Included by vapor_hip.hip after vapor_kernels.h (it reuses the k-mer keys of the
// 4-bit symbol plane, KeyT / extract_key / revcomp_key, and the flag bits HF_* / WF_D1).
//
// The narrow route packs a run record's i and j into 16 + 16 bits and sizes its clean bitmaps for values below 2^17; none of
// its kernels run here.  This route keeps one explicit dot (j, i) per 8 bytes (int2, 32-bit positions) and works pair by pair:
//   1. wide_table_kernel: every k-mer of the read, forward and reverse-complemented (entry e = 2 i + strand, the reference's
//      lookup[key] order SF:951-983), into a chained hash table in HBM (head per bucket, next per entry, the 4-bit keys).
//   2. wide_probe_kernel<EMIT = false>: dots per allele position j (a walk of j's chain, exact key comparison).
//   3. wide_scan_kernel: the exclusive prefix of those counts - every pair's dot slot is sized by this count pass, exactly.
//   4. wide_probe_kernel<EMIT = true>: the dots into the slot.
//   5. cleaning, per axis (i - j + shift, i + j): wide_hist_kernel (occupancy counts over the value range), wide_group_kernel
//      (gap clustering, dis_cluster / dis_cluster_2 SF:551-580: a new group where a value is 10 or more above its predecessor;
//      32-bit group ids and sizes), wide_flag_kernel (the keep rules of C1 SF:432-448 and C2 SF:404-430).  Counts, ids and sizes
//      live in a global scratch buffer of the pair (3 x 4 B per value: 2^21 values do not fit the 160 KiB of LDS).
//   6. wide_reduce_kernel: the integer reductions of the statistics record; wide_dir_kernel (one workgroup): the redefined
//      diagonal (SF:582-591) and the directed distance (SF:718-722) over the C1-kept dots.
// Every value is exact: counts and sums that can pass 2^31 are 64-bit.
#pragma once

#include "vapor_dots_plan.h"   // WideAcc, shared with the host (no HIP)

namespace vapor {

constexpr int WIDE_SCAN_THREADS = 1024;

template <int K>
using WKey = KeyT<4, K>;

template <int K>
__device__ __forceinline__ uint32_t wide_hash(const WKey<K>& k)
{
    uint64_t h = 0x243F6A8885A308D3ull;
#pragma unroll
    for (int t = 0; t < WKey<K>::NW; ++t) {
        h = (h ^ k.w[t]) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    return (uint32_t)(h ^ (h >> 32));
}

// Entry e of the read's table: k-mer e >> 1 of the read, reverse-complemented when e is odd.  Chains are pushed with an atomic
// exchange, so their order is unspecified (the statistics do not depend on it; callers that want the reference's list order
// sort by (j, i), which is that order: for one j the matching entries are i ascending, and a k-mer equal to its own reverse
// complement gives the same (j, i) twice).
template <int K>
__global__ __launch_bounds__(256) void wide_table_kernel(const uint32_t* __restrict__ x4_1, int nk1, WKey<K>* __restrict__ keys,
                                                         int32_t* __restrict__ head, int32_t* __restrict__ next, uint32_t hmask)
{
    const int e = (int)(blockIdx.x * 256u + threadIdx.x);
    if (e >= 2 * nk1) return;
    WKey<K> key = extract_key<4, K>(x4_1, (uint32_t)(e >> 1));
    if (e & 1) key = revcomp_key<4, K>(key);
    keys[e] = key;
    next[e] = atomicExch(&head[wide_hash<K>(key) & hmask], e);
}

// Allele position j (k-mer off2 + j of seq2) against the table: count (EMIT = false) or write its dots at off[j].
// The count pass bounds its own work: a thread books its dots in steps of WIDE_BOOK on the pair's counter `booked` and stops
// walking once the pair has more than `cap` dots ("max_pair_cap"; the pair is then refused with VAPOR_E_OVERFLOW), so a
// low-complexity sequence - a chain of ~2 x 10^6 equal k-mers per position - costs about cap dependent loads, not n^2.
constexpr uint32_t WIDE_BOOK = 4096;
template <int K, bool EMIT>
__global__ __launch_bounds__(256) void wide_probe_kernel(const uint32_t* __restrict__ x4_2, int off2, int nk2,
                                                         const WKey<K>* __restrict__ keys, const int32_t* __restrict__ head,
                                                         const int32_t* __restrict__ next, uint32_t hmask, uint32_t* __restrict__ cnt,
                                                         const long long* __restrict__ off, int2* __restrict__ dots,
                                                         unsigned long long* booked, unsigned long long cap)
{
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= nk2) return;
    const WKey<K> q = extract_key<4, K>(x4_2, (uint32_t)(off2 + j));
    uint32_t c = 0;
    long long at = EMIT ? off[j] : 0;
    for (int e = head[wide_hash<K>(q) & hmask]; e >= 0; e = next[e]) {
        if (keys[e] == q) {
            if (EMIT) dots[at + c] = make_int2(j, e >> 1);
            ++c;
            if (!EMIT && (c % WIDE_BOOK) == 0u && atomicAdd(booked, (unsigned long long)WIDE_BOOK) + WIDE_BOOK > cap) break;
        }
    }
    if (!EMIT) cnt[j] = c;
}

// LDS scan of one value per thread (Hillis-Steele; every thread of the block takes part)
template <typename T>
__device__ __forceinline__ T wide_block_incl_scan(T v, T* part)
{
    const int tid = threadIdx.x;
    part[tid] = v;
    __syncthreads();
    for (int o = 1; o < (int)blockDim.x; o <<= 1) {
        const T add = tid >= o ? part[tid - o] : (T)0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const T r = part[tid];
    __syncthreads();
    return r;
}

// off[q] = cnt[0] + ... + cnt[q-1] for q in [0, n]; one workgroup, a contiguous span per thread
__global__ __launch_bounds__(WIDE_SCAN_THREADS) void wide_scan_kernel(const uint32_t* __restrict__ cnt, int n, long long* __restrict__ off)
{
    __shared__ long long part[WIDE_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (n + WIDE_SCAN_THREADS - 1) / WIDE_SCAN_THREADS;
    const int q0 = min(tid * per, n), q1 = min(q0 + per, n);
    long long s = 0;
    for (int q = q0; q < q1; ++q) s += cnt[q];
    const long long incl = wide_block_incl_scan<long long>(s, part);
    long long run = incl - s;
    for (int q = q0; q < q1; ++q) { off[q] = run; run += cnt[q]; }
    if (tid == WIDE_SCAN_THREADS - 1) off[n] = incl;
}

// (the per-pair results of the cleaning, WideAcc: vapor_dots_plan.h, which turns them into the statistics record)

__device__ __forceinline__ uint32_t wide_value(int2 d, int axis, int shift)
{
    return axis ? (uint32_t)(d.y + d.x) : (uint32_t)(d.y - d.x + shift);
}

// occupancy counts of the axis values of the dots whose flag byte has none of `skip`
__global__ __launch_bounds__(256) void wide_hist_kernel(const int2* __restrict__ dots, const uint8_t* __restrict__ fl, int n, int axis,
                                                        int shift, uint32_t skip, uint32_t* __restrict__ cnt)
{
    const int h = (int)(blockIdx.x * 256u + threadIdx.x);
    if (h >= n) return;
    if (skip && (fl[h] & skip)) return;
    atomicAdd(&cnt[wide_value(dots[h], axis, shift)], 1u);
}

// Gap clustering of the values [0, R) with counts cnt: a present value 10 or more above the previous present value starts a
// group.  gid[v] = group of a present value, gsize[g] = dots in group g (gsize zeroed by the caller), acc->max_group[slot] =
// the largest group.  One workgroup; each thread a contiguous span of values, the group ids of a span offset by a block scan
// of the spans' group starts.
__global__ __launch_bounds__(WIDE_SCAN_THREADS) void wide_group_kernel(const uint32_t* __restrict__ cnt, int R, uint32_t* __restrict__ gid,
                                                                       uint32_t* gsize, WideAcc* acc, int slot)
{
    __shared__ uint32_t part[WIDE_SCAN_THREADS];
    __shared__ uint32_t best;
    const int tid = threadIdx.x;
    if (tid == 0) best = 0;
    const int per = (R + WIDE_SCAN_THREADS - 1) / WIDE_SCAN_THREADS;
    const int q0 = min(tid * per, R), q1 = min(q0 + per, R);
    int last0 = -100;                            // last present value before the span (only the 9 before it matter)
    for (int v = max(0, q0 - 9); v < q0; ++v)
        if (cnt[v]) last0 = v;
    uint32_t starts = 0;
    int last = last0;
    for (int v = q0; v < q1; ++v)
        if (cnt[v]) { if (v - last >= 10) ++starts; last = v; }
    const uint32_t incl = wide_block_incl_scan<uint32_t>(starts, part);
    const uint32_t ng = part[WIDE_SCAN_THREADS - 1];      // groups in all
    // (a span that begins inside a group continues the previous span's last group: incl - starts - 1)
    uint32_t g = incl - starts - 1u, acc_n = 0;
    last = last0;
    for (int v = q0; v < q1; ++v) {
        const uint32_t c = cnt[v];
        if (!c) continue;
        if (v - last >= 10) {
            if (acc_n) atomicAdd(&gsize[g], acc_n);
            ++g;
            acc_n = 0;
        }
        gid[v] = g;
        acc_n += c;
        last = v;
    }
    if (acc_n) atomicAdd(&gsize[g], acc_n);
    __threadfence();
    __syncthreads();
    uint32_t mx = 0;
    for (uint32_t q = (uint32_t)tid; q < ng; q += WIDE_SCAN_THREADS)
        mx = max(mx, __hip_atomic_load(&gsize[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    atomicMax(&best, mx);
    __syncthreads();
    if (tid == 0) acc->max_group[slot] = best;
}

// dis_cluster's rule (SF:560-563): groups of more than 50 survive; when there is none, every group of the largest size
__device__ __forceinline__ bool wide_c2_keep(uint32_t s, uint32_t mx) { return mx > 50u ? s > 50u : s == mx; }

// mode 0: i - j over all dots (flag byte rewritten): WF_D1 for a group of more than 10 (C1), HF_C2D by dis_cluster's rule (C2)
// mode 1: i + j over all dots: HF_C1 unless both groups have at most 10 dots (SF:432-448)
// mode 2: i + j over the dots without HF_C2D: HF_C2A by dis_cluster's rule
__global__ __launch_bounds__(256) void wide_flag_kernel(const int2* __restrict__ dots, uint8_t* __restrict__ fl, int n, int mode, int shift,
                                                        uint32_t pflags, const uint32_t* __restrict__ gid, const uint32_t* __restrict__ gsize,
                                                        const WideAcc* __restrict__ acc)
{
    const int h = (int)(blockIdx.x * 256u + threadIdx.x);
    if (h >= n) return;
    const int2 d = dots[h];
    if (mode == 0) {
        const uint32_t s = gsize[gid[wide_value(d, 0, shift)]];
        uint32_t f = 0;
        if ((pflags & 1u) && s > 10u) f |= WF_D1;
        if ((pflags & 2u) && wide_c2_keep(s, acc->max_group[0])) f |= HF_C2D;
        fl[h] = (uint8_t)f;
    } else if (mode == 1) {
        const uint32_t f = fl[h];
        if ((f & WF_D1) || gsize[gid[wide_value(d, 1, shift)]] > 10u) fl[h] = (uint8_t)(f | HF_C1);
    } else {
        const uint32_t f = fl[h];
        if (!(f & HF_C2D) && wide_c2_keep(gsize[gid[wide_value(d, 1, shift)]], acc->max_group[2])) fl[h] = (uint8_t)(f | HF_C2A);
    }
}

// The integer reductions of the statistics record (SF:705-708, 730-733, 1154-1171) and the range of i - j over the C1-kept
// dots (for wide_dir_kernel); the flag bytes are cut down to the public bits.
__global__ __launch_bounds__(256) void wide_reduce_kernel(const int2* __restrict__ dots, uint8_t* __restrict__ fl, int n, WideAcc* acc)
{
    __shared__ unsigned long long s_u[7];
    __shared__ int s_mn, s_mx, s_klo, s_khi;
    const int tid = threadIdx.x;
    if (tid < 7) s_u[tid] = 0;
    if (tid == 0) { s_mn = 0x7FFFFFFF; s_mx = -1; s_klo = 0x7FFFFFFF; s_khi = -0x7FFFFFFF; }
    __syncthreads();
    const int h = (int)(blockIdx.x * 256u + threadIdx.x);
    if (h < n) {
        const int2 d = dots[h];
        const int j = d.x, i = d.y;
        const uint32_t f = fl[h];
        const long long ad = j > i ? (long long)(j - i) : (long long)(i - j);
        atomicMin(&s_mn, j);
        atomicMax(&s_mx, j);
        if (j == i) atomicAdd(&s_u[0], 1ull);
        else if (j > i) atomicAdd(&s_u[1], 1ull);
        if (f & HF_C1) {
            atomicAdd(&s_u[2], 1ull);
            atomicAdd(&s_u[3], (unsigned long long)ad);
            atomicMin(&s_klo, i - j);
            atomicMax(&s_khi, i - j);
        }
        if (f & (HF_C2D | HF_C2A)) {
            atomicAdd(&s_u[4], 1ull);
            if (j > 0 && 25 * ad < 4 * (long long)j) atomicAdd(&s_u[5], 1ull);
            if (f & HF_C2D) atomicAdd(&s_u[6], 1ull);
        }
        fl[h] = (uint8_t)(f & (HF_C1 | HF_C2D | HF_C2A));
    }
    __syncthreads();
    if (tid == 0) {
        atomicAdd(&acc->n_diag, s_u[0]); atomicAdd(&acc->n_lower, s_u[1]);
        atomicAdd(&acc->c1_kept, s_u[2]); atomicAdd(&acc->c1_sum_abs, s_u[3]);
        atomicAdd(&acc->c2_kept, s_u[4]); atomicAdd(&acc->c2_count10, s_u[5]); atomicAdd(&acc->c2_kept_diag, s_u[6]);
        atomicMin(&acc->min_j, s_mn); atomicMax(&acc->max_j, s_mx);
        atomicMin(&acc->kd_lo, s_klo); atomicMax(&acc->kd_hi, s_khi);
    }
}

// number_cluster's list of v (SF:1104-1118) over edges lo + t*float(range)/10.0: exactly 10*(v-lo) / range (integer division;
// see R4Div in vapor_kernels.h for why), 10 when range == 0.  64-bit: 10 * 2^21 does not fit the narrow route's float trick.
__device__ __forceinline__ int wide_bin(int v, int lo, int range)
{
    return range > 0 ? (int)((10ll * (v - lo)) / range) : 10;
}

// dis_to_diagnal_most_abundant_defined (SF:582-591) and eu_dis_dir_calcu (SF:718-722) over the C1-kept dots, one workgroup.
// hist: scratch of at least kd_hi - kd_lo + 1 words, zeroed by the caller.
__global__ __launch_bounds__(WIDE_SCAN_THREADS) void wide_dir_kernel(const int2* __restrict__ dots, const uint8_t* __restrict__ fl, int n,
                                                                     WideAcc* acc, uint32_t* hist)
{
    __shared__ int cnt1[11], cnt2[11];
    __shared__ int b_lo, b_hi, n_lists, sel_w, sel_b, sel_lo, sel_range, sel_m, c2x, dir_n;
    __shared__ unsigned long long dir_sum;
    __shared__ uint32_t part[WIDE_SCAN_THREADS];
    const int tid = threadIdx.x;
    if (acc->kd_hi < acc->kd_lo) {                     // no kept dots (the initial +/- 2^31 - 1: their difference does not fit an int)
        if (tid == 0) { acc->dir_c2x = 0; acc->dir_n = 0; acc->dir_sum2 = 0; acc->dir_lists = 0; }
        return;
    }
    const int lo1 = acc->kd_lo, range1 = acc->kd_hi - acc->kd_lo;
    if (tid < 11) cnt1[tid] = 0;
    if (tid == 0) { n_lists = 0; c2x = 0; dir_n = 0; dir_sum = 0; sel_w = -1; }
    __syncthreads();
    for (int h = tid; h < n; h += WIDE_SCAN_THREADS)
        if (fl[h] & HF_C1) { const int2 d = dots[h]; atomicAdd(&cnt1[wide_bin(d.y - d.x, lo1, range1)], 1); }
    __syncthreads();
    int best1 = 0;
    for (int b = 0; b < 11; ++b) best1 = max(best1, cnt1[b]);
    for (int w = 0; w < 11; ++w) {
        if (cnt1[w] != best1) continue;                // uniform
        if (tid == 0) { b_lo = 0x7FFFFFFF; b_hi = -0x7FFFFFFF; }
        if (tid < 11) cnt2[tid] = 0;
        __syncthreads();
        {
            int lo = 0x7FFFFFFF, hi = -0x7FFFFFFF;
            for (int h = tid; h < n; h += WIDE_SCAN_THREADS) {
                if (!(fl[h] & HF_C1)) continue;
                const int2 d = dots[h];
                const int v = d.y - d.x;
                if (wide_bin(v, lo1, range1) == w) { lo = min(lo, v); hi = max(hi, v); }
            }
            atomicMin(&b_lo, lo); atomicMax(&b_hi, hi);
        }
        __syncthreads();
        const int lo2 = b_lo, range2 = b_hi - b_lo;
        for (int h = tid; h < n; h += WIDE_SCAN_THREADS) {
            if (!(fl[h] & HF_C1)) continue;
            const int2 d = dots[h];
            const int v = d.y - d.x;
            if (wide_bin(v, lo1, range1) == w) atomicAdd(&cnt2[wide_bin(v, lo2, range2)], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int best2 = 0;
            for (int b = 0; b < 11; ++b) best2 = max(best2, cnt2[b]);
            for (int b = 0; b < 11; ++b)
                if (cnt2[b] == best2) {
                    if (n_lists == 0) { sel_w = w; sel_b = b; sel_lo = lo2; sel_range = range2; sel_m = best2; }
                    ++n_lists;
                }
        }
        __syncthreads();
    }
    if (n_lists == 1) {                                // uniform: the median of the one longest sub-list is the new intercept
        const int w = sel_w, b = sel_b, lo2 = sel_lo, range2 = sel_range, m = sel_m;
        for (int h = tid; h < n; h += WIDE_SCAN_THREADS) {
            if (!(fl[h] & HF_C1)) continue;
            const int2 d = dots[h];
            const int v = d.y - d.x;
            if (wide_bin(v, lo1, range1) == w && wide_bin(v, lo2, range2) == b) atomicAdd(&hist[v - lo2], 1u);
        }
        __threadfence();
        __syncthreads();
        // order statistics (m-1)/2 and m/2 (0-based): np.median is their mean, c2x their sum
        const int width = range2 + 1;
        const int per = (width + WIDE_SCAN_THREADS - 1) / WIDE_SCAN_THREADS;
        const int q0 = min(tid * per, width), q1 = min(q0 + per, width);
        uint32_t local = 0;
        for (int q = q0; q < q1; ++q) local += __hip_atomic_load(&hist[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t run = wide_block_incl_scan<uint32_t>(local, part) - local;
        const uint32_t ks[2] = {(uint32_t)((m - 1) / 2), (uint32_t)(m / 2)};
        for (int t = 0; t < 2; ++t) {
            if (ks[t] >= run && ks[t] < run + local) {
                uint32_t a = run;
                for (int q = q0; q < q1; ++q) {
                    a += __hip_atomic_load(&hist[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (a > ks[t]) { atomicAdd(&c2x, lo2 + q); break; }
                }
            }
        }
        __syncthreads();
    }
    {
        // dots (X, Y) = (2j + c2x, 2i) with 10 * |X - Y| > |X| (X == 0: i >= 1): count and sum of X - Y
        const int cx = c2x;
        int cn = 0;
        long long cs = 0;
        for (int h = tid; h < n; h += WIDE_SCAN_THREADS) {
            if (!(fl[h] & HF_C1)) continue;
            const int2 d = dots[h];
            const long long X = 2ll * d.x + cx, Y = 2ll * d.y, df = X - Y;
            const bool far = (X == 0) ? (d.y >= 1) : (10 * (df < 0 ? -df : df) > (X < 0 ? -X : X));
            if (far) { ++cn; cs += df; }
        }
        atomicAdd(&dir_n, cn);
        atomicAdd(&dir_sum, (unsigned long long)cs);
    }
    __syncthreads();
    if (tid == 0) { acc->dir_c2x = c2x; acc->dir_n = dir_n; acc->dir_sum2 = (long long)dir_sum; acc->dir_lists = n_lists; }
}

}  // namespace vapor
