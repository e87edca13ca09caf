// vapor_anyk.h - the any-k route: kmerhits (SF:951-983) at every k from 1 to VAPOR_MAX_ANY_K, with and without inversions,
// dots in the reference's list order, for gfx950.  Included by vapor_hip.hip after vapor_wide.h (whose scan, cleaning and
// reduction kernels give the statistics record: they do not depend on the order of the dots).
//
// A k-mer is a string of k symbol bytes: key_modify's folding (SF:908-949) of the 4-bit plane - ACGT acgt N n - and, for a
// symbol outside that alphabet, the byte itself where the sequence set kept it (VAPOR_PF_FORWARD compares such symbols byte
// for byte, the way the reference's dict does), 0xFF where it did not (with inversions such a symbol in seq1 is a KeyError,
// and one in seq2 matches nothing).  One pair at a time:
//   1. anyk_sym_kernel: seq1, seq2[off2:] and (with inversions) the reverse complement of seq1 as symbol bytes.
//   2. The read's lookup entries, e = 2 i + strand with inversions (the reference's insertion order: position i, its
//      reverse complement right after it), e = i without, sorted by (k-mer, e): anyk_sort_local_kernel / anyk_sort_global_kernel,
//      a bitonic network (LDS for the strides below 512).  Each run of equal k-mers is one key of the reference's lookup dict,
//      its entries in list order.
//   3. k <= 40 (exact): anyk_probe_kernel, the run of allele k-mer j by binary search (count and first entry);
//      wide_scan_kernel sizes every j's slot exactly; anyk_emit_kernel copies the run: (j, i) for every entry, in list order.
//   4. k > 40 (edit distance, SF:969-973): anyk_group_kernel / wide_scan_kernel / anyk_rank_kernel number the distinct keys in
//      order of first insertion; anyk_edit_kernel<EMIT> gives allele k-mer j one wave, which walks the keys 64 at a time (one
//      per lane), computes the Levenshtein distance (unit costs) by Myers / Hyyro bit-parallel recurrence in one 64-bit word,
//      and for every key within k / 10 appends its entries - a count pass, the exclusive scan, an emit pass in which a wave
//      prefix of the 64 lanes' list lengths keeps the order: j, then key rank, then list position.
#pragma once

namespace vapor {

// (ANYK_EXACT_MAX_K, ANYK_TILE, ANYK_EDIT_WAVES and ANYK_EDIT_PAIRS: vapor_dots_plan.h, where the host's arithmetic reads them too)
constexpr uint32_t ANYK_NONE = 0xFFFFFFFFu;     // padding entry of the sort (after every real one)

// the symbol bytes of one pair's sequences and how entry e maps to a k-mer of them
struct AnykSrc {
    const uint8_t* s1;     // seq1, n1 bytes
    const uint8_t* r1;     // reverse complement of seq1 (inversions only)
    const uint8_t* s2;     // seq2[off2:]
    int n1, k, inv;
};

__device__ __forceinline__ const uint8_t* anyk_entry(const AnykSrc& s, uint32_t e)
{
    if (!s.inv) return s.s1 + e;
    const int i = (int)(e >> 1);
    return (e & 1u) ? s.r1 + (s.n1 - s.k - i) : s.s1 + i;
}

__device__ __forceinline__ int anyk_pos(const AnykSrc& s, uint32_t e) { return s.inv ? (int)(e >> 1) : (int)e; }

// 4 bytes from p (any alignment): the buffers are 4-byte aligned and padded by 8 bytes, so both words are in bounds
__device__ __forceinline__ uint32_t anyk_word(const uint8_t* p)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
    return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(a & 3u));
}

// a total order on k-byte strings (word by word as little-endian integers: not the lexicographic one, but equal strings and
// only they compare equal, which is all the lookup needs)
__device__ __forceinline__ int anyk_cmp(const uint8_t* a, const uint8_t* b, int k)
{
    for (int t = 0; t < k; t += 4) {
        uint32_t x = anyk_word(a + t), y = anyk_word(b + t);
        if (k - t < 4) {
            const uint32_t m = (1u << (8 * (k - t))) - 1u;
            x &= m;
            y &= m;
        }
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

__device__ __forceinline__ bool anyk_less(const AnykSrc& s, uint32_t x, uint32_t y)
{
    if (x == ANYK_NONE || y == ANYK_NONE) return x < y;
    const int c = anyk_cmp(anyk_entry(s, x), anyk_entry(s, y), s.k);
    return c ? c < 0 : x < y;
}

__device__ __forceinline__ uint32_t anyk_comp(uint32_t b)
{
    // invert_base (SF:19-20) on folded symbols; N / n and the bytes it lacks stay (such a seq1 is a KeyError before this)
    switch (b) {
    case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C';
    case 'a': return 't'; case 't': return 'a'; case 'c': return 'g'; case 'g': return 'c';
    default: return b;
    }
}

// symbol bytes of sequence positions [off, off + n) (the set's 4-bit plane x4, the sequence's kept bytes raw or null; upper:
// the set upper-cased it), into out[0 .. n); with rc also the reverse complement into rc[0 .. n)
__global__ __launch_bounds__(256) void anyk_sym_kernel(const uint32_t* __restrict__ x4, const uint8_t* __restrict__ raw, int upper,
                                                       int off, int n, uint8_t* __restrict__ out, uint8_t* __restrict__ rc)
{
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    if (p >= n) return;
    const uint32_t q = (uint32_t)(off + p);
    const uint32_t code = (x4[q >> 3] >> ((q & 7u) * 4u)) & 15u;
    uint32_t b;
    if (code < 8u) b = (uint32_t)"ACGTacgt"[code];
    else if (code == 8u) b = 'N';
    else if (code == 9u) b = 'n';
    else if (raw) { b = raw[q]; if (upper && b >= 'a' && b <= 'z') b -= 32u; }
    else b = 0xFFu;
    out[p] = (uint8_t)b;
    if (rc) rc[n - 1 - p] = (uint8_t)anyk_comp(b);
}

// idx[p] = p for the n entries, ANYK_NONE up to np
__global__ __launch_bounds__(256) void anyk_iota_kernel(uint32_t* __restrict__ idx, int n, int np)
{
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    if (p < np) idx[p] = p < n ? (uint32_t)p : ANYK_NONE;
}

// Bitonic network, the strides below ANYK_TILE in LDS: full = 1 sorts every tile (the sizes 2 .. ANYK_TILE); otherwise the merge
// of size kk (> ANYK_TILE) from stride ANYK_TILE / 2 down.  Direction of element p: ascending when (p & kk) == 0.
__global__ __launch_bounds__(256) void anyk_sort_local_kernel(AnykSrc s, uint32_t* __restrict__ idx, int full, int kk)
{
    __shared__ uint32_t t[ANYK_TILE];
    const int base = (int)blockIdx.x * ANYK_TILE;
    const int tid = threadIdx.x;
    t[tid] = idx[base + tid];
    t[tid + 256] = idx[base + tid + 256];
    __syncthreads();
    for (int size = full ? 2 : kk; size <= (full ? ANYK_TILE : kk); size <<= 1) {
        for (int jj = min(size, ANYK_TILE) >> 1; jj > 0; jj >>= 1) {
            const int lo = 2 * tid - (tid & (jj - 1));          // the pair (lo, lo + jj) of this thread
            const int hi = lo + jj;
            const bool up = ((base + lo) & size) == 0;
            const uint32_t a = t[lo], b = t[hi];
            if (anyk_less(s, b, a) == up) { t[lo] = b; t[hi] = a; }
            __syncthreads();
        }
    }
    idx[base + tid] = t[tid];
    idx[base + tid + 256] = t[tid + 256];
}

// one compare-exchange step of stride jj (>= ANYK_TILE) of the merge of size kk
__global__ __launch_bounds__(256) void anyk_sort_global_kernel(AnykSrc s, uint32_t* __restrict__ idx, int np, int kk, int jj)
{
    const int q = (int)(blockIdx.x * 256u + threadIdx.x);
    if (q >= np / 2) return;
    const int lo = 2 * q - (q & (jj - 1));
    const int hi = lo + jj;
    const bool up = (lo & kk) == 0;
    const uint32_t a = idx[lo], b = idx[hi];
    if (anyk_less(s, b, a) == up) { idx[lo] = b; idx[hi] = a; }
}

// k <= 40: the entries whose k-mer equals allele k-mer j (seq2[off2 + j:][:k]) are the run idx[lo .. hi) of the sorted entries
__device__ __forceinline__ int anyk_bound(const AnykSrc& s, const uint32_t* __restrict__ idx, int n, const uint8_t* q, bool upper_bound)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int c = anyk_cmp(anyk_entry(s, idx[mid]), q, s.k);
        if (c < 0 || (upper_bound && c == 0)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void anyk_probe_kernel(AnykSrc s, const uint32_t* __restrict__ idx, int n, int nk2,
                                                         uint32_t* __restrict__ cnt, uint32_t* __restrict__ first)
{
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= nk2) return;
    const uint8_t* q = s.s2 + j;
    const int lo = anyk_bound(s, idx, n, q, false);
    const int hi = lo < n && anyk_cmp(anyk_entry(s, idx[lo]), q, s.k) == 0 ? anyk_bound(s, idx, n, q, true) : lo;
    cnt[j] = (uint32_t)(hi - lo);
    first[j] = (uint32_t)lo;
}

__global__ __launch_bounds__(256) void anyk_emit_kernel(AnykSrc s, const uint32_t* __restrict__ idx, int nk2, const uint32_t* __restrict__ cnt,
                                                        const uint32_t* __restrict__ first, const long long* __restrict__ off,
                                                        int2* __restrict__ dots)
{
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= nk2) return;
    const uint32_t c = cnt[j], f = first[j];
    const long long at = off[j];
    for (uint32_t r = 0; r < c; ++r) dots[at + r] = make_int2(j, anyk_pos(s, idx[f + r]));
}

// k > 40: sorted position p starts a key when its k-mer differs from that of p - 1.  The key's first entry e0 = idx[p] (the
// smallest e of the run: its first insertion) gets isfirst[e0] = 1 and its run (p, length) in run[e0].
__global__ __launch_bounds__(256) void anyk_group_kernel(AnykSrc s, const uint32_t* __restrict__ idx, int n, uint32_t* __restrict__ isfirst,
                                                         int2* __restrict__ run)
{
    const int p = (int)(blockIdx.x * 256u + threadIdx.x);
    if (p >= n) return;
    const uint8_t* a = anyk_entry(s, idx[p]);
    if (p > 0 && anyk_cmp(anyk_entry(s, idx[p - 1]), a, s.k) == 0) return;
    int q = p + 1;
    while (q < n && anyk_cmp(anyk_entry(s, idx[q]), a, s.k) == 0) ++q;
    isfirst[idx[p]] = 1u;
    run[idx[p]] = make_int2(p, q - p);
}

// the keys in order of first insertion: key r = (first entry, run start, run length); rank = exclusive scan of isfirst
__global__ __launch_bounds__(256) void anyk_rank_kernel(int n, const uint32_t* __restrict__ isfirst, const long long* __restrict__ rank,
                                                        const int2* __restrict__ run, int4* __restrict__ keys)
{
    const int e = (int)(blockIdx.x * 256u + threadIdx.x);
    if (e >= n || !isfirst[e]) return;
    const int2 r = run[e];
    keys[rank[e]] = make_int4(e, r.x, r.y, 0);
}

// Levenshtein distance (unit costs) of the pattern whose match masks are peq (a k-symbol query, k <= 64) and the k-symbol
// text t: Myers' bit-vector recurrence with Hyyro's global boundary (D[0][c] = c: a +1 enters the first row every column)
__device__ __forceinline__ int anyk_lev(const unsigned long long* peq, const uint8_t* t, int k)
{
    unsigned long long pv = ~0ull, mv = 0ull;
    const unsigned long long hb = 1ull << (k - 1);
    int score = k;
    for (int c0 = 0; c0 < k; c0 += 4) {
        const uint32_t w = anyk_word(t + c0);
        const int m = min(4, k - c0);
        for (int u = 0; u < m; ++u) {
            const unsigned long long eq = peq[(w >> (8 * u)) & 0xFFu];
            const unsigned long long xv = eq | mv;
            const unsigned long long xh = (((eq & pv) + pv) ^ pv) | eq;
            unsigned long long ph = mv | ~(xh | pv);
            unsigned long long mh = pv & xh;
            score += (ph & hb) ? 1 : ((mh & hb) ? -1 : 0);
            ph = (ph << 1) | 1ull;
            mh <<= 1;
            pv = mh | ~(xv | ph);
            mv = ph & xv;
        }
    }
    return score;
}

// One wave per allele k-mer j (4 per workgroup; this launch: j0 .. j1 - 1): the keys within distance k / 10 of it, 64 at a time
// in rank order.  EMIT = false: cnt[j] = dots of j; EMIT = true: the dots at off[j], in order (a wave prefix of the lanes' list
// lengths).  The host cuts a pair into launches of at most ANYK_EDIT_PAIRS (query, key) distance computations (~0.1 s each), so
// that a long pair does not hold the device in one kernel; vapor_set_param(ctx, "anyk_edit_pairs", v) puts another number in its
// place (the tests' way to the launches behind the first at small sizes).
template <bool EMIT>
__global__ __launch_bounds__(64 * ANYK_EDIT_WAVES) void anyk_edit_kernel(AnykSrc s, const uint32_t* __restrict__ idx, const int4* __restrict__ keys,
                                                                         const long long* __restrict__ n_keys, int j0, int j1,
                                                                         uint32_t* __restrict__ cnt, const long long* __restrict__ off,
                                                                         int2* __restrict__ dots)
{
    __shared__ unsigned long long peq_all[ANYK_EDIT_WAVES][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j = j0 + (int)blockIdx.x * ANYK_EDIT_WAVES + wv;
    unsigned long long* peq = peq_all[wv];
    for (int c = lane; c < 256; c += 64) peq[c] = 0ull;
    __syncthreads();
    const int k = s.k, tmax = k / 10;
    if (j < j1 && lane < k) atomicOr(&peq[s.s2[j + lane]], 1ull << lane);
    __syncthreads();
    if (j >= j1) return;                               // (wave-uniform; no barrier follows)
    const int D = (int)*n_keys;
    unsigned long long total = 0;
    long long at = EMIT ? off[j] : 0;
    for (int r0 = 0; r0 < D; r0 += 64) {
        const int r = r0 + lane;
        int len = 0, start = 0;
        if (r < D) {
            const int4 key = keys[r];
            if (anyk_lev(peq, anyk_entry(s, (uint32_t)key.x), k) <= tmax) { len = key.z; start = key.y; }
        }
        if (!EMIT) {
            total += (unsigned long long)len;
            continue;
        }
        if (!__any(len)) continue;
        int incl = len;                                   // inclusive wave prefix of the lengths
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        const long long mine = at + (incl - len);
        for (int u = 0; u < len; ++u) dots[mine + u] = make_int2(j, anyk_pos(s, idx[start + u]));
        at += __shfl(incl, 63, 64);
    }
    if (!EMIT) {
        for (int d = 32; d > 0; d >>= 1) total += __shfl_xor(total, d, 64);
        if (lane == 0) cnt[j] = (uint32_t)total;
    }
}

}  // namespace vapor
