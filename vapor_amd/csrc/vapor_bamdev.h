// vapor_bamdev.h - the read extraction of a batch of loci ON the device: `samtools view bam chrom:start-end`
// piped into chop_pacbio_read_by_pos (SF:339-354), which the reference runs as a process per locus and vapor_bam.cpp runs on
// host threads, for hundreds of regions at once.  The host reads the regions' BGZF blocks as they lie in the file and sends
// them over the link COMPRESSED (a third to a fifth of their inflated size); three kernels do the rest:
//
//   bgzf_inflate_kernel   one wavefront per BGZF block: DEFLATE (RFC 1951) decoded by lane 0 out of an LDS copy of the
//                         input straight into the block's place in the arena (HBM), the matches of a batch copied by all 64
//                         lanes, the block's CRC-32 taken by 64 lanes (a slice each, combined by multiplication mod P).
//                         Thousands of blocks are independent: that is the parallelism (a single DEFLATE stream has none),
//                         and twenty of them share a CU so that one's table lookup waits while another's shifts.
//   bam_chop_kernel       one wavefront per region: the BAM records of its index chunks walked in file order, the region
//                         rule of `samtools view`, POS <= start, the CIGAR walked to the window start 64 operations a step
//                         (cigar2alignstart_by_pos, SF:309-337; the CG:B,I long-CIGAR convention included), miss_bp and
//                         the length rule (SF:346-352) - the kept reads as (address of the packed bases, first base, miss_bp).
//   bam_expand_kernel     (vapor_seqset_create_mixed) the kept bases, 4 bits each in the arena, to the ASCII staging layout
//                         pack_kernel reads - what a host buffer and its copy over the link were before.
//
// Anything these kernels do not decide themselves - a block whose Huffman tables exceed the LDS tables, a record that runs
// past the blocks that were sent, a malformed field, a record without CIGAR, more kept reads than a region's slot holds -
// marks the REGION, and the caller sends that region down the host route (vapor_bam_chop), which also words the errors.
//
// The decoder core is written against a small set of macros so that tools/bamdev_emu.cpp compiles it for the host (one
// "lane" doing the wavefront's loops in order) and checks it against zlib on this machine; the kernels proper are HIP.
#pragma once
#include <stdint.h>
#include "vapor_names.h"
#include "vapor_readrec.h"      // BgzfBlk and the records of a region: what the host plans (vapor_readplan.h) and these kernels read

#ifndef VBD_EMU
#include <hip/hip_runtime.h>
#define VBD_DEV __device__ __forceinline__
// the lanes of one wavefront hand data to each other through LDS and through the block's own output in HBM: a wavefront's memory
// operations are performed in program order, so a fence of wavefront scope (which also keeps the compiler from moving accesses
// across it) is all the ordering there is to ask for - no workgroup barrier: the wavefronts of a workgroup decode different blocks
#define VBD_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#define VBD_WAVE_FOR(i, a, b) for (int i = (a) + (int)lane; i < (b); i += 64)
#define VBD_EACH_LANE(l) for (int l = (int)lane, once_ = 1; once_; once_ = 0)
#define VBD_LANE0 lane == 0
#define VBD_LANE_SLOTS 1
// Lane 0's decoding is scalar work: what it reads from LDS is declared uniform (v_readfirstlane), so that the shifts, masks,
// compares and branches on it go to the scalar unit - a vector instruction holds its SIMD for its issue slot however few lanes
// are on, and the wavefronts of a CU were queueing for the vector issue.
// Three flavours of the decoder (template flag SC).  Measured on 8 240 blocks of 64 KB (profiles/r05_bamdev.txt): all vector
// 23.6 ms, all scalar 17.9 ms, scalar control over vector data 16.0 ms - the product's; -DVBD_FLAVOUR=0 / 1 (developer builds)
// the others.
// SC = 1: everything lane 0 reads is declared uniform (data and control on the scalar unit); SC = 2: only what a branch looks at
// (VBD_CTL) - the bit buffer, the table entries, the cursors stay in vector registers, the decisions are scalar branches; SC = 0:
// nothing (vector code under exec masks).
#define VBD_UNI(x) (SC == 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(x)) : (uint32_t)(x))
#define VBD_CTL(x) (SC != 0 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(x)) : (uint32_t)(x))
#else
#define VBD_UNI(x) ((uint32_t)(x))
#define VBD_CTL(x) ((uint32_t)(x))
#define VBD_LANE_SLOTS 64
#define VBD_DEV static inline
#define VBD_SYNC() ((void)0)
#define VBD_WAVE_FOR(i, a, b) for (int i = (a); i < (b); ++i)
#define VBD_EACH_LANE(l) for (int l = 0; l < 64; ++l)
#define VBD_LANE0 (true)
#endif

#if (defined(VBD_TIMING) || defined(VBD_EXP_NOSTORE) || defined(VBD_EXP_NOMATCH) || defined(VBD_FLAVOUR) || defined(VBD_LLB) || defined(VBD_MIN_WAVES)) && \
    !defined(VAPOR_DEV_BUILD) && !defined(VBD_EMU)
#error "developer switch without -DVAPOR_DEV_BUILD: a product library cannot be an experimental one"
#endif
// -DVBD_TIMING (developer builds): lane 0 adds up the shader clock it spends per phase; the kernel stores the sums per block
#if defined(VBD_TIMING) && !defined(VBD_EMU)
#define VBD_T0() const long long vbd_t0_ = clock64()
#define VBD_T1(k) do { if (lane == 0) L.tm[k] += clock64() - vbd_t0_; } while (0)
#define VBD_COUNT(k) (++L.cn[k])
#else
#define VBD_T0() ((void)0)
#define VBD_T1(k) ((void)0)
#define VBD_COUNT(k) ((void)0)
#endif

namespace vapor_bamdev {

#ifndef VBD_LLB
#define VBD_LLB 9
#endif
constexpr int LLB = VBD_LLB, DB = 8, PREB = 7;       // first-level bits of the literal / length, distance and code-length tables
// first + second level entries a complete code can need - the bounds zlib's `enough` finds: 286 symbols, longest code 15, 9 bits
// first: 852 (10: 1334); 30 symbols, 8 bits: 402.  (A block is 7.4 KB of LDS with 9 bits: twenty blocks in flight a CU.)
constexpr int LL_CAP = LLB == 9 ? 852 : 1334, D_CAP = 402;
static_assert(LLB == 9 || LLB == 10, "table bound known for 9 and 10 bits");
constexpr uint32_t E_LIT = 1u << 13, E_EOB = 1u << 14, E_SUB = 1u << 15;
constexpr uint32_t E_LIT2 = 1u << 5;                 // first level of the literal / length table: TWO literals (bits 16-23, 24-31), bits 0-4 their lengths' sum
constexpr uint32_t Q_FILL = 1u << 31;                // match queue, distance word: the match repeats ONE known byte (bits 16-23): no load
constexpr int IN_CAP = 1280;                         // bytes of the compressed stream kept in LDS (twice the longest block header and a bit)
constexpr int Q_CAP = 64;                            // matches decoded before the wavefront copies them
constexpr int U_MAX = 65536;                         // BGZF: at most 64 KB of data a block

// status of a block
constexpr int BLK_OK = 0, BLK_BAD_STREAM = 1, BLK_TABLES = 2, BLK_CRC = 3, BLK_STALLED = 4;

struct InflateState {     // the decoder between batches (LDS; lane 0 works on a copy in registers)
    uint64_t buf;         // bit buffer
    int32_t n;            // valid bits in it (negative: the stream ran out)
    int32_t ip;           // next byte of `in` to load into the bit buffer
    int32_t in_have;      // bytes of `in` that are stream bytes
    uint32_t g_next;      // next byte of the payload (offset in it) to bring into `in`
    uint32_t op;          // output position
    int32_t phase;        // 0 block header next, 1 inside a Huffman block, 2 stored bytes to copy, 3 done, 4 error
    int32_t last;         // the block being decoded is the stream's last
    int32_t nq;           // matches queued in this batch
    uint32_t st_src, st_len;   // phase 2: stored bytes payload[st_src .. + st_len) go to op
    int32_t err;
    uint32_t known;       // the table entry of the literal that is the last output byte, 0 when the last byte came from a match
    uint32_t progress;    // bits consumed + bytes produced, for the no-progress check
};

struct InflateLds {
    uint32_t ll[LL_CAP + 2];
    union {
        uint32_t ds[D_CAP + 2];
        uint32_t pre[1 << PREB];    // (the code-length code is done with before the distance table is built)
    };
#if defined(VBD_TIMING) && !defined(VBD_EMU)
    long long tm[8];                // 0 top-up, 1 decode (tables included), 2 tables, 3 matches, 4 CRC
    long long cn[8];                // 0 fast literal steps, 1 symbols of the careful loop, 2 matches, 3 batches, 4 general symbols in the fast loop, 5 fills
#endif
    union {
        uint32_t q[2 * Q_CAP];      // per match: position | length << 16, distance (| Q_FILL)
        uint8_t sub_bits[1 << LLB]; // (table building only: a batch that reaches a block header with matches queued ends there)
    };
    union {
        uint32_t crc_part[64];      // (the end of a block)
        struct {                    // build_table's small arrays (dynamically indexed: registers would spill to scratch)
            int32_t count[16];
            uint32_t next[16], nx[16];
        };
    };
    InflateState st;
    uint32_t in_w[(IN_CAP + 16) / 4];   // the LDS copy of the stream (bytes; zeros behind in_have)
    uint8_t lens[288 + 32 + 16];
    uint8_t pl[20];
};

// ---------------------------------------------------------------------------------------------------------------------------
// Huffman tables (the entry format of vapor_inflate.h without its double literals: bits 0-4 code length left to consume, 8-12
// extra bits, 13 literal, 14 end of block, 15 second-level pointer, 16-31 payload)
// ---------------------------------------------------------------------------------------------------------------------------
VBD_DEV uint32_t bit_reverse(uint32_t v, int n)
{
#ifndef VBD_EMU
    return __brev(v) >> (32 - n);
#else
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1u); v >>= 1; }
    return r;
#endif
}

// length / distance bases and extra bits, packed (base << 16 | extra << 8) so that a symbol's entry is one table read
#ifndef VBD_EMU
__device__
#endif
static const uint32_t LEN_ENTRY[29] = {
    3u << 16, 4u << 16, 5u << 16, 6u << 16, 7u << 16, 8u << 16, 9u << 16, 10u << 16,
    (11u << 16) | (1u << 8), (13u << 16) | (1u << 8), (15u << 16) | (1u << 8), (17u << 16) | (1u << 8),
    (19u << 16) | (2u << 8), (23u << 16) | (2u << 8), (27u << 16) | (2u << 8), (31u << 16) | (2u << 8),
    (35u << 16) | (3u << 8), (43u << 16) | (3u << 8), (51u << 16) | (3u << 8), (59u << 16) | (3u << 8),
    (67u << 16) | (4u << 8), (83u << 16) | (4u << 8), (99u << 16) | (4u << 8), (115u << 16) | (4u << 8),
    (131u << 16) | (5u << 8), (163u << 16) | (5u << 8), (195u << 16) | (5u << 8), (227u << 16) | (5u << 8), 258u << 16};
#ifndef VBD_EMU
__device__
#endif
static const uint32_t DIST_ENTRY[30] = {
    1u << 16, 2u << 16, 3u << 16, 4u << 16, (5u << 16) | (1u << 8), (7u << 16) | (1u << 8), (9u << 16) | (2u << 8), (13u << 16) | (2u << 8),
    (17u << 16) | (3u << 8), (25u << 16) | (3u << 8), (33u << 16) | (4u << 8), (49u << 16) | (4u << 8), (65u << 16) | (5u << 8),
    (97u << 16) | (5u << 8), (129u << 16) | (6u << 8), (193u << 16) | (6u << 8), (257u << 16) | (7u << 8), (385u << 16) | (7u << 8),
    (513u << 16) | (8u << 8), (769u << 16) | (8u << 8), (1025u << 16) | (9u << 8), (1537u << 16) | (9u << 8), (2049u << 16) | (10u << 8),
    (3073u << 16) | (10u << 8), (4097u << 16) | (11u << 8), (6145u << 16) | (11u << 8), (8193u << 16) | (12u << 8),
    (12289u << 16) | (12u << 8), (16385u << 16) | (13u << 8), (24577u << 16) | (13u << 8)};

// kind: 0 code lengths, 1 literals / lengths, 2 distances.  0xFFFFFFFF: a symbol that must not appear in data.
VBD_DEV uint32_t symbol_entry(int kind, int sym)
{
    if (kind == 0) return (uint32_t)sym << 16;
    if (kind == 1) {
        if (sym < 256) return E_LIT | ((uint32_t)sym << 16);
        if (sym == 256) return E_EOB;
        if (sym > 285) return 0xFFFFFFFFu;
        return LEN_ENTRY[sym - 257];
    }
    if (sym > 29) return 0xFFFFFFFFu;
    return DIST_ENTRY[sym];
}

// Canonical code of n symbols with lengths len[] into a two-level table (vapor_inflate.h build_table, same acceptance rules:
// over-subscribed and - but for zlib's single one-bit code - incomplete codes are refused).  Serial: lane 0 runs it.
// Returns 0, BLK_BAD_STREAM or BLK_TABLES (the code needs more second-level entries than `cap` holds).
VBD_DEV int build_table(int kind, const uint8_t* len, int n, uint32_t* tab, int tbits, int cap, InflateLds& L)
{
    int32_t* count = L.count;
    uint32_t* next = L.next;
    uint32_t* nx = L.nx;
    uint8_t* sub_bits = L.sub_bits;
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[len[s] & 15];
    count[0] = 0;
    uint32_t code = 0;
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
        left = left * 2 - count[l];
        if (left < 0) return BLK_BAD_STREAM;
        code = (code + (uint32_t)count[l - 1]) << 1;
        next[l] = code;
    }
    const int first = 1 << tbits;
    for (int i = 0; i < first; ++i) tab[i] = 0;
    int longest = 15;
    while (longest > 0 && !count[longest]) --longest;
    if (longest == 0) return 0;
    if (left > 0 && (kind == 0 || longest != 1)) return BLK_BAD_STREAM;
    if (longest > tbits) {
        for (int i = 0; i < first; ++i) sub_bits[i] = 0;
        for (int l = 0; l < 16; ++l) nx[l] = next[l];
        for (int s = 0; s < n; ++s) {
            const int l = len[s] & 15;
            if (l <= tbits) { if (l) ++nx[l]; continue; }
            const uint32_t rev = bit_reverse(nx[l]++, l);
            const uint32_t lo = rev & (uint32_t)(first - 1);
            if (l - tbits > sub_bits[lo]) sub_bits[lo] = (uint8_t)(l - tbits);
        }
    }
    int used = first;
    for (int s = 0; s < n; ++s) {
        const int l = len[s] & 15;
        if (!l) continue;
        const uint32_t rev = bit_reverse(next[l]++, l);
        const uint32_t e = symbol_entry(kind, s);
        const bool banned = e == 0xFFFFFFFFu;
        if (l <= tbits) {
            const uint32_t v = banned ? 0u : (e | (uint32_t)l);
            for (uint32_t i = rev; i < (uint32_t)first; i += 1u << l) tab[i] = v;
        } else {
            const uint32_t lo = rev & (uint32_t)(first - 1);
            const int sb = sub_bits[lo];
            uint32_t head = tab[lo];
            if (!(head & E_SUB)) {
                if (used + (1 << sb) > cap) return BLK_TABLES;
                head = E_SUB | ((uint32_t)used << 16) | ((uint32_t)sb << 8) | (uint32_t)tbits;
                tab[lo] = head;
                for (int i = 0; i < (1 << sb); ++i) tab[used + i] = 0;
                used += 1 << sb;
            }
            const uint32_t base = head >> 16;
            const uint32_t v = banned ? 0u : (e | (uint32_t)(l - tbits));
            for (uint32_t i = rev >> tbits; i < (1u << sb); i += 1u << (l - tbits)) tab[base + i] = v;
        }
    }
    return 0;
}

// First-level literal entries whose following bits spell another literal inside the table's width become double entries (the
// decoder is bound by its lookup -> shift -> lookup chain: two symbols a lookup where the codes are short - BAM's packed bases
// are sixteen byte values of four or five bits).  In place, from the top: entry i reads entry i >> l1 < i, which is still single.
VBD_DEV void add_double_literals(uint32_t* tab, int tbits)
{
    for (int i = (1 << tbits) - 1; i >= 1; --i) {
        const uint32_t e = tab[i];
        if ((e & (E_LIT | E_SUB)) != E_LIT) continue;
        const int l1 = (int)(e & 31u);
        if (l1 >= tbits) continue;
        const uint32_t e2 = tab[(uint32_t)i >> l1];
        if ((e2 & (E_LIT | E_SUB | E_LIT2)) != E_LIT) continue;
        const int l2 = (int)(e2 & 31u);
        if (l1 + l2 > tbits) continue;
        tab[i] = E_LIT | E_LIT2 | (uint32_t)(l1 + l2) | (e & 0x00FF0000u) | ((e2 & 0x00FF0000u) << 8);
    }
}

// the bit reader over the LDS copy of the stream (zeros behind its end; n < 0 says bits were taken that are not there)
struct Bits {
    uint64_t buf;
    int n, ip, in_have;
    const uint32_t* in_w;
};
// Whole bytes up to 56..63 valid bits, out of three aligned words of the LDS copy.  The bits above n are not counted but
// they are the stream's own next bits (zeros behind its end): the next refill puts the same bits there again.
template <int SC>
VBD_DEV void refill(Bits& b)
{
    if (b.n < 0) return;
    int adv = (63 - b.n) >> 3;
    const int left = b.in_have - b.ip;
    if (adv > left) adv = left;
    if (adv <= 0) return;
    const uint32_t* w = b.in_w + (b.ip >> 2);
    const int sh = (b.ip & 3) * 8;
    const uint64_t lo = (uint64_t)VBD_UNI(w[0]) | ((uint64_t)VBD_UNI(w[1]) << 32);
    const uint64_t v = sh ? (lo >> sh) | ((uint64_t)VBD_UNI(w[2]) << (64 - sh)) : lo;
    b.buf |= v << b.n;
    b.ip += adv;
    b.n += adv * 8;
}
VBD_DEV uint32_t peek(const Bits& b, int k) { return (uint32_t)(b.buf & ((1ull << k) - 1ull)); }
VBD_DEV void drop(Bits& b, int k) { b.buf >>= k; b.n -= k; }
VBD_DEV uint32_t take(Bits& b, int k) { const uint32_t v = peek(b, k); drop(b, k); return v; }

VBD_DEV int read_fixed(InflateLds& L)
{
    for (int s = 0; s < 144; ++s) L.lens[s] = 8;
    for (int s = 144; s < 256; ++s) L.lens[s] = 9;
    for (int s = 256; s < 280; ++s) L.lens[s] = 7;
    for (int s = 280; s < 288; ++s) L.lens[s] = 8;
    int rc = build_table(1, L.lens, 288, L.ll, LLB, LL_CAP, L);
    if (rc) return rc;
    add_double_literals(L.ll, LLB);
    for (int s = 0; s < 32; ++s) L.lens[s] = 5;
    return build_table(2, L.lens, 32, L.ds, DB, D_CAP, L);
}

// the header of a dynamic block (RFC 1951 3.2.7); the caller has made sure `in` holds the whole of it (it is at most
// 14 + 19 * 3 + 316 * 14 bits = 562 bytes) or the end of the stream
template <int SC>
VBD_DEV int read_dynamic(Bits& b, InflateLds& L)
{
    const uint8_t ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    refill<SC>(b);
    const int hlit = (int)VBD_CTL(take(b, 5)) + 257, hdist = (int)VBD_CTL(take(b, 5)) + 1, hclen = (int)VBD_CTL(take(b, 4)) + 4;
    if (hlit > 286 || hdist > 30) return BLK_BAD_STREAM;
    uint8_t* pl = L.pl;
    for (int i = 0; i < 19; ++i) pl[i] = 0;
    for (int i = 0; i < hclen; ++i) {
        if ((int)VBD_CTL(b.n) < 3) refill<SC>(b);
        pl[ORDER[i]] = (uint8_t)take(b, 3);
    }
    if (b.n < 0) return BLK_BAD_STREAM;
    int rc = build_table(0, pl, 19, L.pre, PREB, 1 << PREB, L);
    if (rc) return rc;
    int i = 0;
    const int total = hlit + hdist;
    while (i < total) {
        refill<SC>(b);
        const uint32_t e = VBD_CTL(L.pre[peek(b, PREB)]);
        if (!e) return BLK_BAD_STREAM;
        drop(b, (int)(e & 31u));
        const int sym = (int)(e >> 16);
        if (sym < 16) { L.lens[i++] = (uint8_t)sym; continue; }
        int rep, val = 0;
        if (sym == 16) {
            if (i == 0) return BLK_BAD_STREAM;
            val = L.lens[i - 1];
            rep = 3 + (int)VBD_CTL(take(b, 2));
        } else if (sym == 17) {
            rep = 3 + (int)VBD_CTL(take(b, 3));
        } else {
            rep = 11 + (int)VBD_CTL(take(b, 7));
        }
        if (i + rep > total) return BLK_BAD_STREAM;
        for (int t = 0; t < rep; ++t) L.lens[i + t] = (uint8_t)val;
        i += rep;
        if (b.n < 0) return BLK_BAD_STREAM;
    }
    if (L.lens[256] == 0) return BLK_BAD_STREAM;
    rc = build_table(1, L.lens, hlit, L.ll, LLB, LL_CAP, L);
    if (rc) return rc;
    add_double_literals(L.ll, LLB);
    // (the distance lengths lie behind the literal / length ones; build_table reads them in place)
    return build_table(2, L.lens + hlit, hdist, L.ds, DB, D_CAP, L);
}

// the refill of the fast loop: the caller has made sure sixteen stream bytes lie behind ip, so nothing is clamped
template <int SC>
VBD_DEV void refill_fast(Bits& b)
{
    const uint32_t* w = b.in_w + (b.ip >> 2);
    const int sh = (b.ip & 3) * 8;
    const uint64_t lo = (uint64_t)VBD_UNI(w[0]) | ((uint64_t)VBD_UNI(w[1]) << 32);
    const uint64_t v = (lo >> sh) | (((uint64_t)VBD_UNI(w[2]) << 1) << (63 - sh));
    b.buf |= v << b.n;
    const int adv = (63 - b.n) >> 3;
    b.ip += adv;
    b.n += adv * 8;
}

// One batch of lane 0's work: block headers and symbols until Q_CAP matches are queued, the LDS copy of the stream runs low,
// stored bytes wait to be copied, the stream ends or an error is found.  Literals go straight to `out`; matches are queued
// (a match of distance 1 behind a byte lane 0 knows - a run - is queued as that byte: its copy needs no load).
template <int SC>
VBD_DEV void decode_batch(InflateLds& L, uint8_t* out, uint32_t u_len, uint32_t c_len)
{
    InflateState& S = L.st;
    VBD_COUNT(3);
    Bits b;
    b.buf = (uint64_t)VBD_UNI((uint32_t)S.buf) | ((uint64_t)VBD_UNI((uint32_t)(S.buf >> 32)) << 32);
    b.n = (int)VBD_UNI(S.n); b.ip = (int)VBD_UNI(S.ip); b.in_have = (int)VBD_CTL(S.in_have); b.in_w = L.in_w;
    uint32_t op = VBD_UNI(S.op), known = VBD_UNI(S.known);
    int phase = (int)VBD_CTL(S.phase), last = (int)VBD_CTL(S.last), nq = 0, err = 0;
    const bool all_loaded = VBD_CTL(S.g_next) >= c_len;
    constexpr uint32_t LL_MASK = (1u << LLB) - 1u, D_MASK = (1u << DB) - 1u;
#define VBD_IS_LIT1(e) (((e) & (E_LIT | E_SUB)) == E_LIT)
    // a match (len, dist) at op into the queue
#define VBD_QUEUE(len, dist)                                                                                     \
    do {                                                                                                         \
        uint32_t dw_ = (dist);                                                                                   \
        VBD_COUNT(2);                                                                                            \
        if (VBD_CTL((uint32_t)(dw_ == 1u && known != 0u))) {                                                     \
            VBD_COUNT(5);                                                                                        \
            const uint32_t byte_ = (known & E_LIT2) ? known >> 24 : (known >> 16) & 0xFFu;                       \
            dw_ = Q_FILL | (byte_ << 16) | 1u;                                                                   \
            known = E_LIT | (byte_ << 16);                                                                       \
        } else {                                                                                                 \
            known = 0;                                                                                           \
        }                                                                                                        \
        L.q[2 * nq] = op | ((len) << 16);                                                                        \
        L.q[2 * nq + 1] = dw_;                                                                                   \
        op += (len);                                                                                             \
        ++nq;                                                                                                    \
    } while (0)
    for (;;) {
        if (phase == 0) {
            // (building tables uses the match queue's bytes: the queued matches are copied first)
            if (nq) break;
            // a block header: all of it must be in `in` (600 bytes cover the longest), or the stream's end
            if (!all_loaded && b.in_have - (int)VBD_CTL(b.ip) < 600) break;
            refill<SC>(b);
            last = (int)VBD_CTL(take(b, 1));
            const uint32_t type = VBD_CTL(take(b, 2));
            if ((int)VBD_CTL(b.n) < 0) { err = BLK_BAD_STREAM; break; }
            if (type == 0) {
                // stored: to the byte boundary; LEN and NLEN; the bytes themselves are copied by the wavefront from the payload
                drop(b, b.n & 7);
                if ((int)VBD_CTL(b.n) < 32) refill<SC>(b);
                if ((int)VBD_CTL(b.n) < 32) { err = BLK_BAD_STREAM; break; }
                const uint32_t len = VBD_CTL(take(b, 16)), nlen = VBD_CTL(take(b, 16));
                if ((len ^ nlen) != 0xFFFFu) { err = BLK_BAD_STREAM; break; }
                // payload offset of the first stored byte: what `in` holds from ip on lies behind the bytes still in the bit buffer
                const uint32_t src = VBD_CTL(S.g_next - (uint32_t)(b.in_have - b.ip) - (uint32_t)(b.n >> 3));
                if (src > c_len || len > c_len - src || len > u_len - VBD_CTL(op)) { err = BLK_BAD_STREAM; break; }
                S.st_src = src; S.st_len = len;
                if (len) known = 0;
                phase = 2;
                break;
            }
            if (type == 3) { err = BLK_BAD_STREAM; break; }
#if defined(VBD_TIMING) && !defined(VBD_EMU)
            const long long tt0 = clock64();
#endif
            err = type == 1 ? read_fixed(L) : read_dynamic<SC>(b, L);
#if defined(VBD_TIMING) && !defined(VBD_EMU)
            L.tm[2] += clock64() - tt0;
#endif
            // (the table builders branch on what they read from LDS: what comes back from them is said to be uniform again, or
            // the compiler keeps the whole decoder state in vector registers from here on)
            err = (int)VBD_CTL(err);
            b.buf = (uint64_t)VBD_UNI((uint32_t)b.buf) | ((uint64_t)VBD_UNI((uint32_t)(b.buf >> 32)) << 32);
            b.n = (int)VBD_UNI(b.n); b.ip = (int)VBD_UNI(b.ip);
            if (err) break;
            phase = 1;
        }
        // ---- the fast loop: sixteen stream bytes behind ip (two refills that clamp nothing - a third could take the zeros behind
        // in_have for stream bits), eight bytes of room in the output (four double literals stored without a test).  The bit budget:
        // a refill leaves 64 stream bits in buf (n counts the whole bytes among them); a general symbol takes 48 at most
        // (15 + 5 + 15 + 13) and the first-level lookup that closes the iteration reads LLB more, so a general symbol is decoded
        // only where bits dropped since the last refill + 48 + LLB <= 64.  No bit count can go negative here.
        nq = (int)VBD_CTL(nq);
        if ((int)VBD_CTL(b.n) >= 0 && (int)VBD_CTL(b.ip) + 16 <= b.in_have && VBD_CTL(op) + 8 <= u_len) {
            refill_fast<SC>(b);
            uint32_t e = VBD_UNI(L.ll[(uint32_t)b.buf & LL_MASK]);
            bool leave = false;
            for (;;) {
                // (e is the first-level entry at the current position, read from LLB stream bits - the bit budget above sees to
                // that; the refill below leaves the bits that are there in place, so e still holds behind it)
                // (said to be uniform once more - it costs nothing where the compiler knows, and keeps the loop on the scalar
                // unit where a branch on something a table builder read made it doubt)
                b.buf = (uint64_t)VBD_UNI((uint32_t)b.buf) | ((uint64_t)VBD_UNI((uint32_t)(b.buf >> 32)) << 32);
                b.n = (int)VBD_UNI(b.n); b.ip = (int)VBD_UNI(b.ip); op = VBD_UNI(op); e = VBD_UNI(e); nq = (int)VBD_UNI(nq); known = VBD_UNI(known);
                if ((int)VBD_CTL(b.ip) + 16 > b.in_have || VBD_CTL(op) + 8 > u_len) break;
                refill_fast<SC>(b);
                if (VBD_IS_LIT1(VBD_CTL(e))) {
                    // up to four table hits out of one refill (40 of its 56 bits at most), each one literal or two: both bytes are
                    // stored either way, the cursor moves by one or two
#ifdef VBD_EXP_NOSTORE
#define VBD_ST(i, v) ((void)0)
#else
#define VBD_ST(i, v) (out[i] = (v))
#endif
#define VBD_EMIT()                                                                  \
    do {                                                                            \
        VBD_ST(op, (uint8_t)(e >> 16));                                             \
        VBD_ST(op + 1, (uint8_t)(e >> 24));                                         \
        op += 1u + ((e >> 5) & 1u);                                                 \
        known = e;                                                                  \
        VBD_COUNT(0);                                                               \
        b.buf >>= (e & 31u);                                                        \
        b.n -= (int)(e & 31u);                                                      \
        e = VBD_UNI(L.ll[(uint32_t)b.buf & LL_MASK]);                                        \
    } while (0)
                    VBD_EMIT();
                    if (VBD_IS_LIT1(VBD_CTL(e))) {
                        VBD_EMIT();
                        if (VBD_IS_LIT1(VBD_CTL(e))) {
                            VBD_EMIT();
                            if (VBD_IS_LIT1(VBD_CTL(e))) VBD_EMIT();
                        }
                    }
#undef VBD_EMIT
                    if (VBD_IS_LIT1(VBD_CTL(e))) continue;
                    if ((int)VBD_CTL(b.ip) + 8 > b.in_have || VBD_CTL(op) + 8 > u_len) break;
                    // (the symbol that follows takes 48 bits at most and the closing lookup LLB more: n >= 48 + LLB says that at most
                    // 63 - 48 - LLB bits were dropped since the refill.  With n < 48 alone the closing lookup could read zeros
                    // above the stream bits that were left - behind literals of 8 and more bits and a symbol of 40 and more -
                    // and a valid block ended as BLK_BAD_STREAM.)
                    if ((int)VBD_CTL(b.n) < 48 + LLB) refill_fast<SC>(b);
                }
                VBD_COUNT(4);
#if defined(VBD_TIMING) && !defined(VBD_EMU)
                const long long tg0 = clock64();
#endif
                uint32_t ec = VBD_CTL(e);                              // (what the branches look at)
                if (ec & E_SUB) {
                    drop(b, LLB);
                    e = VBD_UNI(L.ll[(e >> 16) + peek(b, (int)((e >> 8) & 31u))]);
                    ec = VBD_CTL(e);
                }
                if (!ec) { err = BLK_BAD_STREAM; leave = true; break; }
                drop(b, (int)(e & 31u));
                if (ec & E_LIT) {
                    out[op++] = (uint8_t)(e >> 16);
                    known = e;
                } else if (ec & E_EOB) {
                    phase = last ? 3 : 0;
                    leave = true;
                    break;
                } else {
                    const int xl = (int)((e >> 8) & 31u);
                    const uint32_t len = (e >> 16) + peek(b, xl);
                    drop(b, xl);
                    uint32_t f = VBD_UNI(L.ds[(uint32_t)b.buf & D_MASK]);
                    uint32_t fc = VBD_CTL(f);
                    if (fc & E_SUB) {
                        drop(b, DB);
                        f = VBD_UNI(L.ds[(f >> 16) + peek(b, (int)((f >> 8) & 31u))]);
                        fc = VBD_CTL(f);
                    }
                    if (!fc) { err = BLK_BAD_STREAM; leave = true; break; }
                    drop(b, (int)(f & 31u));
                    const int xd = (int)((f >> 8) & 31u);
                    const uint32_t dist = (f >> 16) + peek(b, xd);
                    drop(b, xd);
                    if (VBD_CTL((uint32_t)(dist > op || len > u_len - op))) { err = BLK_BAD_STREAM; leave = true; break; }
                    VBD_QUEUE(len, dist);
                    if (nq == Q_CAP) { leave = true; break; }
                }
                e = VBD_UNI(L.ll[(uint32_t)b.buf & LL_MASK]);
#if defined(VBD_TIMING) && !defined(VBD_EMU)
                L.tm[5] += clock64() - tg0;
#endif
            }
            if (err || nq == Q_CAP || phase == 3) break;
            if (leave) continue;                  // (the end of a block: the next header)
        }
        // ---- one symbol with every test (the ends of the input and of the output): 48 bits cover the longest (15 + 5 + 15 + 13)
        VBD_COUNT(1);
        if ((int)VBD_CTL(b.n) < 48) {
            if (!all_loaded && (int)VBD_CTL(b.ip) + 8 > b.in_have) break;
            refill<SC>(b);
        }
        uint32_t e = VBD_CTL(L.ll[(uint32_t)b.buf & LL_MASK]);      // (this loop runs a dozen times a block: all of it scalar where any is)
        if (e & E_SUB) {
            drop(b, LLB);
            e = VBD_CTL(L.ll[(e >> 16) + peek(b, (int)((e >> 8) & 31u))]);
        }
        if (!e) { err = BLK_BAD_STREAM; break; }
        drop(b, (int)(e & 31u));
        if ((int)VBD_CTL(b.n) < 0) { err = BLK_BAD_STREAM; break; }
        if (e & E_LIT) {
            if (VBD_CTL(op) >= u_len) { err = BLK_BAD_STREAM; break; }
            out[op++] = (uint8_t)(e >> 16);
            if (e & E_LIT2) {
                if (VBD_CTL(op) >= u_len) { err = BLK_BAD_STREAM; break; }
                out[op++] = (uint8_t)(e >> 24);
            }
            known = e;
            continue;
        }
        if (e & E_EOB) {
            if (last) { phase = 3; break; }
            phase = 0;
            continue;
        }
        const int xl = (int)((e >> 8) & 31u);
        const uint32_t len = (e >> 16) + peek(b, xl);
        drop(b, xl);
        uint32_t f = VBD_CTL(L.ds[(uint32_t)b.buf & D_MASK]);
        if (f & E_SUB) {
            drop(b, DB);
            f = VBD_CTL(L.ds[(f >> 16) + peek(b, (int)((f >> 8) & 31u))]);
        }
        if (!f) { err = BLK_BAD_STREAM; break; }
        drop(b, (int)(f & 31u));
        const int xd = (int)((f >> 8) & 31u);
        const uint32_t dist = (f >> 16) + peek(b, xd);
        drop(b, xd);
        if (VBD_CTL((uint32_t)(b.n < 0 || dist > op || len > u_len - op))) { err = BLK_BAD_STREAM; break; }
        VBD_QUEUE(len, dist);
        if (nq == Q_CAP) break;
    }
#undef VBD_QUEUE
#undef VBD_IS_LIT1
    S.buf = b.buf; S.n = b.n; S.ip = b.ip;
    S.op = op; S.phase = err ? 4 : phase; S.last = last; S.nq = nq; S.known = known;
    if (err) S.err = err;
}

// x^(8 * bytes) mod P in the reflected representation zlib's crc32_combine uses (bit 31 = x^0)
VBD_DEV uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & m) p ^= b;
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------------
// One BGZF block by one wavefront.  `out` is where the block's data goes in the arena (HBM): lane 0 stores the literals as it
// decodes them, the wavefront copies the matches from what it has written before, the CRC is read back from there (L2).  Only
// the tables, the LDS copy of the stream and the match queue live in LDS - 7.4 KB a block, twenty blocks in flight per CU (five
// wavefronts a SIMD: 16 -> 20 blocks a CU took 16.0 -> 12.4 ms on 8 240 blocks), which is what hides the latency of lane 0's
// lookup -> shift -> lookup chain.  crc_pow[l] = x^(8 * 1024 * (63 - l)) mod P.
// ---------------------------------------------------------------------------------------------------------------------------
// the byte table of the CRC-32 (one a workgroup; the CRC is a hundredth of a block's time: slicing tables would cost LDS that
// keeps a fourth workgroup off the CU)
struct CrcTables { uint32_t t[1][256]; };

template <int SC>
VBD_DEV int inflate_block_wave(InflateLds& L, const CrcTables& T, uint8_t* out, const uint8_t* payload, uint32_t c_len, uint32_t u_len,
                               uint32_t want_crc, const uint32_t* crc_pow, uint32_t lane)
{
    (void)lane;
    if (VBD_LANE0) {
        InflateState& S = L.st;
        S.buf = 0; S.n = 0; S.ip = 0; S.in_have = 0; S.g_next = 0; S.op = 0; S.phase = 0; S.last = 0; S.nq = 0;
        S.st_src = 0; S.st_len = 0; S.err = 0; S.known = 0; S.progress = 0xFFFFFFFFu;
    }
    VBD_SYNC();
    // every batch consumes input or produces output or ends; a stream of c_len bytes and u_len bytes of output cannot take more
    // batches than this (the no-progress check below ends a decoder that stops moving long before)
    const uint32_t max_batches = c_len + u_len + 64u;
    for (uint32_t batch = 0; batch < max_batches; ++batch) {
        // ---- top up the LDS copy of the stream: the unread bytes move to the front, new ones behind them
        {
            VBD_T0();
            const int ip = L.st.ip, have = L.st.in_have;
            const uint32_t g_next = L.st.g_next;
            if (g_next < c_len && (have == 0 || ip >= IN_CAP / 2)) {
                const int rest = have - ip;                       // (<= ip: source and destination do not overlap)
                uint8_t* in = reinterpret_cast<uint8_t*>(L.in_w);
                VBD_WAVE_FOR(i, 0, rest) in[i] = in[ip + i];
                uint32_t add = (uint32_t)(IN_CAP - rest);
                if (add > c_len - g_next) add = c_len - g_next;
                VBD_WAVE_FOR(i, 0, (int)add) in[rest + i] = payload[g_next + (uint32_t)i];
                VBD_WAVE_FOR(i, rest + (int)add, rest + (int)add + 16) if (i < IN_CAP + 16) in[i] = 0;
                VBD_SYNC();
                if (VBD_LANE0) { L.st.ip = 0; L.st.in_have = rest + (int)add; L.st.g_next = g_next + add; }
                VBD_SYNC();
            }
            VBD_T1(0);
        }
        {
            VBD_T0();
            if (VBD_LANE0) decode_batch<SC>(L, out, u_len, c_len);
            VBD_T1(1);
        }
        VBD_SYNC();
        VBD_T0();
        // ---- the batch's matches, in order (a match may read what an earlier one of the batch wrote)
#ifdef VBD_EXP_NOMATCH
        const int nq = 0;
#else
        const int nq = L.st.nq;
#endif
        for (int m = 0; m < nq;) {
            const uint32_t w = L.q[2 * m], dw = L.q[2 * m + 1];
            const uint32_t pos = w & 0xFFFFu, len = w >> 16;
            if (dw & Q_FILL) {
                // a run of one byte that lane 0 knew: stores alone
                const uint8_t byte = (uint8_t)(dw >> 16);
                VBD_WAVE_FOR(j, 0, (int)len) out[pos + (uint32_t)j] = byte;
                ++m;
                continue;
            }
            const uint32_t dist = dw;
            // up to four short matches that read nothing the others write (their sources end before the first one's destination):
            // their loads go out together, one wait instead of four
            if (len <= 64u && dist >= len) {
                uint32_t p_[4] = {pos, 0, 0, 0}, l_[4] = {len, 0, 0, 0}, d_[4] = {dist, 0, 0, 0};
                int g = 1;
                for (; g < 4 && m + g < nq; ++g) {
                    const uint32_t w2 = L.q[2 * (m + g)], d2 = L.q[2 * (m + g) + 1];
                    const uint32_t p2 = w2 & 0xFFFFu, l2 = w2 >> 16;
                    if ((d2 & Q_FILL) || l2 > 64u || d2 < l2 || p2 - d2 + l2 > pos) break;
                    p_[g] = p2; l_[g] = l2; d_[g] = d2;
                }
                uint8_t v_[4][VBD_LANE_SLOTS];
                VBD_EACH_LANE(l) {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if ((uint32_t)l < l_[t]) v_[t][l % VBD_LANE_SLOTS] = out[p_[t] - d_[t] + (uint32_t)l];
                }
                VBD_EACH_LANE(l) {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if ((uint32_t)l < l_[t]) out[p_[t] + (uint32_t)l] = v_[t][l % VBD_LANE_SLOTS];
                }
                VBD_SYNC();
                m += g;
                continue;
            }
            // byte j of the match is byte j mod dist of the dist bytes before it (RFC 1951 3.2.3: the copy may overlap itself)
            if (dist >= len) {
                VBD_WAVE_FOR(j, 0, (int)len) out[pos + (uint32_t)j] = out[pos - dist + (uint32_t)j];
            } else {
                VBD_WAVE_FOR(j, 0, (int)len) out[pos + (uint32_t)j] = out[pos - dist + (uint32_t)j % dist];
            }
            VBD_SYNC();
            ++m;
        }
        VBD_T1(3);
        const int phase = L.st.phase;
        if (phase == 2) {
            // stored bytes: payload -> image, then the stream goes on behind them (its LDS copy starts over)
            const uint32_t src = L.st.st_src, len = L.st.st_len, op = L.st.op;
            VBD_WAVE_FOR(i, 0, (int)len) out[op + (uint32_t)i] = payload[src + (uint32_t)i];
            VBD_SYNC();
            if (VBD_LANE0) {
                InflateState& S = L.st;
                S.op = op + len; S.buf = 0; S.n = 0; S.ip = 0; S.in_have = 0; S.g_next = src + len;
                S.phase = S.last ? 3 : 0;
            }
            VBD_SYNC();
        }
        if (L.st.phase >= 3) break;
        // no progress since the last batch: a decoder that waits for input that cannot come (damaged stream)
        const uint32_t prog = (L.st.g_next - (uint32_t)L.st.in_have + (uint32_t)L.st.ip) * 8u - (uint32_t)L.st.n + L.st.op * 16u + (uint32_t)L.st.phase;
        const uint32_t before = L.st.progress;
        VBD_SYNC();
        if (prog == before) { if (VBD_LANE0) { L.st.phase = 4; L.st.err = BLK_STALLED; } VBD_SYNC(); break; }
        if (VBD_LANE0) L.st.progress = prog;
        VBD_SYNC();
    }
    if (L.st.phase != 3) return L.st.err ? L.st.err : BLK_STALLED;
    if (L.st.op != u_len) return BLK_BAD_STREAM;
    VBD_T0();
    // ---- CRC-32: the data as the tail of 64 slices of 1 024 bytes (zeros in front change nothing in a register that starts at
    // zero; the register's start value 0xFFFFFFFF is the first four data bytes inverted), a slice a lane, then
    // crc = sum over lanes of slice_crc * x^(8 * bytes behind the slice) mod P
    if (u_len < 4) {
        if (VBD_LANE0) {
            uint32_t c = 0xFFFFFFFFu;
            for (uint32_t i = 0; i < u_len; ++i) c = T.t[0][(c ^ out[i]) & 0xFFu] ^ (c >> 8);
            L.crc_part[0] = ~c;
        }
        VBD_SYNC();
        return L.crc_part[0] == want_crc ? BLK_OK : BLK_CRC;
    }
    VBD_EACH_LANE(l) {
        const int lead = U_MAX - (int)u_len;                  // zero bytes in front of the data
        int a = l * 1024 - lead, e = a + 1024;                 // the slice in data coordinates
        if (a < 0) a = 0;
        uint32_t c = 0;
        int i = a;
        for (; i < e && i < 4; ++i) c = T.t[0][(c ^ out[i] ^ 0xFFu) & 0xFFu] ^ (c >> 8);
        for (; i < e; ++i) c = T.t[0][(c ^ out[i]) & 0xFFu] ^ (c >> 8);
        L.crc_part[l] = e > 0 ? crc_mulmod(crc_pow[l], c) : 0u;
    }
    VBD_SYNC();
    if (VBD_LANE0) {
        uint32_t c = 0;
        for (int l = 0; l < 64; ++l) c ^= L.crc_part[l];
        L.crc_part[0] = ~c;
    }
    VBD_SYNC();
    VBD_T1(4);
    return L.crc_part[0] == want_crc ? BLK_OK : BLK_CRC;
}

#ifndef VBD_EMU
// ---------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------
// Four wavefronts a workgroup, a BGZF block each.
constexpr int INFLATE_WAVES = 4;
#ifndef VBD_MIN_WAVES
#define VBD_MIN_WAVES 5             // wavefronts per SIMD the register budget is cut for (LDS admits five workgroups of four a CU)
#endif
__global__ __launch_bounds__(64 * INFLATE_WAVES, VBD_MIN_WAVES) void bgzf_inflate_kernel(const uint8_t* __restrict__ comp, const BgzfBlk* __restrict__ blks, int n_blks,
                                                                         uint8_t* arena, const uint32_t* __restrict__ crc_pow,
                                                                         int32_t* __restrict__ blk_status)
{
    __shared__ InflateLds L[INFLATE_WAVES];
    __shared__ CrcTables T;
    {
        const int i = (int)threadIdx.x;                      // (256 threads: an entry of each table a thread)
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        T.t[0][i] = c;
        __syncthreads();
    }
    const int wave = (int)(threadIdx.x >> 6);
    const int b = (int)blockIdx.x * INFLATE_WAVES + wave;
    if (b >= n_blks) return;
    const uint32_t lane = threadIdx.x & 63u;
    // (one block a wavefront: its descriptor is the same in every lane - said so, the addresses are scalar base + 32-bit offset)
    BgzfBlk k = blks[b];
    k.c_off = __builtin_amdgcn_readfirstlane(k.c_off); k.c_len = __builtin_amdgcn_readfirstlane(k.c_len);
    k.u_off = __builtin_amdgcn_readfirstlane(k.u_off); k.u_len = __builtin_amdgcn_readfirstlane(k.u_len);
    k.crc = __builtin_amdgcn_readfirstlane(k.crc);
#if defined(VBD_TIMING)
    if (lane == 0) for (int t = 0; t < 8; ++t) { L[wave].tm[t] = 0; L[wave].cn[t] = 0; }
    const long long t_all = clock64();
#endif
#ifndef VBD_FLAVOUR
#define VBD_FLAVOUR 2
#endif
    const int rc = inflate_block_wave<VBD_FLAVOUR>(L[wave], T, arena + k.u_off, comp + k.c_off, k.c_len, k.u_len, k.crc, crc_pow, lane);
    if (lane == 0) blk_status[b] = rc;
#if defined(VBD_TIMING)
    // (the sums go where the block's compressed bytes were: nothing reads those again)
    if (lane == 0 && k.c_len >= 128) {
        long long* d = reinterpret_cast<long long*>(const_cast<uint8_t*>(comp) + ((k.c_off + 7u) & ~7u));
        for (int t = 0; t < 5; ++t) d[t] = L[wave].tm[t];
        d[5] = clock64() - t_all;
        for (int t = 0; t < 6; ++t) d[6 + t] = L[wave].cn[t];
        d[12] = L[wave].tm[5];
    }
#endif
}

__device__ __forceinline__ uint32_t rd32u(const uint8_t* p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ long long wave_scan64(long long v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(v, (unsigned)d);
        if ((int)lane >= d) v += t;
    }
    return v;
}

// the CG:B,I array among a record's aux fields [p, end) (vapor_bam.cpp find_cg); returns its offset or 0, *count = its length
__device__ __forceinline__ uint32_t find_cg_dev(const uint8_t* arena, uint32_t p, uint32_t end, int32_t* count)
{
    // (every step moves p forward by three bytes at least: the loop ends)
    while (p + 3 <= end) {
        const uint8_t t0 = arena[p], t1 = arena[p + 1], ty = arena[p + 2];
        p += 3;
        int sz = 0;
        switch (ty) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': { while (p < end && arena[p]) ++p; if (p >= end) return 0; ++p; continue; }
        case 'B': {
            if (p + 5 > end) return 0;
            const uint8_t sub = arena[p];
            const int32_t cnt = (int32_t)rd32u(arena + p + 1);
            p += 5;
            const int es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (cnt < 0 || (long long)cnt * es > (long long)(end - p)) return 0;
            if (t0 == 'C' && t1 == 'G' && sub == 'I') { *count = cnt; return p; }
            p += (uint32_t)cnt * (uint32_t)es;
            continue;
        }
        default: return 0;
        }
        if ((uint32_t)sz > end - p) return 0;
        p += (uint32_t)sz;
    }
    return 0;
}

constexpr int HAPLOTAG_WAVES = 4;      // kept records a workgroup of bam_haplotag_kernel takes, a wavefront each

// One walk over a record's aux fields [p, end) for the first HP and PS fields of integer type and - WANT_CG - the CG:B,I array
// (vapor_bam.cpp find_tags and find_cg are the statement).  Wave-uniform like find_cg_dev: every lane reads the same bytes, but
// for a Z / H string, whose NUL is found 64 bytes a step, a byte a lane, with a ballot (methylation strings run to kilobytes).  B
// arrays are skipped by arithmetic.  The walk ends where all it looks for is found or at the end of the record; false for a
// malformed area (an unknown type, a field, string or array that runs past the record).
template <bool WANT_CG>
__device__ __forceinline__ bool walk_aux_dev(const uint8_t* arena, uint32_t p, uint32_t end, uint32_t lane, uint32_t* cg, int32_t* cg_count,
                                             int32_t* hap, long long* ps)
{
    bool have_hp = false, have_ps = false, have_cg = !WANT_CG;
    long long hp = 0;
    *ps = PS_NONE;
    *cg = 0;
    bool ok = true;
    // (every step moves p forward by three bytes at least: the loop ends)
    while (p + 3 <= end && !(have_hp && have_ps && have_cg)) {
        const uint8_t t0 = arena[p], t1 = arena[p + 1], ty = arena[p + 2];
        p += 3;
        if (ty == 'Z' || ty == 'H') {
            bool found = false;
            while (p < end) {
                const uint32_t q = p + lane;
                const unsigned long long m = __ballot(q < end && arena[q] == 0);
                if (m) { p += (uint32_t)__ffsll((long long)m); found = true; break; }
                p += 64u;
            }
            if (!found) { ok = false; break; }
            continue;
        }
        if (ty == 'B') {
            if (p + 5 > end) { ok = false; break; }
            const uint8_t sub = arena[p];
            const int32_t cnt = (int32_t)rd32u(arena + p + 1);
            p += 5;
            const int es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (cnt < 0 || (long long)cnt * es > (long long)(end - p)) { ok = false; break; }
            if (WANT_CG && !have_cg && t0 == 'C' && t1 == 'G' && sub == 'I') { *cg_count = cnt; *cg = p; have_cg = true; }
            p += (uint32_t)cnt * (uint32_t)es;
            continue;
        }
        const bool one = ty == 'c' || ty == 'C', two = ty == 's' || ty == 'S', four = ty == 'i' || ty == 'I';
        const uint32_t sz = (one || ty == 'A') ? 1u : two ? 2u : (four || ty == 'f') ? 4u : 0u;
        if (sz == 0u || sz > end - p) { ok = false; break; }
        if (one || two || four) {
            const bool is_hp = t0 == 'H' && t1 == 'P' && !have_hp, is_ps = t0 == 'P' && t1 == 'S' && !have_ps;
            if (is_hp || is_ps) {
                uint32_t raw = arena[p];
                if (sz >= 2u) raw |= (uint32_t)arena[p + 1] << 8;
                if (sz == 4u) raw |= ((uint32_t)arena[p + 2] << 16) | ((uint32_t)arena[p + 3] << 24);
                long long v = (long long)raw;
                if (ty == 'c') v = (long long)(int8_t)raw;
                else if (ty == 's') v = (long long)(int16_t)raw;
                else if (ty == 'i') v = (long long)(int32_t)raw;
                if (is_hp) { hp = v; have_hp = true; } else { *ps = v; have_ps = true; }
            }
        }
        p += sz;
    }
    *hap = (hp == 1 || hp == 2) ? (int32_t)hp : 0;
    return ok;
}

// One wavefront per region (vapor_bam.cpp bam_chop_impl is the statement this follows, line for line in its decisions).  TAGGED:
// every kept record's HP and PS go to tags[] beside its BamKept entry; a record whose aux area is malformed sends the region to
// the host route (REG_MALFORMED).  The unphased instantiation holds none of it.  RIGHT (`--both-ends`; the
// right-anchored branch of bam_chop_impl is its statement): the alignments whose last reference base is at or behind the window
// end, their CIGAR walked from its far end - a first pass over the operations for the reference length, a second over the tiles in
// reverse, lane l on operation n_ops - 1 - (t0 + l), so that the inclusive scans are suffix sums.  The entry's q0 is then the read
// base the reverse-complemented read starts with (l_seq - 1 - the bases dropped from the read's end), miss counts from the end.
// OPS (`--phase-vcf`): no aux walk for tags; where every kept record's operations, POS and bases lie goes to
// opsv[] beside its BamKept entry, for bam_haplotag_kernel.
template <bool TAGGED, bool RIGHT = false, bool OPS = false>
__device__ __forceinline__ void bam_chop_body(const uint8_t* __restrict__ arena, const BamRegion* __restrict__ regs,
                                              const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status, int n_regs,
                                              BamKept* __restrict__ kept, int32_t* __restrict__ n_kept, int32_t* __restrict__ reg_status,
                                              BamTag* __restrict__ tags, BamOps* __restrict__ opsv = nullptr)
{
    const int g = (int)blockIdx.x;
    if (g >= n_regs) return;
    const uint32_t lane = threadIdx.x;
    const BamRegion R = regs[g];
    const long long start = R.start, end = R.end;
    const long long beg = start - 1 > 0 ? start - 1 : 0, stop = end;
    const uint32_t flt_excl = (uint32_t)R.pad & 0xFFFFu, flt_mapq = ((uint32_t)R.pad >> 16) & 0xFFu;
    int nk = 0, st = REG_OK;
    // (its own walk: the tagged CG step reads the tags too; the evidence kernels share walk_records, below)
    for (int s = 0; s < R.span_n && st == REG_OK; ++s) {
        const BamSpan SP = spans[R.span_first + s];
        int bad = 0;
        for (uint32_t i = lane; i < SP.blk_n; i += 64) bad |= blk_status[SP.blk_first + i] != 0;
        if (__any(bad)) { st = REG_BLOCK; break; }
        uint32_t pos_u = SP.u_begin;
        // (a record is 36 bytes at least: pos_u grows every turn and the loop ends at u_end)
        while (pos_u < SP.u_end) {
            if ((unsigned long long)pos_u + 36ull > SP.u_limit) { st = REG_BEYOND; break; }
            uint32_t w = 0;
            if (lane < 6) w = rd32u(arena + pos_u + 4u * lane);
            const int32_t bs = (int32_t)__shfl(w, 0), ref_id = (int32_t)__shfl(w, 1), pos = (int32_t)__shfl(w, 2);
            const uint32_t w3 = __shfl(w, 3), w4 = __shfl(w, 4);
            const int32_t l_seq = (int32_t)__shfl(w, 5);
            if (bs < 32 || bs > (1 << 29)) { st = REG_MALFORMED; break; }
            if ((unsigned long long)pos_u + 4ull + (unsigned long long)bs > SP.u_limit) { st = REG_BEYOND; break; }
            const uint32_t r = pos_u + 4u;
            pos_u += 4u + (uint32_t)bs;
            const int l_name = (int)(w3 & 0xFFu), n_cig = (int)(w4 & 0xFFFFu);
            if (l_seq < 0 || 32ll + l_name + 4ll * n_cig + ((long long)l_seq + 1) / 2 + (long long)l_seq > (long long)bs) { st = REG_MALFORMED; break; }
            if (ref_id != R.tid || (long long)pos >= stop) {
                if (ref_id > R.tid || (ref_id == R.tid && (long long)pos >= stop)) break;
                continue;
            }
            // the read filter (vapor_bam_set_filter): MAPQ < min_mapq or FLAG & exclude_flags - as if the record
            // were not in the file.  Both fields were loaded with the record's header: no new load.
            if (((w3 >> 8) & 0xFFu) < flt_mapq || ((w4 >> 16) & flt_excl)) continue;
            // chop_pacbio_read_by_pos: only alignments that start at or before the window start (decided before the CIGAR is
            // read: the region rule below only skips)
            if (!RIGHT && !((long long)pos < start)) continue;
            const uint32_t cig = r + 32u + (uint32_t)l_name;
            const uint32_t sq = cig + 4u * (uint32_t)n_cig;
            const uint32_t rec_end = r + (uint32_t)bs;
            uint32_t ops = cig;
            int32_t n_ops = n_cig;
            int32_t hap = 0;
            long long ps = PS_NONE;
            bool have_tags = false;
            if (n_cig == 2) {
                const uint32_t o0 = rd32u(arena + cig), o1 = rd32u(arena + cig + 4);
                if ((o0 & 15u) == 4u && (int32_t)(o0 >> 4) == l_seq && (o1 & 15u) == 3u) {
                    int32_t cnt = 0;
                    if constexpr (TAGGED) {
                        // (the CG array and the tags in one walk)
                        uint32_t cg = 0;
                        if (!walk_aux_dev<true>(arena, sq + (uint32_t)((l_seq + 1) / 2) + (uint32_t)l_seq, rec_end, lane, &cg, &cnt, &hap, &ps)) { st = REG_MALFORMED; break; }
                        have_tags = true;
                        if (cg) { ops = cg; n_ops = cnt; }
                    } else {
                        const uint32_t cg = find_cg_dev(arena, sq + (uint32_t)((l_seq + 1) / 2) + (uint32_t)l_seq, rec_end, &cnt);
                        if (cg) { ops = cg; n_ops = cnt; }
                    }
                }
            }
            // 64 operations a step: the reference length of the region rule (M D N = X) and the walk of cigar2alignstart_by_pos
            // (query cursor: S I M =; reference cursor: M = D - not N, not X, as the reference has it) up to the first operation
            // after which the reference cursor has passed start - 1
            long long r1 = 0, rr = (long long)pos + 1, q = 0;
            bool r1_over = false, walked = false;
            uint32_t last = 0;
            if constexpr (RIGHT) {
                long long span = 0;
                for (int32_t t0 = 0; t0 < n_ops; t0 += 64) {
                    const int32_t t = t0 + (int32_t)lane;
                    const bool valid = t < n_ops;
                    const uint32_t o = valid ? rd32u(arena + ops + 4u * (uint32_t)t) : 15u;
                    const uint32_t code = o & 15u;
                    const long long n = (long long)(o >> 4);
                    const long long a = (code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) ? n : 0;
                    const long long b = (code == 0u || code == 7u || code == 2u) ? n : 0;
                    const long long A = wave_scan64(a, lane), B = wave_scan64(b, lane);
                    if (!r1_over) {
                        if (__any(valid && (long long)pos + r1 + A > beg)) r1_over = true;
                        r1 += __shfl(A, 63);
                    }
                    span += __shfl(B, 63);
                }
                if (!r1_over && (long long)pos + (r1 > 1 ? r1 : 1) <= beg) continue;
                const long long last_ref = (long long)pos + span;                 // 1-based
                if (!(last_ref >= end)) continue;
                if (n_ops <= 0) { st = REG_NO_CIGAR; break; }
                long long back = 0;                                               // reference bases walked from the far end
                for (int32_t t0 = 0; t0 < n_ops && !walked; t0 += 64) {
                    const int32_t t = n_ops - 1 - (t0 + (int32_t)lane);
                    const bool valid = t >= 0;
                    const uint32_t o = valid ? rd32u(arena + ops + 4u * (uint32_t)t) : 15u;
                    const uint32_t code = o & 15u;
                    const long long n = (long long)(o >> 4);
                    const long long b = (code == 0u || code == 7u || code == 2u) ? n : 0;
                    const long long c = (code == 4u || code == 1u || code == 0u || code == 7u) ? n : 0;
                    const long long B = wave_scan64(b, lane), C = wave_scan64(c, lane);
                    const unsigned long long m = __ballot(valid && last_ref - (back + B) < end + 1);
                    int f;
                    if (m) { f = __ffsll((long long)m) - 1; walked = true; }
                    else f = (n_ops - t0 > 64 ? 64 : n_ops - t0) - 1;            // (the tile's last operation)
                    last = __shfl(code, f);
                    q += __shfl(C, f);
                    back += __shfl(B, f);
                }
                rr = last_ref - back;                                             // the cursor: over = end - cursor
            } else
            for (int32_t t0 = 0; t0 < n_ops && !(r1_over && walked); t0 += 64) {
                const int32_t t = t0 + (int32_t)lane;
                const bool valid = t < n_ops;
                const uint32_t o = valid ? rd32u(arena + ops + 4u * (uint32_t)t) : 15u;
                const uint32_t code = o & 15u;
                const long long n = (long long)(o >> 4);
                const long long a = (code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) ? n : 0;
                const long long b = (code == 0u || code == 7u || code == 2u) ? n : 0;
                const long long c = (code == 4u || code == 1u || code == 0u || code == 7u) ? n : 0;
                const long long A = wave_scan64(a, lane), B = wave_scan64(b, lane), C = wave_scan64(c, lane);
                if (!r1_over) {
                    if (__any(valid && (long long)pos + r1 + A > beg)) r1_over = true;
                    r1 += __shfl(A, 63);
                }
                if (!walked) {
                    const unsigned long long m = __ballot(valid && rr + B > start - 1);
                    int f;
                    if (m) { f = __ffsll((long long)m) - 1; walked = true; }
                    else f = (n_ops - t0 > 64 ? 64 : n_ops - t0) - 1;        // (the tile's last operation)
                    last = __shfl(code, f);
                    q += __shfl(C, f);
                    rr += __shfl(B, f);
                }
            }
            // the region rule of `samtools view`
            if (!r1_over && (long long)pos + (r1 > 1 ? r1 : 1) <= beg) continue;
            if (n_ops <= 0) { st = REG_NO_CIGAR; break; }
            const long long over = RIGHT ? end - rr : rr - start;
            long long q0, miss;
            if (last == 0u || last == 7u) { q0 = q - over; miss = 0; } else { q0 = q; miss = over; }
            if (2 * miss > R.flank) continue;                                   // miss_bp > flank_length / 2
            const long long seq_len = l_seq > 0 ? l_seq : 1;
            const long long tail = q0 < seq_len ? seq_len - (q0 > 0 ? q0 : 0) : 0;
            const long long want_len = end - start - miss;
            if (q0 < 0) { st = REG_NEG_Q0; break; }
            if (want_len < 0 || !(tail > want_len)) continue;
            if (l_seq <= 0) { st = REG_NO_SEQ; break; }
            if (nk >= KEPT_CAP) { st = REG_KEPT_FULL; break; }
            if constexpr (TAGGED) {
                if (!have_tags) {
                    uint32_t cg = 0;
                    int32_t cnt = 0;
                    if (!walk_aux_dev<false>(arena, sq + (uint32_t)((l_seq + 1) / 2) + (uint32_t)l_seq, rec_end, lane, &cg, &cnt, &hap, &ps)) { st = REG_MALFORMED; break; }
                }
                if (lane == 0) tags[(size_t)g * KEPT_CAP + (size_t)nk] = BamTag{ps, hap, 0};
            }
            if constexpr (OPS) {
                if (lane == 0) opsv[(size_t)g * KEPT_CAP + (size_t)nk] = BamOps{ops, n_ops, pos, sq};
            }
            if (lane == 0) kept[(size_t)g * KEPT_CAP + (size_t)nk] = BamKept{sq, (int32_t)(RIGHT ? (long long)l_seq - 1 - q0 : q0), (int32_t)miss, l_seq};
            ++nk;
        }
    }
    if (lane == 0) { n_kept[g] = nk; reg_status[g] = st; }
}

__global__ __launch_bounds__(64) void bam_chop_kernel(const uint8_t* __restrict__ arena, const BamRegion* __restrict__ regs,
                                                     const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status, int n_regs,
                                                     BamKept* __restrict__ kept, int32_t* __restrict__ n_kept, int32_t* __restrict__ reg_status)
{
    bam_chop_body<false>(arena, regs, spans, blk_status, n_regs, kept, n_kept, reg_status, nullptr);
}

__global__ __launch_bounds__(64) void bam_chop_right_kernel(const uint8_t* __restrict__ arena, const BamRegion* __restrict__ regs,
                                                           const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status, int n_regs,
                                                           BamKept* __restrict__ kept, int32_t* __restrict__ n_kept, int32_t* __restrict__ reg_status)
{
    bam_chop_body<false, true>(arena, regs, spans, blk_status, n_regs, kept, n_kept, reg_status, nullptr);
}

__global__ __launch_bounds__(64) void bam_chop_tagged_kernel(const uint8_t* __restrict__ arena, const BamRegion* __restrict__ regs,
                                                            const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status, int n_regs,
                                                            BamKept* __restrict__ kept, int32_t* __restrict__ n_kept, int32_t* __restrict__ reg_status,
                                                            BamTag* __restrict__ tags)
{
    bam_chop_body<true>(arena, regs, spans, blk_status, n_regs, kept, n_kept, reg_status, tags);
}

__global__ __launch_bounds__(64) void bam_chop_ops_kernel(const uint8_t* __restrict__ arena, const BamRegion* __restrict__ regs,
                                                         const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status, int n_regs,
                                                         BamKept* __restrict__ kept, int32_t* __restrict__ n_kept, int32_t* __restrict__ reg_status,
                                                         BamOps* __restrict__ opsv)
{
    bam_chop_body<false, false, true>(arena, regs, spans, blk_status, n_regs, kept, n_kept, reg_status, nullptr, opsv);
}

// ---- the evidence readers (`--depth`, `--signatures`, `--links`, `--support`) ---------------------------
// A record that passed the walk, as walk_records hands it to its caller: wave-uniform, by value.
struct RecView {
    int32_t pos, l_seq;
    uint32_t flag_word;             // the header's FLAG << 16 | n_cigar_op
    uint32_t ops;                   // the operations in the arena, n_ops of them: the CG:B,I array of a `kS mN` record
    int32_t n_ops;
    uint32_t aux, end;              // the aux area [aux, end); end is the record's
};

// The record walk of the four evidence kernels, one wavefront a region (vapor_bam.cpp bam_walk_records is the host's statement;
// bam_chop_body's walk is where it comes from): the region's spans in order, a span with a damaged block REG_BLOCK; per record the
// six header words on lanes 0 to 5, the checks of size, staged bytes and layout with their statuses, the contig and order test
// that skips a record or ends the region at `stop`, the read filter (MAPQ below filter bits 16-23 or FLAG &
// filter bits 0-15 - as if the record were not in the file; both fields came with the header), the `kS mN` -> CG:B,I
// replacement.  on_record(RecView) is asked once per passing record and returns REG_OK to go on or the status that ends the
// region; the walk returns the region's status.
template <typename OnRecord>
__device__ __forceinline__ int walk_records(const uint8_t* __restrict__ arena, const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status,
                                            uint32_t lane, int32_t tid, long long stop, int32_t span_first, int span_n, uint32_t filter,
                                            OnRecord on_record)
{
    const uint32_t flt_excl = filter & 0xFFFFu, flt_mapq = (filter >> 16) & 0xFFu;
    int st = REG_OK;
    for (int s = 0; s < span_n && st == REG_OK; ++s) {
        const BamSpan SP = spans[span_first + s];
        int bad = 0;
        for (uint32_t i = lane; i < SP.blk_n; i += 64) bad |= blk_status[SP.blk_first + i] != 0;
        if (__any(bad)) { st = REG_BLOCK; break; }
        uint32_t pos_u = SP.u_begin;
        // (a record is 36 bytes at least: pos_u grows every turn and the loop ends at u_end)
        while (pos_u < SP.u_end) {
            if ((unsigned long long)pos_u + 36ull > SP.u_limit) { st = REG_BEYOND; break; }
            uint32_t w = 0;
            if (lane < 6) w = rd32u(arena + pos_u + 4u * lane);
            const int32_t bs = (int32_t)__shfl(w, 0), ref_id = (int32_t)__shfl(w, 1), pos = (int32_t)__shfl(w, 2);
            const uint32_t wd3 = __shfl(w, 3), wd4 = __shfl(w, 4);
            const int32_t l_seq = (int32_t)__shfl(w, 5);
            if (bs < 32 || bs > (1 << 29)) { st = REG_MALFORMED; break; }
            if ((unsigned long long)pos_u + 4ull + (unsigned long long)bs > SP.u_limit) { st = REG_BEYOND; break; }
            const uint32_t r = pos_u + 4u;
            pos_u += 4u + (uint32_t)bs;
            const int l_name = (int)(wd3 & 0xFFu), n_cig = (int)(wd4 & 0xFFFFu);
            if (l_seq < 0 || 32ll + l_name + 4ll * n_cig + ((long long)l_seq + 1) / 2 + (long long)l_seq > (long long)bs) { st = REG_MALFORMED; break; }
            if (ref_id != tid || (long long)pos >= stop) {
                if (ref_id > tid || (ref_id == tid && (long long)pos >= stop)) break;
                continue;
            }
            if (((wd3 >> 8) & 0xFFu) < flt_mapq || ((wd4 >> 16) & flt_excl)) continue;
            const uint32_t cig = r + 32u + (uint32_t)l_name;
            RecView rec{pos, l_seq, wd4, cig, n_cig, cig + 4u * (uint32_t)n_cig + (uint32_t)((l_seq + 1) / 2) + (uint32_t)l_seq, r + (uint32_t)bs};
            if (n_cig == 2) {
                const uint32_t o0 = rd32u(arena + cig), o1 = rd32u(arena + cig + 4);
                if ((o0 & 15u) == 4u && (int32_t)(o0 >> 4) == l_seq && (o1 & 15u) == 3u) {
                    int32_t cnt = 0;
                    const uint32_t cg = find_cg_dev(arena, rec.aux, rec.end, &cnt);
                    if (cg) { rec.ops = cg; rec.n_ops = cnt; }
                }
            }
            st = on_record(rec);
            if (st != REG_OK) break;
        }
    }
    return st;
}

__device__ __forceinline__ bool sig_is_clip(uint32_t o) { return (o & 15u) == 4u || (o & 15u) == 5u; }

// The clipped bases at a record's two ends, for a kernel that walks the operations 64 a step: tile(o, t0, n_ops) once per tile
// with the lane's operation.  The leading clip is operations 0 and 1 of the first tile; the trailing clip the last two
// operations, of which n_ops - 2 may be lane 63 of the tile before (carried in prev63).  A record of at most two operations
// that are all clips has neither event: lead = -1.
struct ClipEnds {
    long long lead = 0, trail = 0;
    uint32_t prev63 = 15u;          // operation t0 - 1
    __device__ __forceinline__ void tile(uint32_t o, int32_t t0, int32_t n_ops)
    {
        if (t0 == 0) {
            const uint32_t o0 = __shfl(o, 0), o1 = __shfl(o, 1);
            if (sig_is_clip(o0)) lead = (long long)(o0 >> 4) + ((n_ops >= 2 && sig_is_clip(o1)) ? (long long)(o1 >> 4) : 0);
            if (sig_is_clip(o0) && (n_ops == 1 || (n_ops == 2 && sig_is_clip(o1)))) lead = -1;
        }
        if (t0 + 64 >= n_ops) {
            const int32_t l = n_ops - 1 - t0;       // the lane of the last operation, 0..63
            const uint32_t ol = __shfl(o, l), op = l > 0 ? __shfl(o, l - 1) : prev63;
            if (sig_is_clip(ol)) trail = (long long)(ol >> 4) + ((n_ops >= 2 && sig_is_clip(op)) ? (long long)(op >> 4) : 0);
        }
        prev63 = __shfl(o, 63);
    }
};

// The mode of a histogram of offsets -tol .. tol (hist[i] counts offset i - tol; width = 2 tol + 1): one wave maximum over
// key = count << 10 | 1023 - rank, rank = 2 |offset| + (offset > 0) - the largest key is the largest count, then the smallest
// |offset|, then the negative one.  The same on every lane; offset 0 for an empty histogram.
struct HistMode { int32_t off; uint32_t cnt; };
__device__ __forceinline__ HistMode hist_mode(const uint32_t* hist, uint32_t width, long long tol, uint32_t lane)
{
    unsigned long long key = 0;
    for (uint32_t i = lane; i < width; i += 64) {
        const long long off = (long long)i - tol;
        const uint32_t rank = (uint32_t)(off < 0 ? -2 * off : 2 * off + 1);
        const unsigned long long k = ((unsigned long long)hist[i] << 10) | (unsigned long long)(1023u - rank);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d);
        key = o > key ? o : key;
    }
    const uint32_t cnt = (uint32_t)(key >> 10), rank = 1023u - (uint32_t)(key & 1023u);
    return {cnt ? ((rank & 1u) ? (int32_t)(rank >> 1) : -(int32_t)(rank >> 1)) : 0, cnt};
}

// Read depth of three consecutive intervals per region (`--depth`; vapor_bam.cpp bam_depth_impl is the host's
// statement, vapor_amd/depth.py cover the rule): one wavefront a region, walk_records to b3 with the depth question behind
// it.  Per passing record the operations go 64 a step: one wave_scan64 of the reference
// advance (M D N = X) gives every lane where its operation starts, the total is carried from tile to tile, and an M, = or X
// operation adds its overlap with each interval to the lane's three 64-bit sums.  A tile that ends at or behind b3 is the
// record's last (what follows starts behind every interval); a record at or behind b3 ends the region.  The sums are reduced
// across the wavefront once, at the end.  No kept-read table, no LDS; a record without operations covers nothing.
__device__ __forceinline__ unsigned long long depth_overlap(long long s, long long e, long long lo, long long hi)
{
    const long long a = s > lo ? s : lo, b = e < hi ? e : hi;
    return b > a ? (unsigned long long)(b - a) : 0ull;
}

__global__ __launch_bounds__(64) void bam_depth_kernel(const uint8_t* __restrict__ arena, const DepthRegion* __restrict__ regs,
                                                      const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status, int n_regs,
                                                      unsigned long long* __restrict__ cov, int32_t* __restrict__ reg_status)
{
    const int g = (int)blockIdx.x;
    if (g >= n_regs) return;
    const uint32_t lane = threadIdx.x;
    const DepthRegion R = regs[g];
    const long long b0 = R.b[0], b1 = R.b[1], b2 = R.b[2], b3 = R.b[3];
    unsigned long long c0 = 0, c1 = 0, c2 = 0;
    const int st = walk_records(arena, spans, blk_status, lane, R.tid, b3, R.span_first, R.span_n, R.filter, [&](const RecView rec) {
        long long cur = (long long)rec.pos;             // the reference cursor where the tile starts, 0-based
        for (int32_t t0 = 0; t0 < rec.n_ops && cur < b3; t0 += 64) {
            const int32_t t = t0 + (int32_t)lane;
            const uint32_t o = t < rec.n_ops ? rd32u(arena + rec.ops + 4u * (uint32_t)t) : 15u;
            const uint32_t code = o & 15u;
            const long long n = (long long)(o >> 4);
            const bool covers = code == 0u || code == 7u || code == 8u;
            const long long adv = (covers || code == 2u || code == 3u) ? n : 0;
            const long long A = wave_scan64(adv, lane);
            if (covers) {
                const long long e = cur + A, sb = e - n;
                c0 += depth_overlap(sb, e, b0, b1);
                c1 += depth_overlap(sb, e, b1, b2);
                c2 += depth_overlap(sb, e, b2, b3);
            }
            cur += __shfl(A, 63);
        }
        return (int)REG_OK;
    });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c0 += __shfl_down(c0, (unsigned)d);
        c1 += __shfl_down(c1, (unsigned)d);
        c2 += __shfl_down(c2, (unsigned)d);
    }
    if (lane == 0) {
        cov[3 * (size_t)g] = c0;
        cov[3 * (size_t)g + 1] = c1;
        cov[3 * (size_t)g + 2] = c2;
        reg_status[g] = st;
    }
}

// Split-read and CIGAR evidence per region (`--signatures`; vapor_bam.cpp bam_signature_impl is the host's
// statement, vapor_amd/signature.py answer the rule): one wavefront a region, walk_records to w3, and behind it the events of
// a record.  The operations go 64 a step to the record's end (RCLIP needs the reference end): one wave_scan64 of the reference
// advance gives every lane the cursor where its operation starts, and a D or N (GAP) or an I (INSOP) is tested on the lane
// that holds it; ClipEnds keeps the two clips.  Lanes 0 to 3 own the four clip bits (bit k: the leading clip for even k, the
// trailing for odd; target x0 below 2, x1 above), so a record's clip events cost one comparison on four lanes.  Counts are
// per-lane registers, reduced once; the two histograms are 2 * (2 * tol + 1) words of LDS, updated with LDS atomics by the lane
// that owns the event; the mode of each is hist_mode's.
__global__ __launch_bounds__(64) void bam_signature_kernel(const uint8_t* __restrict__ arena, const SigRegion* __restrict__ regs,
                                                          const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status, int n_regs,
                                                          uint32_t* __restrict__ ans, int32_t* __restrict__ reg_status)
{
    __shared__ uint32_t hist[SIG_HIST_WORDS];
    const int g = (int)blockIdx.x;
    if (g >= n_regs) return;
    const uint32_t lane = threadIdx.x;
    const SigRegion R = regs[g];
    const long long w3 = R.w3, x0 = R.x0, x1 = R.x1;
    // (the host made tol 0..255; the clamp keeps every histogram index inside the array whatever the table holds)
    const long long tol = R.tol < 0 ? 0 : (R.tol > SIG_TOL_MAX ? SIG_TOL_MAX : R.tol);
    const uint32_t width = 2u * (uint32_t)tol + 1u;
    const long long nmin = R.nmin, nmax = R.nmax, min_clip = R.min_clip;
    const uint32_t mask = R.mask;
    for (uint32_t i = lane; i < 2u * width; i += 64) hist[i] = 0u;
    __syncthreads();
    // this lane's clip bit, for lanes 0 to 3: which end of the record, which target, which histogram
    const bool my_clip = lane < 4u && ((mask >> lane) & 1u);
    const long long my_x = (lane & 2u) ? x1 : x0;
    const uint32_t my_hist = (lane & 2u) ? width : 0u;
    uint32_t c_clip = 0, c_gap = 0, c_ins = 0;
    // (an empty window has no records, whatever chunks came with it)
    const int st = walk_records(arena, spans, blk_status, lane, R.tid, w3, R.span_first, w3 > R.w0 ? R.span_n : 0, R.filter, [&](const RecView rec) {
        const int32_t n_ops = rec.n_ops;
        if (n_ops <= 0) return (int)REG_OK;             // no CIGAR: nothing, and no error
        long long cur = (long long)rec.pos;             // the reference cursor where the tile starts, 0-based
        ClipEnds clip;
        for (int32_t t0 = 0; t0 < n_ops; t0 += 64) {
            const int32_t t = t0 + (int32_t)lane;
            const uint32_t o = t < n_ops ? rd32u(arena + rec.ops + 4u * (uint32_t)t) : 15u;
            const uint32_t code = o & 15u;
            const long long n = (long long)(o >> 4);
            const long long adv = (code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) ? n : 0;
            const long long A = wave_scan64(adv, lane);
            const long long a = cur + A - adv;          // where this lane's operation starts
            if ((code == 2u || code == 3u) && (mask & SIG_GAP) && n >= nmin && n <= nmax) {
                const long long d0 = a - x0, d1 = a + n - x1;
                if (d0 >= -tol && d0 <= tol && d1 >= -tol && d1 <= tol) {
                    ++c_gap;
                    atomicAdd(&hist[(uint32_t)(d0 + tol)], 1u);
                    atomicAdd(&hist[width + (uint32_t)(d1 + tol)], 1u);
                }
            }
            if (code == 1u && (mask & SIG_INSOP) && n >= nmin && n <= nmax && a >= x0 - tol && a <= x1 + tol) {
                ++c_ins;
                const long long d0 = a - x0;
                if (d0 >= -tol && d0 <= tol) atomicAdd(&hist[(uint32_t)(d0 + tol)], 1u);
            }
            clip.tile(o, t0, n_ops);
            cur += __shfl(A, 63);
        }
        if (clip.lead < 0) return (int)REG_OK;
        if (my_clip) {
            const long long have = (lane & 1u) ? clip.trail : clip.lead;
            const long long d = ((lane & 1u) ? cur : (long long)rec.pos) - my_x;
            if (have >= min_clip && d >= -tol && d <= tol) {
                ++c_clip;
                atomicAdd(&hist[my_hist + (uint32_t)(d + tol)], 1u);
            }
        }
        return (int)REG_OK;
    });
    __syncthreads();
    // the six counts: lanes 0 to 3 hold the clip bits', the GAP and INSOP counts are sums over the wavefront
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c_gap += __shfl_down(c_gap, (unsigned)d);
        c_ins += __shfl_down(c_ins, (unsigned)d);
    }
    const uint32_t k0 = __shfl(c_clip, 0), k1 = __shfl(c_clip, 1), k2 = __shfl(c_clip, 2), k3 = __shfl(c_clip, 3);
    const HistMode m0 = hist_mode(hist, width, tol, lane), m1 = hist_mode(hist + width, width, tol, lane);
    if (lane == 0) {
        uint32_t* o = ans + (size_t)SIG_ANSWER_WORDS * (size_t)g;
        o[0] = k0; o[1] = k1; o[2] = k2; o[3] = k3; o[4] = c_gap; o[5] = c_ins;
        o[6] = (uint32_t)m0.off; o[7] = m0.cnt; o[8] = (uint32_t)m1.off; o[9] = m1.cnt;
        reg_status[g] = st;
    }
}

// ---- `--links` ----------------------------------------------------------------------------------------------
// The first aux field named SA among [p, end) (vapor_sa.h find_sa is the statement): 1 with the bytes before its NUL when its type
// is Z, 0 when there is none or its type is another, 2 for an area that is damaged before one is found.  walk_aux_dev's walk -
// wave-uniform, the NUL of a Z / H string found 64 bytes a step with a ballot, B arrays skipped by arithmetic - as a sibling:
// walk_aux_dev's instantiations are what they were.
__device__ __forceinline__ int find_sa_dev(const uint8_t* arena, uint32_t p, uint32_t end, uint32_t lane, uint32_t* value, uint32_t* len)
{
    *value = 0;
    *len = 0;
    // (every step moves p forward by three bytes at least: the loop ends)
    while (p + 3 <= end) {
        const uint8_t t0 = arena[p], t1 = arena[p + 1], ty = arena[p + 2];
        p += 3;
        const bool sa = t0 == 'S' && t1 == 'A';
        if (sa && ty != 'Z') return 0;
        if (ty == 'Z' || ty == 'H') {
            const uint32_t s = p;
            bool found = false;
            while (p < end) {
                const uint32_t q = p + lane;
                const unsigned long long m = __ballot(q < end && arena[q] == 0);
                if (m) { p += (uint32_t)__ffsll((long long)m); found = true; break; }
                p += 64u;
            }
            if (!found) return 2;
            if (sa) { *value = s; *len = p - 1u - s; return 1; }
            continue;
        }
        if (ty == 'B') {
            if (p + 5 > end) return 2;
            const uint8_t sub = arena[p];
            const int32_t cnt = (int32_t)rd32u(arena + p + 1);
            p += 5;
            const int es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (cnt < 0 || (long long)cnt * es > (long long)(end - p)) return 2;
            p += (uint32_t)cnt * (uint32_t)es;
            continue;
        }
        const uint32_t sz = (ty == 'A' || ty == 'c' || ty == 'C') ? 1u : (ty == 's' || ty == 'S') ? 2u : (ty == 'i' || ty == 'I' || ty == 'f') ? 4u : 0u;
        if (sz == 0u || sz > end - p) return 2;
        p += sz;
    }
    return 0;
}

__device__ __forceinline__ bool link_is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
// 1 for an operation letter that moves the reference cursor (M D N = X), 0 for another letter (I S H P), -1 for another byte
__device__ __forceinline__ int link_op_kind(uint8_t c)
{
    return (c == 'M' || c == 'D' || c == 'N' || c == '=' || c == 'X') ? 1 : (c == 'I' || c == 'S' || c == 'H' || c == 'P') ? 0 : -1;
}
__device__ __forceinline__ long long wave_sum64(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// a decimal field [s, e) of 1 .. max_digits (at most 10) digits, wave-uniform: a bounded field, ten bytes at the most
__device__ __forceinline__ bool link_number(const uint8_t* arena, uint32_t s, uint32_t e, uint32_t max_digits, long long* v)
{
    if (e <= s || e - s > max_digits) return false;
    long long x = 0;
    for (uint32_t q = s; q < e; ++q) {
        const uint8_t c = arena[q];
        if (!link_is_digit(c)) return false;
        x = 10 * x + (long long)(c - '0');
    }
    *v = x;
    return true;
}

// The entries of an SA value [v, vend) across the wavefront (vapor_sa.h for_each_piece / parse_piece is the statement).  Bit 0 of
// the result: the value has an entry (a well-formed piece at or above min_mapq); bit 1: one matches, *off = c - y of the first
// that does, in text order.  Piece by piece; the tiles of a piece are 64 bytes from the piece's start, a byte a lane.
//   The cut: one pass of tiles from the piece's start with a ballot for ';' and one for ','.  What is carried from tile to tile is
//   the number of commas seen and the places of the first five (five scalars, no array); the commas of the tile that holds the
//   ';' count only below it.  A sixth comma is an extra field, fewer than five a missing one.
//   pos, strand and mapq are bounded fields (10, 1 and 3 bytes) between known commas, read wave-uniformly; NM is unbounded: its
//   tiles are tested with a ballot for a byte that is no digit.
//   The CIGAR: a lane per byte; a lane that holds an operation letter reads its digits backwards from memory, up to ten bytes
//   or to the field's start - so a digit run that crosses a tile edge, or a letter on lane 0, needs no carry - and refuses
//   no digit, ten or more, or a length above 2^28 - 1; a byte that is neither a digit nor a letter, and a last byte that is no
//   letter, refuse the piece.  Every digit run then ends in a letter and has 1..9 digits: the field matches the grammar.  The
//   reference length is a wave sum a tile, carried in a 64-bit scalar.
//   The name is compared with the partner's 64 bytes a step, after the lengths.
__device__ __forceinline__ uint32_t link_scan_sa(const uint8_t* arena, uint32_t v, uint32_t vend, uint32_t lane, const uint8_t* __restrict__ pname,
                                                 uint32_t pname_len, bool rec_minus, bool differ, bool use_b, long long y, long long tol,
                                                 uint32_t min_mapq, long long* off)
{
    uint32_t res = 0;
    uint32_t s = v;
    // (every turn moves s behind a ';' or to the value's end: the loop ends)
    while (s < vend) {
        uint32_t e = vend, nc = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
        for (uint32_t t0 = s; t0 < vend; t0 += 64u) {
            const uint32_t q = t0 + lane;
            const uint8_t ch = q < vend ? arena[q] : (uint8_t)0;
            const unsigned long long ms = __ballot(ch == ';');
            unsigned long long mc = __ballot(ch == ',');
            uint32_t stop = 64u;
            if (ms) {
                stop = (uint32_t)__ffsll((long long)ms) - 1u;
                mc &= (1ull << stop) - 1ull;
            }
            while (mc && nc < 5u) {
                const uint32_t at = t0 + (uint32_t)__ffsll((long long)mc) - 1u;
                mc &= mc - 1ull;
                if (nc == 0u) c0 = at; else if (nc == 1u) c1 = at; else if (nc == 2u) c2 = at; else if (nc == 3u) c3 = at; else c4 = at;
                ++nc;
            }
            nc += (uint32_t)__popcll(mc);
            if (ms) { e = t0 + stop; break; }
        }
        const uint32_t piece = s;
        s = e + 1u;
        if (e == piece) continue;                               // an empty piece is dropped
        if (nc != 5u || c0 == piece) continue;                  // a missing or an extra field, an empty name
        long long pos = 0, mapq = 0;
        if (!link_number(arena, c0 + 1u, c1, 10u, &pos) || pos < 1 || pos > 0x7FFFFFFFll) continue;
        if (c2 - c1 != 2u) continue;
        const uint8_t strand = arena[c1 + 1u];
        if (strand != '+' && strand != '-') continue;
        if (!link_number(arena, c3 + 1u, c4, 3u, &mapq) || mapq > 255) continue;
        if (c4 + 1u >= e) continue;                             // an empty NM
        bool ok = true;
        for (uint32_t t0 = c4 + 1u; t0 < e; t0 += 64u) {
            const uint32_t q = t0 + lane;
            if (__any(q < e && !link_is_digit(arena[q]))) { ok = false; break; }
        }
        if (!ok) continue;
        const uint32_t cs = c2 + 1u, ce = c3;
        if (cs >= ce || link_op_kind(arena[ce - 1u]) < 0) continue;    // an empty CIGAR, one without its last letter
        long long span = 0;
        for (uint32_t t0 = cs; t0 < ce; t0 += 64u) {
            const uint32_t q = t0 + lane;
            const bool in = q < ce;
            const uint8_t ch = in ? arena[q] : (uint8_t)'0';
            const int kind = link_op_kind(ch);
            bool bad = !link_is_digit(ch) && kind < 0;
            long long n = 0;
            if (in && kind >= 0) {
                long long mul = 1;
                uint32_t d = 0;
                // (q - k >= cs: the lane reads inside the field, whatever tile the digits lie in)
                for (uint32_t k = 1; k <= 10u && q >= cs + k; ++k) {
                    const uint8_t c = arena[q - k];
                    if (!link_is_digit(c)) break;
                    d = k;
                    if (k <= 9u) { n += (long long)(c - '0') * mul; mul *= 10; }
                }
                bad = d < 1u || d > 9u || n > 0xFFFFFFFll;
            }
            if (__any(bad)) { ok = false; break; }
            span += wave_sum64(kind == 1 ? n : 0);
        }
        if (!ok) continue;
        if ((uint32_t)mapq < min_mapq) continue;                // a well-formed piece below the cut is ignored too
        res |= 1u;
        const long long a = pos - 1, c = use_b ? a + span : a;
        const long long d = c - y;
        if (d < -tol || d > tol || ((strand == '-') != rec_minus) != differ) continue;
        const uint32_t nlen = c0 - piece;
        if (nlen != pname_len) continue;
        bool same = true;
        for (uint32_t t0 = 0; t0 < nlen; t0 += 64u) {
            const uint32_t i = t0 + lane;
            if (__any(i < nlen && arena[piece + i] != pname[i])) { same = false; break; }
        }
        if (!same) continue;
        *off = d;
        return res | 2u;
    }
    return res;
}

// Split reads joined through their SA tags, per region (`--links`; vapor_bam.cpp bam_links_impl is the host's
// statement, vapor_amd/links.py answer the rule): one wavefront a region; the name check, then walk_records to w3.  A region asks
// for one clip event.  LCLIP needs the first two operations only; RCLIP the last two and the reference end, a wave sum per 64
// operations: the four operations are loaded directly, not through ClipEnds, so that a record without the event costs no tile.
// Only a clip record - the event within tol of x - pays for the aux walk to SA (find_sa_dev) and the scan of its value
// (link_scan_sa); a damaged aux area ends the region.  Everything about a record is wave-uniform here: the three counts are
// scalars, the histogram - 2 * tol + 1 words of LDS - takes one LDS atomic from lane 0 per linked record, and the mode is
// hist_mode's.
__global__ __launch_bounds__(64) void bam_link_kernel(const uint8_t* __restrict__ arena, const LinkRegion* __restrict__ regs,
                                                     const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status,
                                                     const uint8_t* __restrict__ names, uint32_t names_len, int n_regs,
                                                     uint32_t* __restrict__ ans, int32_t* __restrict__ reg_status)
{
    __shared__ uint32_t hist[LINK_HIST_WORDS];
    const int g = (int)blockIdx.x;
    if (g >= n_regs) return;
    const uint32_t lane = threadIdx.x;
    const LinkRegion R = regs[g];
    const long long w3 = R.w3, x = R.x, y = R.y;
    // (the host made tol 0..255; the clamp keeps every histogram index inside the array whatever the table holds)
    const long long tol = R.tol < 0 ? 0 : (R.tol > SIG_TOL_MAX ? SIG_TOL_MAX : R.tol);
    const uint32_t width = 2u * (uint32_t)tol + 1u;
    const long long min_clip = R.min_clip;
    const bool want_r = R.bits & LINK_EV, use_b = R.bits & LINK_PEND, differ = R.bits & LINK_REL;
    for (uint32_t i = lane; i < width; i += 64) hist[i] = 0u;
    __syncthreads();
    uint32_t n_clip = 0, n_split = 0, n_link = 0;
    int st = REG_OK;
    // (the host checked the name against the blob; a table that says otherwise is the host route's to refuse)
    if (R.name_len == 0u || R.name_off > names_len || R.name_len > names_len - R.name_off) st = REG_MALFORMED;
    const uint8_t* pname = names + R.name_off;
    // (an empty window has no records, whatever chunks came with it)
    if (st == REG_OK) st = walk_records(arena, spans, blk_status, lane, R.tid, w3, R.span_first, w3 > R.w0 ? R.span_n : 0, R.filter, [&](const RecView rec) {
        const uint32_t ops = rec.ops;
        const int32_t n_ops = rec.n_ops;
        if (n_ops <= 0) return (int)REG_OK;             // no CIGAR: nothing, and no error
        const uint32_t o0 = rd32u(arena + ops), o1 = n_ops >= 2 ? rd32u(arena + ops + 4u) : 15u;
        // (a record of at most two operations that are all clips has neither event)
        if (sig_is_clip(o0) && (n_ops == 1 || (n_ops == 2 && sig_is_clip(o1)))) return (int)REG_OK;
        long long have = 0, at = (long long)rec.pos;
        if (!want_r) {
            // LCLIP: the operations behind the first two are not walked
            if (sig_is_clip(o0)) have = (long long)(o0 >> 4) + (sig_is_clip(o1) ? (long long)(o1 >> 4) : 0);
        } else {
            const uint32_t ol = rd32u(arena + ops + 4u * (uint32_t)(n_ops - 1)), op = n_ops >= 2 ? rd32u(arena + ops + 4u * (uint32_t)(n_ops - 2)) : 15u;
            if (sig_is_clip(ol)) have = (long long)(ol >> 4) + (sig_is_clip(op) ? (long long)(op >> 4) : 0);
            if (have < min_clip) return (int)REG_OK;    // (no event: its reference end is not needed)
            for (int32_t t0 = 0; t0 < n_ops; t0 += 64) {
                const int32_t t = t0 + (int32_t)lane;
                const uint32_t o = t < n_ops ? rd32u(arena + ops + 4u * (uint32_t)t) : 15u;
                const uint32_t code = o & 15u;
                at += wave_sum64((code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) ? (long long)(o >> 4) : 0);
            }
        }
        const long long d = at - x;
        if (have < min_clip || d < -tol || d > tol) return (int)REG_OK;
        ++n_clip;
        uint32_t value = 0, len = 0;
        const int found = find_sa_dev(arena, rec.aux, rec.end, lane, &value, &len);
        if (found == 2) return (int)REG_MALFORMED;
        if (found != 1) return (int)REG_OK;
        long long off = 0;
        const uint32_t got = link_scan_sa(arena, value, value + len, lane, pname, R.name_len, ((rec.flag_word >> 16) & 0x10u) != 0u, differ, use_b, y, tol,
                                          (R.filter >> 16) & 0xFFu, &off);
        if (got & 1u) ++n_split;
        if (got & 2u) {
            ++n_link;
            if (lane == 0) atomicAdd(&hist[(uint32_t)(off + tol)], 1u);
        }
        return (int)REG_OK;
    });
    __syncthreads();
    const HistMode m = hist_mode(hist, width, tol, lane);
    if (lane == 0) {
        uint32_t* o = ans + (size_t)LINK_ANSWER_WORDS * (size_t)g;
        o[0] = n_clip; o[1] = n_split; o[2] = n_link; o[3] = (uint32_t)m.off; o[4] = m.cnt;
        reg_status[g] = st;
    }
}

// Alt and ref alignments per region (`--support`; vapor_bam.cpp bam_support_impl is the host's statement,
// vapor_amd/support.py answer the rule): one wavefront a region, walk_records to w3, and per record the signature kernel's tiles
// of 64 operations with ClipEnds.  The question is per record, not per event: each lane tests its own
// operation for "a GAP or INSOP that 4.20 counts", "blocks target 0" and "blocks target 1", __any makes the three answers
// wave-uniform and they are OR-ed over the record's tiles.  Behind the last tile the reference end, the two clips and the three
// flags are uniform, so the record's class and its coverage are a few uniform comparisons, and the seven counts are uniform
// registers: no LDS, no atomics, no reduction.  Lane 0 stores them.
__global__ __launch_bounds__(64) void bam_support_kernel(const uint8_t* __restrict__ arena, const SupRegion* __restrict__ regs,
                                                        const BamSpan* __restrict__ spans, const int32_t* __restrict__ blk_status, int n_regs,
                                                        uint32_t* __restrict__ ans, int32_t* __restrict__ reg_status)
{
    const int g = (int)blockIdx.x;
    if (g >= n_regs) return;
    const uint32_t lane = threadIdx.x;
    const SupRegion R = regs[g];
    const long long w3 = R.w3, x0 = R.x0, x1 = R.x1;
    const long long tol = R.tol, nmin = R.nmin, nmax = R.nmax, min_clip = R.min_clip;
    const long long F = R.flank, gmin = R.gmin;
    const uint32_t mask = R.mask;
    uint32_t n_cg = 0, n_l = 0, n_r = 0, n_ref0 = 0, n_ref1 = 0, n_cov0 = 0, n_cov1 = 0;
    // (an empty window has no records, whatever chunks came with it)
    const int st = walk_records(arena, spans, blk_status, lane, R.tid, w3, R.span_first, w3 > R.w0 ? R.span_n : 0, R.filter, [&](const RecView rec) {
        const int32_t n_ops = rec.n_ops;
        if (n_ops <= 0) return (int)REG_OK;             // no CIGAR: nothing, and no error
        long long cur = (long long)rec.pos;             // the reference cursor where the tile starts, 0-based
        ClipEnds clip;
        bool cg = false, blk0 = false, blk1 = false;    // the record's three flags, wave-uniform, OR-ed over its tiles
        for (int32_t t0 = 0; t0 < n_ops; t0 += 64) {
            const int32_t t = t0 + (int32_t)lane;
            const uint32_t o = t < n_ops ? rd32u(arena + rec.ops + 4u * (uint32_t)t) : 15u;
            const uint32_t code = o & 15u;
            const long long n = (long long)(o >> 4);
            const long long adv = (code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) ? n : 0;
            const long long A = wave_scan64(adv, lane);
            const long long a = cur + A - adv;          // where this lane's operation starts
            const bool gap = code == 2u || code == 3u, ins = code == 1u;
            bool my_cg = false;
            if (gap && (mask & SIG_GAP) && n >= nmin && n <= nmax) {
                const long long d0 = a - x0, d1 = a + n - x1;
                my_cg = d0 >= -tol && d0 <= tol && d1 >= -tol && d1 <= tol;
            }
            if (ins && (mask & SIG_INSOP) && n >= nmin && n <= nmax && a >= x0 - tol && a <= x1 + tol) my_cg = true;
            const bool big = n >= gmin;
            const bool my_b0 = big && ((gap && a < x0 + F && a + n > x0 - F) || (ins && a >= x0 - F && a <= x0 + F));
            const bool my_b1 = big && ((gap && a < x1 + F && a + n > x1 - F) || (ins && a >= x1 - F && a <= x1 + F));
            cg = cg || __any(my_cg);
            blk0 = blk0 || __any(my_b0);
            blk1 = blk1 || __any(my_b1);
            clip.tile(o, t0, n_ops);
            cur += __shfl(A, 63);
        }
        if (clip.lead < 0) return (int)REG_OK;          // (it covers no base either: nothing of the rule holds for it)
        // the record: [pos, q) on the reference, every value below is the same on all lanes
        const long long p = (long long)rec.pos, q = cur;
        const bool lc = clip.lead >= min_clip, tc = clip.trail >= min_clip;
        const long long dp0 = p - x0, dq0 = q - x0, dp1 = p - x1, dq1 = q - x1;
        const bool clip0 = ((mask & SIG_LCLIP0) && lc && dp0 >= -tol && dp0 <= tol) || ((mask & SIG_RCLIP0) && tc && dq0 >= -tol && dq0 <= tol);
        const bool clip1 = ((mask & SIG_LCLIP1) && lc && dp1 >= -tol && dp1 <= tol) || ((mask & SIG_RCLIP1) && tc && dq1 >= -tol && dq1 <= tol);
        const bool span0 = p <= x0 - F && q >= x0 + F && !blk0, span1 = p <= x1 - F && q >= x1 + F && !blk1;
        n_cg += cg ? 1u : 0u;
        n_l += (clip0 && !cg) ? 1u : 0u;
        n_r += (clip1 && !cg) ? 1u : 0u;
        n_ref0 += ((mask & SUP_REF0) && span0 && !cg && !clip0) ? 1u : 0u;
        n_ref1 += ((mask & SUP_REF1) && span1 && !cg && !clip1) ? 1u : 0u;
        n_cov0 += (p <= x0 && x0 < q) ? 1u : 0u;
        n_cov1 += (p <= x1 && x1 < q) ? 1u : 0u;
        return (int)REG_OK;
    });
    if (lane == 0) {
        uint32_t* o = ans + (size_t)SUP_ANSWER_WORDS * (size_t)g;
        o[0] = n_cg; o[1] = n_l; o[2] = n_r; o[3] = n_ref0; o[4] = n_ref1; o[5] = n_cov0; o[6] = n_cov1;
        reg_status[g] = st;
    }
}

// One record of a molecule per region (`--dedup-qname`, DESIGN.md 4.18 rule W; vapor_names.h holds the arithmetic, vapor_bam.cpp
// bam_chop_impl the host's statement): one wavefront a region, right behind the chop kernel on its stream and before
// bam_haplotag_kernel / bam_select_kernel, launched only for a handle with the option.  BamKept has no record offset, so the
// region's spans are walked once more as bam_chop_body walks them - six header words on lanes 0 to 5, pos_u += 4 + block_size,
// the same end of a span - and merged with the kept entries, which are in record order: the record whose packed bases start at
// kept[next].sq_off IS entry next.  Its name is hashed by the wavefront (lane l bytes 4l .. 4l + 3, never one behind the name;
// the powers of M from NAME_POW; a butterfly of shuffles), key and (FLAG & 0x900) != 0 go to LDS, the key to name_key[] as well.
// The layout was validated by the walk before this one; the bounds are tested again all the same, and a walk that ends before
// every kept entry was met sends the region to the host route (REG_MALFORMED).  Entry i is dropped iff an entry j has its key and
// (sec_j, j) < (sec_i, i) - all against all over LDS, a broadcast read.  A region without two equal keys - nearly every one - ends
// there.  Else kept[], tags[] (tagged call), opsv[] (ops flavour) and name_key[] are compacted in place in record order, a tile
// of 64 at a time: ballot of the survivors, prefix popcount, entries to registers, fence, store - the destination index is never
// above the source index and the tiles ascend, so nothing unread is overwritten - and lane 0 rewrites n_kept.
__device__ static const vapor_names::PowTable NAME_POW = vapor_names::PowTable();

__global__ __launch_bounds__(64) void bam_dedup_kernel(const uint8_t* __restrict__ arena, const BamRegion* __restrict__ regs,
                                                      const BamSpan* __restrict__ spans, int n_regs, BamKept* kept, int32_t* n_kept,
                                                      int32_t* reg_status, BamTag* tags, BamOps* opsv, uint64_t* name_key)
{
    __shared__ uint64_t s_key[KEPT_CAP];
    __shared__ uint8_t s_sec[KEPT_CAP];
    const int g = (int)blockIdx.x;
    if (g >= n_regs) return;
    const uint32_t lane = threadIdx.x;
    if (reg_status[g] != REG_OK) return;
    int n = n_kept[g];
    n = n < 0 ? 0 : (n > KEPT_CAP ? KEPT_CAP : n);
    // (a single kept record is walked for as well: its key is part of the call's answer)
    if (n < 1) return;
    BamKept* K = kept + (size_t)g * KEPT_CAP;
    uint64_t* NK = name_key + (size_t)g * KEPT_CAP;
    const BamRegion R = regs[g];
    const long long stop = R.end;
    // ---- the walk
    int next = 0;
    bool bad = false;
    uint32_t want = K[0].sq_off;
    for (int s = 0; s < R.span_n && next < n && !bad; ++s) {
        const BamSpan SP = spans[R.span_first + s];
        uint32_t pos_u = SP.u_begin;
        while (pos_u < SP.u_end && next < n) {
            if ((unsigned long long)pos_u + 36ull > SP.u_limit) { bad = true; break; }
            uint32_t w = 0;
            if (lane < 6) w = rd32u(arena + pos_u + 4u * lane);
            const int32_t bs = (int32_t)__shfl(w, 0), ref_id = (int32_t)__shfl(w, 1), pos = (int32_t)__shfl(w, 2);
            const uint32_t w3 = __shfl(w, 3), w4 = __shfl(w, 4);
            if (bs < 32 || bs > (1 << 29) || (unsigned long long)pos_u + 4ull + (unsigned long long)bs > SP.u_limit) { bad = true; break; }
            const uint32_t r = pos_u + 4u;
            pos_u += 4u + (uint32_t)bs;
            const int l_name = (int)(w3 & 0xFFu), n_cig = (int)(w4 & 0xFFFFu);
            if (32ll + l_name + 4ll * n_cig > (long long)bs) { bad = true; break; }
            if (ref_id != R.tid || (long long)pos >= stop) {
                if (ref_id > R.tid || (ref_id == R.tid && (long long)pos >= stop)) break;
                continue;
            }
            if (r + 32u + (uint32_t)l_name + 4u * (uint32_t)n_cig != want) continue;
            const int nl = l_name > 0 ? l_name - 1 : 0;
            uint64_t sum = vapor_names::lane_terms(arena + r + 32u, nl, (int)lane, NAME_POW.p);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum += (uint64_t)__shfl_xor((unsigned long long)sum, d);
            const uint64_t key = vapor_names::key_of_sum(nl, sum);
            if (lane == 0) {
                s_key[next] = key;
                s_sec[next] = (uint8_t)((((w4 >> 16) & vapor_names::SEC_FLAGS) != 0u) ? 1 : 0);
                NK[next] = key;
            }
            ++next;
            if (next < n) want = K[next].sq_off;
        }
    }
    if (bad || next != n) {
        if (lane == 0) reg_status[g] = REG_MALFORMED;
        return;
    }
    __syncthreads();
    if (n < 2) return;
    // ---- mark
    bool any = false;
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int i = t0 + (int)lane;
        if (__any(i < n && vapor_names::drops(s_key, s_sec, n, i))) any = true;
    }
    if (!any) return;
    // ---- compact
    BamTag* T = tags ? tags + (size_t)g * KEPT_CAP : nullptr;
    BamOps* O = opsv ? opsv + (size_t)g * KEPT_CAP : nullptr;
    int wr = 0;
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int i = t0 + (int)lane;
        const bool keep = i < n && !vapor_names::drops(s_key, s_sec, n, i);
        const unsigned long long m = __ballot(keep);
        const int dst = wr + __popcll(m & ((1ull << lane) - 1ull));
        // (a lane without a survivor loads entry 0 and stores nothing)
        const int src = keep ? i : 0;
        const BamKept k = K[src];
        const uint64_t ky = s_key[src];
        const BamTag tg = T ? T[src] : BamTag{0, 0, 0};
        const BamOps op = O ? O[src] : BamOps{0, 0, 0, 0};
        VBD_SYNC();
        if (keep && dst != i) {
            K[dst] = k;
            NK[dst] = ky;
            if (T) T[dst] = tg;
            if (O) O[dst] = op;
        }
        VBD_SYNC();
        wr += __popcll(m);
    }
    if (lane == 0) n_kept[g] = wr;
}

// The haplotag of every kept record from the phased heterozygous SNVs of its region (`--phase-vcf`, DESIGN.md 4.15;
// vapor_amd/phase.py haplotag is the statement, vapor_bam.cpp haplotag_record the host's): between bam_chop_ops_kernel and
// bam_select_kernel on their stream, one wavefront a kept record (HAPLOTAG_WAVES of them a workgroup, KEPT_CAP / HAPLOTAG_WAVES
// workgroups a region; a wavefront without a record ends at once).  The record's operations go 64 a step, a lane each, with
// SAM's cursors as inclusive scans (reference: M D N = X; query: M I S = X).  The region's sites, in position order, are
// consumed against each tile's reference range 64 a step; the lane whose M / = / X operation covers a site reads its base - the
// nibble arena[sq_off + (qi >> 1)], the high one for an even qi - and the vote goes to the lane that holds the site's phase set
// (its index in the region's table is below 64).  The pick - most votes, ties to the smallest ps value - is one wave reduction.
// What the chop kernel has checked is relied on: the operations and the packed bases lie inside the record (n_cig, l_seq and the
// CG array against the record's size), so no read here leaves it - a base index at or behind l_seq votes nothing.
__global__ __launch_bounds__(64 * HAPLOTAG_WAVES) void bam_haplotag_kernel(const uint8_t* __restrict__ arena, const BamKept* __restrict__ kept,
                                                                          const BamOps* __restrict__ opsv, const int32_t* __restrict__ n_kept,
                                                                          const int32_t* __restrict__ reg_status, int n_regs,
                                                                          const BamSiteRange* __restrict__ ranges, const BamSite* __restrict__ sites,
                                                                          const long long* __restrict__ ps_values, BamTag* __restrict__ tags)
{
    constexpr int PER = KEPT_CAP / HAPLOTAG_WAVES;
    const int g = (int)(blockIdx.x / PER);
    const int slot = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % PER) * HAPLOTAG_WAVES + (int)(threadIdx.x >> 6));
    if (g >= n_regs || reg_status[g] != REG_OK || slot >= n_kept[g]) return;
    const uint32_t lane = threadIdx.x & 63u;
    const size_t e = (size_t)g * KEPT_CAP + (size_t)slot;
    const BamOps O = opsv[e];
    const long long l_seq = kept[e].l_seq;
    const BamSiteRange SR = ranges[g];
    const BamSite* S = sites + SR.site_first;
    const int ns = SR.site_n;
    int n1 = 0, n2 = 0;                         // lane p: the votes of phase set p for haplotype 1 / 2
    long long rr = (long long)O.pos + 1, q = 0; // the cursors before the tile: 1-based reference position, query index
    int si = 0;                                 // sites consumed (wave-uniform)
    // the sites before the alignment's first base
    while (si < ns) {
        const int j = si + (int)lane;
        const unsigned long long m = __ballot(j < ns && (long long)S[j].pos < rr);
        const int c = m == ~0ull ? 64 : __ffsll((long long)~m) - 1;
        si += c;
        if (c < 64) break;
    }
    for (int32_t t0 = 0; t0 < O.n_ops && si < ns; t0 += 64) {
        const int32_t t = t0 + (int32_t)lane;
        const uint32_t o = t < O.n_ops ? rd32u(arena + O.ops_off + 4u * (uint32_t)t) : 15u;     // (code 15 advances nothing)
        const uint32_t code = o & 15u;
        const long long n = (long long)(o >> 4);
        const bool both = code == 0u || code == 7u || code == 8u;
        const long long a = (both || code == 2u || code == 3u) ? n : 0;
        const long long c = (both || code == 1u || code == 4u) ? n : 0;
        const long long A = wave_scan64(a, lane), C = wave_scan64(c, lane);
        const long long lo = rr + A - a, hi = rr + A, qs = q + C - c;     // this lane's operation: reference [lo, hi), query from qs
        const long long tile_end = rr + __shfl(A, 63);
        // the sites below the tile's end, in order (a site inside a D or N operation finds no lane)
        while (si < ns) {
            const int j = si + (int)lane;
            int32_t s_pos = 0;
            uint32_t s_al = 0;
            if (j < ns) { const BamSite s = S[j]; s_pos = s.pos; s_al = (uint32_t)s.a1 | ((uint32_t)s.a2 << 8) | ((uint32_t)s.ps_idx << 16); }
            const unsigned long long m = __ballot(j < ns && (long long)s_pos < tile_end);
            const int cnt = m == ~0ull ? 64 : __ffsll((long long)~m) - 1;
            for (int k = 0; k < cnt; ++k) {
                const long long v = (long long)__shfl(s_pos, k);
                const uint32_t al = __shfl(s_al, k);
                int vote = 0;
                if (both && v >= lo && v < hi) {
                    const long long qi = qs + (v - lo);
                    if (qi < l_seq) {
                        const uint32_t byte = arena[O.sq_off + (uint32_t)(qi >> 1)];
                        const uint32_t nib = (qi & 1) ? (byte & 15u) : (byte >> 4);
                        vote = nib == (al & 255u) ? 1 : nib == ((al >> 8) & 255u) ? 2 : 0;
                    }
                }
                const int v1 = __any(vote == 1) ? 1 : 0, v2 = __any(vote == 2) ? 1 : 0;
                if (lane == ((al >> 16) & 63u)) { n1 += v1; n2 += v2; }
            }
            si += cnt;
            if (cnt < 64) break;
        }
        rr = tile_end;
        q += __shfl(C, 63);
    }
    // the phase set with the most votes, ties to the smallest value
    int bt = n1 + n2, b1 = n1, b2 = n2;
    long long bk = (int)lane < SR.ps_n ? ps_values[SR.ps_first + (int)lane] : 0x7FFFFFFFFFFFFFFFll;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int ot = __shfl_xor(bt, d), o1 = __shfl_xor(b1, d), o2 = __shfl_xor(b2, d);
        const long long ok = __shfl_xor(bk, d);
        if (ot > bt || (ot == bt && ok < bk)) { bt = ot; b1 = o1; b2 = o2; bk = ok; }
    }
    if (lane == 0) {
        const bool called = bt > 0 && b1 != b2;
        tags[e] = BamTag{called ? bk : PS_NONE, called ? (b1 > b2 ? 1 : 2) : 0, 0};
    }
}

// The groups of a phased region (vapor_amd/phase.py select is the statement): one wavefront a region, right after the chop
// kernel on its stream.  From the region's up to KEPT_CAP kept entries and their tags: P = the ps value most frequent among the
// entries with hap != 0 (ties to the smallest value, "none" below every number); the lists of A (all entries), H1 and H2 (hap ==
// h and ps == P) under minimize_pacbio_read_list (SF:1091-1102: at most max_keep, record order when the group has no more, else
// a stable rank by (miss_bp, index)); the union of the three lists in record order, every member with its 3-bit membership and
// its position in each of its lists.  Counting is all-against-all over LDS (n <= 256: every lane reads the same entry, a
// broadcast); only the union - at most 3 * max_keep entries - and the region's BamPhase are for the host.
__global__ __launch_bounds__(64) void bam_select_kernel(const BamKept* __restrict__ kept, const BamTag* __restrict__ tags,
                                                       const int32_t* __restrict__ n_kept, const int32_t* __restrict__ reg_status, int n_regs,
                                                       int max_keep, BamPick* __restrict__ picks, BamPhase* __restrict__ phase)
{
    __shared__ long long s_key[KEPT_CAP];
    __shared__ int32_t s_miss[KEPT_CAP];
    __shared__ uint32_t s_grp[KEPT_CAP];       // the entry's hap, then its group bits
    __shared__ uint32_t s_mem[KEPT_CAP];       // its member word (0: in no list)
    const int g = (int)blockIdx.x;
    if (g >= n_regs) return;
    const int lane = (int)threadIdx.x;
    int n = reg_status[g] == REG_OK ? n_kept[g] : 0;
    n = n < 0 ? 0 : (n > KEPT_CAP ? KEPT_CAP : n);
    const BamKept* K = kept + (size_t)g * KEPT_CAP;
    const BamTag* T = tags + (size_t)g * KEPT_CAP;
    for (int e = lane; e < n; e += 64) {
        s_key[e] = T[e].ps;
        s_grp[e] = (uint32_t)T[e].hap;
        s_miss[e] = K[e].miss;
    }
    __syncthreads();
    // P: per tagged entry the number of tagged entries with its ps; the best (count, then the smallest ps) of the wavefront
    int best_c = 0;
    long long best_k = 0x7FFFFFFFFFFFFFFFll;
    for (int e = lane; e < n; e += 64) {
        if (s_grp[e] == 0u) continue;
        const long long key = s_key[e];
        int c = 0;
        for (int m = 0; m < n; ++m) c += (s_grp[m] != 0u && s_key[m] == key) ? 1 : 0;
        if (c > best_c || (c == best_c && key < best_k)) { best_c = c; best_k = key; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int oc = __shfl_xor(best_c, d);
        const long long ok = __shfl_xor(best_k, d);
        if (oc > best_c || (oc == best_c && ok < best_k)) { best_c = oc; best_k = ok; }
    }
    const bool tagged = best_c > 0;
    const long long P = tagged ? best_k : PS_NONE;
    __syncthreads();
    int cnt0 = 0, cnt1 = 0, cnt2 = 0;
    for (int e = lane; e < n; e += 64) {
        const uint32_t h = s_grp[e];
        const bool mine = tagged && s_key[e] == P;
        const uint32_t bits = 1u | ((mine && h == 1u) ? 2u : 0u) | ((mine && h == 2u) ? 4u : 0u);
        s_grp[e] = bits;
        cnt0 += 1; cnt1 += (int)((bits >> 1) & 1u); cnt2 += (int)((bits >> 2) & 1u);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { cnt0 += __shfl_xor(cnt0, d); cnt1 += __shfl_xor(cnt1, d); cnt2 += __shfl_xor(cnt2, d); }
    __syncthreads();
    const bool by_miss0 = cnt0 > max_keep, by_miss1 = cnt1 > max_keep, by_miss2 = cnt2 > max_keep;
    for (int e = lane; e < n; e += 64) {
        const uint32_t bits = s_grp[e];
        const int me = s_miss[e];
        int r0 = 0, r1 = 0, r2 = 0;
        for (int m = 0; m < n; ++m) {
            const uint32_t b = s_grp[m];
            const bool before = m < e, less = s_miss[m] < me || (s_miss[m] == me && before);
            r0 += (by_miss0 ? less : before) ? 1 : 0;
            r1 += (((b >> 1) & 1u) && (by_miss1 ? less : before)) ? 1 : 0;
            r2 += (((b >> 2) & 1u) && (by_miss2 ? less : before)) ? 1 : 0;
        }
        uint32_t w = 0;
        if (r0 < max_keep) w |= 1u | ((uint32_t)r0 << 8);
        if ((bits & 2u) && r1 < max_keep) w |= 2u | ((uint32_t)r1 << 16);
        if ((bits & 4u) && r2 < max_keep) w |= 4u | ((uint32_t)r2 << 24);
        s_mem[e] = w;
    }
    __syncthreads();
    int n_union = 0;
    BamPick* out = picks + (size_t)g * 3u * (size_t)max_keep;
    for (int e = lane; e < n; e += 64) {
        const uint32_t w = s_mem[e];
        if (!(w & 7u)) continue;
        int u = 0;
        for (int m = 0; m < e; ++m) u += (s_mem[m] & 7u) ? 1 : 0;
        // (every list holds at most max_keep entries: u < 3 * max_keep)
        if (u < 3 * max_keep) out[u] = BamPick{K[e].sq_off, K[e].q0, K[e].miss, w};
        ++n_union;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n_union += __shfl_xor(n_union, d);
    if (lane == 0) phase[g] = BamPhase{P, tagged ? 1 : 0, n_union};
}

// The bases of device-held reads (4 bits each, BAM's "=ACMGRSVTWYHKDBN") into the ASCII staging layout of pack_kernel: one
// thread per 32-byte chunk.  src[s] = 0 for a sequence that came from the host; else the address of its packed bases, first[s]
// its first base.  chunk_seq as pack_kernel reads it; seq_words = the sequence descriptors pack_kernel reads (vapor::SeqDesc,
// eight words each: word 1 the length, word 4 the first ASCII chunk).  A source with bit 63 of its address set (src_kind 2) is
// taken reverse complemented: base t of the sequence is the complement of base first[s] - t - the nibble with its bits reversed.
__global__ __launch_bounds__(256) void bam_expand_kernel(uint8_t* __restrict__ ascii, const uint32_t* __restrict__ chunk_seq, uint32_t n_chunks,
                                                        const uint32_t* __restrict__ seq_words,
                                                        const unsigned long long* __restrict__ src, const int32_t* __restrict__ first)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const uint32_t s = chunk_seq[c];
    const unsigned long long a0 = src[s];
    if (!a0) return;
    const bool rc = (a0 >> 63) != 0ull;
    const unsigned long long a = a0 & 0x7FFFFFFFFFFFFFFFull;
    const uint8_t* sq = reinterpret_cast<const uint8_t*>(a);
    const int base = (int)(c - seq_words[8u * s + 4u]) * 32;
    int valid = (int)seq_words[8u * s + 1u] - base;
    if (valid > 32) valid = 32;
    const long long i0 = rc ? (long long)first[s] - base : (long long)first[s] + base;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t < valid; ++t) {
        const long long i = rc ? i0 - t : i0 + t;
        const uint32_t byte = sq[i >> 1];
        uint32_t nib = (i & 1) ? (byte & 15u) : (byte >> 4);
        if (rc) nib = __brev(nib) >> 28;
        const uint32_t ch = (uint32_t)(uint8_t)"=ACMGRSVTWYHKDBN"[nib];
        w[t >> 2] |= ch << ((t & 3) * 8);
    }
    uint4* dst = reinterpret_cast<uint4*>(ascii + (size_t)c * 32);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
#endif  // VBD_EMU

}  // namespace vapor_bamdev
