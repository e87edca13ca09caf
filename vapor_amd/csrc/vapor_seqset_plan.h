// vapor_seqset_plan.h - the host plan of one vapor_seqset_create* call, without HIP: everything the four entries
// compute before their first allocation, between their copies and after their synchronisation.  The refusals of every entry in
// their order (check_args), the descriptors of the literal, derived and hidden sequences with the plane and staging chunks they
// take (Layout), the staging buffer with each table's place stated once (Staging), what is written into it (stage_range,
// fill_sources, fill_derived), the threaded staging that hands every slice on as soon as it is staged (stage_sliced), and what
// follows the counts the kernels send back (revcomp_refusal, raw_layout, fill_seq_info).  The messages carry the entries' names:
// an entry prepends nothing.  tools/seqset_check.cpp holds all of it to direct statements on the host under the sanitizers; the
// function in vapor_hip.hip is allocations, copies, the launches and one synchronisation.
#pragma once

#include "vapor_image.h"
#include "vapor_planner.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace vapor_seqset_plan {

using vapor::DSeg;
using vapor::HSeg;
using vapor::SeqDesc;
using vapor::ShareGroup;
using vapor_image::Refusal;
using vapor_image::Table;

constexpr uint64_t MAX_PLANE_CHUNKS = 0xFFFFFFF0ull;     // chunk0 is 32 bits: the planes of a set end below this many chunks
constexpr int64_t MAX_DERIVED_LEN = 0x7FFFFFF0LL;        // symbols of a derived sequence
constexpr int64_t MAX_SEQS = 0x7FFFFFF0LL;               // literals and derived sequences of a set
constexpr int64_t MAX_SRC_FIRST = 0x7FFFFFF0LL;          // first base of a device-held source
// the staging is threaded when the ASCII layout holds STAGE_SWITCH_BYTES or more in STAGE_SWITCH_SEQS sequences or more: slices of
// equal shares of the bytes, staged by the threads in order
constexpr size_t STAGE_SWITCH_BYTES = (size_t)4 << 20;
constexpr int32_t STAGE_SWITCH_SEQS = 8;
constexpr int STAGE_SLICES = 12;

inline size_t chunks_of(int64_t len) { return ((size_t)len + 31) / 32; }      // 32-symbol chunks (staged: 32 bytes each)

// A call as one of the four entries states it.  handles: context and output are there.  BLOB reads blob and off, the others seq;
// src_kind and src_first are MIXED's, the derived arguments DERIVED's and MIXED's (n_derived 0 and null elsewhere).
enum Entry { BLOB, PTRS, DERIVED, MIXED };
struct Call {
    Entry entry;
    bool handles;
    int32_t n_seqs;
    const uint8_t* blob;
    const int64_t* off;
    const uint8_t* const* seq;
    const int32_t* len;
    const uint8_t* flags;
    const uint8_t* src_kind;
    const int64_t* src_first;
    int32_t n_derived;
    const int32_t* seg_first;
    const vapor_segment* segs;
    const uint8_t* derived_flags;
    const uint8_t* src(int32_t i) const { return entry == BLOB ? blob + off[i] : seq[i]; }      // host bytes, or MIXED's device address
};

constexpr const char* NULL_ARGUMENT[4] = {"vapor_seqset_create: null argument", "vapor_seqset_create_ptrs: null argument",
                                          "vapor_seqset_create_derived: null argument", "vapor_seqset_create_mixed: null argument"};
constexpr const char* TOO_MANY[4] = {nullptr, nullptr, "vapor_seqset_create_derived: too many sequences", "vapor_seqset_create_mixed: too many sequences"};
constexpr const char* NULL_SEQUENCE[4] = {nullptr, "vapor_seqset_create_ptrs: null sequence", "vapor_seqset_create_derived: null sequence",
                                          "vapor_seqset_create_mixed: null sequence"};
constexpr const char* NEGATIVE_LENGTH = "negative sequence length";
constexpr const char* BAD_SOURCE = "vapor_seqset_create_mixed: bad source description";
constexpr const char* OUTSIDE_BATCH = "vapor_seqset_create_mixed: a device source outside every live batch";
constexpr const char* SET_TOO_LARGE = "sequence set too large";
// (the mixed entry lays out as the derived one does, and says so)
constexpr const char* BAD_SEGMENT_COUNT = "vapor_seqset_create_derived: bad segment count";
constexpr const char* SEGMENT_OUTSIDE = "vapor_seqset_create_derived: segment outside its parent";
constexpr const char* UPPER_RULE = "vapor_seqset_create_derived: a derived sequence without VAPOR_SEQ_UPPER over a parent uploaded with it";
constexpr const char* TOO_LONG = "vapor_seqset_create_derived: sequence too long";
constexpr const char* REVCOMP_DROPS = "vapor_seqset_create_derived: a reverse-complemented segment's parent holds characters complementary() drops "
                                      "(outside ATGCN/atgcn, SF:471-478); upload that allele as bytes";

// What an entry refuses before anything is laid out, in its order.  in_live_batch(a, b): the bytes a .. b (device addresses, both
// inclusive) lie inside the arena of one batch that is alive - nothing here reads them.  The mixed entry meets a negative length
// before a null sequence; the others leave it to Layout, which meets it sequence by sequence with the set's size.
template <typename InLiveBatch>
inline Refusal check_args(const Call& c, InLiveBatch in_live_batch)
{
    const bool der = c.entry == DERIVED || c.entry == MIXED;
    const bool sources = c.entry == BLOB ? c.blob && c.off : c.seq != nullptr;
    if (!c.handles || c.n_seqs < 0 || c.n_derived < 0 || (c.n_seqs && (!sources || !c.len)) || (c.n_derived && (!c.seg_first || !c.segs)))
        return {VAPOR_E_ARG, NULL_ARGUMENT[c.entry]};
    if (der && (int64_t)c.n_seqs + c.n_derived > MAX_SEQS) return {VAPOR_E_ARG, TOO_MANY[c.entry]};
    for (int32_t i = 0; c.entry != BLOB && i < c.n_seqs; ++i) {
        if (c.entry == MIXED && c.len[i] < 0) return {VAPOR_E_ARG, NEGATIVE_LENGTH};
        if (c.len[i] > 0 && !c.seq[i]) return {VAPOR_E_ARG, NULL_SEQUENCE[c.entry]};
        if (c.entry != MIXED || !c.src_kind || !c.src_kind[i]) continue;
        const int64_t len = c.len[i];
        if ((c.src_kind[i] != 1 && c.src_kind[i] != 2) || !c.src_first || c.src_first[i] < 0 || c.src_first[i] > MAX_SRC_FIRST ||
            (c.src_kind[i] == 2 && len > c.src_first[i] + 1))
            return {VAPOR_E_ARG, BAD_SOURCE};
        if (len == 0) continue;
        // the bytes that will be read must lie inside the arena of a batch that is alive
        const int64_t lo = c.src_kind[i] == 2 ? c.src_first[i] - len + 1 : c.src_first[i];      // (kind 2 reads downwards)
        if (!in_live_batch(c.seq[i] + (lo >> 1), c.seq[i] + ((lo + len - 1) >> 1))) return {VAPOR_E_ARG, OUTSIDE_BATCH};
    }
    return {};
}

// Where every sequence of the set lies: the literals, the caller's derived sequences, then the hidden shared ones (share_layout),
// each in whole chunks of the planes with VP_PAD_CHUNKS zeroed chunks behind it and VP_PAD_CHUNKS + 1 at the planes' end.  asc0 is
// a literal's first chunk of the ASCII staging, a derived or hidden sequence's first chunk among the derived chunks derive_kernel
// is launched over.  Built from the call's lengths and segments alone: no sequence byte is read.
struct Layout {
    int32_t n_lit = 0, n = 0;                      // literals; sequences the caller sees
    bool mixed = false;                            // some literal is held by the device (src_kind 1 or 2)
    std::vector<SeqDesc> h;                        // at least one, so that the set's descriptor block is never empty
    std::vector<std::vector<HSeg>> derived, hidden;
    std::vector<ShareGroup> groups;
    std::vector<int32_t> group_of, slot_of;
    size_t plane_chunks = 0, n_asc = 0, der_chunks = 0, n_seg = 0;
    size_t n_dseq() const { return h.size() - (size_t)n_lit; }      // derived and hidden sequences

    Refusal build(const Call& c, bool shared_join)
    {
        const int32_t n_seqs = c.n_seqs, n_derived = c.n_derived;
        n_lit = n_seqs;
        n = n_seqs + n_derived;
        h.assign((size_t)std::max(n, 1), SeqDesc{});
        size_t pl = 0;
        for (int32_t i = 0; i < n_seqs; ++i) {
            if (c.len[i] < 0) return {VAPOR_E_ARG, NEGATIVE_LENGTH};
            SeqDesc& d = h[(size_t)i];
            const size_t ch = chunks_of(c.len[i]);
            d.asc0 = (uint32_t)n_asc;
            d.chunk0 = (uint32_t)pl;
            d.len = c.len[i];
            d.flags = c.flags ? c.flags[i] : 0;
            mixed = mixed || (c.src_kind && c.src_kind[i]);
            n_asc += ch;
            pl += ch + VP_PAD_CHUNKS;
            if (pl > MAX_PLANE_CHUNKS) return {VAPOR_E_ARG, SET_TOO_LARGE};
        }
        // derived sequences (the caller's, then the hidden shared ones): planes behind the literals', assembled by derive_kernel
        if (n_derived > 0) {
            std::vector<uint8_t> dfl((size_t)n_derived, 0);
            derived.resize((size_t)n_derived);
            for (int32_t d = 0; d < n_derived; ++d) {
                const int32_t g0 = c.seg_first[d], g1 = c.seg_first[d + 1];
                if (g1 < g0 || g1 - g0 > VAPOR_MAX_SEGMENTS) return {VAPOR_E_ARG, BAD_SEGMENT_COUNT};
                int64_t tot = 0;
                for (int32_t g = g0; g < g1; ++g) {
                    const vapor_segment& x = c.segs[g];
                    if (x.parent < 0 || x.parent >= n_seqs || x.off < 0 || x.len < 0 || (int64_t)x.off + x.len > c.len[x.parent])
                        return {VAPOR_E_ARG, SEGMENT_OUTSIDE};
                    if (x.len == 0) continue;
                    // (a derived sequence is slices of its parents' BYTES: one that is not upper-cased itself cannot be cut from a
                    // parent that was upper-cased at upload - its planes hold the upper-cased text)
                    if (c.flags && (c.flags[x.parent] & VAPOR_SEQ_UPPER) && !(c.derived_flags && (c.derived_flags[d] & VAPOR_SEQ_UPPER)))
                        return {VAPOR_E_ARG, UPPER_RULE};
                    derived[(size_t)d].push_back(HSeg{x.parent, x.off, x.len, (int32_t)tot, (x.flags & VAPOR_SEG_REVCOMP) != 0});
                    tot += x.len;
                    if (tot > MAX_DERIVED_LEN) return {VAPOR_E_ARG, TOO_LONG};
                }
                dfl[(size_t)d] = c.derived_flags ? c.derived_flags[d] : 0;
                SeqDesc& dd = h[(size_t)(n_seqs + d)];
                dd.len = (int32_t)tot;
                dd.flags = dfl[(size_t)d];
            }
            if (shared_join) hidden = vapor::share_layout(h, n, n_seqs, derived, dfl, &groups, &group_of, &slot_of);
            h.resize((size_t)n + hidden.size(), SeqDesc{});
            for (size_t t = 0; t < hidden.size(); ++t) {
                int64_t tot = 0;
                for (const HSeg& x : hidden[t]) tot += x.len;
                h[(size_t)n + t].len = (int32_t)tot;
            }
            for (const ShareGroup& g : groups)
                if (g.t_seq >= 0 && g.upper) h[(size_t)g.t_seq].flags = VAPOR_SEQ_UPPER;
            for (size_t i = (size_t)n_seqs; i < h.size(); ++i) {
                SeqDesc& dd = h[i];
                const size_t ch = chunks_of(dd.len);
                dd.asc0 = (uint32_t)der_chunks;             // (first chunk among the derived sequences' chunks)
                dd.chunk0 = (uint32_t)pl;
                der_chunks += ch;
                pl += ch + VP_PAD_CHUNKS;
                if (pl > MAX_PLANE_CHUNKS) return {VAPOR_E_ARG, SET_TOO_LARGE};
            }
        }
        plane_chunks = pl + VP_PAD_CHUNKS + 1;
        for (const auto& v : derived) n_seg += v.size();
        for (const auto& v : hidden) n_seg += v.size();
        return {};
    }
    // the segments of derived or hidden sequence t (sequence n_lit + t)
    const std::vector<HSeg>& segments(size_t t) const { return t < derived.size() ? derived[t] : hidden[t - derived.size()]; }
};

// the first literal of every staging slice: slice k holds literals cut[k] .. cut[k + 1], which begin at or behind share k of the chunks
inline std::array<int32_t, STAGE_SLICES + 1> slice_cuts(const Layout& L)
{
    std::array<int32_t, STAGE_SLICES + 1> cut{};
    for (int t = 1; t < STAGE_SLICES; ++t) {
        const uint32_t want = (uint32_t)(L.n_asc * (size_t)t / (size_t)STAGE_SLICES);
        int32_t i = cut[(size_t)t - 1];
        while (i < L.n_lit && L.h[(size_t)i].asc0 < want) ++i;
        cut[(size_t)t] = i;
    }
    cut[STAGE_SLICES] = L.n_lit;
    return cut;
}

// The staging buffer of a call, kept in the context and sent piece by piece: the ASCII of the literals at offset 0 in 32-byte
// chunks, the chunk -> sequence map directly behind it (a set staged by one thread sends both in one copy of 36 bytes a chunk), on
// 8 bytes what bam_expand_kernel reads of a mixed set (a source word and a first base per literal), on 64 bytes what derive_kernel
// reads (the segment list, every derived sequence's first segment, the chunk -> sequence map of the derived chunks).  A table the
// call does not have takes no room.
struct Staging {
    Table<uint8_t> asc;
    Table<uint32_t> map;
    Table<unsigned long long> src;                 // mixed: the device address of a device-held literal, bit 63: reverse complemented
    Table<int32_t> first;                          // mixed: its first base
    Table<DSeg> segs;
    Table<int32_t> seg_first;
    Table<uint32_t> der_map;
    size_t mix_bytes = 0, der_bytes = 0;           // of the mixed block (from src.off) and of the derived block (from segs.off): one copy each
    size_t need = 0;                               // bytes of the buffer
    size_t host_end = 0;                           // the ASCII chunks the host has bytes for end here
    bool sliced = false;                           // enough to stage on several threads, in the slices `cut` (slice_cuts)
    std::array<int32_t, STAGE_SLICES + 1> cut{};

    template <typename T>
    static size_t put(Table<T>& t, size_t off, size_t n) { t.off = off; t.n = n; return off + t.bytes(); }

    Staging(const Call& c, const Layout& L)
    {
        const size_t n_seqs = (size_t)L.n_lit;
        size_t at = put(asc, 0, L.n_asc * 32);
        at = put(map, at, L.n_asc);
        at = (at + 7) & ~(size_t)7;
        const size_t mix_off = at;
        at = put(src, at, L.mixed ? n_seqs : 0);
        at = put(first, at, L.mixed ? n_seqs : 0);
        mix_bytes = at - mix_off;
        at = (at + 63) & ~(size_t)63;
        const size_t der_off = at;
        at = put(segs, at, L.der_chunks ? std::max<size_t>(L.n_seg, 1) : 0);
        at = put(seg_first, at, L.der_chunks ? L.n_dseq() + 1 : 0);
        at = put(der_map, at, L.der_chunks);
        der_bytes = at - der_off;
        need = std::max<size_t>(at, 64);
        // (the reads of a chunk of loci lie behind its windows: the usual mixed set sends the windows alone over the link)
        host_end = L.mixed ? 0 : L.n_asc;
        for (size_t i = 0; L.mixed && i < n_seqs; ++i)
            if (!c.src_kind[i] && L.h[i].len > 0) host_end = std::max(host_end, (size_t)L.h[i].asc0 + chunks_of(L.h[i].len));
        sliced = !L.mixed && L.n_asc * 32 >= STAGE_SWITCH_BYTES && L.n_lit >= STAGE_SWITCH_SEQS;
        if (sliced) cut = slice_cuts(L);
    }
    // the ASCII chunk slice k begins at (k = STAGE_SLICES: where the last one ends)
    size_t slice_chunk(const Layout& L, int k) const { return cut[(size_t)k] < L.n_lit ? L.h[(size_t)cut[(size_t)k]].asc0 : L.n_asc; }
};

// literals i0 .. i1 into the image: the map entries of their chunks, and - unless the device holds the literal - its bytes, zero
// padded to whole chunks
inline void stage_range(const Call& c, const Layout& L, const Staging& st, uint8_t* image, int32_t i0, int32_t i1)
{
    uint8_t* asc = st.asc.in(image);
    uint32_t* map = st.map.in(image);
    for (int32_t i = i0; i < i1; ++i) {
        const SeqDesc& d = L.h[(size_t)i];
        const size_t ch = chunks_of(d.len);
        for (size_t k = 0; k < ch; ++k) map[d.asc0 + k] = (uint32_t)i;
        if (L.mixed && c.src_kind[i]) continue;
        uint8_t* dst = asc + (size_t)d.asc0 * 32;
        if (d.len) memcpy(dst, c.src(i), (size_t)d.len);
        memset(dst + d.len, 0, ch * 32 - (size_t)d.len);
    }
}

// the mixed block: a device-held literal's address and first base travel instead of its bytes
inline void fill_sources(const Call& c, const Staging& st, uint8_t* image)
{
    unsigned long long* src = st.src.in(image);
    int32_t* first = st.first.in(image);
    for (size_t i = 0; i < st.src.n; ++i) {
        // (src_kind 2: the source reverse complemented from base src_first downwards - bit 63 tells bam_expand_kernel)
        src[i] = c.src_kind[i] ? (unsigned long long)reinterpret_cast<uintptr_t>(c.seq[i]) | (c.src_kind[i] == 2 ? 1ull << 63 : 0ull) : 0ull;
        first[i] = c.src_kind[i] ? (int32_t)c.src_first[i] : 0;
    }
}

// the derived block: every segment with its parent's first plane chunk, and the owner of every derived chunk
inline void fill_derived(const Layout& L, const Staging& st, uint8_t* image)
{
    if (!L.der_chunks) return;
    DSeg* segs = st.segs.in(image);
    int32_t* seg_first = st.seg_first.in(image);
    uint32_t* der_map = st.der_map.in(image);
    const size_t n_dseq = L.n_dseq();
    size_t w = 0;
    for (size_t t = 0; t < n_dseq; ++t) {
        seg_first[t] = (int32_t)w;
        for (const HSeg& x : L.segments(t)) segs[w++] = DSeg{L.h[(size_t)x.parent].chunk0, x.off, x.len, x.dst, x.rc ? 1u : 0u};
        const SeqDesc& dd = L.h[(size_t)L.n_lit + t];
        for (size_t k = 0; k < chunks_of(dd.len); ++k) der_map[dd.asc0 + k] = (uint32_t)((size_t)L.n_lit + t);
    }
    seg_first[n_dseq] = (int32_t)w;
}

// The threaded staging: n_thr threads stage the slices in turn (thread t slices t, t + n_thr, ..), and this thread hands
// send(c0, c1) the ASCII chunks c0 .. c1 of every slice that has any, in order, as soon as the slice is staged - the link works
// while the cores still copy.  The map is whole when this returns.
template <typename Send>
inline void stage_sliced(const Call& c, const Layout& L, const Staging& st, uint8_t* image, int n_thr, Send send)
{
    std::atomic<int> staged[STAGE_SLICES];
    for (auto& f : staged) f.store(0, std::memory_order_relaxed);
    std::vector<std::thread> th;
    for (int t = 0; t < n_thr; ++t)
        th.emplace_back([&, t] {
            for (int k = t; k < STAGE_SLICES; k += n_thr) {
                stage_range(c, L, st, image, st.cut[(size_t)k], st.cut[(size_t)k + 1]);
                staged[k].store(1, std::memory_order_release);
            }
        });
    for (int k = 0; k < STAGE_SLICES; ++k) {
        while (!staged[k].load(std::memory_order_acquire)) std::this_thread::yield();
        const size_t c0 = st.slice_chunk(L, k), c1 = st.slice_chunk(L, k + 1);
        if (c1 > c0) send(c0, c1);
    }
    for (auto& x : th) x.join();
}

// ---- after the synchronisation: L.h holds the counts the kernels made ----
// complementary() drops what is not ATGCN / atgcn (SF:471-478): a reversed slice of a window that holds such a character is not
// what the reference would have built
inline Refusal revcomp_refusal(const Layout& L)
{
    for (const auto& v : L.derived)
        for (const HSeg& x : v)
            if (x.rc && L.h[(size_t)x.parent].n_nocomp > 0) return {VAPOR_E_ARG, REVCOMP_DROPS};
    return {};
}

// where the bytes of the literals with symbols outside the alphabet (rare) are kept: raw_off[i] in a block of the returned size,
// every one on 16 bytes; -1: none
inline size_t raw_layout(const Layout& L, std::vector<int64_t>& raw_off)
{
    raw_off.assign(L.h.size(), -1);
    size_t raw_bytes = 0;
    for (int32_t i = 0; i < L.n_lit; ++i)
        if (L.h[(size_t)i].n_invalid > 0) { raw_off[(size_t)i] = (int64_t)raw_bytes; raw_bytes += ((size_t)L.h[(size_t)i].len + 15) & ~(size_t)15; }
    return raw_bytes;
}

inline void fill_seq_info(const Layout& L, int32_t* seq_info)
{
    for (int32_t i = 0; seq_info && i < L.n; ++i) {
        seq_info[2 * i] = L.h[(size_t)i].n_exc;
        seq_info[2 * i + 1] = L.h[(size_t)i].n_invalid;
    }
}

}  // namespace vapor_seqset_plan
