// vapor_readplan.h - the plan of a device reader call (the planning is host arithmetic without HIP), for
// vapor_bam_chop_device*, the four evidence calls and vapor_fasta_windows_device in vapor_hip.hip.  Plain C++17 over vapor_readrec.h and vapor_bgzf.h: which
// regions are refused and why, which file ranges are read and where they go in the staging block, where every span, stretch and
// block lands in the arena, where the tables lie in the call's metadata block, what the host reads back and how that becomes the
// caller's arrays.  The .hip keeps the reads, the allocations, the copies and the launches.  tools/readplan_check.cpp holds all of
// it to direct statements of its rules on the host under the sanitizers.
#pragma once

#include "vapor_bgzf.h"
#include "vapor_hip.h"
#include "vapor_readrec.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace vapor_readplan {

using namespace vapor_bamdev;
using namespace vapor_fasta;
using vapor_bgzf::FaStretch;
using vapor_bgzf::HostSpan;

// why a call as a whole is refused: a VAPOR_E_* code and the text of vapor_last_error (code 0: it is not)
struct Refusal {
    int code = 0;
    const char* msg = nullptr;
    explicit operator bool() const { return code != 0; }
};

inline size_t pad64(size_t bytes) { return (bytes + 63) & ~(size_t)63; }

// A table of a metadata block.  The block is carved once, by the constructor of ChopMeta or FastaMeta; everything else asks the
// table for its entries in the host's or the device's copy of the block.  A table the call's mode does not have takes no room.
template <typename T>
struct Table {
    size_t off = 0, n = 0;
    T* in(uint8_t* block) const { return n ? reinterpret_cast<T*>(block + off) : nullptr; }
    const T* in(const uint8_t* block) const { return n ? reinterpret_cast<const T*>(block + off) : nullptr; }
    size_t end() const { return off + pad64(sizeof(T) * n); }
};
struct Carve {                     // a running offset: every table starts on a multiple of 64
    size_t off = 0;
    template <typename T>
    void take(Table<T>& t, size_t n) { t.off = off; t.n = n; off = t.end(); }
};

inline BgzfBlk bgzf_blk(size_t stage_off, const vapor_bgzf::Block& b, uint64_t arena)     // (arena + b.u below 2^31: the callers' limits)
{
    return {(uint32_t)(stage_off + b.payload()), b.c_len(), (uint32_t)(arena + b.u), b.isize, b.crc, 0};
}

// minimize_pacbio_read_list (SF:1091-1102): of the kept reads `order` lists in file order, at most max_keep - the smallest miss_bp
// first, file order inside one value
template <typename MissOf>
inline void keep_smallest_miss(std::vector<int32_t>& order, int32_t max_keep, MissOf miss_of)
{
    if ((int64_t)order.size() <= (int64_t)max_keep) return;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return miss_of(a) < miss_of(b); });
    order.resize((size_t)max_keep);
}

// ------------------------------------------------------------------------------------------------------------------------------
// vapor_bam_chop_device*
// ------------------------------------------------------------------------------------------------------------------------------
enum class ChopMode { PLAIN, RIGHT, TAGGED, HAPLOTAG };     // bam_chop_kernel; bam_chop_right_kernel; the tagged kernel and the select kernel; the tags from phased sites

struct ChopCall {                  // what a call is
    int32_t n_regions = 0;
    const int32_t* tid = nullptr;
    const int64_t *start = nullptr, *end = nullptr, *flank = nullptr;
    const int32_t* chunk_first = nullptr;
    const uint64_t* chunks = nullptr;
    int32_t max_keep = 0;
    ChopMode mode = ChopMode::PLAIN;
    uint32_t filter_word = 0;      // the handle's read filter: every region of the call carries it
    bool dedup = false;            // `--dedup-qname`: bam_dedup_kernel behind the chop kernel
    // HAPLOTAG: the phased sites as the caller gave them
    const int32_t* site_first = nullptr;
    const BamSite* sites = nullptr;
    const int32_t* ps_first = nullptr;
    const int64_t* ps_values = nullptr;
    bool phased() const { return mode == ChopMode::TAGGED || mode == ChopMode::HAPLOTAG; }
    bool haplo() const { return mode == ChopMode::HAPLOTAG; }
    size_t n_sites() const { return haplo() && n_regions ? (size_t)site_first[n_regions] : 0; }
    size_t n_ps_values() const { return haplo() && n_regions ? (size_t)ps_first[n_regions] : 0; }
};

struct ChopOut {                   // the caller's arrays
    int32_t* kept_first = nullptr;
    uint64_t* sq_addr = nullptr;
    int64_t *q0 = nullptr, *miss = nullptr;
    int32_t* status = nullptr;
    uint32_t* member = nullptr;    // phased
    int64_t* phase_set = nullptr;
    int32_t* tagged = nullptr;
};

// the argument rules: what must hold before a region is looked at
inline Refusal check_args(const ChopCall& c, const ChopOut& o)
{
    const int32_t n = c.n_regions;
    if (n < 0 || c.max_keep < 1 || c.max_keep > KEPT_CAP ||
        (n && (!c.tid || !c.start || !c.end || !c.flank || !c.chunk_first || !o.kept_first || !o.sq_addr || !o.q0 || !o.miss || !o.status)) ||
        (c.phased() && n && (!o.phase_set || !o.tagged)) ||
        (c.haplo() && n && (!c.site_first || !c.ps_first || c.site_first[0] != 0 || c.ps_first[0] != 0)))
        return {VAPOR_E_ARG, "vapor_bam_chop_device: bad argument"};
    if (c.haplo() && n) {
        // (the two tables are the caller's: their offsets must ascend and their arrays be there before a region is looked at)
        for (int32_t g = 0; g < n; ++g)
            if (c.site_first[g + 1] < c.site_first[g] || c.ps_first[g + 1] < c.ps_first[g])
                return {VAPOR_E_ARG, "vapor_bam_chop_device_haplotag: site_first / ps_first do not ascend"};
        if ((c.site_first[n] && !c.sites) || (c.ps_first[n] && !c.ps_values))
            return {VAPOR_E_ARG, "vapor_bam_chop_device_haplotag: bad argument"};
    }
    return {};
}

struct SpanPlan {
    std::vector<HostSpan> spans;           // the chunks of the regions that are read, in region order
    std::vector<int32_t> span_first;       // region g's are spans[span_first[g], span_first[g + 1])
    size_t stage_bytes = 0;                // the staging block: every span's range starts on a multiple of 64
};

// The region rules (a call that passed check_args): status[g] = 0 and the region's spans, or why the host route must do it - a
// refused region leaves no span behind and takes no staging bytes.  plan_spans_of is the walk over the regions' chunks that the
// chop call and the depth call share; plan_spans states a call's own rules for a region.
// (region_ok(g, &why): whether region g's own fields let the device take it - `why` is the status of one they do not;
// `too_big`: the entry's size error, whose "in one call" the Python side reads to halve a group)
template <typename RegionOk>
inline Refusal plan_spans_of(int32_t n_regions, const int32_t* chunk_first, const uint64_t* chunks, int32_t* status, SpanPlan& p, const char* too_big,
                             RegionOk region_ok)
{
    p.spans.clear();
    p.span_first.assign((size_t)n_regions + 1, 0);
    p.stage_bytes = 0;
    for (int32_t g = 0; g < n_regions; ++g) {
        p.span_first[(size_t)g] = (int32_t)p.spans.size();
        status[g] = 0;
        const int32_t c0 = chunk_first[g], c1 = chunk_first[g + 1];
        int why = REG_MALFORMED;
        bool ok = c1 >= c0 && (c0 == c1 || chunks) && region_ok(g, &why);
        for (int32_t k = c0; ok && k < c1; ++k) {
            const uint64_t cs = chunks[2 * (size_t)k], ce = chunks[2 * (size_t)k + 1];
            if (ce < cs || (ce >> 16) - (cs >> 16) > ((uint64_t)1 << 27)) { ok = false; break; }
            HostSpan sp;
            sp.region = g; sp.cs = cs; sp.ce = ce;
            sp.file_off = (int64_t)(cs >> 16);
            sp.want = (size_t)((int64_t)(ce >> 16) - sp.file_off) + ((ce & 0xFFFFu) ? ((size_t)1 << 16) + 64 : 0);
            sp.got = 0;
            sp.stage_off = p.stage_bytes;
            p.stage_bytes += pad64(sp.want);
            p.spans.push_back(std::move(sp));
        }
        if (!ok) {
            status[g] = why;
            while (!p.spans.empty() && p.spans.back().region == g) { p.stage_bytes = p.spans.back().stage_off; p.spans.pop_back(); }
        }
    }
    p.span_first[(size_t)n_regions] = (int32_t)p.spans.size();
    if (p.stage_bytes > ((size_t)3 << 29)) return {VAPOR_E_ARG, too_big};
    return {};
}

inline Refusal plan_spans(const ChopCall& c, int32_t* status, SpanPlan& p)
{
    return plan_spans_of(c.n_regions, c.chunk_first, c.chunks, status, p, "vapor_bam_chop_device: more than 1.5 GB of blocks in one call (use smaller batches)",
                         [&](int32_t g, int* why) {
        // (positions are 32-bit in a BAM file; a region that is not is the host route's to refuse)
        bool ok = c.start[g] >= 0 && c.end[g] >= c.start[g] && c.end[g] < ((int64_t)1 << 31) && c.flank[g] >= 0 && c.tid[g] >= 0;
        if (ok && c.haplo()) {
            // a wavefront tallies PHASE_SETS_CAP phase sets; the sites in position order, their indices inside the region's table
            const int32_t n_ps = c.ps_first[g + 1] - c.ps_first[g];
            if (n_ps > PHASE_SETS_CAP) { ok = false; *why = REG_PHASE_SETS; }
            for (int32_t i = c.site_first[g]; ok && i < c.site_first[g + 1]; ++i)
                ok = c.sites[i].ps_idx < n_ps && c.sites[i].pos >= 1 && (i == c.site_first[g] || c.sites[i - 1].pos < c.sites[i].pos);
        }
        return ok;
    });
}

struct ChopLayout;

// Where each table of a chop call lies in its metadata block - blocks, spans, regions and the haplotag tables go in; block status,
// kept counts, region status and the kept reads (phased: the regions' BamPhase and their unions, 3 * max_keep picks each) come
// back; the rest stays on the device.  De-duplicating, the kept entries' name keys lie behind them and come back with them;
// without the option the slot is empty and every offset is what it was.
struct ChopMeta {
    Table<BgzfBlk> blks;
    Table<BamSpan> spans;
    Table<BamRegion> regs;
    Table<BamSiteRange> site_ranges;       // HAPLOTAG: every region's range of sites and of phase-set values, the sites, the values
    Table<BamSite> sites;
    Table<long long> ps_values;
    Table<int32_t> blk_status, n_kept, reg_status;
    Table<BamPhase> phases;                // phased
    Table<BamPick> picks;                  // phased: 3 * max_keep a region
    Table<BamKept> kept;                   // KEPT_CAP a region, as are keys, tags and ops
    Table<uint64_t> keys;                  // de-duplicating
    Table<BamTag> tags;                    // phased
    Table<BamOps> ops;                     // HAPLOTAG
    size_t in_bytes = 0;                   // the block's first bytes are what the host sends
    size_t back_end = 0;                   // what the host reads back is [blk_status.off, back_end)
    size_t bytes = 0;                      // the device's block
    int32_t picks_per_region = 0;

    ChopMeta() = default;
    ChopMeta(const ChopCall& c, size_t n_blks, size_t n_spans)
    {
        const size_t nr = (size_t)std::max(c.n_regions, 1);
        const bool phased = c.phased(), haplo = c.haplo();
        picks_per_region = 3 * c.max_keep;
        Carve m;
        m.take(blks, std::max<size_t>(n_blks, 1));
        m.take(spans, std::max<size_t>(n_spans, 1));
        m.take(regs, nr);
        m.take(site_ranges, haplo ? nr : 0);
        m.take(sites, haplo ? std::max<size_t>(c.n_sites(), 1) : 0);
        m.take(ps_values, haplo ? std::max<size_t>(c.n_ps_values(), 1) : 0);
        in_bytes = m.off;
        m.take(blk_status, std::max<size_t>(n_blks, 1));
        m.take(n_kept, nr);
        m.take(reg_status, nr);
        m.take(phases, phased ? nr : 0);
        m.take(picks, phased ? (size_t)picks_per_region * nr : 0);
        // (phased, the kept entries and their tags stay on the device: the selection is made there)
        if (phased) back_end = m.off;
        m.take(kept, (size_t)KEPT_CAP * nr);
        m.take(keys, c.dedup ? (size_t)KEPT_CAP * nr : 0);
        if (!phased) back_end = m.off;
        m.take(tags, phased ? (size_t)KEPT_CAP * nr : 0);
        m.take(ops, haplo ? (size_t)KEPT_CAP * nr : 0);
        bytes = m.off;
    }
    size_t host_bytes() const { return std::max(back_end, in_bytes); }         // the host's block: what goes in, what comes back
    size_t back_bytes() const { return back_end - blk_status.off; }
    template <typename B> B* back(B* block) const { return block + blk_status.off; }   // where the read-back begins, in either copy

    // the tables that go in, into the host's block; a region that is not sent (status[g] != 0) gets an empty site range: its wavefronts end on its status
    inline void fill(uint8_t* h_meta, const ChopCall& c, const ChopLayout& L, const int32_t* status) const;
};

struct ChopLayout {
    std::vector<BgzfBlk> blks;
    std::vector<BamSpan> spans;
    std::vector<BamRegion> regs;
    size_t arena = 0;                      // bytes of block data: every span's range starts on a multiple of 64
    ChopMeta meta;
};

// After the scan: a region with a span that did not scan gets REG_MALFORMED; the spans of the others one after the other in the
// arena, their blocks behind each other in the block table.  layout_of is that walk for the chop call and the depth call alike.
// (regs: the call's region records, any struct with span_first and span_n; set(R, g) writes the rest of region g's)
template <typename Region, typename SetRegion>
inline Refusal layout_of(int32_t n_regions, const SpanPlan& p, int32_t* status, std::vector<BgzfBlk>& blks, std::vector<BamSpan>& spans,
                         std::vector<Region>& regs, size_t* arena_out, const char* too_big, SetRegion set)
{
    for (const HostSpan& sp : p.spans)
        if (sp.bad) status[sp.region] = REG_MALFORMED;
    blks.clear();
    spans.clear();
    regs.assign((size_t)std::max(n_regions, 1), Region());
    size_t arena = 0;
    for (int32_t g = 0; g < n_regions; ++g) {
        Region& R = regs[(size_t)g];
        set(R, g);
        R.span_first = (int32_t)spans.size();
        R.span_n = 0;
        if (status[g]) continue;
        for (int32_t si = p.span_first[(size_t)g]; si < p.span_first[(size_t)g + 1]; ++si) {
            const HostSpan& sp = p.spans[(size_t)si];
            if (arena + sp.u_total + 64 > ((size_t)1 << 31)) return {VAPOR_E_ARG, too_big};
            BamSpan d;
            d.u_begin = (uint32_t)arena + (uint32_t)sp.u_begin;
            d.u_end = (uint32_t)arena + (uint32_t)sp.u_end;
            d.u_limit = (uint32_t)arena + (uint32_t)sp.u_total;
            d.blk_first = (uint32_t)blks.size();
            d.blk_n = (uint32_t)sp.blks.size();
            d.pad = 0;
            for (const vapor_bgzf::Block& k : sp.blks) blks.push_back(bgzf_blk(sp.stage_off, k, arena));
            spans.push_back(d);
            ++R.span_n;
            arena += pad64((size_t)sp.u_total);
        }
    }
    *arena_out = arena;
    return {};
}

inline Refusal layout(const ChopCall& c, const SpanPlan& p, int32_t* status, ChopLayout& L)
{
    if (const Refusal r = layout_of(c.n_regions, p, status, L.blks, L.spans, L.regs, &L.arena,
                                    "vapor_bam_chop_device: more than 2 GB of block data in one call (use smaller batches)", [&](BamRegion& R, int32_t g) {
            R.start = c.start[g]; R.end = c.end[g]; R.flank = c.flank[g]; R.tid = c.tid[g]; R.pad = (int32_t)c.filter_word;
        }))
        return r;
    L.meta = ChopMeta(c, L.blks.size(), L.spans.size());
    return {};
}

inline void ChopMeta::fill(uint8_t* h_meta, const ChopCall& c, const ChopLayout& L, const int32_t* status) const
{
    if (!L.blks.empty()) memcpy(blks.in(h_meta), L.blks.data(), sizeof(BgzfBlk) * L.blks.size());
    if (!L.spans.empty()) memcpy(spans.in(h_meta), L.spans.data(), sizeof(BamSpan) * L.spans.size());
    memcpy(regs.in(h_meta), L.regs.data(), sizeof(BamRegion) * L.regs.size());
    if (!c.haplo()) return;
    BamSiteRange* sr = site_ranges.in(h_meta);
    for (int32_t g = 0; g < c.n_regions; ++g) {
        const bool on = status[g] == 0;
        sr[g] = {c.site_first[g], on ? c.site_first[g + 1] - c.site_first[g] : 0, c.ps_first[g], on ? c.ps_first[g + 1] - c.ps_first[g] : 0};
    }
    if (c.n_regions == 0) sr[0] = {0, 0, 0, 0};
    if (c.n_sites()) memcpy(sites.in(h_meta), c.sites, sizeof(BamSite) * c.n_sites());
    if (c.n_ps_values()) memcpy(ps_values.in(h_meta), c.ps_values, 8 * c.n_ps_values());
}

// The read-back block into the caller's arrays.  Region g's entries are o.*[kept_first[g], kept_first[g + 1]), their packed bases at
// arena_base + sq_off.  A region the host refused keeps its status and has no entries; one the device refused takes the device's
// status.  Phased, the selection was made on the device: the union as it lies, at most 3 * max_keep entries.  Otherwise
// keep_smallest_miss; de-duplicating, name_keys receives the entries' name keys in their order.
inline void collect(const ChopCall& c, const ChopMeta& M, const uint8_t* h_meta, uint64_t arena_base, const ChopOut& o, std::vector<uint64_t>& name_keys)
{
    const int32_t n_regions = c.n_regions;
    const int32_t* nk = M.n_kept.in(h_meta);
    const int32_t* rst = M.reg_status.in(h_meta);
    const BamKept* kept = M.kept.in(h_meta);
    const uint64_t* keys = M.keys.in(h_meta);
    const bool phased = c.phased();
    int32_t w = 0;
    std::vector<int32_t> order;
    name_keys.clear();
    for (int32_t g = 0; g < n_regions; ++g) {
        o.kept_first[g] = w;
        if (phased) {
            o.phase_set[g] = INT64_MIN;
            o.tagged[g] = 0;
        }
        if (o.status[g]) continue;
        if (rst[g] != REG_OK) { o.status[g] = rst[g]; continue; }
        if (phased) {
            const BamPhase& ph = M.phases.in(h_meta)[g];
            if (ph.n_union < 0 || ph.n_union > M.picks_per_region) { o.status[g] = REG_MALFORMED; continue; }
            o.phase_set[g] = (int64_t)ph.ps;
            o.tagged[g] = ph.tagged;
            const BamPick* pk = M.picks.in(h_meta) + (size_t)g * (size_t)M.picks_per_region;
            for (int32_t i = 0; i < ph.n_union; ++i) {
                o.sq_addr[w] = arena_base + pk[i].sq_off;
                o.q0[w] = pk[i].q0;
                o.miss[w] = pk[i].miss;
                o.member[w] = pk[i].member;
                ++w;
            }
            continue;
        }
        const BamKept* k = kept + (size_t)g * KEPT_CAP;
        order.resize((size_t)nk[g]);
        for (int32_t i = 0; i < nk[g]; ++i) order[(size_t)i] = i;
        keep_smallest_miss(order, c.max_keep, [&](int32_t i) { return k[i].miss; });
        for (int32_t i : order) {
            o.sq_addr[w] = arena_base + k[i].sq_off;
            o.q0[w] = k[i].q0;
            o.miss[w] = k[i].miss;
            if (c.dedup) name_keys.push_back(keys[(size_t)g * KEPT_CAP + (size_t)i]);
            ++w;
        }
    }
    o.kept_first[n_regions] = w;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The evidence calls: vapor_bam_depth_device, _signature_device, _links_device, _support_device.  One plan
// shape over (the region record the kernel reads, the answer word it writes, the words a region, which of them are signed); a
// call's own rules - *_region_ok, *_region_set, plan_spans, the texts of its refusals - stand in its section below.
// ------------------------------------------------------------------------------------------------------------------------------
// Where each table of an evidence call lies in its metadata block: blocks, spans, regions and - a call that has one - the name
// blob go in; block status, WORDS answer words a region and the region status come back.  The host's block is the device's.
template <typename Region, typename Word, int WORDS, uint32_t SIGNED = 0>
struct EvidenceMeta {
    Table<BgzfBlk> blks;
    Table<BamSpan> spans;
    Table<Region> regs;
    Table<uint8_t> names;                  // links: the partner contigs' names, once, whatever number of regions name a contig
    Table<int32_t> blk_status;
    Table<Word> ans;                       // WORDS a region; bit k of SIGNED: word k is an int32
    Table<int32_t> reg_status;
    size_t in_bytes = 0, bytes = 0;

    EvidenceMeta() = default;
    EvidenceMeta(int32_t n_regions, size_t n_blks, size_t n_spans, size_t names_room)      // names_room 0: the call has no blob
    {
        const size_t nr = (size_t)std::max(n_regions, 1);
        Carve m;
        m.take(blks, std::max<size_t>(n_blks, 1));
        m.take(spans, std::max<size_t>(n_spans, 1));
        m.take(regs, nr);
        m.take(names, names_room);
        in_bytes = m.off;
        m.take(blk_status, std::max<size_t>(n_blks, 1));
        m.take(ans, (size_t)WORDS * nr);
        m.take(reg_status, nr);
        bytes = m.off;
    }
    size_t back_bytes() const { return bytes - blk_status.off; }       // [blk_status.off, bytes) comes back
    template <typename B> B* back(B* block) const { return block + blk_status.off; }
};

template <typename Region, typename Word, int WORDS, uint32_t SIGNED = 0>
struct EvidenceLayout {
    using Meta = EvidenceMeta<Region, Word, WORDS, SIGNED>;
    std::vector<BgzfBlk> blks;
    std::vector<BamSpan> spans;
    std::vector<Region> regs;
    const uint8_t* names = nullptr;        // links
    size_t names_len = 0;
    size_t arena = 0;
    Meta meta;
    void fill(uint8_t* h_meta) const       // the tables that go in, into the host's block
    {
        if (!blks.empty()) memcpy(meta.blks.in(h_meta), blks.data(), sizeof(BgzfBlk) * blks.size());
        if (!spans.empty()) memcpy(meta.spans.in(h_meta), spans.data(), sizeof(BamSpan) * spans.size());
        memcpy(meta.regs.in(h_meta), regs.data(), sizeof(Region) * regs.size());
        if (names_len) memcpy(meta.names.in(h_meta), names, names_len);
    }
};

// layout_of with the call's region records, then the metadata block.  (set(R, g) as layout_of takes it; names_room as EvidenceMeta)
template <typename Call, typename Layout, typename SetRegion>
inline Refusal layout_evidence(const Call& c, const SpanPlan& p, int32_t* status, Layout& L, const char* too_big, SetRegion set, size_t names_room = 0)
{
    if (const Refusal r = layout_of(c.n_regions, p, status, L.blks, L.spans, L.regs, &L.arena, too_big, set)) return r;
    L.meta = typename Layout::Meta(c.n_regions, L.blks.size(), L.spans.size(), names_room);
    return {};
}

// The read-back block into the caller's arrays: a region the host refused keeps its status and zeros, one the device refused
// takes the device's status (its answer is then the host route's to make), the others their WORDS words.
template <typename Call, typename Region, typename Word, int WORDS, uint32_t SIGNED, typename Out>
inline void collect(const Call& c, const EvidenceMeta<Region, Word, WORDS, SIGNED>& M, const uint8_t* h_meta, Out* out, int32_t* status)
{
    const Word* da = M.ans.in(h_meta);
    const int32_t* rst = M.reg_status.in(h_meta);
    for (int32_t g = 0; g < c.n_regions; ++g) {
        Out* o = out + (size_t)WORDS * (size_t)g;
        for (int k = 0; k < WORDS; ++k) o[k] = 0;
        if (status[g]) continue;
        if (rst[g] != REG_OK) { status[g] = rst[g]; continue; }
        const Word* a = da + (size_t)WORDS * (size_t)g;
        for (int k = 0; k < WORDS; ++k) o[k] = ((SIGNED >> k) & 1u) ? (Out)(int32_t)a[k] : (Out)a[k];
    }
}

// the argument rules: what must hold before a region is looked at (fields: the call's bounds or regions; more_ok: its own conditions)
template <typename Call>
inline Refusal check_evidence_args(const Call& c, const int64_t* fields, const void* out, const int32_t* status, const char* msg, bool more_ok = true)
{
    if (c.n_regions < 0 || !more_ok || (c.n_regions && (!c.tid || !fields || !c.chunk_first || !out || !status))) return {VAPOR_E_ARG, msg};
    return {};
}

// ------------------------------------------------------------------------------------------------------------------------------
// vapor_bam_depth_device (`--depth`)
// ------------------------------------------------------------------------------------------------------------------------------
struct DepthCall {
    int32_t n_regions = 0;
    const int32_t* tid = nullptr;
    const int64_t* bounds = nullptr;       // four a region: b0 <= b1 <= b2 <= b3, 0-based
    const int32_t* chunk_first = nullptr;
    const uint64_t* chunks = nullptr;
    uint32_t filter_word = 0;              // the handle's read filter with DEPTH_EXCLUDE among its flags (depth_filter_word)
};

// the handle's filter word as a depth region carries it: unmapped, secondary, QC-fail and duplicate records never count
inline uint32_t depth_filter_word(uint32_t handle_word) { return handle_word | DEPTH_EXCLUDE; }

inline Refusal check_args(const DepthCall& c, const uint64_t* cov, const int32_t* status)
{
    return check_evidence_args(c, c.bounds, cov, status, "vapor_bam_depth_device: bad argument");
}

// The region rules: the bounds ascend from 0, b3 is a BAM position, the contig is one - else REG_MALFORMED and the host route's
// to refuse.  The spans and the staging block as plan_spans makes them.
inline Refusal plan_spans(const DepthCall& c, int32_t* status, SpanPlan& p)
{
    return plan_spans_of(c.n_regions, c.chunk_first, c.chunks, status, p, "vapor_bam_depth_device: more than 1.5 GB of blocks in one call (use smaller batches)",
                         [&](int32_t g, int*) {
        const int64_t* b = c.bounds + 4 * (size_t)g;
        return b[0] >= 0 && b[1] >= b[0] && b[2] >= b[1] && b[3] >= b[2] && b[3] < ((int64_t)1 << 31) && c.tid[g] >= 0;
    });
}

// three sums a region, 64-bit.  A refused region's record carries its fields all the same.
using DepthLayout = EvidenceLayout<DepthRegion, uint64_t, 3>;
using DepthMeta = DepthLayout::Meta;

inline Refusal layout(const DepthCall& c, const SpanPlan& p, int32_t* status, DepthLayout& L)
{
    return layout_evidence(c, p, status, L, "vapor_bam_depth_device: more than 2 GB of block data in one call (use smaller batches)", [&](DepthRegion& R, int32_t g) {
        for (int k = 0; k < 4; ++k) R.b[k] = c.bounds[4 * (size_t)g + (size_t)k];
        R.tid = c.tid[g]; R.filter = c.filter_word;
    });
}

// ------------------------------------------------------------------------------------------------------------------------------
// vapor_bam_signature_device (`--signatures`)
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int SIG_FIELDS = 9;              // a region as the caller gives it: w0, w3, x0, x1, tol, min_clip, nmin, nmax, mask
struct SigCall {
    int32_t n_regions = 0;
    const int32_t* tid = nullptr;
    const int64_t* regions = nullptr;      // SIG_FIELDS a region
    const int32_t* chunk_first = nullptr;
    const uint64_t* chunks = nullptr;
    uint32_t filter_word = 0;              // the handle's read filter with DEPTH_EXCLUDE among its flags (depth_filter_word)
};

inline Refusal check_args(const SigCall& c, const int64_t* out, const int32_t* status)
{
    return check_evidence_args(c, c.regions, out, status, "vapor_bam_signature_device: bad argument");
}

// Whether a region's own fields are a question the readers answer: the window ascends from 0 and ends at a BAM position, the
// tolerance fits the histograms, the length bounds ascend, the contig is one.  One statement for the device's plan and the host
// reader (vapor_bam.cpp bam_signature_impl).
inline bool sig_region_ok(int32_t tid, const int64_t* f)
{
    return f[0] >= 0 && f[1] >= f[0] && f[1] < ((int64_t)1 << 31) && f[4] >= 0 && f[4] <= SIG_TOL_MAX && f[6] <= f[7] && tid >= 0;
}

// The caller's fields as the kernel and the host reader take them: the length bounds clamped to [-1, 2^28] (no operation is
// longer than 2^28 - 1, none shorter than 0: the clamped bounds admit the same operations), the minimum clip to [1, 2^30] (a
// clip event has one clipped base at least; two operations sum to less than 2^29), the targets to +-2^40 (far from every
// coordinate either way), the mask to its six bits.
inline void sig_region_set(SigRegion& R, int32_t tid, const int64_t* f, uint32_t filter_word)
{
    const int64_t far = (int64_t)1 << 40;
    R.w0 = f[0]; R.w3 = f[1];
    R.x0 = std::min(std::max(f[2], -far), far); R.x1 = std::min(std::max(f[3], -far), far);
    R.tol = (int32_t)f[4];
    R.min_clip = (int32_t)std::min<int64_t>(std::max<int64_t>(f[5], 1), (int64_t)1 << 30);
    R.nmin = (int32_t)std::min<int64_t>(std::max<int64_t>(f[6], -1), (int64_t)1 << 28);
    R.nmax = (int32_t)std::min<int64_t>(std::max<int64_t>(f[7], -1), (int64_t)1 << 28);
    R.mask = (uint32_t)f[8] & 63u;
    R.tid = tid; R.filter = filter_word; R.pad = 0;
}

// The region rules: sig_region_ok - else REG_MALFORMED and the host route's to refuse.  The spans and the staging block as
// plan_spans makes them.
inline Refusal plan_spans(const SigCall& c, int32_t* status, SpanPlan& p)
{
    return plan_spans_of(c.n_regions, c.chunk_first, c.chunks, status, p, "vapor_bam_signature_device: more than 1.5 GB of blocks in one call (use smaller batches)",
                         [&](int32_t g, int*) { return sig_region_ok(c.tid[g], c.regions + SIG_FIELDS * (size_t)g); });
}

// SIG_ANSWER_WORDS words a region: six counts, then (offset, count) of each mode - the two offsets are int32
using SigLayout = EvidenceLayout<SigRegion, uint32_t, SIG_ANSWER_WORDS, (1u << 6) | (1u << 8)>;
using SigMeta = SigLayout::Meta;

inline Refusal layout(const SigCall& c, const SpanPlan& p, int32_t* status, SigLayout& L)
{
    return layout_evidence(c, p, status, L, "vapor_bam_signature_device: more than 2 GB of block data in one call (use smaller batches)", [&](SigRegion& R, int32_t g) {
        // (a region the plan refused keeps a record that asks nothing: no kernel reads it, its span_n is 0)
        if (status[g]) { R = SigRegion(); return; }
        sig_region_set(R, c.tid[g], c.regions + SIG_FIELDS * (size_t)g, c.filter_word);
    });
}

// ------------------------------------------------------------------------------------------------------------------------------
// vapor_bam_links_device (`--links`)
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int LINK_FIELDS = 11;            // a region as the caller gives it: w0, w3, x, y, tol, min_clip, ev, pend, rel, name_off, name_len
struct LinkCall {
    int32_t n_regions = 0;
    const int32_t* tid = nullptr;
    const int64_t* regions = nullptr;      // LINK_FIELDS a region
    const uint8_t* names = nullptr;        // the partner contigs' names, one blob: region g's is names[name_off, name_off + name_len)
    int64_t names_len = 0;
    const int32_t* chunk_first = nullptr;
    const uint64_t* chunks = nullptr;
    uint32_t filter_word = 0;              // the handle's read filter with DEPTH_EXCLUDE among its flags (depth_filter_word)
};

inline Refusal check_args(const LinkCall& c, const int64_t* out, const int32_t* status)
{
    return check_evidence_args(c, c.regions, out, status, "vapor_bam_links_device: bad argument",
                               c.names_len >= 0 && c.names_len < ((int64_t)1 << 30) && (!c.names_len || c.names));
}

// Whether a region's own fields are a question the readers answer: the window ascends from 0 and ends at a BAM position, the
// tolerance fits the histogram, ev, pend and rel are 0 or 1, the partner's name is not empty and lies inside the blob, the contig
// is one.  One statement for the device's plan and the host reader (vapor_bam.cpp bam_links_impl).
inline bool link_region_ok(int32_t tid, const int64_t* f, int64_t names_len)
{
    return f[0] >= 0 && f[1] >= f[0] && f[1] < ((int64_t)1 << 31) && f[4] >= 0 && f[4] <= SIG_TOL_MAX && f[6] >= 0 && f[6] <= 1 &&
           f[7] >= 0 && f[7] <= 1 && f[8] >= 0 && f[8] <= 1 && f[10] >= 1 && f[9] >= 0 && f[9] <= names_len && f[10] <= names_len - f[9] && tid >= 0;
}

// The caller's fields as the kernel and the host reader take them: the minimum clip clamped to [1, 2^30] and the two targets to
// +-2^40, as sig_region_set clamps them.
inline void link_region_set(LinkRegion& R, int32_t tid, const int64_t* f, uint32_t filter_word)
{
    const int64_t far = (int64_t)1 << 40;
    R.w0 = f[0]; R.w3 = f[1];
    R.x = std::min(std::max(f[2], -far), far); R.y = std::min(std::max(f[3], -far), far);
    R.tol = (int32_t)f[4];
    R.min_clip = (int32_t)std::min<int64_t>(std::max<int64_t>(f[5], 1), (int64_t)1 << 30);
    R.bits = (f[6] ? LINK_EV : 0u) | (f[7] ? LINK_PEND : 0u) | (f[8] ? LINK_REL : 0u);
    R.name_off = (uint32_t)f[9]; R.name_len = (uint32_t)f[10];
    R.tid = tid; R.filter = filter_word; R.pad = 0;
}

// The region rules: link_region_ok - else REG_MALFORMED and the host route's to refuse.  The spans and the staging block as
// plan_spans makes them.
inline Refusal plan_spans(const LinkCall& c, int32_t* status, SpanPlan& p)
{
    return plan_spans_of(c.n_regions, c.chunk_first, c.chunks, status, p, "vapor_bam_links_device: more than 1.5 GB of blocks in one call (use smaller batches)",
                         [&](int32_t g, int*) { return link_region_ok(c.tid[g], c.regions + LINK_FIELDS * (size_t)g, c.names_len); });
}

// LINK_ANSWER_WORDS words a region: n_clip, n_split, n_link, the mode's offset (int32) and count.  The name blob goes up inside
// the metadata block, a byte of room at least.
using LinkLayout = EvidenceLayout<LinkRegion, uint32_t, LINK_ANSWER_WORDS, 1u << 3>;
using LinkMeta = LinkLayout::Meta;

inline Refusal layout(const LinkCall& c, const SpanPlan& p, int32_t* status, LinkLayout& L)
{
    L.names = c.names;
    L.names_len = (size_t)c.names_len;
    return layout_evidence(c, p, status, L, "vapor_bam_links_device: more than 2 GB of block data in one call (use smaller batches)", [&](LinkRegion& R, int32_t g) {
        // (a region the plan refused keeps a record that asks nothing: no kernel reads it, its span_n is 0)
        if (status[g]) { R = LinkRegion(); return; }
        link_region_set(R, c.tid[g], c.regions + LINK_FIELDS * (size_t)g, c.filter_word);
    }, std::max<size_t>(L.names_len, 1));
}

// ------------------------------------------------------------------------------------------------------------------------------
// vapor_bam_support_device (`--support`)
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int SUP_FIELDS = 11;             // a region as the caller gives it: the nine SIG_FIELDS, then flank and gmin
struct SupCall {
    int32_t n_regions = 0;
    const int32_t* tid = nullptr;
    const int64_t* regions = nullptr;      // SUP_FIELDS a region
    const int32_t* chunk_first = nullptr;
    const uint64_t* chunks = nullptr;
    uint32_t filter_word = 0;              // the handle's read filter with DEPTH_EXCLUDE among its flags (depth_filter_word)
};

inline Refusal check_args(const SupCall& c, const int64_t* out, const int32_t* status)
{
    return check_evidence_args(c, c.regions, out, status, "vapor_bam_support_device: bad argument");
}

// Whether a region's own fields are a question the readers answer: sig_region_ok of its first nine, a flank of 1..65535 and a
// blocking length of 1 at least.  One statement for the device's plan and the host reader (vapor_bam.cpp bam_support_impl).
inline bool sup_region_ok(int32_t tid, const int64_t* f)
{
    return sig_region_ok(tid, f) && f[9] >= 1 && f[9] <= SUP_FLANK_MAX && f[10] >= 1;
}

// The caller's fields as the kernel and the host reader take them: sig_region_set's clamps for the first nine (the mask keeps
// its eight bits), and the blocking length clamped to 2^28 (no operation is that long: the clamped bound admits the same - none).
inline void sup_region_set(SupRegion& R, int32_t tid, const int64_t* f, uint32_t filter_word)
{
    const int64_t far = (int64_t)1 << 40;
    R.w0 = f[0]; R.w3 = f[1];
    R.x0 = std::min(std::max(f[2], -far), far); R.x1 = std::min(std::max(f[3], -far), far);
    R.tol = (int32_t)f[4];
    R.min_clip = (int32_t)std::min<int64_t>(std::max<int64_t>(f[5], 1), (int64_t)1 << 30);
    R.nmin = (int32_t)std::min<int64_t>(std::max<int64_t>(f[6], -1), (int64_t)1 << 28);
    R.nmax = (int32_t)std::min<int64_t>(std::max<int64_t>(f[7], -1), (int64_t)1 << 28);
    R.mask = (uint32_t)f[8] & 255u;
    R.flank = (int32_t)f[9];
    R.gmin = (int32_t)std::min<int64_t>(f[10], (int64_t)1 << 28);
    R.tid = tid; R.filter = filter_word; R.pad = 0;
}

// The region rules: sup_region_ok - else REG_MALFORMED and the host route's to refuse.  The spans and the staging block as
// plan_spans makes them.
inline Refusal plan_spans(const SupCall& c, int32_t* status, SpanPlan& p)
{
    return plan_spans_of(c.n_regions, c.chunk_first, c.chunks, status, p, "vapor_bam_support_device: more than 1.5 GB of blocks in one call (use smaller batches)",
                         [&](int32_t g, int*) { return sup_region_ok(c.tid[g], c.regions + SUP_FIELDS * (size_t)g); });
}

// SUP_ANSWER_WORDS counts a region: alt_cg, alt_l, alt_r, ref_0, ref_1, cov_0, cov_1
using SupLayout = EvidenceLayout<SupRegion, uint32_t, SUP_ANSWER_WORDS>;
using SupMeta = SupLayout::Meta;

inline Refusal layout(const SupCall& c, const SpanPlan& p, int32_t* status, SupLayout& L)
{
    return layout_evidence(c, p, status, L, "vapor_bam_support_device: more than 2 GB of block data in one call (use smaller batches)", [&](SupRegion& R, int32_t g) {
        // (a region the plan refused keeps a record that asks nothing: no kernel reads it, its span_n is 0)
        if (status[g]) { R = SupRegion(); return; }
        sup_region_set(R, c.tid[g], c.regions + SUP_FIELDS * (size_t)g, c.filter_word);
    });
}

// ------------------------------------------------------------------------------------------------------------------------------
// vapor_fasta_windows_device
// ------------------------------------------------------------------------------------------------------------------------------
constexpr uint64_t ARENA_CAP = (uint64_t)1 << 30;       // inflated bytes of a call; a stretch that would pass it leaves its windows to the host
constexpr uint64_t STAGE_CAP = (uint64_t)1 << 29;       // compressed bytes of a call, likewise

struct FastaCall {
    int32_t n = 0;
    const uint64_t *vbeg = nullptr, *vend = nullptr;    // the windows' raw bytes as virtual offsets
    int64_t text_cap = 0;
};

struct StretchPlan {
    std::vector<FaStretch> sts;            // ascending and disjoint
    std::vector<int32_t> st_of;            // a non-empty window's stretch, -1 for the others
    uint64_t stage_bytes = 0;
};

// The windows in file order, merged into stretches: the ranges that share a block or touch are read as one stretch, so that every
// distinct block is read, sent and inflated once however many windows hold it.  status[i] = WIN_RANGE where vend < vbeg.
inline void plan_stretches(const FastaCall& c, int32_t* status, uint8_t* traits, StretchPlan& p)
{
    const int32_t n = c.n;
    const uint64_t *vbeg = c.vbeg, *vend = c.vend;
    std::vector<int32_t> order;
    order.reserve((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        status[i] = WIN_OK;
        traits[i] = 0;
        if (vend[i] < vbeg[i]) status[i] = WIN_RANGE;
        else if (vend[i] > vbeg[i]) order.push_back(i);
    }
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return vbeg[a] != vbeg[b] ? vbeg[a] < vbeg[b] : a < b; });
    p.sts.clear();
    p.st_of.assign((size_t)n, -1);
    p.stage_bytes = 0;
    for (int32_t i : order) {
        const int64_t c0 = (int64_t)(vbeg[i] >> 16), cl = (int64_t)(vend[i] >> 16);
        const bool nl = (vend[i] & 0xFFFFu) != 0;
        if (!p.sts.empty() && c0 <= p.sts.back().c_last) {          // (shares a block with the stretch, or starts where it ends)
            FaStretch& s = p.sts.back();
            if (cl > s.c_last || (cl == s.c_last && nl)) { s.c_last = cl; s.need_last = nl; }
        } else {
            FaStretch s;
            s.c0 = c0; s.c_last = cl; s.need_last = nl;
            p.sts.push_back(std::move(s));
        }
        p.st_of[(size_t)i] = (int32_t)p.sts.size() - 1;
    }
}

// What is read of every stretch and where it goes in the staging block.  read_header(file offset, h) brings up to 64 bytes of the
// file there into h and says how many: a stretch's last block is read in full, its BSIZE from its header.  A stretch that would
// pass STAGE_CAP has no room.
template <typename ReadHeader>
inline void stage_stretches(StretchPlan& p, ReadHeader read_header)
{
    p.stage_bytes = 0;
    for (FaStretch& s : p.sts) {
        uint64_t last_size = 0;
        if (s.need_last) {
            uint8_t h[64];
            last_size = vapor_bgzf::last_block_size(h, read_header(s.c_last, h));
        }
        const uint64_t want = (uint64_t)(s.c_last - s.c0) + last_size;
        if (p.stage_bytes + want > STAGE_CAP) { s.room = false; continue; }
        s.want = (size_t)want;
        s.stage_off = (size_t)p.stage_bytes;
        p.stage_bytes += (want + 63) & ~(uint64_t)63;
    }
}

struct FastaLayout {
    std::vector<BgzfBlk> blks;             // the non-empty blocks of the stretches that have room
    uint64_t arena = 0;
    std::vector<FastaWin> wins;
    uint64_t slots = 0;                    // bytes of the text buffer
};

// After the scan: the stretches one after the other in the arena (64-bit offsets; one that would pass ARENA_CAP has no room)
inline void layout_arena(StretchPlan& p, FastaLayout& L)
{
    L.blks.clear();
    uint64_t arena = 0;
    for (FaStretch& s : p.sts) {
        if (!s.room) continue;
        const uint64_t size = s.blks.back().u;
        if (arena + size + 64 > ARENA_CAP) { s.room = false; continue; }
        s.arena_off = arena;
        for (size_t k = 0; k < s.blks.size(); ++k) {
            s.gidx[k] = (uint32_t)L.blks.size();
            if (s.blks[k].isize) L.blks.push_back(bgzf_blk(s.stage_off, s.blks[k], arena));
        }
        arena += (size + 63) & ~(uint64_t)63;
    }
    L.arena = arena;
}

// The windows: their bytes in the arena, their blocks in the block table, their slots in the text buffer
inline void place_windows(const FastaCall& c, const StretchPlan& p, int32_t* status, FastaLayout& L)
{
    const int32_t n = c.n;
    L.wins.assign((size_t)std::max(n, 1), FastaWin{0, 0, 0, 0, 0});
    uint64_t slots = 0;
    auto find = [](const FaStretch& s, int64_t coff) -> int64_t {
        const size_t pos = (size_t)(coff - s.c0);
        auto it = std::lower_bound(s.blks.begin(), s.blks.end(), pos, [](const vapor_bgzf::Block& b, size_t q) { return b.pos < q; });
        return it != s.blks.end() && it->pos == pos ? (int64_t)(it - s.blks.begin()) : -1;
    };
    for (int32_t i = 0; i < n; ++i) {
        FastaWin& W = L.wins[(size_t)i];
        const int32_t si = p.st_of[(size_t)i];
        if (status[i] || si < 0) continue;
        const FaStretch& s = p.sts[(size_t)si];
        if (!s.room) { status[i] = WIN_ROOM; continue; }
        const int64_t kb = find(s, (int64_t)(c.vbeg[i] >> 16)), ke = find(s, (int64_t)(c.vend[i] >> 16));
        const uint32_t ub = (uint32_t)(c.vbeg[i] & 0xFFFFu), ue = (uint32_t)(c.vend[i] & 0xFFFFu);
        const bool last_is_sentinel = ke == (int64_t)s.blks.size() - 1;
        if (kb < 0 || ke < 0 || kb == (int64_t)s.blks.size() - 1 || ub > s.blks[(size_t)kb].isize || ue > s.blks[(size_t)ke].isize || (last_is_sentinel && ue)) {
            status[i] = s.cut ? WIN_BLOCK : WIN_RANGE;
            continue;
        }
        W.a_beg = s.arena_off + s.blks[(size_t)kb].u + ub;
        W.a_end = s.arena_off + s.blks[(size_t)ke].u + ue;
        if (W.a_end < W.a_beg) { status[i] = WIN_RANGE; W.a_end = W.a_beg; continue; }
        const uint64_t len = W.a_end - W.a_beg;
        if (slots + len > (uint64_t)c.text_cap) { status[i] = WIN_ROOM; W.a_end = W.a_beg; continue; }
        W.t_off = slots;
        slots += len;
        W.blk_first = s.gidx[(size_t)kb];
        W.blk_n = s.gidx[(size_t)ke] + (ue ? 1u : 0u) - W.blk_first;
    }
    L.slots = slots;
}

// Where each table of a windows call lies in its metadata block: blocks, windows and the host's verdicts go in; the verdicts, the
// texts' lengths, the traits and the blocks' status come back.
struct FastaMeta {
    Table<BgzfBlk> blks;
    Table<FastaWin> wins;
    Table<int32_t> status;
    Table<int64_t> text_len;
    Table<uint8_t> traits;
    Table<int32_t> blk_status;
    size_t in_bytes = 0;                   // the block's first bytes are what the host sends
    size_t bytes = 0;                      // the block, the host's and the device's; what the host reads back is [status.off, bytes)

    FastaMeta(int32_t n, size_t n_blks)
    {
        const size_t nw = (size_t)std::max(n, 1);
        Carve m;
        m.take(blks, std::max<size_t>(n_blks, 1));
        m.take(wins, nw);
        m.take(status, nw);
        in_bytes = m.off;
        m.take(text_len, nw);
        m.take(traits, nw);
        m.take(blk_status, std::max<size_t>(n_blks, 1));
        bytes = blk_status.off + sizeof(int32_t) * blk_status.n;
    }
    size_t back_bytes() const { return bytes - status.off; }
    template <typename B> B* back(B* block) const { return block + status.off; }

    void fill(uint8_t* h_meta, const FastaLayout& L, const int32_t* st, int32_t n) const
    {
        if (!L.blks.empty()) memcpy(blks.in(h_meta), L.blks.data(), sizeof(BgzfBlk) * L.blks.size());
        memcpy(wins.in(h_meta), L.wins.data(), sizeof(FastaWin) * L.wins.size());
        if (n) memcpy(status.in(h_meta), st, 4 * (size_t)n);
    }
};

// The read-back block and the text buffer into the caller's arrays: the answered windows' texts back to back, window i's at
// text[text_off[i], text_off[i + 1])
inline void gather_texts(int32_t n, const FastaMeta& M, const uint8_t* h_meta, const uint8_t* h_text, const std::vector<FastaWin>& wins,
                         uint8_t* text, int64_t* text_off, uint8_t* traits, int32_t* status)
{
    const int32_t* d_status = M.status.in(h_meta);
    const int64_t* tlen = M.text_len.in(h_meta);
    const uint8_t* d_traits = M.traits.in(h_meta);
    int64_t pos = 0;
    text_off[0] = 0;
    for (int32_t i = 0; i < n; ++i) {
        status[i] = d_status[i];
        traits[i] = d_traits[i];
        if (!status[i] && tlen[i]) {
            memcpy(text + pos, h_text + wins[(size_t)i].t_off, (size_t)tlen[i]);
            pos += tlen[i];
        }
        text_off[i + 1] = pos;
    }
}

}   // namespace vapor_readplan
