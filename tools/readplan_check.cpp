// readplan_check.cpp - the plan of a device reader call (vapor_amd/csrc/vapor_readplan.h: check_args, plan_spans, layout, ChopMeta,
// collect for vapor_bam_chop_device*; the same five over the one EvidenceMeta / EvidenceLayout of the four evidence calls, vapor_bam_depth_device,
// _signature_device, _links_device and _support_device (check_evidence<Mode>); plan_stretches, stage_stretches, layout_arena, place_windows, FastaMeta, gather_texts for
// vapor_fasta_windows_device) on a CPU, against direct statements of its rules.  It needs neither zlib nor files: the spans and
// stretches are block tables the program fills in itself, the calls come from fixed seeds, and every buffer is a heap allocation
// of exactly the bytes the header says it needs.  Nothing here is compared with recorded plans.
// Built and run once for the tests that quote it (tests/readplan_program.py):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DVBD_EMU -Iinclude -Ivapor_amd/csrc tools/readplan_check.cpp
#include "vapor_readplan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <numeric>
#include <random>
#include <string>

using namespace vapor_readplan;
using vapor_bgzf::Block;

static long g_case = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (case %ld)\n", g_case); exit(1); } } while (0)

static std::mt19937_64 rng(20261019);
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }      // lo .. hi
static bool one_in(int n) { return rng() % (uint64_t)n == 0; }
static uint64_t up64(uint64_t x) { return (x + 63) / 64 * 64; }

// ================================================================================================================================
// vapor_bam_chop_device*
// ================================================================================================================================
// why a region is refused, in the order of the issue's list
enum Bad { GOOD = 0, CHUNK_FIRST_DESCENDS, NO_CHUNKS, NEG_START, END_BELOW_START, END_2_31, NEG_FLANK, NEG_TID, CE_BELOW_CS, WIDE_CHUNK,
           PHASE_SETS, SITES_ORDER, PS_IDX, POS_BELOW_1, N_BAD };
static bool haplo_only(int b) { return b >= PHASE_SETS; }

struct Region {
    int32_t tid = 0;
    int64_t start = 0, end = 0, flank = 0;
    std::vector<std::pair<uint64_t, uint64_t>> chunks;
    std::vector<BamSite> sites;
    std::vector<int64_t> ps;
    int bad = GOOD;
};

static Region good_region(bool haplo)
{
    Region r;
    r.tid = rnd(0, 30);
    r.start = one_in(8) ? 0 : rnd(0, 1 << 30);
    r.end = one_in(8) ? r.start : one_in(8) ? ((int64_t)1 << 31) - 1 : r.start + rnd(0, 100000);
    r.flank = one_in(4) ? 0 : rnd(0, 5000);
    for (int k = rnd(0, 3); k > 0; --k) {
        const uint64_t c0 = (uint64_t)rnd(0, 1 << 28), len = one_in(20) ? ((uint64_t)1 << 27) : one_in(4) ? 0 : (uint64_t)rnd(0, 300000);
        const uint64_t u0 = (uint64_t)rnd(0, 65535), u1 = len == 0 ? (uint64_t)rnd((int)u0, 65535) : one_in(3) ? 0 : (uint64_t)rnd(0, 65535);
        r.chunks.push_back({c0 << 16 | u0, (c0 + len) << 16 | u1});
    }
    if (haplo) {
        const int n_ps = one_in(10) ? PHASE_SETS_CAP : rnd(0, 4);
        for (int p = 0; p < n_ps; ++p) r.ps.push_back((int64_t)rnd(1, 1 << 30));
        int32_t pos = 0;
        for (int k = n_ps ? rnd(0, 6) : 0; k > 0; --k) {
            pos += rnd(1, 1000);
            r.sites.push_back(BamSite{pos, (uint8_t)rnd(1, 8), (uint8_t)rnd(1, 8), (uint8_t)rnd(0, n_ps - 1), 0});
        }
    }
    return r;
}

// one reason to refuse it, put into a good region (CHUNK_FIRST_DESCENDS and NO_CHUNKS are the call's to arrange)
static Region bad_region(bool haplo, int bad)
{
    Region r = good_region(haplo);
    r.bad = bad;
    const uint64_t c0 = (uint64_t)rnd(1, 1 << 28);
    switch (bad) {
    case CHUNK_FIRST_DESCENDS: r.chunks.clear(); break;
    case NO_CHUNKS: if (r.chunks.empty()) r.chunks.push_back({c0 << 16, (c0 + 100) << 16}); break;
    case NEG_START: r.start = -rnd(1, 1000); break;
    case END_BELOW_START: r.start = rnd(1, 1 << 30); r.end = r.start - rnd(1, (int)std::min<int64_t>(r.start, 1000)); break;
    case END_2_31: r.end = ((int64_t)1 << 31) + (one_in(2) ? 0 : rnd(1, 1000)); break;
    case NEG_FLANK: r.flank = -rnd(1, 1000); break;
    case NEG_TID: r.tid = -rnd(1, 3); break;
    case CE_BELOW_CS: r.chunks.insert(r.chunks.begin() + rnd(0, (int)r.chunks.size()), {c0 << 16 | 7, one_in(2) ? (c0 << 16 | 6) : ((c0 - 1) << 16 | 9)}); break;
    case WIDE_CHUNK: r.chunks.insert(r.chunks.begin() + rnd(0, (int)r.chunks.size()), {c0 << 16, (c0 + ((uint64_t)1 << 27) + 1) << 16}); break;
    case PHASE_SETS: r.ps.assign((size_t)PHASE_SETS_CAP + 1, 5); r.sites.clear(); break;
    case SITES_ORDER: r.ps = {3, 4}; r.sites = {BamSite{100, 1, 2, 0, 0}, BamSite{one_in(2) ? 100 : 99, 1, 2, 1, 0}}; break;
    case PS_IDX: r.ps = {3, 4}; r.sites = {BamSite{100, 1, 2, 0, 0}, BamSite{200, 1, 2, 2, 0}}; break;
    case POS_BELOW_1: r.ps = {3}; r.sites = {BamSite{one_in(2) ? 0 : -5, 1, 2, 0, 0}, BamSite{200, 1, 2, 0, 0}}; break;
    }
    return r;
}

// the arrays of a call, owned
struct Call {
    std::vector<Region> regs;
    std::vector<int32_t> tid, chunk_first, site_first, ps_first, kept_first, status, tagged;
    std::vector<int64_t> start, end, flank, ps_values, q0, miss, phase_set;
    std::vector<uint64_t> chunks, sq_addr;
    std::vector<uint32_t> member;
    std::vector<BamSite> sites;
    ChopCall c;
    ChopOut o;

    Call(std::vector<Region> r, ChopMode mode, int max_keep, uint32_t filter_word, bool dedup) : regs(std::move(r))
    {
        const size_t n = regs.size();
        // (a chunk in front of the regions' for every range that is to end before it starts: no offset goes below 0.  The region behind
        // such a one then begins a chunk early, and has that chunk too)
        for (const Region& g : regs)
            if (g.bad == CHUNK_FIRST_DESCENDS) { chunks.push_back(5 << 16); chunks.push_back(6 << 16); }
        chunk_first.push_back((int32_t)(chunks.size() / 2)); site_first.push_back(0); ps_first.push_back(0);
        bool no_chunks = false;
        for (const Region& g : regs) {
            tid.push_back(g.tid); start.push_back(g.start); end.push_back(g.end); flank.push_back(g.flank);
            if (g.bad == CHUNK_FIRST_DESCENDS) {
                chunk_first.push_back(chunk_first.back() - 1);      // (the region's range of chunks ends before it starts)
            } else {
                for (const auto& k : g.chunks) { chunks.push_back(k.first); chunks.push_back(k.second); }
                chunk_first.push_back((int32_t)(chunks.size() / 2));
            }
            no_chunks |= g.bad == NO_CHUNKS;
            sites.insert(sites.end(), g.sites.begin(), g.sites.end());
            ps_values.insert(ps_values.end(), g.ps.begin(), g.ps.end());
            site_first.push_back((int32_t)sites.size());
            ps_first.push_back((int32_t)ps_values.size());
        }
        const size_t cap = n * (size_t)max_keep * 3;
        kept_first.assign(n + 1, -1); status.assign(n, -1); tagged.assign(n, -1); phase_set.assign(n, -1);
        sq_addr.assign(cap, 0); q0.assign(cap, 0); miss.assign(cap, 0); member.assign(cap, 0);
        c.n_regions = (int32_t)n; c.tid = tid.data(); c.start = start.data(); c.end = end.data(); c.flank = flank.data();
        c.chunk_first = chunk_first.data(); c.chunks = no_chunks || chunks.empty() ? nullptr : chunks.data();
        c.max_keep = max_keep; c.mode = mode; c.filter_word = filter_word; c.dedup = dedup;
        if (mode == ChopMode::HAPLOTAG) { c.site_first = site_first.data(); c.sites = sites.data(); c.ps_first = ps_first.data(); c.ps_values = ps_values.data(); }
        o.kept_first = kept_first.data(); o.sq_addr = sq_addr.data(); o.q0 = q0.data(); o.miss = miss.data(); o.status = status.data();
        if (c.phased()) { o.member = member.data(); o.phase_set = phase_set.data(); o.tagged = tagged.data(); }
    }
    Call(const Call&) = delete;
};

// the rule, stated region by region from the call's own arrays: 0, or why the host route must do the region
static int region_rule(const ChopCall& c, int32_t g)
{
    const int32_t a = c.chunk_first[g], b = c.chunk_first[g + 1];
    if (b < a) return REG_MALFORMED;
    if (b > a && !c.chunks) return REG_MALFORMED;
    if (c.start[g] < 0 || c.end[g] < c.start[g] || c.end[g] > 0x7FFFFFFFLL || c.flank[g] < 0 || c.tid[g] < 0) return REG_MALFORMED;
    if (c.haplo()) {
        const int32_t n_ps = c.ps_first[g + 1] - c.ps_first[g];
        if (n_ps > PHASE_SETS_CAP) return REG_PHASE_SETS;
        for (int32_t i = c.site_first[g]; i < c.site_first[g + 1]; ++i) {
            if ((int)c.sites[i].ps_idx >= n_ps || c.sites[i].pos < 1) return REG_MALFORMED;
            if (i > c.site_first[g] && c.sites[i].pos <= c.sites[i - 1].pos) return REG_MALFORMED;
        }
    }
    for (int32_t k = a; k < b; ++k) {
        const uint64_t cs = c.chunks[2 * k], ce = c.chunks[2 * k + 1];
        if (ce < cs) return REG_MALFORMED;
        if ((ce >> 16) - (cs >> 16) > 134217728u) return REG_MALFORMED;
    }
    return 0;
}

// plan_spans against the rule: statuses, and the spans of the regions that are read in region order, each chunk's file range at the
// next multiple of 64 of the staging block
static void check_spans(const Call& k, const SpanPlan& p)
{
    const ChopCall& c = k.c;
    CHECK((int32_t)p.span_first.size() == c.n_regions + 1, "span_first");
    size_t si = 0;
    uint64_t stage = 0;
    for (int32_t g = 0; g < c.n_regions; ++g) {
        const int want = region_rule(c, g);
        CHECK(k.status[(size_t)g] == want, "region %d: status %d, the rule says %d (reason %d)", g, k.status[(size_t)g], want, k.regs[(size_t)g].bad);
        // (a region refused for two reasons - its own and the call's missing chunk array, say - has the status of either)
        if (k.regs[(size_t)g].bad) CHECK(want == REG_MALFORMED || (want == REG_PHASE_SETS && k.regs[(size_t)g].bad == PHASE_SETS), "region %d: reason %d gives %d", g, k.regs[(size_t)g].bad, want);
        CHECK(p.span_first[(size_t)g] == (int32_t)si, "region %d: span_first", g);
        if (want) continue;
        for (int32_t q = c.chunk_first[g]; q < c.chunk_first[g + 1]; ++q, ++si) {
            CHECK(si < p.spans.size(), "region %d: a span is missing", g);
            const HostSpan& sp = p.spans[si];
            const uint64_t cs = c.chunks[2 * q], ce = c.chunks[2 * q + 1];
            // (through the block that holds the chunk's end: a whole block of 64 KB at the most and the header of the next)
            const uint64_t bytes = (ce >> 16) - (cs >> 16) + ((ce & 0xFFFF) ? 65536 + 64 : 0);
            CHECK(sp.region == g && sp.cs == cs && sp.ce == ce && sp.file_off == (int64_t)(cs >> 16) && sp.want == bytes && sp.got == 0, "region %d chunk %d: the span", g, q);
            CHECK(sp.stage_off == stage && stage % 64 == 0, "region %d chunk %d: staged at %zu, not %llu", g, q, sp.stage_off, (unsigned long long)stage);
            stage += up64(bytes);
        }
    }
    CHECK(si == p.spans.size() && p.span_first[(size_t)c.n_regions] == (int32_t)si, "%zu spans, %zu expected", p.spans.size(), si);
    CHECK(p.stage_bytes == stage, "staging size");
}

// the same call without region `drop`
static std::vector<Region> without(const std::vector<Region>& r, size_t drop)
{
    std::vector<Region> o;
    for (size_t i = 0; i < r.size(); ++i)
        if (i != drop) o.push_back(r[i]);
    return o;
}

static ChopMode mode_of(int m) { return m == 0 ? ChopMode::PLAIN : m == 1 ? ChopMode::RIGHT : m == 2 ? ChopMode::TAGGED : ChopMode::HAPLOTAG; }

static void check_statuses()
{
    long n_calls = 0, n_alone = 0, n_refused = 0;
    // each reason on its own, in the middle of good regions
    for (int m = 0; m < 4; ++m)
        for (int bad = 1; bad < N_BAD; ++bad) {
            if (haplo_only(bad) && m != 3) continue;
            for (int rep = 0; rep < 20; ++rep, ++g_case) {
                std::vector<Region> regs;
                const int before = rnd(1, 3), after = rnd(1, 3);
                for (int i = 0; i < before; ++i) regs.push_back(good_region(m == 3));
                regs.push_back(bad_region(m == 3, bad));
                for (int i = 0; i < after; ++i) regs.push_back(good_region(m == 3));
                // (without a chunk array no region that has chunks is read: the good ones of such a call have none)
                if (bad == NO_CHUNKS) for (Region& r : regs) if (!r.bad) r.chunks.clear();
                Call k(regs, mode_of(m), 20, 0, false);
                const Refusal ra = check_args(k.c, k.o);
                CHECK(!ra, "a call of good and refused regions is refused: %s", ra.msg);
                SpanPlan p;
                const Refusal r = plan_spans(k.c, k.status.data(), p);
                CHECK(!r, "refused: %s", r.msg);
                check_spans(k, p);
                for (size_t g = 0; g < regs.size(); ++g) CHECK(k.status[g] == ((int)g != before ? 0 : bad == PHASE_SETS ? REG_PHASE_SETS : REG_MALFORMED), "region %zu: status %d", g, k.status[g]);
                CHECK(p.span_first[(size_t)before] == p.span_first[(size_t)before + 1], "the refused region has spans");
                // the others are staged where the same call without it stages them (the two reasons that lie in the arrays the regions
                // share have no such call: check_spans holds them to the rule)
                if (bad != NO_CHUNKS && bad != CHUNK_FIRST_DESCENDS) {
                    Call k2(without(regs, (size_t)before), mode_of(m), 20, 0, false);
                    SpanPlan p2;
                    CHECK(!plan_spans(k2.c, k2.status.data(), p2), "refused");
                    CHECK(p2.spans.size() == p.spans.size() && p2.stage_bytes == p.stage_bytes, "%zu spans and %zu bytes with it, %zu and %zu without", p.spans.size(), p.stage_bytes, p2.spans.size(), p2.stage_bytes);
                    for (size_t i = 0; i < p.spans.size(); ++i)
                        CHECK(p.spans[i].stage_off == p2.spans[i].stage_off && p.spans[i].cs == p2.spans[i].cs && p.spans[i].region - (p.spans[i].region > before) == p2.spans[i].region, "span %zu", i);
                }
                ++n_alone;
            }
        }
    // mixed: any number of regions, a third of them refused for a reason drawn per region
    for (int t = 0; t < 3000; ++t, ++g_case) {
        const int m = rnd(0, 3);
        std::vector<Region> regs;
        bool no_chunks = false;
        for (int i = rnd(0, 9); i > 0; --i) {
            int bad = one_in(3) ? rnd(1, (m == 3 ? N_BAD : (int)PHASE_SETS) - 1) : GOOD;
            if (bad == NO_CHUNKS && !one_in(6)) bad = GOOD;
            no_chunks |= bad == NO_CHUNKS;
            regs.push_back(bad ? bad_region(m == 3, bad) : good_region(m == 3));
            n_refused += bad != GOOD;
        }
        Call k(regs, mode_of(m), rnd(1, KEPT_CAP), (uint32_t)rng(), one_in(2));
        CHECK(!check_args(k.c, k.o), "refused");
        SpanPlan p;
        CHECK(!plan_spans(k.c, k.status.data(), p), "refused");
        check_spans(k, p);
        (void)no_chunks;
        ++n_calls;
    }
    // the caller's tables themselves: an argument error, not a status
    {
        std::vector<Region> regs = {good_region(true), good_region(true), good_region(true)};
        regs[1].ps = {1, 2}; regs[1].sites = {BamSite{10, 1, 2, 0, 0}};
        auto refused = [&](int what, const char* msg) {
            Call k(regs, ChopMode::HAPLOTAG, 20, 0, false);
            switch (what) {
            case 0: k.site_first[0] = 1; break;
            case 1: k.ps_first[0] = 1; break;
            case 2: k.site_first[2] = k.site_first[1] - 1; break;
            case 3: k.ps_first[2] = k.ps_first[1] - 1; break;
            case 4: k.c.sites = nullptr; break;
            case 5: k.c.ps_values = nullptr; break;
            case 6: k.c.site_first = nullptr; break;
            case 7: k.c.max_keep = KEPT_CAP + 1; break;
            case 8: k.c.max_keep = 0; break;
            case 9: k.o.status = nullptr; break;
            case 10: k.o.tagged = nullptr; break;
            case 11: k.c.n_regions = -1; break;
            }
            const Refusal r = check_args(k.c, k.o);
            CHECK(r.code == VAPOR_E_ARG && std::string(r.msg) == msg, "table fault %d: %d %s", what, r.code, r.msg ? r.msg : "-");
        };
        for (int w : {0, 1, 6, 7, 8, 9, 10, 11}) refused(w, "vapor_bam_chop_device: bad argument");
        for (int w : {2, 3}) refused(w, "vapor_bam_chop_device_haplotag: site_first / ps_first do not ascend");
        for (int w : {4, 5}) refused(w, "vapor_bam_chop_device_haplotag: bad argument");
        Call ok(regs, ChopMode::HAPLOTAG, KEPT_CAP, 0, false);
        CHECK(!check_args(ok.c, ok.o), "the same call without a fault is refused");
    }
    printf("statuses: %d reasons, each alone among good regions in %ld calls and mixed in %ld calls with %ld refused regions, equal the rule\n", N_BAD - 1, n_alone, n_calls, n_refused);
}

// what scan_span leaves in a span, made up: blocks of up to 64 KB that hold data, the chunk's records between u_begin and u_end
static void fake_scan(HostSpan& sp)
{
    size_t pos = 0;
    uint64_t u = 0;
    for (int k = one_in(6) ? 0 : rnd(1, 5); k > 0; --k) {
        const int xlen = 6 + 4 * rnd(0, 2), c_len = rnd(1, 400);
        const uint32_t isize = (uint32_t)(one_in(5) ? 65536 : rnd(1, 3000));
        if (one_in(7)) pos += 28;               // (an empty block before it: the scan keeps none)
        sp.blks.push_back(Block{pos, xlen, xlen + 20 + c_len, (uint32_t)rng(), isize, u});
        pos += (size_t)(xlen + 20 + c_len);
        u += isize;
    }
    sp.got = sp.want;
    sp.u_total = u;
    sp.u_begin = u ? (uint64_t)rnd(0, (int)std::min<uint64_t>(u, 65535)) : 0;
    sp.u_end = sp.u_begin + (uint64_t)rnd(0, (int)(u - sp.u_begin));
    sp.bad = one_in(12);
    if (sp.bad) sp.blks.clear();
}

struct Tab { const char* name; size_t off, bytes; bool in, back; };
static std::vector<Tab> tables_of(const ChopMeta& M, bool phased, bool dedup)
{
    auto b = [](auto& t) { return sizeof(*t.in((uint8_t*)nullptr)) * t.n; };
    return {{"blks", M.blks.off, b(M.blks), true, false}, {"spans", M.spans.off, b(M.spans), true, false}, {"regs", M.regs.off, b(M.regs), true, false},
            {"site_ranges", M.site_ranges.off, b(M.site_ranges), true, false}, {"sites", M.sites.off, b(M.sites), true, false},
            {"ps_values", M.ps_values.off, b(M.ps_values), true, false},
            {"blk_status", M.blk_status.off, b(M.blk_status), false, true}, {"n_kept", M.n_kept.off, b(M.n_kept), false, true},
            {"reg_status", M.reg_status.off, b(M.reg_status), false, true}, {"phases", M.phases.off, b(M.phases), false, phased},
            {"picks", M.picks.off, b(M.picks), false, phased}, {"kept", M.kept.off, b(M.kept), false, !phased},
            {"keys", M.keys.off, b(M.keys), false, !phased && dedup}, {"tags", M.tags.off, b(M.tags), false, false}, {"ops", M.ops.off, b(M.ops), false, false}};
}

// Where the tables of a call lie, stated as the list of their sizes in the block's order.  `dedup` false: the list before the
// option existed.
static std::vector<size_t> sizes_of(const ChopCall& c, size_t n_blks, size_t n_spans, bool dedup)
{
    const size_t nr = (size_t)std::max(c.n_regions, 1), nb = std::max<size_t>(n_blks, 1), ns = std::max<size_t>(n_spans, 1);
    const bool ph = c.phased(), hp = c.haplo();
    std::vector<size_t> s = {24 * nb, 24 * ns, 40 * nr, hp ? 16 * nr : 0, hp ? 8 * std::max<size_t>(c.n_sites(), 1) : 0, hp ? 8 * std::max<size_t>(c.n_ps_values(), 1) : 0,
                             4 * nb, 4 * nr, 4 * nr, ph ? 16 * nr : 0, ph ? 16 * 3 * (size_t)c.max_keep * nr : 0, 16 * 256 * nr};
    s.push_back(dedup ? 8 * 256 * nr : 0);
    s.push_back(ph ? 16 * 256 * nr : 0);
    s.push_back(hp ? 16 * 256 * nr : 0);
    return s;
}

static void check_meta(const Call& k, const ChopMeta& M, size_t n_blks, size_t n_spans)
{
    const ChopCall& c = k.c;
    const bool phased = c.phased(), haplo = c.haplo();
    const std::vector<Tab> T = tables_of(M, phased, c.dedup);
    const std::vector<size_t> S = sizes_of(c, n_blks, n_spans, c.dedup);
    size_t off = 0, in_end = 0, back_lo = SIZE_MAX, back_hi = 0;
    for (size_t i = 0; i < T.size(); ++i) {
        CHECK(T[i].off % 64 == 0, "%s at %zu", T[i].name, T[i].off);
        CHECK(T[i].off == off && T[i].bytes == S[i], "%s: %zu bytes at %zu, the list says %zu at %zu", T[i].name, T[i].bytes, T[i].off, S[i], off);
        off += up64(S[i]);                      // (so they do not overlap, and an absent table takes no room)
        if (T[i].in && T[i].bytes) { CHECK(T[i].off == in_end, "%s: the inputs are not one prefix", T[i].name); in_end = off; }
        if (T[i].back) { back_lo = std::min(back_lo, T[i].off); back_hi = std::max(back_hi, off); }
        else CHECK(!T[i].bytes || T[i].in || T[i].off >= M.back_end, "%s lies in the read-back range", T[i].name);
    }
    CHECK(M.in_bytes == in_end && M.blks.off == 0, "in_bytes %zu, the inputs end at %zu", M.in_bytes, in_end);
    CHECK(M.bytes == off, "the block is %zu bytes, the tables end at %zu", M.bytes, off);
    CHECK(M.blk_status.off == back_lo && M.blk_status.off >= M.in_bytes && M.back_end == back_hi && M.back_bytes() == back_hi - back_lo, "read-back [%zu, %zu), collect reads [%zu, %zu)", M.blk_status.off, M.back_end, back_lo, back_hi);
    uint8_t* base = reinterpret_cast<uint8_t*>((uintptr_t)4096);
    CHECK(M.back(base) == base + back_lo, "back()");
    CHECK(M.host_bytes() == std::max(M.back_end, M.in_bytes), "host_bytes");
    // a mode's absent tables
    CHECK((M.site_ranges.n != 0) == haplo && (M.sites.n != 0) == haplo && (M.ps_values.n != 0) == haplo && (M.ops.n != 0) == haplo, "the haplotag tables");
    CHECK((M.phases.n != 0) == phased && (M.picks.n != 0) == phased && (M.tags.n != 0) == phased && (M.keys.n != 0) == c.dedup, "the phased tables, the keys");
    CHECK(reinterpret_cast<uint8_t*>(M.keys.in(base)) == (c.dedup ? base + M.keys.off : nullptr), "keys.in");
    if (!haplo) CHECK(!M.ops.in(base) && !M.sites.in(base) && M.ops.end() == M.ops.off, "an absent table");
    CHECK(M.picks_per_region == 3 * c.max_keep, "picks a region");
    if (c.dedup) {
        // with the option off every offset is what it was before the option existed
        ChopCall c0 = c;
        c0.dedup = false;
        const ChopMeta M0(c0, n_blks, n_spans);
        const std::vector<Tab> T0 = tables_of(M0, phased, false);
        const std::vector<size_t> S0 = sizes_of(c0, n_blks, n_spans, false);
        size_t o0 = 0;
        for (size_t i = 0; i < T0.size(); ++i) { CHECK(T0[i].off == o0 && T0[i].bytes == S0[i], "without the option, %s", T0[i].name); o0 += up64(S0[i]); }
        CHECK(M0.keys.n == 0 && M0.bytes == o0, "without the option, the keys");
    }
}

static void check_layout()
{
    long n_calls = 0, n_spans = 0, n_blks = 0, n_meta[8] = {0};
    for (int t = 0; t < 4000; ++t, ++g_case) {
        const int m = t % 4;
        const bool dedup = (t / 4) % 2;
        std::vector<Region> regs;
        for (int i = t < 16 ? 0 : rnd(0, 9); i > 0; --i) regs.push_back(one_in(5) ? bad_region(m == 3, rnd(NEG_START, (m == 3 ? N_BAD : (int)PHASE_SETS) - 1)) : good_region(m == 3));
        const uint32_t word = (uint32_t)rng();
        Call k(regs, mode_of(m), rnd(1, KEPT_CAP), word, dedup);
        SpanPlan p;
        CHECK(!check_args(k.c, k.o) && !plan_spans(k.c, k.status.data(), p), "refused");
        const std::vector<int32_t> host_status = k.status;
        for (HostSpan& sp : p.spans) fake_scan(sp);
        ChopLayout L;
        CHECK(!layout(k.c, p, k.status.data(), L), "refused");
        // a region with a span that did not scan is the host route's
        std::vector<int32_t> st = host_status;
        for (const HostSpan& sp : p.spans) if (sp.bad) st[(size_t)sp.region] = REG_MALFORMED;
        CHECK(st == k.status, "statuses after the scan");
        CHECK(L.regs.size() == std::max<size_t>(regs.size(), 1), "regions");
        uint64_t arena = 0;
        size_t ds = 0, nb = 0;
        for (size_t g = 0; g < regs.size(); ++g) {
            const BamRegion& R = L.regs[g];
            CHECK(R.start == regs[g].start && R.end == regs[g].end && R.flank == regs[g].flank && R.tid == regs[g].tid, "region %zu", g);
            CHECK((uint32_t)R.pad == word, "region %zu: the filter word", g);
            CHECK(R.span_first == (int32_t)ds, "region %zu: span_first", g);
            const int32_t have = st[g] ? 0 : p.span_first[g + 1] - p.span_first[g];
            CHECK(R.span_n == have, "region %zu: %d spans, %d expected", g, R.span_n, have);
            for (int32_t q = 0; q < have; ++q, ++ds) {
                const HostSpan& sp = p.spans[(size_t)(p.span_first[g] + q)];
                const BamSpan& D = L.spans[ds];
                CHECK(arena % 64 == 0 && D.u_begin == arena + sp.u_begin && D.u_end == arena + sp.u_end && D.u_limit == arena + sp.u_total, "span %zu in the arena at %llu", ds, (unsigned long long)arena);
                CHECK(D.blk_first == nb && D.blk_n == sp.blks.size() && D.pad == 0, "span %zu: blocks [%u, +%u), %zu expected from %zu", ds, D.blk_first, D.blk_n, sp.blks.size(), nb);
                for (const Block& b : sp.blks) {
                    const BgzfBlk& B = L.blks[nb++];
                    CHECK(B.u_off == arena + b.u && B.u_len == b.isize && B.crc == b.crc && B.pad == 0, "block %zu: its data", nb - 1);
                    CHECK(B.c_off == sp.stage_off + b.pos + 12 + (size_t)b.xlen && B.c_len == (uint32_t)(b.bsize - b.xlen - 20), "block %zu: its stream", nb - 1);
                    CHECK((uint64_t)B.u_off + B.u_len <= arena + sp.u_total, "block %zu: its data inside its span's", nb - 1);
                }
                arena += up64(sp.u_total);
            }
        }
        CHECK(ds == L.spans.size() && nb == L.blks.size() && L.arena == arena, "%zu spans, %zu blocks, arena %zu", L.spans.size(), L.blks.size(), L.arena);
        check_meta(k, L.meta, nb, ds);
        // fill: the tables in a block of exactly the host's size
        const ChopMeta& M = L.meta;
        std::vector<uint8_t> h(M.host_bytes(), 0xEE);
        M.fill(h.data(), k.c, L, k.status.data());
        CHECK(!nb || !memcmp(M.blks.in(h.data()), L.blks.data(), 24 * nb), "fill: blocks");
        CHECK(!ds || !memcmp(M.spans.in(h.data()), L.spans.data(), 24 * ds), "fill: spans");
        CHECK(!memcmp(M.regs.in(h.data()), L.regs.data(), 40 * L.regs.size()), "fill: regions");
        if (m == 3) {
            const BamSiteRange* sr = M.site_ranges.in(h.data());
            for (size_t g = 0; g < regs.size(); ++g) {
                const bool on = st[g] == 0;
                CHECK(sr[g].site_first == k.site_first[g] && sr[g].ps_first == k.ps_first[g] && sr[g].site_n == (on ? (int32_t)regs[g].sites.size() : 0) &&
                      sr[g].ps_n == (on ? (int32_t)regs[g].ps.size() : 0), "fill: region %zu's sites (status %d)", g, st[g]);
            }
            if (regs.empty()) CHECK(sr[0].site_n == 0 && sr[0].ps_n == 0, "fill: no region");
            CHECK(k.sites.empty() || !memcmp(M.sites.in(h.data()), k.sites.data(), 8 * k.sites.size()), "fill: sites");
            CHECK(k.ps_values.empty() || !memcmp(M.ps_values.in(h.data()), k.ps_values.data(), 8 * k.ps_values.size()), "fill: phase-set values");
        }
        ++n_calls; n_spans += (long)ds; n_blks += (long)nb; ++n_meta[m * 2 + dedup];
    }
    printf("staging and arena: %ld calls, %ld spans, %ld blocks lie where the rule says\n", n_calls, n_spans, n_blks);
    printf("metadata: 4 modes with and without de-duplication, %ld to %ld calls each: aligned, disjoint, inputs one prefix, the read-back range what collect reads\n",
           *std::min_element(n_meta, n_meta + 8), *std::max_element(n_meta, n_meta + 8));
}

static void check_limits()
{
    // 1.5 GB of staging: twelve chunks of 2^27 bytes are exactly that; one byte more is 64 more
    for (int extra = 0; extra < 2; ++extra, ++g_case) {
        std::vector<Region> regs;
        for (int i = 0; i < 12; ++i) {
            Region r;
            r.end = 100;
            const uint64_t c0 = (uint64_t)i << 28;
            r.chunks.push_back({c0 << 16, (c0 + ((uint64_t)1 << 27)) << 16});
            regs.push_back(r);
        }
        if (extra) { Region r; r.end = 100; r.chunks.push_back({(uint64_t)7 << 16, (uint64_t)8 << 16}); regs.insert(regs.begin() + 5, r); }
        Call k(regs, ChopMode::PLAIN, 20, 0, false);
        SpanPlan p;
        const Refusal r = plan_spans(k.c, k.status.data(), p);
        CHECK(p.stage_bytes == ((size_t)3 << 29) + (extra ? 64 : 0), "staging %zu", p.stage_bytes);
        if (!extra) CHECK(!r, "1.5 GB refused");
        else CHECK(r.code == VAPOR_E_ARG && std::string(r.msg) == "vapor_bam_chop_device: more than 1.5 GB of blocks in one call (use smaller batches)", "not refused: %s", r.msg ? r.msg : "-");
    }
    // 2 GB of block data: the arena and the 64 bytes behind it may be 2^31 bytes and no more
    for (int extra = 0; extra < 2; ++extra, ++g_case) {
        std::vector<Region> regs(3);
        for (size_t i = 0; i < 3; ++i) { regs[i].end = 100; regs[i].chunks.push_back({(uint64_t)(i + 1) << 24, (uint64_t)(i + 2) << 24}); }
        Call k(regs, ChopMode::PLAIN, 20, 0, false);
        SpanPlan p;
        CHECK(!plan_spans(k.c, k.status.data(), p) && p.spans.size() == 3, "refused");
        p.spans[0].u_total = ((uint64_t)1 << 30) - 1;         // (rounds up to 2^30)
        p.spans[1].u_total = ((uint64_t)1 << 29) + 64;
        p.spans[2].u_total = ((uint64_t)1 << 31) - ((uint64_t)1 << 30) - ((uint64_t)1 << 29) - 64 - 64 + (uint64_t)extra;
        ChopLayout L;
        const Refusal r = layout(k.c, p, k.status.data(), L);
        if (!extra) CHECK(!r && L.arena + 64 == (size_t)1 << 31 && L.spans[2].u_limit == 0x7FFFFFC0u, "2 GB refused, or arena %zu", L.arena);
        else CHECK(r.code == VAPOR_E_ARG && std::string(r.msg) == "vapor_bam_chop_device: more than 2 GB of block data in one call (use smaller batches)", "not refused: %s", r.msg ? r.msg : "-");
    }
    printf("limits: 1.5 GB of blocks and 2 GB of block data pass, 64 bytes and one byte more are refused\n");
}

// minimize_pacbio_read_list, by brute force: all of them in file order when there are no more than max_keep, else max_keep times the
// smallest miss_bp left, the earliest of several
static std::vector<int32_t> brute_select(const std::vector<int32_t>& miss, int32_t max_keep)
{
    std::vector<int32_t> out;
    if ((int32_t)miss.size() <= max_keep) {
        for (size_t i = 0; i < miss.size(); ++i) out.push_back((int32_t)i);
        return out;
    }
    std::vector<bool> taken(miss.size(), false);
    for (int32_t t = 0; t < max_keep; ++t) {
        int32_t best = -1;
        for (size_t i = 0; i < miss.size(); ++i)
            if (!taken[i] && (best < 0 || miss[i] < miss[(size_t)best])) best = (int32_t)i;
        taken[(size_t)best] = true;
        out.push_back(best);
    }
    return out;
}

static void check_collect()
{
    long n_regions = 0, n_entries = 0, n_calls = 0, n_full = 0, n_dev_status = 0, n_bad_union = 0;
    for (int t = 0; t < 1500; ++t, ++g_case) {
        const int m = t % 4;
        const bool phased = m >= 2, dedup = (t / 4) % 2;
        const int max_keep = one_in(4) ? 20 : rnd(1, KEPT_CAP);
        std::vector<Region> regs;
        for (int i = t < 8 ? 0 : rnd(1, 7); i > 0; --i) regs.push_back(good_region(m == 3));
        Call k(regs, mode_of(m), max_keep, 0, dedup);
        const size_t n = regs.size();
        const ChopMeta M(k.c, (size_t)rnd(0, 50), (size_t)rnd(0, 20));
        std::vector<uint8_t> h(M.host_bytes(), 0xEE);
        const uint64_t base = (uint64_t)0x7f0000000000ull + (rng() & 0xFFFFFF00u);
        // what the call must answer, written beside the block
        std::vector<int32_t> e_first(n + 1, 0), e_status(n, 0), e_tagged(n, 0);
        std::vector<int64_t> e_ps(n, INT64_MIN), e_q0, e_miss;
        std::vector<uint64_t> e_addr, e_keys;
        std::vector<uint32_t> e_member;
        for (size_t g = 0; g < n; ++g) {
            e_first[g] = (int32_t)e_addr.size();
            const int host = one_in(6) ? (one_in(2) ? REG_MALFORMED : REG_PHASE_SETS) : 0;
            const int dev = one_in(5) ? rnd(REG_BEYOND, REG_NO_SEQ) : 0;
            k.status[g] = host;
            e_status[g] = host ? host : dev;
            n_dev_status += !host && dev;
            M.reg_status.in(h.data())[g] = dev;
            const int nk = one_in(6) ? KEPT_CAP : one_in(3) ? rnd(0, std::min(max_keep, KEPT_CAP)) : rnd(0, KEPT_CAP);
            n_full += nk == KEPT_CAP;
            M.n_kept.in(h.data())[g] = nk;
            if (!phased) {
                std::vector<int32_t> ms;
                for (int i = 0; i < nk; ++i) {
                    const BamKept e{(uint32_t)rng(), rnd(0, 1 << 20), one_in(3) ? 0 : rnd(0, 6), rnd(1, 30000)};      // (few values: ties)
                    M.kept.in(h.data())[g * KEPT_CAP + (size_t)i] = e;
                    if (dedup) M.keys.in(h.data())[g * KEPT_CAP + (size_t)i] = rng();
                    ms.push_back(e.miss);
                }
                if (e_status[g]) continue;
                for (int32_t i : brute_select(ms, max_keep)) {
                    const BamKept& e = M.kept.in(h.data())[g * KEPT_CAP + (size_t)i];
                    e_addr.push_back(base + e.sq_off); e_q0.push_back(e.q0); e_miss.push_back(e.miss);
                    if (dedup) e_keys.push_back(M.keys.in(h.data())[g * KEPT_CAP + (size_t)i]);
                }
            } else {
                const int bad_union = one_in(8) ? (one_in(2) ? -1 : 3 * max_keep + rnd(1, 5)) : 0;
                const int nu = bad_union ? bad_union : one_in(4) ? 3 * max_keep : rnd(0, 3 * max_keep);
                M.phases.in(h.data())[g] = BamPhase{one_in(3) ? PS_NONE : (long long)rnd(1, 1 << 30), rnd(0, 1), nu};
                for (int i = 0; i < 3 * max_keep; ++i)
                    M.picks.in(h.data())[g * 3 * (size_t)max_keep + (size_t)i] = BamPick{(uint32_t)rng(), rnd(0, 1 << 20), rnd(0, 500), (uint32_t)rng()};
                if (e_status[g]) continue;
                if (bad_union) { e_status[g] = REG_MALFORMED; ++n_bad_union; continue; }
                e_ps[g] = M.phases.in(h.data())[g].ps;
                e_tagged[g] = M.phases.in(h.data())[g].tagged;
                for (int i = 0; i < nu; ++i) {
                    const BamPick& e = M.picks.in(h.data())[g * 3 * (size_t)max_keep + (size_t)i];
                    e_addr.push_back(base + e.sq_off); e_q0.push_back(e.q0); e_miss.push_back(e.miss); e_member.push_back(e.member);
                }
            }
        }
        e_first[n] = (int32_t)e_addr.size();
        // the caller's arrays: exactly as many entries as the answer has
        k.sq_addr.assign(e_addr.size(), 1); k.q0.assign(e_addr.size(), -1); k.miss.assign(e_addr.size(), -1); k.member.assign(e_member.size(), 1);
        k.sq_addr.shrink_to_fit(); k.q0.shrink_to_fit(); k.miss.shrink_to_fit(); k.member.shrink_to_fit();
        k.o.sq_addr = k.sq_addr.data(); k.o.q0 = k.q0.data(); k.o.miss = k.miss.data();
        if (phased) k.o.member = k.member.data();
        std::vector<uint64_t> keys = {1, 2, 3};
        collect(k.c, M, h.data(), base, k.o, keys);
        CHECK(k.kept_first == e_first, "kept_first");
        for (size_t g = 0; g < n; ++g) CHECK(k.kept_first[g] <= k.kept_first[g + 1], "kept_first descends at %zu", g);
        CHECK(std::vector<int32_t>(k.status.begin(), k.status.begin() + (long)n) == e_status, "statuses");
        CHECK(k.sq_addr == e_addr && k.q0 == e_q0 && k.miss == e_miss, "entries");
        if (phased) {
            CHECK(k.member == e_member && k.phase_set == e_ps && k.tagged == e_tagged, "members, phase sets, tagged");
            CHECK(keys.empty(), "keys of a phased call");
        } else {
            CHECK(keys == e_keys, "name keys: %zu, %zu expected", keys.size(), e_keys.size());
        }
        if (n == 0) CHECK(k.kept_first[0] == 0, "no region");
        ++n_calls; n_regions += (long)n; n_entries += (long)e_addr.size();
    }
    CHECK(n_full > 50 && n_dev_status > 50 && n_bad_union > 20, "the cases were not drawn");
    // the rule itself, as vapor_bam.cpp calls it
    for (int t = 0; t < 2000; ++t, ++g_case) {
        std::vector<int32_t> ms((size_t)rnd(0, 60)), order(ms.size());
        for (int32_t& x : ms) x = rnd(0, 5);
        std::iota(order.begin(), order.end(), 0);
        const int keep = rnd(1, 30);
        keep_smallest_miss(order, keep, [&](int32_t i) { return ms[(size_t)i]; });
        CHECK(order == brute_select(ms, keep), "keep_smallest_miss");
    }
    printf("collect: %ld calls, %ld regions (%ld full slots, %ld device statuses, %ld bad unions), %ld entries equal minimize_pacbio_read_list by brute force\n",
           n_calls, n_regions, n_full, n_dev_status, n_bad_union, n_entries);
}

// ================================================================================================================================
// vapor_fasta_windows_device
// ================================================================================================================================
// A file of blocks, made up: where each starts, how long it is, its data
struct FBlock { int64_t coff; int bsize; std::string data; uint32_t crc; };
struct File {
    std::vector<FBlock> b;
    std::map<int64_t, size_t> at;      // block start -> index
    int64_t end = 0;
    explicit File(int n)
    {
        int64_t c = rnd(0, 3) * 100;
        for (int i = 0; i < n; ++i) {
            FBlock k;
            k.coff = c;
            k.bsize = rnd(28, 400);
            const int isize = one_in(8) ? 0 : rnd(1, 500);
            for (int j = 0; j < isize; ++j) k.data.push_back((char)('!' + rng() % 90));
            k.crc = isize ? (uint32_t)rng() | 1u : 0;
            at[c] = b.size();
            b.push_back(k);
            c += k.bsize;
        }
        end = c;
    }
    // the first bytes of the block at `coff`, as the .hip's pread brings them: a BGZF header with BSIZE, or nothing
    size_t header(int64_t coff, uint8_t* h) const
    {
        auto it = at.find(coff);
        if (it == at.end()) return 0;
        const int bs = b[it->second].bsize - 1;
        const uint8_t hd[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, (uint8_t)(bs & 0xFF), (uint8_t)(bs >> 8)};
        memcpy(h, hd, sizeof hd);
        return sizeof hd;
    }
    uint64_t voff(size_t k, uint32_t u) const { return (uint64_t)(k < b.size() ? b[k].coff : end) << 16 | u; }
};

// what scan_stretch leaves in a stretch, from the made-up file: every block from c0 through the last needed one, a sentinel behind
// them; `cut_after` >= 0: the scan stopped behind that many blocks
static void fake_scan(FaStretch& s, const File& f, int cut_after = -1)
{
    uint64_t u = 0;
    size_t k = f.at.at(s.c0);
    int64_t c = s.c0;
    s.blks.clear();
    s.cut = false;
    for (; k < f.b.size() && (c < s.c_last || (c == s.c_last && s.need_last)); ++k) {
        if (cut_after >= 0 && (int)s.blks.size() == cut_after) { s.cut = true; break; }
        s.blks.push_back(Block{(size_t)(c - s.c0), 6, f.b[k].bsize, f.b[k].crc, (uint32_t)f.b[k].data.size(), u});
        u += f.b[k].data.size();
        c += f.b[k].bsize;
    }
    s.got = (size_t)(c - s.c0);
    s.blks.push_back(Block{(size_t)(c - s.c0), 0, 0, 0, 0, u});
    s.gidx.assign(s.blks.size(), 0);
}

struct Wins {
    std::vector<uint64_t> vbeg, vend;
    std::vector<int32_t> status;
    std::vector<uint8_t> traits;
    FastaCall call(int64_t text_cap) { status.assign(vbeg.size(), -1); traits.assign(vbeg.size(), 0xEE); return FastaCall{(int32_t)vbeg.size(), vbeg.data(), vend.data(), text_cap}; }
};

// random windows over the file: a few blocks long, neighbours that share blocks or touch, empty ones, reversed ones
static Wins random_windows(const File& f, int n)
{
    Wins w;
    for (int i = 0; i < n; ++i) {
        const size_t kb = (size_t)rnd(0, (int)f.b.size() - 1), ke = std::min(f.b.size(), kb + (size_t)rnd(0, 4));
        const uint32_t ub = (uint32_t)rnd(0, (int)f.b[kb].data.size());
        uint32_t ue = ke < f.b.size() ? (uint32_t)rnd(0, (int)f.b[ke].data.size()) : 0;
        if (ke == kb && ue < ub) ue = ub;
        uint64_t vb = f.voff(kb, ub), ve = f.voff(ke, ue);
        if (one_in(12)) ve = vb;
        if (one_in(15) && ve > vb) std::swap(vb, ve);
        w.vbeg.push_back(vb);
        w.vend.push_back(ve);
    }
    return w;
}

static void check_stretches(const FastaCall& c, const Wins& w, const StretchPlan& p)
{
    const int32_t n = c.n;
    // the chain of shared or touching blocks: windows whose ranges of block starts [first, last] meet are together, and so on
    std::vector<int32_t> comp((size_t)n);
    std::iota(comp.begin(), comp.end(), 0);
    auto root = [&](int32_t i) { while (comp[(size_t)i] != i) i = comp[(size_t)i]; return i; };
    auto live = [&](int32_t i) { return c.vend[i] > c.vbeg[i]; };
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < i; ++j)
            if (live(i) && live(j) && (c.vbeg[i] >> 16) <= (c.vend[j] >> 16) && (c.vbeg[j] >> 16) <= (c.vend[i] >> 16)) comp[(size_t)root(i)] = root(j);
    for (int32_t i = 0; i < n; ++i) {
        CHECK(w.traits[(size_t)i] == 0, "traits");
        if (!live(i)) {
            CHECK(p.st_of[(size_t)i] == -1 && w.status[(size_t)i] == (c.vend[i] < c.vbeg[i] ? WIN_RANGE : WIN_OK), "window %d: empty or reversed, status %d", i, w.status[(size_t)i]);
            continue;
        }
        const int32_t si = p.st_of[(size_t)i];
        CHECK(w.status[(size_t)i] == WIN_OK && si >= 0 && si < (int32_t)p.sts.size(), "window %d: no stretch", i);
        const FaStretch& s = p.sts[(size_t)si];
        const int64_t cb = (int64_t)(c.vbeg[i] >> 16), ce = (int64_t)(c.vend[i] >> 16);
        CHECK(s.c0 <= cb && (ce < s.c_last || (ce == s.c_last && (s.need_last || !(c.vend[i] & 0xFFFF)))), "window %d outside its stretch", i);
        for (int32_t j = 0; j < i; ++j)
            if (live(j)) CHECK((p.st_of[(size_t)j] == si) == (root(i) == root(j)), "windows %d and %d: one stretch %d, one chain %d", j, i, p.st_of[(size_t)j] == si, root(i) == root(j));
    }
    for (size_t q = 0; q < p.sts.size(); ++q) {
        const FaStretch& s = p.sts[q];
        if (q) CHECK(p.sts[q - 1].c_last < s.c0, "stretches %zu and %zu meet", q - 1, q);
        // the window that ends latest says where it ends and whether that block is needed
        uint64_t latest = 0;
        int64_t first = INT64_MAX;
        for (int32_t i = 0; i < n; ++i)
            if (p.st_of[(size_t)i] == (int32_t)q) { latest = std::max(latest, c.vend[i]); first = std::min(first, (int64_t)(c.vbeg[i] >> 16)); }
        CHECK(first == s.c0 && s.c_last == (int64_t)(latest >> 16) && s.need_last == ((latest & 0xFFFF) != 0), "stretch %zu: its ends", q);
    }
}

static void check_fasta()
{
    long n_calls = 0, n_st = 0, n_placed = 0, n_bytes = 0, n_refused = 0, n_cut = 0, n_short = 0, n_gather = 0;
    for (int t = 0; t < 1500; ++t, ++g_case) {
        const File f(rnd(1, 40));
        Wins w = random_windows(f, t < 5 ? 0 : rnd(1, 30));
        // the odd windows: a start that names no block, an in-block offset beyond the block's data
        const int n_ok = (int)w.vbeg.size();
        if (one_in(3)) {
            const size_t k = (size_t)rnd(0, (int)f.b.size() - 1);
            w.vbeg.push_back((uint64_t)(f.b[k].coff + 1) << 16); w.vend.push_back(f.voff(k + 1, 0));
            w.vbeg.push_back(f.voff(k, (uint32_t)f.b[k].data.size() + 1)); w.vend.push_back(f.voff(k + 1, 0));
            if (k + 1 < f.b.size()) { w.vbeg.push_back(f.voff(k, 0)); w.vend.push_back(f.voff(k + 1, (uint32_t)f.b[k + 1].data.size() + 1)); }
        }
        int64_t cap = 0;
        for (size_t i = 0; i < w.vbeg.size(); ++i) cap += 5 * 500;
        FastaCall c = w.call(cap);
        const int32_t n = c.n;
        StretchPlan p;
        plan_stretches(c, w.status.data(), w.traits.data(), p);
        check_stretches(c, w, p);
        // staging: the stretch through its last needed block, whose size its header says
        stage_stretches(p, [&](int64_t coff, uint8_t* h) { return f.header(coff, h); });
        uint64_t stage = 0;
        for (const FaStretch& s : p.sts) {
            uint64_t want = (uint64_t)(s.c_last - s.c0);
            if (s.need_last) want += f.at.count(s.c_last) ? (uint64_t)f.b[f.at.at(s.c_last)].bsize : 65536u;
            CHECK(s.room && s.want == want && s.stage_off == stage && stage % 64 == 0, "a stretch's staging: %zu bytes at %zu, %llu at %llu expected", s.want, s.stage_off, (unsigned long long)want, (unsigned long long)stage);
            stage += up64(want);
        }
        CHECK(p.stage_bytes == stage, "staging size");
        // the scan, some of them cut short
        std::vector<bool> named(p.sts.size());
        for (size_t q = 0; q < p.sts.size(); ++q) {
            named[q] = f.at.count(p.sts[q].c0) != 0;
            if (!named[q]) { p.sts[q].blks = {Block{0, 0, 0, 0, 0, 0}}; p.sts[q].gidx = {0}; p.sts[q].cut = true; continue; }       // (no block starts there)
            fake_scan(p.sts[q], f);
            if (one_in(6)) { fake_scan(p.sts[q], f, rnd(0, (int)p.sts[q].blks.size() - 1)); n_cut += p.sts[q].cut; }
        }
        FastaLayout L;
        layout_arena(p, L);
        // the arena from the file's own data
        std::string arena;
        std::vector<size_t> model;          // the file's block of every entry of the block table
        for (const FaStretch& s : p.sts) {
            CHECK(s.room && s.arena_off == arena.size() && arena.size() % 64 == 0, "a stretch's place in the arena");
            const size_t base = arena.size();
            for (size_t k = 0; k + 1 < s.blks.size(); ++k) {
                const size_t fb = f.at.at(s.c0 + (int64_t)s.blks[k].pos);
                CHECK(s.gidx[k] == model.size(), "gidx");
                CHECK(arena.size() == base + s.blks[k].u, "a block's data");
                if (f.b[fb].data.empty()) continue;
                const BgzfBlk& B = L.blks[model.size()];
                CHECK(B.u_off == arena.size() && B.u_len == f.b[fb].data.size() && B.crc == f.b[fb].crc && B.c_off == s.stage_off + s.blks[k].pos + 18 && B.c_len == (uint32_t)(f.b[fb].bsize - 26), "block table entry %zu", model.size());
                model.push_back(fb);
                arena += f.b[fb].data;
            }
            CHECK(s.gidx.back() == model.size(), "gidx of the sentinel");
            arena.resize(up64(arena.size()), '\0');
        }
        CHECK(model.size() == L.blks.size() && L.arena == arena.size(), "%zu blocks, arena %llu", L.blks.size(), (unsigned long long)L.arena);
        place_windows(c, p, w.status.data(), L);
        CHECK((int32_t)L.wins.size() == std::max(n, 1), "windows");
        uint64_t slots = 0;
        int last_placed = -1;
        for (int32_t i = 0; i < n; ++i) {
            const FastaWin& W = L.wins[(size_t)i];
            const int32_t si = p.st_of[(size_t)i];
            if (si < 0) { CHECK(W.a_beg == W.a_end && W.blk_n == 0 && w.status[(size_t)i] == (c.vend[i] < c.vbeg[i] ? WIN_RANGE : WIN_OK), "window %d", i); continue; }
            const FaStretch& s = p.sts[(size_t)si];
            // what the window spells, from the file: the data between its two virtual offsets
            const int64_t cb = (int64_t)(c.vbeg[i] >> 16), ce = (int64_t)(c.vend[i] >> 16);
            const uint32_t ub = (uint32_t)(c.vbeg[i] & 0xFFFF), ue = (uint32_t)(c.vend[i] & 0xFFFF);
            const int64_t scanned_end = s.c0 + (int64_t)s.blks.back().pos;
            bool ok = f.at.count(cb) && cb < scanned_end && (ce < scanned_end ? f.at.count(ce) != 0 : ce == scanned_end && ue == 0);
            if (ok) ok = ub <= f.b[f.at.at(cb)].data.size() && (ce == scanned_end || ue <= f.b[f.at.at(ce)].data.size());
            if (!ok) {
                CHECK(w.status[(size_t)i] == (s.cut ? WIN_BLOCK : WIN_RANGE) && W.a_beg == W.a_end && W.blk_n == 0, "window %d: status %d in a %s stretch", i, w.status[(size_t)i], s.cut ? "cut" : "whole");
                ++n_refused;
                continue;
            }
            std::string text;
            std::vector<size_t> holds;      // the non-empty blocks from the block of vbeg through that of vend (when it takes bytes of it)
            for (size_t k = f.at.at(cb); k < f.b.size() && f.b[k].coff <= ce; ++k) {
                const size_t a = f.b[k].coff == cb ? ub : 0, e = f.b[k].coff == ce ? ue : f.b[k].data.size();
                text += f.b[k].data.substr(a, e - a);
                if (!f.b[k].data.empty() && (f.b[k].coff < ce || ue)) holds.push_back(k);
            }
            CHECK(w.status[(size_t)i] == WIN_OK, "window %d: status %d", i, w.status[(size_t)i]);
            CHECK(W.a_end <= arena.size() && W.a_beg <= W.a_end && arena.substr(W.a_beg, W.a_end - W.a_beg) == text, "window %d does not spell its bytes", i);
            CHECK(W.t_off == slots, "window %d: slot at %llu, %llu expected", i, (unsigned long long)W.t_off, (unsigned long long)slots);
            slots += text.size();
            CHECK(W.blk_n == holds.size() && (holds.empty() || (W.blk_first + holds.size() <= model.size() && std::equal(holds.begin(), holds.end(), model.begin() + W.blk_first))), "window %d: its blocks", i);
            for (uint64_t a = W.a_beg; a < W.a_end; ++a) {
                bool in = false;
                for (uint32_t q = W.blk_first; q < W.blk_first + W.blk_n; ++q) in |= a >= L.blks[q].u_off && a < (uint64_t)L.blks[q].u_off + L.blks[q].u_len;
                CHECK(in, "window %d: byte %llu in none of its blocks", i, (unsigned long long)a);
            }
            if (!text.empty()) last_placed = i;
            ++n_placed; n_bytes += (long)text.size();
        }
        CHECK(L.slots == slots, "slots");
        (void)n_ok;
        // a text buffer one byte short: the last window with text no longer fits, the others keep their slots
        if (last_placed >= 0) {
            std::vector<int32_t> st2 = w.status;
            for (int32_t i = 0; i < n; ++i) if (p.st_of[(size_t)i] >= 0) st2[(size_t)i] = WIN_OK;
            FastaLayout L2;
            L2.blks = L.blks; L2.arena = L.arena;
            FastaCall c2 = c;
            c2.text_cap = (int64_t)slots - 1;
            place_windows(c2, p, st2.data(), L2);
            for (int32_t i = 0; i < n; ++i) {
                if (i == last_placed) { CHECK(st2[(size_t)i] == WIN_ROOM && L2.wins[(size_t)i].a_beg == L2.wins[(size_t)i].a_end, "the window that no longer fits: status %d", st2[(size_t)i]); continue; }
                // (behind it only windows without a byte of text are placed: where their empty slot lies says nothing)
                CHECK(st2[(size_t)i] == w.status[(size_t)i] && (i > last_placed || L2.wins[(size_t)i].t_off == L.wins[(size_t)i].t_off) && L2.wins[(size_t)i].a_beg == L.wins[(size_t)i].a_beg && L2.wins[(size_t)i].a_end == L.wins[(size_t)i].a_end, "window %d moved", i);
            }
            CHECK(L2.slots == L.wins[(size_t)last_placed].t_off, "slots of the short buffer");
            ++n_short;
        }
        // the metadata block, and the answers gathered from one of exactly its size
        const FastaMeta M(n, L.blks.size());
        {
            const size_t nw = (size_t)std::max(n, 1), nb = std::max<size_t>(L.blks.size(), 1);
            const size_t sz[6] = {24 * nb, 32 * nw, 4 * nw, 8 * nw, nw, 4 * nb};
            const size_t off[6] = {M.blks.off, M.wins.off, M.status.off, M.text_len.off, M.traits.off, M.blk_status.off};
            size_t o = 0;
            for (int q = 0; q < 6; ++q) { CHECK(off[q] == o && o % 64 == 0, "fasta table %d at %zu, %zu expected", q, off[q], o); if (q == 2) CHECK(M.in_bytes == o + up64(sz[q]), "in_bytes"); o += up64(sz[q]); }
            CHECK(M.bytes == M.blk_status.off + sz[5] && M.back_bytes() == M.bytes - M.status.off && M.status.off < M.in_bytes, "the block's size, the read-back range");
        }
        std::vector<uint8_t> h(M.bytes, 0xEE);
        M.fill(h.data(), L, w.status.data(), n);
        CHECK(L.blks.empty() || !memcmp(M.blks.in(h.data()), L.blks.data(), 24 * L.blks.size()), "fill: blocks");
        CHECK(!memcmp(M.wins.in(h.data()), L.wins.data(), 32 * L.wins.size()) && (!n || !memcmp(M.status.in(h.data()), w.status.data(), 4 * (size_t)n)), "fill: windows");
        std::vector<uint8_t> h_text((size_t)slots);
        for (uint8_t& x : h_text) x = (uint8_t)('a' + rng() % 26);
        std::string e_text;
        std::vector<int64_t> e_off(1, 0);
        std::vector<int32_t> d_status((size_t)n);
        std::vector<uint8_t> d_traits((size_t)n);
        for (int32_t i = 0; i < n; ++i) {
            // (the kernel leaves the host's verdict, finds a block or a byte it refuses, or answers: a text no longer than the raw bytes)
            d_status[(size_t)i] = w.status[(size_t)i] ? w.status[(size_t)i] : one_in(8) ? (one_in(2) ? WIN_BLOCK : WIN_NON_ASCII) : WIN_OK;
            d_traits[(size_t)i] = (uint8_t)rnd(0, 15);
            const FastaWin& W = L.wins[(size_t)i];
            const int64_t len = d_status[(size_t)i] ? (one_in(2) ? 0 : 7) : (int64_t)(W.a_end - W.a_beg) - rnd(0, (int)std::min<uint64_t>(W.a_end - W.a_beg, 9));
            M.status.in(h.data())[i] = d_status[(size_t)i];
            M.text_len.in(h.data())[i] = len;
            M.traits.in(h.data())[i] = d_traits[(size_t)i];
            if (!d_status[(size_t)i]) e_text.append(reinterpret_cast<const char*>(h_text.data()) + W.t_off, (size_t)len);
            e_off.push_back((int64_t)e_text.size());
        }
        std::vector<uint8_t> text(e_text.size());
        std::vector<int64_t> text_off((size_t)n + 1, -1);
        std::vector<int32_t> status((size_t)n, -1);
        std::vector<uint8_t> traits((size_t)n, 0xEE);
        gather_texts(n, M, h.data(), h_text.data(), L.wins, text.data(), text_off.data(), traits.data(), status.data());
        CHECK(text_off == e_off && std::string(text.begin(), text.end()) == e_text && status == d_status && traits == d_traits, "gather_texts");
        ++n_gather; ++n_calls; n_st += (long)p.sts.size();
    }
    printf("fasta stretches: %ld calls, %ld stretches: every window in one, ascending, disjoint, together by the chain of shared blocks\n", n_calls, n_st);
    printf("fasta windows: %ld windows spell their %ld bytes from their blocks, %ld refused (%ld stretches cut), %ld buffers one byte short\n", n_placed, n_bytes, n_refused, n_cut, n_short);
    printf("fasta answers: %ld calls gathered back to back\n", n_gather);
}

static void check_fasta_caps()
{
    // a stretch past STAGE_CAP, a stretch past ARENA_CAP: no room, for all its windows and only those
    Wins w;
    const uint64_t far = (uint64_t)1 << 32, big = STAGE_CAP + 1;
    w.vbeg = {(uint64_t)100 << 16, (far) << 16, (far + 10) << 16 | 5, (uint64_t)150 << 16 | 3, (2 * far) << 16, (3 * far) << 16, (3 * far + 50) << 16};
    w.vend = {(uint64_t)200 << 16, (far + big) << 16, (far + 20) << 16, (uint64_t)200 << 16, (2 * far + 300) << 16, (3 * far + 100) << 16, (3 * far + 100) << 16};
    FastaCall c = w.call((int64_t)1 << 31);      // (room for every text: nothing is allocated here)
    StretchPlan p;
    plan_stretches(c, w.status.data(), w.traits.data(), p);
    CHECK(p.sts.size() == 4 && p.st_of == (std::vector<int32_t>{0, 1, 1, 0, 2, 3, 3}), "stretches");
    stage_stretches(p, [](int64_t, uint8_t*) { return (size_t)0; });
    CHECK(p.sts[0].room && !p.sts[1].room && p.sts[2].room && p.sts[3].room && p.sts[0].stage_off == 0 && p.sts[2].stage_off == 128 && p.sts[3].stage_off == 128 + 320 && p.stage_bytes == 128 + 320 + 128, "the stretch past STAGE_CAP");
    // (a stretch of exactly the cap has room)
    {
        Wins w1;
        w1.vbeg = {0}; w1.vend = {STAGE_CAP << 16};
        FastaCall c1 = w1.call(0);
        StretchPlan p1;
        plan_stretches(c1, w1.status.data(), w1.traits.data(), p1);
        stage_stretches(p1, [](int64_t, uint8_t*) { return (size_t)0; });
        CHECK(p1.sts.size() == 1 && p1.sts[0].room && p1.stage_bytes == STAGE_CAP, "a stretch of STAGE_CAP bytes");
    }
    // the data of stretch 0 is small, that of stretch 2 fills the arena to its cap, that of stretch 3 passes it by one byte
    auto blocks = [](FaStretch& s, uint64_t u) { s.blks = {Block{0, 6, 100, 1, 10, 0}, Block{(size_t)(s.c_last - s.c0), 0, 0, 0, 0, u}}; s.gidx.assign(2, 0); };
    blocks(p.sts[0], 10);
    blocks(p.sts[2], ARENA_CAP - 64 - 64);
    blocks(p.sts[3], 1);
    FastaLayout L;
    layout_arena(p, L);
    CHECK(p.sts[0].room && p.sts[2].room && !p.sts[3].room && p.sts[2].arena_off == 64 && L.arena == ARENA_CAP - 64 && L.blks.size() == 2, "the stretch past ARENA_CAP: arena %llu", (unsigned long long)L.arena);
    place_windows(c, p, w.status.data(), L);
    CHECK(w.status == (std::vector<int32_t>{0, WIN_ROOM, WIN_ROOM, WIN_RANGE, 0, WIN_ROOM, WIN_ROOM}), "statuses %d %d %d %d %d %d %d", w.status[0], w.status[1], w.status[2], w.status[3], w.status[4], w.status[5], w.status[6]);
    printf("fasta caps: a stretch past STAGE_CAP or ARENA_CAP has no room, for all its windows and only those\n");
}

// ================================================================================================================================
// The evidence calls: vapor_bam_depth_device, _signature_device, _links_device, _support_device.  The header
// has one plan shape for the four (EvidenceMeta, EvidenceLayout, collect over plan_spans_of / layout_of), and so has the check:
// check_evidence<Mode> states the spans, the staging block, the arena, the block table, the metadata block, fill, collect and the
// two size refusals once.  A Mode below holds what is a call's own: how it is drawn, its argument rules, the rule of a region's
// record, its sizes and which of its words are signed.
// ================================================================================================================================
typedef std::vector<std::pair<uint64_t, uint64_t>> Chunks;

struct EvRegion {
    int32_t tid = 0;
    int64_t f[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // the call's fields, FIELDS of them
    Chunks chunks;
    bool bad = false;
};

// the arrays of a call as they were drawn
struct EvDrawn {
    int n = 0;
    std::vector<int32_t> tid, chunk_first = {0};
    std::vector<int64_t> fields;
    std::vector<uint64_t> chunks;
    std::vector<char> bad;
    std::vector<uint8_t> names;       // links
    void push(const EvRegion& r, int n_fields)
    {
        tid.push_back(r.tid);
        fields.insert(fields.end(), r.f, r.f + n_fields);
        for (auto& c : r.chunks) { chunks.push_back(c.first); chunks.push_back(c.second); }
        chunk_first.push_back((int32_t)(chunks.size() / 2));
        bad.push_back(r.bad);
    }
};

static Chunks evidence_chunks()
{
    Chunks out;
    for (int k = rnd(0, 3); k > 0; --k) {
        const uint64_t c0 = (uint64_t)rnd(0, 1 << 28), len = one_in(4) ? 0 : (uint64_t)rnd(0, 300000);
        const uint64_t u0 = (uint64_t)rnd(0, 65535), u1 = len == 0 ? (uint64_t)rnd((int)u0, 65535) : (uint64_t)rnd(0, 65535);
        out.push_back({c0 << 16 | u0, (c0 + len) << 16 | u1});
    }
    return out;
}

// a chunk of the region that ends before it starts, or one wider than 2^27
static void spoil_chunk(Chunks& chunks, bool wide)
{
    if (chunks.empty()) chunks.push_back({(uint64_t)5 << 16, (uint64_t)9 << 16});
    auto& c = chunks[(size_t)rnd(0, (int)chunks.size() - 1)];
    if (wide) c.second = ((c.first >> 16) + ((uint64_t)1 << 27) + 1) << 16;
    else c.second = c.first - 1 - (c.first > 1 ? (uint64_t)rnd(0, 1) : 0);
}

static EvRegion depth_region(int bad)       // bad: 0 good; 1 b0 < 0; 2..4 bounds descend; 5 b3 = 2^31; 6 tid < 0; 7 ce < cs; 8 a chunk wider than 2^27
{
    EvRegion r;
    r.tid = rnd(0, 30);
    int64_t x = one_in(6) ? 0 : rnd(0, 1 << 30);
    for (int k = 0; k < 4; ++k) { r.f[k] = x; x += one_in(3) ? 0 : rnd(0, 20000); }
    if (one_in(10)) r.f[3] = ((int64_t)1 << 31) - 1;
    r.chunks = evidence_chunks();
    r.bad = bad != 0;
    if (bad == 1) { r.f[0] = -1 - rnd(0, 5); }
    if (bad >= 2 && bad <= 4) { r.f[bad - 1] = r.f[bad - 2] - 1 - rnd(0, 9); if (bad == 2 && r.f[1] < 0) r.f[0] = 0, r.f[1] = -1; }
    if (bad == 5) r.f[3] = (int64_t)1 << 31;
    if (bad == 6) r.tid = -1 - rnd(0, 3);
    if (bad == 7 || bad == 8) spoil_chunk(r.chunks, bad == 8);
    return r;
}

static EvRegion sig_region(int bad)       // bad: 0 good; 1 w0 < 0; 2 w0 > w3; 3 w3 = 2^31; 4 tol < 0; 5 tol > 255; 6 nmin > nmax; 7 tid < 0; 8 ce < cs
{
    EvRegion r;
    r.tid = rnd(0, 30);
    r.f[0] = one_in(6) ? 0 : rnd(0, 1 << 30);
    r.f[1] = r.f[0] + (one_in(5) ? 0 : rnd(0, 20000));
    if (one_in(10)) r.f[1] = ((int64_t)1 << 31) - 1;
    r.f[2] = r.f[0] + rnd(-300, 300);
    r.f[3] = r.f[2] + rnd(0, 12000);
    r.f[4] = one_in(4) ? (one_in(2) ? 0 : 255) : rnd(0, 255);
    r.f[5] = one_in(5) ? rnd(-5, 0) : rnd(1, 100);
    r.f[6] = one_in(6) ? -(int64_t)rnd(0, 1 << 30) : rnd(0, 5000);
    r.f[7] = r.f[6] + (one_in(6) ? ((int64_t)1 << 40) : rnd(0, 9000));
    r.f[8] = one_in(8) ? 0xFFFF : rnd(0, 63);
    r.chunks = evidence_chunks();
    r.bad = bad != 0;
    if (bad == 1) { r.f[0] = -1 - rnd(0, 5); }
    if (bad == 2) { r.f[0] = r.f[1] + 1 + rnd(0, 9); }
    if (bad == 3) r.f[1] = (int64_t)1 << 31;
    if (bad == 4) r.f[4] = -1 - rnd(0, 3);
    if (bad == 5) r.f[4] = 256 + rnd(0, 1000);
    if (bad == 6) r.f[6] = r.f[7] + 1 + rnd(0, 9);
    if (bad == 7) r.tid = -1 - rnd(0, 3);
    if (bad == 8) spoil_chunk(r.chunks, false);
    return r;
}

// the length bounds of a signature or support region as its record carries them
static int64_t clamped_len(int64_t v) { return v < -1 ? (int64_t)-1 : (v > ((int64_t)1 << 28) ? ((int64_t)1 << 28) : v); }

// the first nine fields of a signature or support record: as given where they are in range, clamped where a clamp admits the same operations
template <typename Region>
static void sig_fields_rule(const Region& R, const int64_t* f, uint32_t mask_bits, int g)
{
    CHECK(R.w0 == f[0] && R.w3 == f[1] && R.x0 == f[2] && R.x1 == f[3] && R.tol == f[4], "region %d: its record", g);
    CHECK(R.min_clip == (f[5] < 1 ? 1 : f[5]) && R.mask == ((uint32_t)f[8] & mask_bits), "region %d: min_clip %d of %lld, mask %u", g, R.min_clip, (long long)f[5], R.mask);
    CHECK(R.nmin == clamped_len(f[6]) && R.nmax == clamped_len(f[7]) && R.nmin <= R.nmax, "region %d: length bounds", g);
}

struct DepthMode {
    using Call = DepthCall; using Layout = DepthLayout; using Word = uint64_t; using Out = uint64_t;
    static constexpr int FIELDS = 4, WORDS = 3, ITERS = 1500;
    static constexpr size_t REG_BYTES = 48, ANS_BYTES = 24;
    static constexpr uint32_t SIGNED = 0;
    static constexpr bool NAMES = false;
    static constexpr const char* ENTRY = "vapor_bam_depth_device";
    static constexpr const char* NAME = "depth";
    static constexpr const char* EQUAL = "statuses, spans, arena, tables and collected sums";
    static constexpr int64_t EXAMPLE[FIELDS] = {0, 10, 20, 30};
    static void draw(EvDrawn& d) { for (int g = 0; g < d.n; ++g) d.push(depth_region(one_in(4) ? rnd(1, 8) : 0), FIELDS); }
    static void bind(Call& c, const int64_t* fields, const EvDrawn&) { c.bounds = fields; }
    static void more_args(const Call&, Out*, int32_t*) {}
    // a refused region's record carries its fields all the same
    static void record(const DepthRegion& R, const Call& c, int g, bool)
    {
        CHECK(R.tid == c.tid[g] && R.filter == c.filter_word && !memcmp(R.b, c.bounds + 4 * (size_t)g, 32), "region %d: its record", g);
    }
};

struct SigMode {
    using Call = SigCall; using Layout = SigLayout; using Word = uint32_t; using Out = int64_t;
    static constexpr int FIELDS = SIG_FIELDS, WORDS = SIG_ANSWER_WORDS, ITERS = 1500;
    static constexpr size_t REG_BYTES = 72, ANS_BYTES = 40;
    static constexpr uint32_t SIGNED = (1u << 6) | (1u << 8);
    static constexpr bool NAMES = false;
    static constexpr const char* ENTRY = "vapor_bam_signature_device";
    static constexpr const char* NAME = "signature";
    static constexpr const char* EQUAL = "statuses, spans, arena, tables, clamped fields and collected words";
    static constexpr int64_t EXAMPLE[FIELDS] = {0, 100, 40, 60, 50, 30, 30, 200, 63};
    static void draw(EvDrawn& d) { for (int g = 0; g < d.n; ++g) d.push(sig_region(one_in(4) ? rnd(1, 8) : 0), FIELDS); }
    static void bind(Call& c, const int64_t* fields, const EvDrawn&) { c.regions = fields; }
    static void more_args(const Call&, Out*, int32_t*) {}
    static void record(const SigRegion& R, const Call& c, int g, bool refused)
    {
        const int64_t* f = c.regions + (size_t)FIELDS * (size_t)g;
        // a region the plan or the scan refused carries a record that asks nothing
        if (refused) { CHECK(R.mask == 0 && R.tol == 0 && R.w0 == 0 && R.w3 == 0, "region %d: a refused region's record", g); return; }
        sig_fields_rule(R, f, 63u, g);
        for (int64_t len : {(int64_t)0, (int64_t)1, f[6] - 1, f[6], f[7], f[7] + 1, ((int64_t)1 << 28) - 1})
            if (len >= 0 && len < ((int64_t)1 << 28))
                CHECK((len >= f[6] && len <= f[7]) == (len >= R.nmin && len <= R.nmax), "region %d: the clamped bounds admit other operations at %lld", g, (long long)len);
    }
};

struct LinkMode {
    using Call = LinkCall; using Layout = LinkLayout; using Word = uint32_t; using Out = int64_t;
    static constexpr int FIELDS = LINK_FIELDS, WORDS = LINK_ANSWER_WORDS, ITERS = 1000;
    static constexpr size_t REG_BYTES = 72, ANS_BYTES = 20;
    static constexpr uint32_t SIGNED = 1u << 3;
    static constexpr bool NAMES = true;
    static constexpr const char* ENTRY = "vapor_bam_links_device";
    static constexpr const char* NAME = "links";
    static constexpr const char* EQUAL = "statuses, tables, the name blob, clamped fields and collected words";
    static constexpr int64_t EXAMPLE[FIELDS] = {0, 100, 40, 60, 50, 30, 1, 0, 0, 0, 2};
    static void draw(EvDrawn& d)
    {
        const int64_t names_len = one_in(10) ? 0 : rnd(1, 400);
        d.names.resize((size_t)names_len);
        for (auto& ch : d.names) ch = (uint8_t)rnd(33, 126);
        for (int g = 0; g < d.n; ++g) {
            EvRegion r;
            int64_t* f = r.f;
            r.tid = rnd(0, 30);
            f[0] = one_in(6) ? 0 : rnd(0, 1 << 30);
            f[1] = f[0] + (one_in(5) ? 0 : rnd(0, 200));
            if (one_in(10)) f[1] = ((int64_t)1 << 31) - 1;
            f[2] = one_in(8) ? ((int64_t)1 << 50) : f[0] + rnd(-300, 300);
            f[3] = one_in(8) ? -((int64_t)1 << 50) : rnd(0, 1 << 30);
            f[4] = one_in(4) ? (one_in(2) ? 0 : 255) : rnd(0, 255);
            f[5] = one_in(5) ? rnd(-5, 0) : rnd(1, 100);
            f[6] = rnd(0, 1); f[7] = rnd(0, 1); f[8] = rnd(0, 1);
            f[10] = names_len ? rnd(1, (int)names_len) : 1;
            f[9] = names_len ? rnd(0, (int)(names_len - f[10])) : 0;
            r.chunks = evidence_chunks();
            // 1 w0 < 0; 2 w0 > w3; 3 w3 = 2^31; 4 tol < 0; 5 tol > 255; 6 ev; 7 pend; 8 rel; 9 an empty name; 10 a name past the blob;
            // 11 a negative offset; 12 tid < 0
            const int how = one_in(3) ? rnd(1, 12) : 0;
            if (how == 1) f[0] = -1 - rnd(0, 5);
            if (how == 2) f[0] = f[1] + 1 + rnd(0, 9);
            if (how == 3) f[1] = (int64_t)1 << 31;
            if (how == 4) f[4] = -1 - rnd(0, 3);
            if (how == 5) f[4] = 256 + rnd(0, 1000);
            if (how >= 6 && how <= 8) f[how] = one_in(2) ? 2 + rnd(0, 5) : -1 - rnd(0, 5);
            if (how == 9) f[10] = 0;
            if (how == 10) f[10] = names_len - f[9] + 1 + rnd(0, 5);
            if (how == 11) f[9] = -1 - rnd(0, 5);
            if (how == 12) r.tid = -1 - rnd(0, 3);
            r.bad = how != 0 || names_len == 0;
            // the one statement, against the rule spelled out
            CHECK(link_region_ok(r.tid, f, names_len) == !r.bad, "region %d: link_region_ok, how %d", g, how);
            d.push(r, FIELDS);
        }
    }
    static void bind(Call& c, const int64_t* fields, const EvDrawn& d)
    {
        c.regions = fields; c.names = d.names.empty() ? nullptr : d.names.data(); c.names_len = (int64_t)d.names.size();
    }
    static void more_args(const Call& c, Out* out, int32_t* status)
    {
        Call d = c; d.names_len = -1;
        CHECK(check_args(d, out, status).code == VAPOR_E_ARG, "a negative blob passes");
        if (c.names_len) { d = c; d.names = nullptr; CHECK(check_args(d, out, status).code == VAPOR_E_ARG, "a null blob passes"); }
    }
    static void record(const LinkRegion& R, const Call& c, int g, bool refused)
    {
        const int64_t* f = c.regions + (size_t)FIELDS * (size_t)g;
        if (refused) { CHECK(R.name_len == 0 && R.tol == 0 && R.w0 == 0 && R.w3 == 0 && R.bits == 0, "region %d: a refused region's record", g); return; }
        const int64_t far = (int64_t)1 << 40;
        CHECK(R.w0 == f[0] && R.w3 == f[1] && R.tol == f[4], "region %d: its record", g);
        CHECK(R.x == (f[2] > far ? far : f[2]) && R.y == (f[3] < -far ? -far : f[3]) && R.min_clip == (f[5] < 1 ? 1 : f[5]), "region %d: clamped fields", g);
        CHECK(R.bits == ((uint32_t)f[6] | (uint32_t)f[7] << 1 | (uint32_t)f[8] << 2) && R.name_off == (uint32_t)f[9] && R.name_len == (uint32_t)f[10], "region %d: bits and name", g);
        CHECK((uint64_t)R.name_off + R.name_len <= (uint64_t)c.names_len, "region %d: its name leaves the blob", g);
    }
};

struct SupMode {
    using Call = SupCall; using Layout = SupLayout; using Word = uint32_t; using Out = int64_t;
    static constexpr int FIELDS = SUP_FIELDS, WORDS = SUP_ANSWER_WORDS, ITERS = 1000;
    static constexpr size_t REG_BYTES = 80, ANS_BYTES = 28;
    static constexpr uint32_t SIGNED = 0;
    static constexpr bool NAMES = false;
    static constexpr const char* ENTRY = "vapor_bam_support_device";
    static constexpr const char* NAME = "support";
    static constexpr const char* EQUAL = "statuses, spans, arena, tables, clamped fields and collected words";
    static constexpr int64_t EXAMPLE[FIELDS] = {0, 100, 40, 60, 50, 30, 30, 200, 255, 51, 30};
    static void draw(EvDrawn& d)
    {
        for (int g = 0; g < d.n; ++g) {
            // the nine signature fields with their eight ways to be bad, then 9 flank < 1; 10 flank > 65535; 11 gmin < 1
            const int how = one_in(3) ? rnd(1, 11) : 0;
            EvRegion r = sig_region(how <= 8 ? how : 0);
            int64_t* f = r.f;
            if (one_in(8)) f[8] = rnd(0, 255);
            f[9] = one_in(4) ? (one_in(2) ? 1 : 65535) : rnd(1, 65535);
            f[10] = one_in(6) ? ((int64_t)1 << rnd(28, 40)) : rnd(1, 5000);
            if (how == 9) f[9] = -(int64_t)rnd(0, 9);
            if (how == 10) f[9] = 65536 + rnd(0, 1 << 20);
            if (how == 11) f[10] = -(int64_t)rnd(0, 9);
            r.bad = how != 0;
            // the one statement, against the rule spelled out (how 8 is a chunk that descends: the fields are good)
            const bool fields_bad = how != 0 && how != 8;
            CHECK(sup_region_ok(r.tid, f) == !fields_bad, "region %d: sup_region_ok, how %d", g, how);
            CHECK(!sup_region_ok(r.tid, f) || sig_region_ok(r.tid, f), "region %d: a support region is a signature region", g);
            d.push(r, FIELDS);
        }
    }
    static void bind(Call& c, const int64_t* fields, const EvDrawn&) { c.regions = fields; }
    static void more_args(const Call&, Out*, int32_t*) {}
    static void record(const SupRegion& R, const Call& c, int g, bool refused)
    {
        const int64_t* f = c.regions + (size_t)FIELDS * (size_t)g;
        if (refused) { CHECK(R.mask == 0 && R.tol == 0 && R.w0 == 0 && R.w3 == 0 && R.flank == 0 && R.gmin == 0, "region %d: a refused region's record", g); return; }
        sig_fields_rule(R, f, 255u, g);
        CHECK(R.flank == f[9], "region %d: flank %d", g, R.flank);
        CHECK(R.gmin == (f[10] > ((int64_t)1 << 28) ? ((int64_t)1 << 28) : f[10]) && R.gmin >= 1, "region %d: gmin %d of %lld", g, R.gmin, (long long)f[10]);
        for (int64_t len : {(int64_t)0, (int64_t)1, f[10] - 1, f[10], f[10] + 1, ((int64_t)1 << 28) - 1})
            if (len >= 0 && len < ((int64_t)1 << 28))
                CHECK((len >= f[10]) == (len >= R.gmin), "region %d: the clamped blocking length admits other operations at %lld", g, (long long)len);
    }
};

template <typename Mode>
static void check_evidence()
{
    using Call = typename Mode::Call;
    using Layout = typename Mode::Layout;
    using Word = typename Mode::Word;
    using Out = typename Mode::Out;
    constexpr size_t F = (size_t)Mode::FIELDS, W = (size_t)Mode::WORDS;
    long n_calls = 0, n_refused = 0, n_regions_seen = 0;
    for (int it = 0; it < Mode::ITERS; ++it) {
        g_case = it;
        EvDrawn d;
        d.n = one_in(15) ? 0 : rnd(1, 12);
        Mode::draw(d);
        const int n = d.n;
        Call c;
        c.n_regions = n; c.tid = d.tid.data(); c.chunk_first = d.chunk_first.data(); c.chunks = d.chunks.empty() ? nullptr : d.chunks.data();
        Mode::bind(c, d.fields.data(), d);
        const uint32_t low = (uint32_t)rnd(0, 65535), handle_word = low | ((uint32_t)rnd(0, 255) << 16);
        c.filter_word = depth_filter_word(handle_word);
        CHECK((c.filter_word & 0x704u) == 0x704u && (c.filter_word | 0x704u) == (handle_word | 0x704u), "filter word %x of %x", c.filter_word, handle_word);
        std::vector<Out> out(W * (size_t)std::max(n, 1), 77);
        std::vector<int32_t> status((size_t)std::max(n, 1), -9);
        CHECK(!check_args(c, out.data(), status.data()), "a good call is refused");
        if (n) {
            CHECK(check_args(c, nullptr, status.data()).code == VAPOR_E_ARG && check_args(c, out.data(), nullptr).code == VAPOR_E_ARG, "null outputs pass");
            Call e = c; Mode::bind(e, nullptr, d);
            CHECK(check_args(e, out.data(), status.data()).code == VAPOR_E_ARG, "null bounds or regions pass");
            e = c; e.n_regions = -1;
            CHECK(check_args(e, out.data(), status.data()).code == VAPOR_E_ARG, "a negative count passes");
            Mode::more_args(c, out.data(), status.data());
        }
        SpanPlan p;
        CHECK(!plan_spans(c, status.data(), p), "a call below the size limit is refused");
        // the statuses and the spans, against the rule stated per region
        size_t si = 0, stage = 0;
        for (int g = 0; g < n; ++g) {
            CHECK(status[(size_t)g] == (d.bad[(size_t)g] ? REG_MALFORMED : 0), "region %d: status %d, bad %d", g, status[(size_t)g], (int)d.bad[(size_t)g]);
            CHECK(p.span_first[(size_t)g] == (int32_t)si, "region %d: span_first", g);
            if (d.bad[(size_t)g]) { ++n_refused; continue; }
            for (int32_t k = d.chunk_first[(size_t)g]; k < d.chunk_first[(size_t)g + 1]; ++k) {
                const uint64_t cs = d.chunks[2 * (size_t)k], ce = d.chunks[2 * (size_t)k + 1];
                CHECK(si < p.spans.size(), "region %d: a span is missing", g);
                const HostSpan& sp = p.spans[si++];
                const size_t want = (size_t)((ce >> 16) - (cs >> 16)) + ((ce & 0xFFFFu) ? 65536 + 64 : 0);
                CHECK(sp.region == g && sp.cs == cs && sp.ce == ce && sp.file_off == (int64_t)(cs >> 16) && sp.want == want && sp.stage_off == stage, "region %d: span fields", g);
                stage += up64(want);
            }
        }
        CHECK(si == p.spans.size() && p.span_first[(size_t)n] == (int32_t)si && p.stage_bytes == stage, "spans %zu of %zu, stage %zu of %zu", si, p.spans.size(), stage, p.stage_bytes);
        // the layout after a made-up scan
        for (HostSpan& sp : p.spans) fake_scan(sp);
        const std::vector<int32_t> before = status;
        Layout L;
        CHECK(!layout(c, p, status.data(), L), "a layout below the size limit is refused");
        size_t arena = 0, n_blk = 0, n_sp = 0;
        CHECK((int)L.regs.size() == std::max(n, 1), "regions in the layout");
        for (int g = 0; g < n; ++g) {
            bool scan_bad = false;
            for (int32_t s = p.span_first[(size_t)g]; s < p.span_first[(size_t)g + 1]; ++s) scan_bad |= p.spans[(size_t)s].bad;
            CHECK(status[(size_t)g] == (scan_bad ? REG_MALFORMED : before[(size_t)g]), "region %d: status after the scan", g);
            const auto& R = L.regs[(size_t)g];
            const bool refused = status[(size_t)g] != 0;
            CHECK(R.span_first == (int32_t)n_sp, "region %d: span_first in the layout", g);
            Mode::record(R, c, g, refused);
            if (refused) { CHECK(R.span_n == 0, "a refused region has spans"); continue; }
            CHECK(R.tid == d.tid[(size_t)g] && R.filter == c.filter_word, "region %d: contig and filter", g);
            CHECK(R.span_n == p.span_first[(size_t)g + 1] - p.span_first[(size_t)g], "region %d: span_n", g);
            for (int32_t s = p.span_first[(size_t)g]; s < p.span_first[(size_t)g + 1]; ++s) {
                const HostSpan& sp = p.spans[(size_t)s];
                const BamSpan& b = L.spans[n_sp++];
                CHECK(b.u_begin == arena + sp.u_begin && b.u_end == arena + sp.u_end && b.u_limit == arena + sp.u_total && b.blk_first == n_blk && b.blk_n == sp.blks.size(),
                      "region %d: a span in the arena", g);
                for (const Block& k : sp.blks) {
                    const BgzfBlk& B = L.blks[n_blk++];
                    CHECK(B.c_off == sp.stage_off + k.payload() && B.c_len == k.c_len() && B.u_off == arena + k.u && B.u_len == k.isize && B.crc == k.crc, "a block of region %d", g);
                }
                arena += up64(sp.u_total);
            }
        }
        CHECK(L.arena == arena && L.blks.size() == n_blk && L.spans.size() == n_sp, "arena %zu of %zu", arena, L.arena);
        // the metadata block: the tables in order, on multiples of 64, without overlap (a call without a blob has a names table of
        // no bytes); what goes in first, what comes back last
        const auto& M = L.meta;
        const size_t nr = (size_t)std::max(n, 1), nb = std::max<size_t>(n_blk, 1), ns = std::max<size_t>(n_sp, 1);
        const size_t offs[7] = {M.blks.off, M.spans.off, M.regs.off, M.names.off, M.blk_status.off, M.ans.off, M.reg_status.off};
        const size_t sizes[7] = {24 * nb, 24 * ns, Mode::REG_BYTES * nr, Mode::NAMES ? std::max<size_t>(d.names.size(), 1) : 0, 4 * nb, Mode::ANS_BYTES * nr, 4 * nr};
        size_t at = 0;
        for (int t = 0; t < 7; ++t) { CHECK(offs[t] == at && at % 64 == 0, "table %d at %zu, not %zu", t, offs[t], at); at += up64(sizes[t]); }
        CHECK(M.bytes == at && M.in_bytes == M.blk_status.off && M.back_bytes() == M.bytes - M.blk_status.off, "the block's sizes");
        // fill and collect on a heap block of exactly those bytes
        std::vector<uint8_t> h(M.bytes, 0xEE);
        L.fill(h.data());
        CHECK(!memcmp(M.regs.in(h.data()), L.regs.data(), Mode::REG_BYTES * nr) && (!n_blk || !memcmp(M.blks.in(h.data()), L.blks.data(), 24 * n_blk)) &&
              (!n_sp || !memcmp(M.spans.in(h.data()), L.spans.data(), 24 * n_sp)) && (d.names.empty() || !memcmp(M.names.in(h.data()), d.names.data(), d.names.size())), "fill");
        Word* da = M.ans.in(h.data());
        int32_t* rs = M.reg_status.in(h.data());
        for (size_t g = 0; g < nr; ++g) {
            for (size_t k = 0; k < W; ++k) da[W * g + k] = (Word)rng();
            for (size_t k = 0; k < W; ++k) if ((Mode::SIGNED >> k) & 1u) da[W * g + k] = (Word)(uint32_t)(int32_t)rnd(-255, 255);
            rs[g] = one_in(5) ? rnd(1, 5) : 0;
        }
        std::vector<int32_t> st2 = status;
        collect(c, M, h.data(), out.data(), st2.data());
        for (int g = 0; g < n; ++g) {
            const bool host_refused = status[(size_t)g] != 0, dev_refused = rs[(size_t)g] != 0;
            CHECK(st2[(size_t)g] == (host_refused ? status[(size_t)g] : rs[(size_t)g]), "region %d: collected status", g);
            for (size_t k = 0; k < W; ++k) {
                const Word wd = da[W * (size_t)g + k];
                const Out want = host_refused || dev_refused ? (Out)0 : ((Mode::SIGNED >> k) & 1u) ? (Out)(int32_t)wd : (Out)wd;
                CHECK(out[W * (size_t)g + k] == want, "region %d: word %zu", g, k);
            }
        }
        ++n_calls;
        n_regions_seen += n;
    }
    // the two "in one call" refusals the Python side halves a group on
    {
        std::vector<int32_t> tid(40, 0), chunk_first(41), status(40);
        std::vector<int64_t> fields;
        std::vector<uint64_t> chunks;
        for (int g = 0; g < 40; ++g) {
            fields.insert(fields.end(), Mode::EXAMPLE, Mode::EXAMPLE + F);
            chunks.push_back((uint64_t)g << 44); chunks.push_back(((uint64_t)g << 44) + (((uint64_t)1 << 26) << 16));
            chunk_first[(size_t)g + 1] = g + 1;
        }
        EvDrawn d;
        d.names = {'c', '1'};
        Call c;
        c.n_regions = 40; c.tid = tid.data(); c.chunk_first = chunk_first.data(); c.chunks = chunks.data();
        Mode::bind(c, fields.data(), d);
        SpanPlan p;
        const Refusal r = plan_spans(c, status.data(), p);
        CHECK(r.code == VAPOR_E_ARG && strstr(r.msg, Mode::ENTRY) && strstr(r.msg, "in one call"), "2.5 GB of blocks pass");
        c.n_regions = 20;
        CHECK(!plan_spans(c, status.data(), p), "1.25 GB of blocks are refused");
        for (HostSpan& sp : p.spans) { sp.blks.push_back(Block{0, 6, 100, 0, 65536, 0}); sp.u_total = (uint64_t)120 << 20; sp.u_begin = 0; sp.u_end = 100; sp.got = sp.want; }
        Layout L;
        const Refusal r2 = layout(c, p, status.data(), L);
        CHECK(r2.code == VAPOR_E_ARG && strstr(r2.msg, Mode::ENTRY) && strstr(r2.msg, "in one call"), "2.4 GB of block data pass");
    }
    printf("%s plan: %ld calls with %ld regions (%ld refused): %s equal the rule; both size refusals say \"in one call\"\n", Mode::NAME, n_calls, n_regions_seen, n_refused,
           Mode::EQUAL);
}

// ================================================================================================================================
// The metadata blocks of the four evidence calls, pinned: one small call of each kind - three regions of which the second is
// refused (tid -1), chunks 2 + 1 + 2 so that four spans are left, a made-up scan of 2 + 1 + 1 + 1 = 5 blocks - and the literal
// in_bytes, bytes, back_bytes() and every table's offset.  The numbers were taken by running the four separate plans
// (DepthMeta, SigMeta, LinkMeta, SupMeta as structs of their own) before they became one template: what the device and the
// host agree on byte for byte must not move.  Nothing here draws from the seeded stream.
// ================================================================================================================================
template <typename Call, typename Layout>
static void pin_layout(const char* what, Call& c, std::initializer_list<size_t> want, bool none = false)      // none: a links call without a blob - no region has a name, all are refused
{
    const int32_t tid[3] = {0, -1, 0}, chunk_first[4] = {0, 2, 3, 5};
    uint64_t chunks[10];
    for (uint64_t k = 0; k < 5; ++k) { chunks[2 * k] = (k << 20) << 16; chunks[2 * k + 1] = ((k << 20) + 3000) << 16 | 100; }
    c.n_regions = 3; c.tid = tid; c.chunk_first = chunk_first; c.chunks = chunks;
    int32_t status[3];
    SpanPlan p;
    CHECK(!plan_spans(c, status, p), "%s: the pinned call is refused", what);
    CHECK(status[1] == REG_MALFORMED && p.spans.size() == (none ? 0u : 4u), "%s: %zu spans", what, p.spans.size());
    for (size_t s = 0; s < p.spans.size(); ++s) {
        HostSpan& sp = p.spans[s];
        for (int k = 0; k < (s == 0 ? 2 : 1); ++k) sp.blks.push_back(Block{(size_t)k * 500, 6, 426, 7u, 1000u, (uint64_t)k * 1000});
        sp.got = sp.want; sp.u_total = 1000 * sp.blks.size(); sp.u_begin = 10; sp.u_end = 900;
    }
    Layout L;
    CHECK(!layout(c, p, status, L), "%s: the pinned layout is refused", what);
    CHECK(L.blks.size() == (none ? 0u : 5u) && L.spans.size() == p.spans.size() && L.regs.size() == 3, "%s: blocks, spans, regions", what);
    const auto& M = L.meta;
    std::vector<size_t> got = {M.in_bytes, M.bytes, M.back_bytes(), M.blks.off, M.spans.off, M.regs.off};
    if constexpr (std::is_same<Call, LinkCall>::value) got.push_back(M.names.off);
    got.insert(got.end(), {M.blk_status.off, M.ans.off, M.reg_status.off});
    std::string s;
    for (size_t v : got) s += " " + std::to_string(v);
    CHECK(got == std::vector<size_t>(want), "%s: in_bytes, bytes, back_bytes, offsets:%s", what, s.c_str());
}

static void check_pins()
{
    const int64_t bounds[12] = {0, 10, 20, 30, 0, 10, 20, 30, 0, 10, 20, 30};
    int64_t sig[3 * SIG_FIELDS], link[3 * LINK_FIELDS], sup[3 * SUP_FIELDS];
    for (int g = 0; g < 3; ++g) {
        const int64_t f[SUP_FIELDS] = {0, 100, 40, 60, 5, 30, 1, 50, 63, 500, 50}, l[LINK_FIELDS] = {0, 100, 40, 60, 5, 30, 1, 0, 0, 0, 1};
        std::copy(f, f + SIG_FIELDS, sig + g * SIG_FIELDS);
        std::copy(f, f + SUP_FIELDS, sup + g * SUP_FIELDS);
        std::copy(l, l + LINK_FIELDS, link + g * LINK_FIELDS);
    }
    DepthCall d; d.bounds = bounds;
    pin_layout<DepthCall, DepthLayout>("depth", d, {448, 704, 256, 0, 128, 256, 448, 512, 640});
    SigCall s; s.regions = sig;
    pin_layout<SigCall, SigLayout>("signature", s, {512, 768, 256, 0, 128, 256, 512, 576, 704});
    const std::vector<uint8_t> names(70, 'c');
    LinkCall k; k.regions = link; k.names = names.data();
    k.names_len = 0;
    pin_layout<LinkCall, LinkLayout>("links, no blob", k, {448, 640, 192, 0, 64, 128, 384, 448, 512, 576}, true);
    k.names_len = 1;
    pin_layout<LinkCall, LinkLayout>("links, 1 byte", k, {576, 768, 192, 0, 128, 256, 512, 576, 640, 704});
    k.names_len = 70;
    pin_layout<LinkCall, LinkLayout>("links, 70 bytes", k, {640, 832, 192, 0, 128, 256, 512, 640, 704, 768});
    SupCall u; u.regions = sup;
    pin_layout<SupCall, SupLayout>("support", u, {512, 768, 256, 0, 128, 256, 512, 576, 704});
    printf("evidence pins: the metadata blocks of six small calls lie where the four separate plans put them\n");
}

int main()
{
    check_pins();
    check_statuses();
    check_layout();
    check_limits();
    check_collect();
    check_fasta();
    check_fasta_caps();
    check_evidence<DepthMode>();          // (behind the others: the calls above draw from the one seeded stream, and their counts are quoted)
    check_evidence<SigMode>();
    check_evidence<LinkMode>();
    check_evidence<SupMode>();
    printf("readplan_check: all equal\n");
    return 0;
}
