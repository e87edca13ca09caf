// bgzf_scan_check.cpp - the BGZF block parser, the block walk and the device readers' scans (vapor_amd/csrc/vapor_bgzf.h) on the
// host, against files this program writes itself with zlib - so it knows every block's offset, sizes and CRC - and against a direct
// statement of the span rule.  Every buffer the parser or a walk sees is a heap allocation of exactly the bytes that are
// available, so that the address sanitizer sees one byte of over-read.  Built and run by tests/test_bgzf_scan_cpu.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DVBD_EMU -Ivapor_amd/csrc tools/bgzf_scan_check.cpp -lz
#include "vapor_bgzf.h"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

using namespace vapor_bgzf;
typedef std::vector<uint8_t> Bytes;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

struct Rec { size_t off; int bsize, xlen; uint32_t crc, isize; size_t payload; uint64_t u; };   // what the writer knows of a block
struct File { Bytes raw; std::vector<Rec> recs; uint64_t u = 0; };

static std::mt19937_64 rng(20240611);

static void put16(Bytes& b, unsigned v) { b.push_back((uint8_t)v); b.push_back((uint8_t)(v >> 8)); }
static void put32(Bytes& b, uint32_t v) { put16(b, v & 0xFFFFu); put16(b, v >> 16); }

// a block of `data`; kind 0: the standard header (xlen 6), 1 and 2: one and two foreign subfields in front of BC, 3: one behind it
static void append_block(File& f, const Bytes& data, int kind, int level = 1)
{
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) abort();
    Bytes comp(deflateBound(&zs, (uLong)data.size()) + 16);
    uint8_t none = 0;
    zs.next_in = data.empty() ? &none : const_cast<Bytef*>(data.data());
    zs.avail_in = (uInt)data.size();
    zs.next_out = comp.data();
    zs.avail_out = (uInt)comp.size();
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
    comp.resize(zs.total_out);
    deflateEnd(&zs);
    Bytes extra;
    auto foreign = [&](char a, char b, int slen) { extra.push_back((uint8_t)a); extra.push_back((uint8_t)b); put16(extra, (unsigned)slen); for (int i = 0; i < slen; ++i) extra.push_back((uint8_t)rng()); };
    if (kind == 1 || kind == 2) foreign('X', 'Y', 2);
    if (kind == 2) foreign('B', 'D', 5);                       // (B without C, an odd length)
    const size_t bc = extra.size();
    extra.push_back('B'); extra.push_back('C'); put16(extra, 2); put16(extra, 0);
    if (kind == 3) foreign('Q', 'Q', 3);
    const size_t bsize = 12 + extra.size() + comp.size() + 8;
    CHECK(bsize <= 65536, "block of %zu bytes", bsize);
    extra[bc + 4] = (uint8_t)(bsize - 1); extra[bc + 5] = (uint8_t)((bsize - 1) >> 8);
    Rec r;
    r.off = f.raw.size(); r.bsize = (int)bsize; r.xlen = (int)extra.size(); r.isize = (uint32_t)data.size(); r.u = f.u;
    r.crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), data.empty() ? &none : data.data(), (uInt)data.size());
    r.payload = r.off + 12 + extra.size();
    const uint8_t head[10] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff};
    f.raw.insert(f.raw.end(), head, head + 10);
    put16(f.raw, (unsigned)extra.size());
    f.raw.insert(f.raw.end(), extra.begin(), extra.end());
    f.raw.insert(f.raw.end(), comp.begin(), comp.end());
    put32(f.raw, r.crc); put32(f.raw, r.isize);
    f.recs.push_back(r);
    f.u += data.size();
}

static Bytes dna(size_t n)
{
    Bytes d(n);
    for (auto& c : d) c = (uint8_t)"ACGT"[rng() & 3];
    return d;
}

// exactly n bytes on the heap, `lead` bytes in front of them (a stage offset)
struct Exact {
    std::unique_ptr<uint8_t[]> p;
    Exact(const uint8_t* src, size_t n, size_t lead = 0) : p(new uint8_t[lead + n]) { memset(p.get(), 0xEE, lead); if (n) memcpy(p.get() + lead, src, n); }
    const uint8_t* get() const { return p.get(); }
};

static std::vector<Block> walk_all(const uint8_t* bytes, size_t n, Walked& w)
{
    Exact e(bytes, n);
    std::vector<Block> got;
    w = walk(e.get(), n, 1000, [](int64_t) { return false; }, [&](const Block& b) { got.push_back(b); return true; });
    return got;
}

static void same(const Block& b, const Rec& r, size_t base_off, uint64_t base_u)
{
    CHECK(b.pos == r.off - base_off && b.bsize == r.bsize && b.xlen == r.xlen && b.crc == r.crc && b.isize == r.isize && b.payload() == r.payload - base_off &&
          b.c_len() == (uint32_t)(r.bsize - r.xlen - 20) && b.u == r.u - base_u, "block at %zu: pos %zu bsize %d xlen %d isize %u u %llu", r.off, b.pos, b.bsize, b.xlen, b.isize, (unsigned long long)b.u);
}

static void well_formed()
{
    long n_blocks = 0;
    for (int file = 0; file < 2; ++file) {
        File f;
        for (int i = 0; i < 300; ++i) {
            const unsigned pick = (unsigned)(rng() % 10);
            const size_t n = i == 299 || pick == 0 ? 0 : pick == 1 ? 65536 : pick == 2 ? 1 + rng() % 40 : rng() % 65537;
            append_block(f, dna(n), (int)(rng() % 4));
        }
        Walked w;
        const std::vector<Block> got = walk_all(f.raw.data(), f.raw.size(), w);
        CHECK(got.size() == f.recs.size() && w.end == End::MORE && w.pos == f.raw.size() && w.u == f.u, "%zu blocks of %zu", got.size(), f.recs.size());
        for (size_t k = 0; k < got.size(); ++k) {
            same(got[k], f.recs[k], 0, 0);
            // the block by itself, and with one byte missing
            Exact one(f.raw.data() + f.recs[k].off, (size_t)f.recs[k].bsize), less(f.raw.data() + f.recs[k].off, (size_t)f.recs[k].bsize - 1);
            Header h;
            CHECK(parse_block(one.get(), (size_t)f.recs[k].bsize, h) == Parse::BLOCK && h.bsize == f.recs[k].bsize && h.isize == f.recs[k].isize, "block %zu alone", k);
            CHECK(parse_block(less.get(), (size_t)f.recs[k].bsize - 1, h) == Parse::MORE && h.bsize == f.recs[k].bsize, "block %zu short of a byte", k);
        }
        n_blocks += (long)got.size();
    }
    printf("well-formed: %ld blocks equal the writer's table\n", n_blocks);
}

static void truncation()
{
    File f;
    append_block(f, dna(700), 0); append_block(f, dna(0), 1); append_block(f, dna(900), 3);
    for (size_t cut = 0; cut <= f.raw.size(); ++cut) {
        Walked w;
        const std::vector<Block> got = walk_all(f.raw.data(), cut, w);
        size_t whole = 0;
        while (whole < f.recs.size() && f.recs[whole].off + (size_t)f.recs[whole].bsize <= cut) ++whole;
        CHECK(w.end == End::MORE && got.size() == whole && w.pos == (whole ? f.recs[whole - 1].off + (size_t)f.recs[whole - 1].bsize : 0), "cut at %zu: %zu blocks, end %d", cut, got.size(), (int)w.end);
        for (size_t k = 0; k < whole; ++k) same(got[k], f.recs[k], 0, 0);
    }
    printf("truncation: a three-block file cut at every length gives its whole blocks, then more bytes (%zu cuts)\n", f.raw.size() + 1);
}

static HostSpan span_over(const File& f, size_t first, uint64_t cs_u, uint64_t ce, size_t lead, Exact** keep)
{
    HostSpan sp;
    sp.region = 0; sp.cs = ((uint64_t)f.recs[first].off << 16) | cs_u; sp.ce = ce;
    sp.file_off = (int64_t)f.recs[first].off;
    sp.want = (size_t)((int64_t)(ce >> 16) - sp.file_off) + ((ce & 0xFFFFu) ? ((size_t)1 << 16) + 64 : 0);      // (as bam_chop_device_impl reads it)
    sp.got = std::min(sp.want, f.raw.size() - f.recs[first].off);
    sp.stage_off = lead;
    *keep = new Exact(f.raw.data() + f.recs[first].off, sp.got, lead);
    scan_span(sp, (*keep)->get());
    return sp;
}

static void refusals()
{
    int n = 0;
    // `bytes` written over the middle block of three, at `at` from its start (or, negative, from its end)
    auto refused = [&](const char* what, long at, std::initializer_list<int> bytes, bool parse_refuses = true) {
        File f;
        append_block(f, dna(500), 0); append_block(f, dna(what[0] == 'e' ? 0 : 600), 0); append_block(f, dna(300), 0);
        const Rec& r = f.recs[1];
        size_t p = (size_t)((long)r.off + (at < 0 ? (long)r.bsize : 0) + at);
        for (int b : bytes) f.raw[p++] = (uint8_t)b;
        Exact one(f.raw.data() + r.off, (size_t)r.bsize);
        Header h;
        CHECK((parse_block(one.get(), (size_t)r.bsize, h) == Parse::NOT_BGZF) == parse_refuses, "%s: the parser", what);
        if (parse_refuses) {
            Walked w;
            const std::vector<Block> got = walk_all(f.raw.data(), f.raw.size(), w);
            CHECK(got.size() == 1 && w.end == End::BAD && w.pos == r.off, "%s: the walk", what);
        }
        Exact* e = nullptr;
        const HostSpan sp = span_over(f, 0, 0, (uint64_t)f.raw.size() << 16, 0, &e);
        CHECK(sp.bad, "%s: the span scan", what);
        FaStretch s;
        s.c0 = 0; s.c_last = (int64_t)f.recs[2].off; s.need_last = true; s.want = s.got = f.raw.size();
        scan_stretch(s, e->get());
        CHECK(s.cut && s.blks.size() == 2 && s.blks.back().pos == r.off, "%s: the stretch scan", what);
        delete e;
        ++n;
    };
    refused("magic byte 0", 0, {0x1e});
    refused("magic byte 1", 1, {0x8a});
    refused("magic byte 2", 2, {9});
    refused("FEXTRA clear", 3, {0});
    refused("no BC", 12, {'B', 'D'});
    refused("BC with SLEN 3", 14, {3, 0});
    refused("BC with SLEN 0", 14, {0, 0});
    refused("BC cut by the extra field's end, xlen 4", 10, {4, 0});
    refused("BC cut by the extra field's end, xlen 5", 10, {5, 0});
    refused("bsize below xlen + 20", 16, {6 + 20 - 2, 0});
    refused("isize 65537", -4, {1, 0, 1, 0});
    refused("empty block with a CRC", -8, {1}, false);
    printf("refusals: %d kinds refused by the parser, the walk, the span scan and the stretch scan\n", n);
}

static void spans()
{
    File f;
    for (int i = 0; i < 40; ++i) append_block(f, dna(i % 7 == 3 || i == 39 ? 0 : i % 5 == 0 ? 65536 : 1 + rng() % 30000), (int)(rng() % 4));
    int n_bad = 0, n_boundary = 0, n_zero = 0, n_inside = 0;
    for (int trial = 0; trial < 3000; ++trial) {
        const size_t i = rng() % f.recs.size(), j = i + rng() % std::min<size_t>(f.recs.size() - i, 6);
        const int kind = (int)(rng() % 4);
        // an end on the boundary behind block j, at block j with a zero in-block offset, inside block j, beyond its data
        uint64_t ce;
        if (kind == 0) ce = (uint64_t)(f.recs[j].off + (size_t)f.recs[j].bsize) << 16;
        else if (kind == 1) ce = (uint64_t)f.recs[j].off << 16;
        else if (kind == 2) ce = ((uint64_t)f.recs[j].off << 16) | (1 + rng() % 65535);
        else ce = ((uint64_t)f.recs[j].off << 16) | std::min<uint64_t>((uint64_t)f.recs[j].isize + 1 + rng() % 9, 65535);
        const uint64_t b0 = rng() % 8 == 0 ? std::min<uint64_t>((uint64_t)f.recs[i].isize + 1 + rng() % 50, 65535) : f.recs[i].isize ? rng() % ((uint64_t)f.recs[i].isize + 1) : 0;
        if (ce < (((uint64_t)f.recs[i].off << 16) | b0)) continue;                       // (the caller refuses such a chunk)
        const size_t lead = (rng() & 1) ? 64 : 0;
        Exact* e = nullptr;
        const HostSpan sp = span_over(f, i, b0, ce, lead, &e);
        delete e;
        // the rule, from the writer's table
        const uint64_t end_coff = ce >> 16, end_uoff = ce & 0xFFFFu;
        uint64_t u = 0, u_end = 0;
        bool have_end = false;
        std::vector<size_t> want;
        for (size_t k = i; k < f.recs.size(); ++k) {
            const Rec& r = f.recs[k];
            if (r.off > end_coff || (r.off == end_coff && end_uoff == 0)) break;
            if (r.off + (size_t)r.bsize - f.recs[i].off > sp.got) break;
            if (r.off == end_coff) { have_end = true; u_end = u + std::min<uint64_t>(end_uoff, r.isize); }
            if (r.isize) want.push_back(k);
            u += r.isize;
        }
        if (!have_end) u_end = u;
        const bool first_seen = !(f.recs[i].off == end_coff && end_uoff == 0);
        const bool bad = b0 > (first_seen ? f.recs[i].isize : 0u);
        CHECK(sp.bad == bad && sp.u_total == u && sp.u_end == u_end && sp.blks.size() == want.size() && (bad || sp.u_begin == b0), "trial %d: bad %d/%d total %llu/%llu end %llu/%llu blocks %zu/%zu",
              trial, (int)sp.bad, (int)bad, (unsigned long long)sp.u_total, (unsigned long long)u, (unsigned long long)sp.u_end, (unsigned long long)u_end, sp.blks.size(), want.size());
        for (size_t k = 0; k < want.size(); ++k) same(sp.blks[k], f.recs[want[k]], f.recs[i].off, f.recs[i].u);
        n_bad += bad; n_boundary += kind == 0; n_zero += kind == 1; n_inside += kind >= 2;
    }
    CHECK(n_bad > 50 && n_boundary > 300 && n_zero > 300 && n_inside > 600, "the trials miss a kind");
    printf("spans: 3000 chunks equal the rule (%d with a begin offset outside the first block)\n", n_bad);
}

static void wrap()
{
    File one;
    append_block(one, Bytes(65536, 0), 0, 6);
    for (long n : {65537L, 32767L}) {
        Bytes raw;
        raw.reserve(one.raw.size() * (size_t)n);
        for (long i = 0; i < n; ++i) raw.insert(raw.end(), one.raw.begin(), one.raw.end());
        HostSpan sp;
        sp.region = 0; sp.cs = 0; sp.ce = (uint64_t)raw.size() << 16; sp.file_off = 0; sp.want = sp.got = raw.size(); sp.stage_off = 0;
        Exact e(raw.data(), raw.size());
        scan_span(sp, e.get());
        const uint64_t total = (uint64_t)n * 65536u;
        CHECK(sp.u_total == total && sp.u_end == total && sp.blks.size() == (size_t)n && sp.blks.back().u == total - 65536u, "%ld blocks: total %llu", n, (unsigned long long)sp.u_total);
        CHECK(sp.bad == (total >= ((uint64_t)1 << 31)), "%ld blocks: bad %d", n, (int)sp.bad);
    }
    printf("wrap: 65537 blocks of 64 KB total 4295032832 bytes and are refused, 32767 are not\n");
}

static void stretches()
{
    File f;
    for (int i = 0; i < 12; ++i) append_block(f, dna(i == 5 ? 0 : 1000 + rng() % 3000), (int)(rng() % 4));
    int n = 0;
    for (size_t i = 0; i < f.recs.size(); ++i)
        for (size_t j = i; j < f.recs.size(); ++j)
            for (int need_last = 0; need_last < 2; ++need_last)
                for (int shorten = 0; shorten < 2; ++shorten) {
                    if (j == i && !need_last) continue;
                    FaStretch s;
                    s.c0 = (int64_t)f.recs[i].off; s.c_last = (int64_t)f.recs[j].off; s.need_last = need_last != 0;
                    Exact head(f.raw.data() + f.recs[j].off, std::min<size_t>(64, (size_t)f.recs[j].bsize));
                    CHECK(last_block_size(head.get(), std::min<size_t>(64, (size_t)f.recs[j].bsize)) == (uint64_t)f.recs[j].bsize, "the last block's size");
                    s.want = f.recs[j].off - f.recs[i].off + (need_last ? (size_t)f.recs[j].bsize : 0);
                    s.got = s.want - (size_t)shorten;                   // (the file ends a byte early)
                    s.stage_off = 64;
                    Exact e(f.raw.data() + f.recs[i].off, s.got, 64);
                    scan_stretch(s, e.get());
                    const size_t whole = j - i + (need_last ? 1 : 0) - (size_t)shorten;
                    CHECK(s.cut == (shorten != 0) && s.blks.size() == whole + 1 && s.gidx.size() == whole + 1, "stretch %zu..%zu: %zu blocks, cut %d", i, j, s.blks.size(), (int)s.cut);
                    for (size_t k = 0; k < whole; ++k) same(s.blks[k], f.recs[i + k], f.recs[i].off, f.recs[i].u);
                    const Block& end = s.blks.back();
                    const Rec* last = whole ? &f.recs[i + whole - 1] : nullptr;
                    CHECK(end.pos == (last ? last->off + (size_t)last->bsize - f.recs[i].off : 0) && end.isize == 0 && end.u == (last ? last->u + last->isize - f.recs[i].u : 0), "the sentinel");
                    ++n;
                }
    const uint8_t junk[64] = {0x1f, 0x8b, 8, 0};
    Exact j64(junk, 64), j10(f.raw.data(), 10);
    CHECK(last_block_size(j64.get(), 64) == 65536u && last_block_size(j10.get(), 10) == 65536u, "the fallback of the last block's size");
    printf("stretches: %d stretches equal the writer's table\n", n);
}

int main()
{
    well_formed();
    truncation();
    refusals();
    spans();
    wrap();
    stretches();
    printf("bgzf_scan_check: all equal\n");
    return 0;
}
