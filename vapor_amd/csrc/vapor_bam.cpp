// vapor_bam.cpp - host side of the read extraction: `samtools view bam chrom:start-end` + chop_pacbio_read_by_pos
// (SF:339-354) for one region, straight from a BGZF/BAM file.  No device code.
//
// The reference starts a samtools process per locus and parses its text; vapor_amd/bamio.py does the same work
// in-process in Python (and stays the statement this file is tested against, tests/test_bamio.py); this is the native
// form of its hot loop: the region's BGZF blocks are read with one pread, inflated by a few host threads (vapor_inflate.h),
// the records of the wanted reference are walked in file order, each CIGAR is walked in its binary form up to the window
// start (cigar2alignstart_by_pos, SF:309-337; the CG:B,I long-CIGAR convention included) and only the bases that are
// kept are decoded.  The .bai lookup (bins, linear index) stays in Python: it is a few dictionary reads per locus.
#include "vapor_hip.h"
#include "vapor_bgzf.h"
#include "vapor_inflate.h"
#include "vapor_names.h"
#include "vapor_readplan.h"
#include "vapor_sa.h"

#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

struct vapor_bam {
    int fd = -1;
    std::string path;
    int n_threads = 4;
    uint32_t min_mapq = 0, exclude_flags = 0;   // the read filter (vapor_bam_set_filter): (0, 0) filters nothing
    bool dedup = false;                         // one kept record per QNAME and region (vapor_bam_set_dedup; DESIGN.md 4.18 rule W)
    // the blocks of the chunk being walked: `comp` holds the file bytes from `comp_base` on, `data` their inflated bytes
    std::vector<uint8_t> comp, data;
    int64_t comp_base = 0;
    size_t scan_pos = 0;                // first byte of `comp` that is not part of a parsed block
    std::vector<int64_t> blk_coff;      // compressed file offset of every block
    std::vector<int64_t> blk_cpos;      // its position inside `comp`
    std::vector<int32_t> blk_csize;     // whole block size (header .. trailer)
    std::vector<int64_t> blk_ustart;    // where its inflated bytes start in `data`
    std::vector<int32_t> blk_usize;
    std::vector<vapor_inflate::Decoder> dec;   // decoder tables, one per inflate thread
};

static thread_local std::string g_bam_err;
extern "C" const char* vapor_bam_last_error(void) { return g_bam_err.c_str(); }
static int bfail(int code, const std::string& m) { g_bam_err = m; return code; }

extern "C" int vapor_bam_open(const char* path, vapor_bam** out)
{
    if (!path || !out) return bfail(VAPOR_E_ARG, "vapor_bam_open: null argument");
    int fd = open(path, O_RDONLY);
    if (fd < 0) return bfail(VAPOR_E_ARG, std::string("vapor_bam_open: cannot open ") + path);
    vapor_bam* b = new vapor_bam();
    b->fd = fd;
    b->path = path;
    const unsigned hc = std::thread::hardware_concurrency();
    b->n_threads = (int)std::max(1u, std::min(4u, hc ? hc / 2 : 1u));
    *out = b;
    return VAPOR_OK;
}

extern "C" int vapor_bam_close(vapor_bam* b)
{
    if (b) {
        if (b->fd >= 0) close(b->fd);
        delete b;
    }
    return VAPOR_OK;
}

// the descriptor and inflate-thread count of an open file, for vapor_bam_chop_device (vapor_hip.hip: it reads the file's blocks with
// positioned reads of its own and leaves the handle's buffers alone)
extern "C" int vapor_bam_fileno(vapor_bam* b) { return b ? b->fd : -1; }
extern "C" int vapor_bam_threads(vapor_bam* b) { return b ? b->n_threads : 1; }

extern "C" int vapor_bam_set_threads(vapor_bam* b, int32_t n)
{
    if (!b || n < 1 || n > 64) return bfail(VAPOR_E_ARG, "vapor_bam_set_threads: out of range");
    b->n_threads = n;
    return VAPOR_OK;
}

// The read filter of the handle: a record is filtered iff MAPQ < min_mapq or (FLAG & exclude_flags) != 0, and a
// filtered record is as if it were not in the file - every reader of this handle skips it behind the record checks.
extern "C" int vapor_bam_set_filter(vapor_bam* b, int32_t min_mapq, uint32_t exclude_flags)
{
    if (!b || min_mapq < 0 || min_mapq > 255 || exclude_flags > 65535u) return bfail(VAPOR_E_ARG, "vapor_bam_set_filter: out of range");
    b->min_mapq = (uint32_t)min_mapq;
    b->exclude_flags = exclude_flags;
    return VAPOR_OK;
}

// De-duplication by QNAME (`--dedup-qname`, DESIGN.md 4.18 rule W): among the records a reader of this handle keeps for one
// region, those with one name key (vapor_names.h) leave one survivor - the first that is neither secondary nor supplementary,
// else the first - and the others are as if they were not in the file.
extern "C" int vapor_bam_set_dedup(vapor_bam* b, int32_t on)
{
    if (!b || (on != 0 && on != 1)) return bfail(VAPOR_E_ARG, "vapor_bam_set_dedup: 0 or 1");
    b->dedup = on == 1;
    return VAPOR_OK;
}
// (for the device reader, vapor_hip.hip; not part of the C ABI)
extern "C" __attribute__((visibility("hidden"))) int vapor_bam_dedup_on(vapor_bam* b) { return b && b->dedup ? 1 : 0; }

// the filter as the device reader carries it in a region's spare word (vapor_hip.hip; not part of the C ABI):
// exclude_flags | min_mapq << 16
extern "C" __attribute__((visibility("hidden"))) uint32_t vapor_bam_filter_word(vapor_bam* b)
{
    return b ? (b->exclude_flags | (b->min_mapq << 16)) : 0u;
}

// Parses the BGZF blocks from scan_pos on (vapor_bgzf.h) and appends the whole ones to the block lists (a truncated last block
// is left for the next read); -1 when the bytes at scan_pos, behind them, are not BGZF.
static int scan_blocks(vapor_bam* b)
{
    int n = 0;
    const size_t p0 = b->scan_pos;
    const vapor_bgzf::Walked w = vapor_bgzf::walk(b->comp.data() + p0, b->comp.size() - p0, b->comp_base + (int64_t)p0,
        [](int64_t) { return false; },
        [&](const vapor_bgzf::Block& k) {
            b->blk_coff.push_back(b->comp_base + (int64_t)(p0 + k.pos));
            b->blk_cpos.push_back((int64_t)(p0 + k.pos));
            b->blk_csize.push_back(k.bsize);
            b->blk_usize.push_back((int32_t)k.isize);
            ++n;
            return true;
        });
    b->scan_pos = p0 + w.pos;
    return w.end == vapor_bgzf::End::BAD ? -1 : n;
}

// the block's own CRC32 (the four bytes before ISIZE) against the inflated bytes, as htslib checks it: a decoder bug or a
// damaged block that still inflates to ISIZE bytes must not become reads
static bool crc_ok(const uint8_t* blk, int bsize, const uint8_t* out, int isize)
{
    const uint8_t* t = blk + bsize - 8;
    const uint32_t want = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    return vapor_inflate::crc32_fast(out, (size_t)isize) == want;
}

static bool inflate_block(const uint8_t* blk, int bsize, uint8_t* out, int isize, vapor_inflate::Decoder& dec)
{
    const int xlen = blk[10] | (blk[11] << 8);
    if (bsize - xlen - 20 < 0 || isize < 0 || isize > 65536) return false;
    if (isize == 0) return crc_ok(blk, bsize, out, 0);
    if (vapor_inflate::inflate_raw(blk + 12 + xlen, (size_t)(bsize - xlen - 20), out, (size_t)isize, dec)) return crc_ok(blk, bsize, out, isize);
    // refused: zlib has the last word on whether the block is damaged
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<Bytef*>(blk + 12 + xlen);
    zs.avail_in = (uInt)(bsize - xlen - 20);
    zs.next_out = out;
    zs.avail_out = (uInt)isize;
    const int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    return rc == Z_STREAM_END && zs.avail_out == 0 && crc_ok(blk, bsize, out, isize);
}

extern "C" int vapor_inflate_raw(const uint8_t* in, int64_t in_n, uint8_t* out, int64_t out_n)
{
    if (in_n < 0 || out_n < 0 || (in_n && !in) || (out_n && !out)) return bfail(VAPOR_E_ARG, "vapor_inflate_raw: bad argument");
    static thread_local vapor_inflate::Decoder* dec = nullptr;
    if (!dec) dec = new vapor_inflate::Decoder();
    uint8_t none = 0;
    if (!vapor_inflate::inflate_raw(in ? in : &none, (size_t)in_n, out ? out : &none, (size_t)out_n, *dec))
        return bfail(VAPOR_E_ARG, "vapor_inflate_raw: not a DEFLATE stream of that size");
    return VAPOR_OK;
}

// the CRC-32 the block trailers are checked with, by itself (tests compare it with zlib's; `tables_only` takes the path of a
// host without carry-less multiply)
extern "C" uint32_t vapor_crc32(const uint8_t* data, int64_t n, int32_t tables_only)
{
    if (!data || n <= 0) return 0u;
    return vapor_inflate::crc32_fast(data, (size_t)n, !tables_only);
}

// inflates blocks [b0, b1) into data (their ustart already laid out), a few threads when there are several
static bool inflate_range(vapor_bam* b, size_t b0, size_t b1)
{
    const size_t n = b1 - b0;
    const int nt = (int)std::min<size_t>((size_t)b->n_threads, n);
    if (b->dec.size() < (size_t)std::max(nt, 1)) b->dec.resize((size_t)std::max(nt, 1));
    std::vector<char> ok((size_t)std::max(nt, 1), 1);
    auto work = [&](int t) {
        for (size_t i = b0 + (size_t)t; i < b1; i += (size_t)nt)
            if (!inflate_block(b->comp.data() + b->blk_cpos[i], b->blk_csize[i], b->data.data() + b->blk_ustart[i], b->blk_usize[i], b->dec[(size_t)t])) ok[(size_t)t] = 0;
    };
    if (nt <= 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
    }
    for (char c : ok)
        if (!c) return false;
    return true;
}

// lays the next scanned blocks, up to block b1, out behind the inflated bytes and inflates them (blocks are inflated in file
// order: the first blk_ustart.size() of the scanned ones are)
static bool take_blocks(vapor_bam* b, size_t b1)
{
    const size_t b0 = b->blk_ustart.size();
    b1 = std::min(b1, b->blk_coff.size());
    if (b1 <= b0) return true;
    int64_t u = (int64_t)b->data.size();
    for (size_t i = b0; i < b1; ++i) { b->blk_ustart.push_back(u); u += b->blk_usize[i]; }
    b->data.resize((size_t)u);
    return inflate_range(b, b0, b1);
}

// reads `bytes` more file bytes behind `comp`; false at end of file
static bool read_more(vapor_bam* b, size_t bytes)
{
    const size_t old = b->comp.size();
    b->comp.resize(old + bytes);
    const ssize_t got = pread(b->fd, b->comp.data() + old, bytes, (off_t)(b->comp_base + (int64_t)old));
    b->comp.resize(old + (size_t)std::max<ssize_t>(got, 0));
    return got > 0;
}

// makes sure `data` holds at least `upto` inflated bytes (a record may run past the chunk's own blocks); false at the end
// of the file or on bytes that are not BGZF
static thread_local bool g_bam_damaged = false;          // ensure() failed on damaged bytes, not at the end of the file
static bool ensure(vapor_bam* b, int64_t upto)
{
    g_bam_damaged = false;
    while ((int64_t)b->data.size() < upto) {
        // blocks that were read with the chunk but lie behind its end (a record runs into them), a few at a time
        if (b->blk_ustart.size() < b->blk_coff.size()) {
            if (!take_blocks(b, b->blk_ustart.size() + (size_t)std::max(b->n_threads, 1))) { g_bam_damaged = true; return false; }
            continue;
        }
        // (bytes that are not BGZF behind the chunk's end are met here, with or without more of the file behind them)
        const bool more = read_more(b, (size_t)1 << 17);
        if (scan_blocks(b) < 0) { g_bam_damaged = true; return false; }
        if (!more) return false;
    }
    return true;
}

static inline int32_t rd32(const uint8_t* p) { return (int32_t)(p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24)); }

// the CG:B,I array of a record's aux fields, or null
static const uint8_t* find_cg(const uint8_t* p, const uint8_t* end, int32_t* count)
{
    while (p + 3 <= end) {
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
        p += 3;
        int sz = 0;
        switch (ty) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': { while (p < end && *p) ++p; if (p >= end) return nullptr; ++p; continue; }
        case 'B': {
            if (p + 5 > end) return nullptr;
            const uint8_t sub = p[0];
            const int32_t cnt = rd32(p + 1);
            p += 5;
            const int es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            // (the array must lie inside the record)
            if (cnt < 0 || (int64_t)cnt * es > (int64_t)(end - p)) return nullptr;
            if (t0 == 'C' && t1 == 'G' && sub == 'I') { *count = cnt; return p; }
            p += (size_t)cnt * (size_t)es;
            continue;
        }
        default: return nullptr;
        }
        if (sz > end - p) return nullptr;
        p += sz;
    }
    return nullptr;
}

// The haplotype and phase set of a record's aux fields (`--phased`; vapor_amd/phase.py tags_from_aux is the same
// walk in Python): *hap = the value of the first HP field of integer type (c C s S i I) if it is 1 or 2, else 0; *ps = the value
// of the first PS field of integer type, VAPOR_PS_NONE without one.  find_cg's walk; it ends where both are found, at the end
// of the record, or at the first malformed field - what was found before that point stands.
static const int64_t VAPOR_PS_NONE = INT64_MIN;
static void find_tags(const uint8_t* p, const uint8_t* end, int64_t* hap, int64_t* ps)
{
    bool have_hp = false, have_ps = false;
    int64_t hp = 0;
    *ps = VAPOR_PS_NONE;
    while (p + 3 <= end && !(have_hp && have_ps)) {
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
        p += 3;
        int sz = 0;
        bool is_int = true;
        switch (ty) {
        case 'A': is_int = false; sz = 1; break;
        case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'f': is_int = false; sz = 4; break;
        case 'i': case 'I': sz = 4; break;
        case 'Z': case 'H': {
            const void* nul = memchr(p, 0, (size_t)(end - p));
            if (!nul) goto done;
            p = (const uint8_t*)nul + 1;
            continue;
        }
        case 'B': {
            if (p + 5 > end) goto done;
            const uint8_t sub = p[0];
            const int32_t cnt = rd32(p + 1);
            p += 5;
            const int es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (cnt < 0 || (int64_t)cnt * es > (int64_t)(end - p)) goto done;
            p += (size_t)cnt * (size_t)es;
            continue;
        }
        default: goto done;
        }
        if (sz > end - p) goto done;
        if (is_int) {
            const bool is_hp = t0 == 'H' && t1 == 'P' && !have_hp, is_ps = t0 == 'P' && t1 == 'S' && !have_ps;
            if (is_hp || is_ps) {
                int64_t v;
                switch (ty) {
                case 'c': v = (int8_t)p[0]; break;
                case 'C': v = p[0]; break;
                case 's': v = (int16_t)(p[0] | (p[1] << 8)); break;
                case 'S': v = p[0] | (p[1] << 8); break;
                case 'i': v = rd32(p); break;
                default:  v = (uint32_t)rd32(p); break;
                }
                if (is_hp) { hp = v; have_hp = true; } else { *ps = v; have_ps = true; }
            }
        }
        p += sz;
    }
done:
    *hap = (hp == 1 || hp == 2) ? hp : 0;
}

// The haplotag of a record from the phased heterozygous SNVs of its locus (`--phase-vcf`; vapor_amd/phase.py
// haplotag is the statement): n sites in position order - pos 1-based, a1 / a2 what haplotype 1 / 2 carries as BAM 4-bit codes,
// ps the site's phase set.  The record's operations are walked with SAM's cursors (M = X advance reference and query, I S the
// query, D N the reference, H P neither); a site inside an M, = or X operation reads its base from the packed SEQ and votes for
// haplotype 1 (a1), haplotype 2 (a2) or not at all.  The phase set with the most votes decides, ties to the smallest value.
struct HapSites {
    int32_t n;
    const int64_t* pos;
    const uint8_t* a1;
    const uint8_t* a2;
    const int64_t* ps;
};
static void haplotag_record(const uint8_t* ops, int32_t n_ops, int64_t pos1, const uint8_t* sq, int32_t l_seq, const HapSites& hs,
                            int64_t* hap, int64_t* ps)
{
    struct Tally { int64_t ps, n1, n2; };
    std::vector<Tally> tally;
    int64_t rr = pos1, q = 0;
    int32_t si = 0;
    for (int32_t t = 0; t < n_ops && si < hs.n; ++t) {
        const uint32_t o = (uint32_t)rd32(ops + 4 * t), code = o & 15u;
        const int64_t n = o >> 4;
        if (code == 0u || code == 7u || code == 8u) {
            while (si < hs.n && hs.pos[si] < rr) ++si;
            for (; si < hs.n && hs.pos[si] < rr + n; ++si) {
                const int64_t qi = q + hs.pos[si] - rr;
                if (qi >= l_seq) continue;
                const uint8_t byte = sq[qi >> 1];
                const uint8_t nib = (qi & 1) ? (byte & 15) : (byte >> 4);
                const int vote = nib == hs.a1[si] ? 1 : nib == hs.a2[si] ? 2 : 0;
                if (!vote) continue;
                size_t k = 0;
                while (k < tally.size() && tally[k].ps != hs.ps[si]) ++k;
                if (k == tally.size()) tally.push_back({hs.ps[si], 0, 0});
                ++(vote == 1 ? tally[k].n1 : tally[k].n2);
            }
            rr += n; q += n;
        } else if (code == 1u || code == 4u) {
            q += n;
        } else if (code == 2u || code == 3u) {
            rr += n;
        }
    }
    *hap = 0;
    *ps = VAPOR_PS_NONE;
    const Tally* best = nullptr;
    for (const Tally& t : tally)
        if (!best || t.n1 + t.n2 > best->n1 + best->n2 || (t.n1 + t.n2 == best->n1 + best->n2 && t.ps < best->ps)) best = &t;
    if (best && best->n1 != best->n2) { *hap = best->n1 > best->n2 ? 1 : 2; *ps = best->ps; }
}

// Every size field of the file is checked before it is used (a damaged ISIZE reached the inflaters as a
// buffer size); a file that breaks a rule is VAPOR_E_ARG with a message, never a read or write outside `comp` / `data`.
static int bam_chop_impl(vapor_bam* b, int32_t tid, int64_t start, int64_t end, int64_t flank, int32_t n_chunks,
                         const uint64_t* chunks, uint8_t* seq_out, int64_t seq_cap, char* names_out, int64_t names_cap,
                         int64_t* meta, int32_t max_reads, int32_t* n_reads, int64_t* need, int meta_w = 4, bool right = false,
                         const HapSites* sites = nullptr)
{
    if (!b || !n_reads || (n_chunks && !chunks)) return bfail(VAPOR_E_ARG, "vapor_bam_chop: null argument");
    if (seq_cap < 0 || names_cap < 0 || max_reads < 0 || (max_reads && (!meta || !seq_out || !names_out)))
        return bfail(VAPOR_E_ARG, "vapor_bam_chop: bad output buffers");
    static const char* NT16 = "=ACMGRSVTWYHKDBN";
    const int64_t beg = std::max<int64_t>(start - 1, 0), stop = end;     // 0-based half-open region
    int64_t seq_used = 0, names_used = 0;
    int32_t nr = 0;
    bool overflow = false;
    std::vector<uint64_t> dd_key;         // `--dedup-qname`: key and (FLAG & 0x900) != 0 of every kept record, in record order
    std::vector<uint8_t> dd_sec;
    for (int32_t c = 0; c < n_chunks; ++c) {
        const uint64_t cs = chunks[2 * c], ce = chunks[2 * c + 1];
        // the chunk's own compressed range in one read, its blocks inflated together
        b->comp.clear(); b->data.clear(); b->scan_pos = 0;
        b->blk_coff.clear(); b->blk_cpos.clear(); b->blk_csize.clear(); b->blk_ustart.clear(); b->blk_usize.clear();
        b->comp_base = (int64_t)(cs >> 16);
        // (index chunks come from a file as well: an end before the start, or gigabytes for one locus, is a damaged .bai)
        if (ce < cs || (ce >> 16) - (cs >> 16) > ((uint64_t)1 << 31))
            return bfail(VAPOR_E_ARG, "vapor_bam_chop: implausible index chunk for " + b->path);
        // through the block that holds the chunk's end (none of it when the chunk ends on a block boundary)
        const size_t span = (size_t)((int64_t)(ce >> 16) - b->comp_base) + ((ce & 0xFFFFu) ? ((size_t)1 << 16) + 64 : 0);
        if (span == 0 || !read_more(b, span)) continue;
        // (the read holds more than the chunk: what is not BGZF behind the chunk's end is refused when a record runs into it, ensure(),
        // as the device reader, whose scan ends with the chunk, leaves such a region to this one)
        if (scan_blocks(b) < 0 && ((uint64_t)(b->comp_base + (int64_t)b->scan_pos) << 16) < ce)
            return bfail(VAPOR_E_ARG, "vapor_bam_chop: not a BGZF block in " + b->path);
        // the blocks the chunk covers (the read holds a few more behind its end block: those wait until a record needs them)
        size_t own = 0;
        while (own < b->blk_coff.size() && ((uint64_t)b->blk_coff[own] << 16) < ce) ++own;
        if (!take_blocks(b, own)) return bfail(VAPOR_E_ARG, "vapor_bam_chop: inflate failed in " + b->path);
        int64_t pos_u = (int64_t)(cs & 0xFFFF);                              // position in `data`
        size_t blk = 0;
        for (;;) {
            // virtual offset of pos_u
            // virtual offset of pos_u: inside a block that is here, or the start of the block that follows them - decided
            // before anything more is read, so that the end of the chunk does not cost another read and inflate
            uint64_t voff;
            if (pos_u >= (int64_t)b->data.size()) {
                const size_t taken = b->blk_ustart.size();
                if (taken == 0) break;
                voff = (uint64_t)(b->blk_coff[taken - 1] + b->blk_csize[taken - 1]) << 16;
            } else {
                while (blk + 1 < b->blk_ustart.size() && pos_u >= b->blk_ustart[blk + 1]) ++blk;
                voff = ((uint64_t)b->blk_coff[blk] << 16) | (uint64_t)(pos_u - b->blk_ustart[blk]);
            }
            if (voff >= ce) break;
            if (!ensure(b, pos_u + 4)) {
                // the end of the file inside a chunk is the end of its records; bytes that are not BGZF, or a block that
                // does not inflate to its CRC, are an error
                if (!g_bam_damaged) break;
                return bfail(VAPOR_E_ARG, "vapor_bam_chop: damaged BGZF block in " + b->path);
            }
            const int32_t bs = rd32(b->data.data() + pos_u);
            if (bs < 32 || bs > (1 << 29)) return bfail(VAPOR_E_ARG, "vapor_bam_chop: implausible record size in " + b->path);
            if (!ensure(b, pos_u + 4 + bs)) return bfail(VAPOR_E_ARG, "vapor_bam_chop: truncated record (or damaged block) in " + b->path);
            const uint8_t* r = b->data.data() + pos_u + 4;
            pos_u += 4 + bs;
            const int32_t ref_id = rd32(r), pos = rd32(r + 4);
            const int l_name = r[8];
            const int n_cig = r[12] | (r[13] << 8);
            const int32_t l_seq = rd32(r + 16);
            // name, CIGAR, packed bases and qualities must lie inside the record
            if (l_seq < 0 || 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)l_seq + 1) / 2 + (int64_t)l_seq > (int64_t)bs)
                return bfail(VAPOR_E_ARG, "vapor_bam_chop: record fields exceed the record in " + b->path);
            if (ref_id != tid || pos >= stop) {
                if (ref_id > tid || (ref_id == tid && pos >= stop)) break;
                continue;
            }
            // the read filter: a filtered record is as if it were not in the file
            if ((uint32_t)r[9] < b->min_mapq || (((uint32_t)r[14] | ((uint32_t)r[15] << 8)) & b->exclude_flags)) continue;
            const uint8_t* name = r + 32;
            const uint8_t* cig = name + l_name;
            const uint8_t* sq = cig + 4 * n_cig;
            const uint8_t* rec_end = r + bs;
            const uint8_t* ops = cig;
            int32_t n_ops = n_cig;
            if (n_cig == 2) {
                const uint32_t o0 = (uint32_t)rd32(cig), o1 = (uint32_t)rd32(cig + 4);
                if ((o0 & 15u) == 4u && (int32_t)(o0 >> 4) == l_seq && (o1 & 15u) == 3u) {
                    int32_t cnt = 0;
                    const uint8_t* cg = find_cg(sq + (l_seq + 1) / 2 + l_seq, rec_end, &cnt);
                    if (cg) { ops = cg; n_ops = cnt; }
                }
            }
            // reference length; the region-overlap rule of `samtools view`
            // (only as far as the answer: a long read's thousands of operations end far behind the window)
            int64_t rlen = 0;
            for (int32_t t = 0; t < n_ops && (int64_t)pos + rlen <= beg; ++t) {
                const uint32_t o = (uint32_t)rd32(ops + 4 * t), code = o & 15u;
                if (code == 0 || code == 2 || code == 3 || code == 7 || code == 8) rlen += o >> 4;
            }
            if ((int64_t)pos + std::max<int64_t>(rlen, 1) <= beg) continue;
            int64_t q0, miss;
            if (right) {
                // the right-anchored chop (vapor_chop_records_right is the statement): alignments whose last reference base is
                // at or behind the window end, walked from the far end of the CIGAR; q0 = bases dropped from the read's end
                int64_t span = 0;
                for (int32_t t = 0; t < n_ops; ++t) {
                    const uint32_t o = (uint32_t)rd32(ops + 4 * t), code = o & 15u;
                    if (code == 0u || code == 7u || code == 2u) span += o >> 4;
                }
                const int64_t last_ref = (int64_t)pos + span;                     // 1-based
                if (!(last_ref >= end)) continue;
                if (n_ops <= 0) return bfail(VAPOR_E_ARG, "vapor_bam_chop: record without CIGAR (the reference raises IndexError, SF:331)");
                int64_t q = 0, c = last_ref;
                uint32_t last = 0;
                for (int32_t t = n_ops; t-- > 0;) {
                    const uint32_t o = (uint32_t)rd32(ops + 4 * t);
                    const int64_t n = o >> 4;
                    last = o & 15u;
                    if (last == 4u || last == 1u) q += n;
                    else if (last == 0u || last == 7u) { q += n; c -= n; }
                    else if (last == 2u) c -= n;
                    if (c < end + 1) break;
                }
                const int64_t over = end - c;
                if (last == 0u || last == 7u) { q0 = q - over; miss = 0; } else { q0 = q; miss = over; }
            } else {
            // chop_pacbio_read_by_pos: only alignments that start at or before the window start
            if (!((int64_t)pos + 1 < start + 1)) continue;
            if (n_ops <= 0) return bfail(VAPOR_E_ARG, "vapor_bam_chop: record without CIGAR (the reference raises IndexError, SF:331)");
            int64_t q = 0, rr = (int64_t)pos + 1;
            uint32_t last = 0;
            for (int32_t t = 0; t < n_ops; ++t) {
                const uint32_t o = (uint32_t)rd32(ops + 4 * t);
                const int64_t n = o >> 4;
                last = o & 15u;
                if (last == 4u || last == 1u) q += n;
                else if (last == 0u || last == 7u) { q += n; rr += n; }
                else if (last == 2u) rr += n;
                if (rr > start - 1) break;
            }
            const int64_t over = rr - start;
            if (last == 0u || last == 7u) { q0 = q - over; miss = 0; } else { q0 = q; miss = over; }
            }
            if (2 * miss > flank) continue;                                   // miss_bp > flank_length / 2
            const int64_t seq_len = l_seq > 0 ? l_seq : 1;                    // an absent sequence reads "*"
            const int64_t tail = q0 < seq_len ? seq_len - std::max<int64_t>(q0, 0) : 0;
            const int64_t want_len = end - start - miss;
            if (q0 < 0) return bfail(VAPOR_E_ARG, "vapor_bam_chop: negative read offset");
            if (want_len < 0 || !(tail > want_len)) continue;
            const int64_t nl = l_name > 0 ? l_name - 1 : 0;
            if (b->dedup) {
                dd_key.push_back(vapor_names::name_key(name, (int)nl));
                dd_sec.push_back((uint8_t)(((((uint32_t)r[14] | ((uint32_t)r[15] << 8)) & vapor_names::SEC_FLAGS) != 0u) ? 1 : 0));
            }
            if (nr >= max_reads || seq_used + want_len > seq_cap || names_used + nl + 1 > names_cap) {
                overflow = true;
                seq_used += want_len; names_used += nl + 1; ++nr;
                continue;
            }
            uint8_t* dst = seq_out + seq_used;
            if (right && l_seq > 0) {
                // the want_len bases that end before the dropped ones, last base first, complemented ("=ACMGRSVTWYHKDBN" with the
                // nibble's bits reversed)
                static const char* NT16_RC = "=TGKCYSBAWRDMHVN";
                int64_t i = (int64_t)l_seq - q0 - 1;
                for (int64_t t = 0; t < want_len; ++t, --i) {
                    const uint8_t byte = sq[i >> 1];
                    dst[t] = (uint8_t)NT16_RC[(i & 1) ? (byte & 15) : (byte >> 4)];
                }
            } else if (l_seq > 0) {
                int64_t t = 0, i = q0;
                if ((i & 1) && t < want_len) { dst[t++] = (uint8_t)NT16[sq[i >> 1] & 15]; ++i; }
                for (; t + 2 <= want_len; t += 2, i += 2) {              // two bases a byte
                    const uint8_t byte = sq[i >> 1];
                    dst[t] = (uint8_t)NT16[byte >> 4];
                    dst[t + 1] = (uint8_t)NT16[byte & 15];
                }
                if (t < want_len) dst[t] = (uint8_t)NT16[sq[i >> 1] >> 4];
            } else if (want_len > 0) {
                dst[0] = '*';
            }
            memcpy(names_out + names_used, name, (size_t)nl);
            names_out[names_used + nl] = 0;
            int64_t* m = meta + (size_t)meta_w * (size_t)nr;
            m[0] = seq_used; m[1] = want_len; m[2] = miss; m[3] = names_used;
            // (hap and ps: from the phased sites where the caller gave them - the record's own tags are not read then)
            if (meta_w == 6 && sites) haplotag_record(ops, n_ops, (int64_t)pos + 1, sq, l_seq, *sites, m + 4, m + 5);
            else if (meta_w == 6) find_tags(sq + (l_seq + 1) / 2 + l_seq, rec_end, m + 4, m + 5);
            seq_used += want_len; names_used += nl + 1; ++nr;
        }
    }
    if (b->dedup && !overflow && nr > 1) {
        // rule W on the records kept: the survivors move to the front of the three outputs, in record order.
        // (With buffers too small the sizes below are those of all kept records - enough for the call that follows.)
        int64_t s_used = 0, n_used = 0;
        int32_t w = 0;
        for (int32_t i = 0; i < nr; ++i) {
            if (vapor_names::drops(dd_key.data(), dd_sec.data(), nr, i)) continue;
            const int64_t* mi = meta + (size_t)meta_w * (size_t)i;
            const int64_t len = mi[1], nlen = (int64_t)strlen(names_out + mi[3]) + 1;
            memmove(seq_out + s_used, seq_out + mi[0], (size_t)len);
            memmove(names_out + n_used, names_out + mi[3], (size_t)nlen);
            int64_t* mw = meta + (size_t)meta_w * (size_t)w;
            if (w != i) memmove(mw, mi, sizeof(int64_t) * (size_t)meta_w);
            mw[0] = s_used; mw[3] = n_used;
            s_used += len; n_used += nlen; ++w;
        }
        seq_used = s_used; names_used = n_used; nr = w;
    }
    *n_reads = nr;
    if (need) { need[0] = seq_used; need[1] = names_used; need[2] = nr; }
    if (overflow) return bfail(VAPOR_E_OVERFLOW, "vapor_bam_chop: output buffers too small");
    return VAPOR_OK;
}

extern "C" int vapor_bam_chop(vapor_bam* b, int32_t tid, int64_t start, int64_t end, int64_t flank, int32_t n_chunks,
                              const uint64_t* chunks, uint8_t* seq_out, int64_t seq_cap, char* names_out, int64_t names_cap,
                              int64_t* meta, int32_t max_reads, int32_t* n_reads, int64_t* need)
{
    // no exception crosses the C boundary (a std::bad_alloc / length_error from a buffer resize would end the process)
    try {
        return bam_chop_impl(b, tid, start, end, flank, n_chunks, chunks, seq_out, seq_cap, names_out, names_cap, meta, max_reads, n_reads, need);
    } catch (const std::bad_alloc&) {
        return bfail(VAPOR_E_NOMEM, "vapor_bam_chop: out of memory");
    } catch (const std::exception& e) {
        return bfail(VAPOR_E_ARG, std::string("vapor_bam_chop: ") + e.what());
    }
}

// vapor_bam_chop for the right-anchored reads of the window (`--both-ends`): the same outputs, every read the
// reverse complement of its part that ends on the window end, miss_bp counted from there.
extern "C" int vapor_bam_chop_right(vapor_bam* b, int32_t tid, int64_t start, int64_t end, int64_t flank, int32_t n_chunks,
                                    const uint64_t* chunks, uint8_t* seq_out, int64_t seq_cap, char* names_out, int64_t names_cap,
                                    int64_t* meta, int32_t max_reads, int32_t* n_reads, int64_t* need)
{
    try {
        return bam_chop_impl(b, tid, start, end, flank, n_chunks, chunks, seq_out, seq_cap, names_out, names_cap, meta, max_reads, n_reads, need, 4, true);
    } catch (const std::bad_alloc&) {
        return bfail(VAPOR_E_NOMEM, "vapor_bam_chop_right: out of memory");
    } catch (const std::exception& e) {
        return bfail(VAPOR_E_ARG, std::string("vapor_bam_chop_right: ") + e.what());
    }
}

// vapor_bam_chop with six numbers per read in `meta`: the four above, then the record's hap and ps (find_tags).
extern "C" int vapor_bam_chop_tagged(vapor_bam* b, int32_t tid, int64_t start, int64_t end, int64_t flank, int32_t n_chunks,
                                     const uint64_t* chunks, uint8_t* seq_out, int64_t seq_cap, char* names_out, int64_t names_cap,
                                     int64_t* meta, int32_t max_reads, int32_t* n_reads, int64_t* need)
{
    try {
        return bam_chop_impl(b, tid, start, end, flank, n_chunks, chunks, seq_out, seq_cap, names_out, names_cap, meta, max_reads, n_reads, need, 6);
    } catch (const std::bad_alloc&) {
        return bfail(VAPOR_E_NOMEM, "vapor_bam_chop_tagged: out of memory");
    } catch (const std::exception& e) {
        return bfail(VAPOR_E_ARG, std::string("vapor_bam_chop_tagged: ") + e.what());
    }
}

// vapor_bam_chop_tagged with hap and ps made from the phased heterozygous SNVs of the locus instead of the record's HP / PS
// fields, which are not read (`--phase-vcf`; haplotag_record): n_sites sites in position order, none twice.
extern "C" int vapor_bam_chop_haplotag(vapor_bam* b, int32_t tid, int64_t start, int64_t end, int64_t flank, int32_t n_chunks,
                                       const uint64_t* chunks, uint8_t* seq_out, int64_t seq_cap, char* names_out, int64_t names_cap,
                                       int64_t* meta, int32_t max_reads, int32_t* n_reads, int64_t* need, int32_t n_sites,
                                       const int64_t* site_pos, const uint8_t* site_a1, const uint8_t* site_a2, const int64_t* site_ps)
{
    if (n_sites < 0 || (n_sites && (!site_pos || !site_a1 || !site_a2 || !site_ps)))
        return bfail(VAPOR_E_ARG, "vapor_bam_chop_haplotag: bad site arrays");
    for (int32_t i = 1; i < n_sites; ++i)
        if (!(site_pos[i - 1] < site_pos[i])) return bfail(VAPOR_E_ARG, "vapor_bam_chop_haplotag: the sites are not in position order");
    try {
        const HapSites hs{n_sites, site_pos, site_a1, site_a2, site_ps};
        return bam_chop_impl(b, tid, start, end, flank, n_chunks, chunks, seq_out, seq_cap, names_out, names_cap, meta, max_reads, n_reads, need, 6,
                             false, &hs);
    } catch (const std::bad_alloc&) {
        return bfail(VAPOR_E_NOMEM, "vapor_bam_chop_haplotag: out of memory");
    } catch (const std::exception& e) {
        return bfail(VAPOR_E_ARG, std::string("vapor_bam_chop_haplotag: ") + e.what());
    }
}

// an entry of the evidence readers: its body, with what it throws worded under its name
template <typename Body>
static int bam_guarded(const char* who, Body body)
{
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return bfail(VAPOR_E_NOMEM, std::string(who) + ": out of memory");
    } catch (const std::exception& e) {
        return bfail(VAPOR_E_ARG, std::string(who) + ": " + e.what());
    }
}

// The walk of the four evidence readers (`--depth`, `--signatures`, `--links`, `--support`; walk_records in vapor_bamdev.h is the
// device's form): bam_chop_impl's walk over the chunks' records with its checks, the handle's read filter with DEPTH_EXCLUDE
// among its flags, a CG:B,I array in place of its stand-in.  A record at or behind `stop` ends a chunk.  rec(pos, ops, n_ops): a
// passing record of contig `tid`, its operations as the file holds them.
template <typename PerRecord>
static int bam_walk_records(vapor_bam* b, const char* who, int32_t tid, int64_t stop, int32_t n_chunks, const uint64_t* chunks, PerRecord rec)
{
    const uint32_t excl = b->exclude_flags | vapor_bamdev::DEPTH_EXCLUDE;
    for (int32_t c = 0; c < n_chunks; ++c) {
        const uint64_t cs = chunks[2 * c], ce = chunks[2 * c + 1];
        b->comp.clear(); b->data.clear(); b->scan_pos = 0;
        b->blk_coff.clear(); b->blk_cpos.clear(); b->blk_csize.clear(); b->blk_ustart.clear(); b->blk_usize.clear();
        b->comp_base = (int64_t)(cs >> 16);
        if (ce < cs || (ce >> 16) - (cs >> 16) > ((uint64_t)1 << 31))
            return bfail(VAPOR_E_ARG, std::string(who) + ": implausible index chunk for " + b->path);
        const size_t span = (size_t)((int64_t)(ce >> 16) - b->comp_base) + ((ce & 0xFFFFu) ? ((size_t)1 << 16) + 64 : 0);
        if (span == 0 || !read_more(b, span)) continue;
        if (scan_blocks(b) < 0 && ((uint64_t)(b->comp_base + (int64_t)b->scan_pos) << 16) < ce)
            return bfail(VAPOR_E_ARG, std::string(who) + ": not a BGZF block in " + b->path);
        size_t own = 0;
        while (own < b->blk_coff.size() && ((uint64_t)b->blk_coff[own] << 16) < ce) ++own;
        if (!take_blocks(b, own)) return bfail(VAPOR_E_ARG, std::string(who) + ": inflate failed in " + b->path);
        int64_t pos_u = (int64_t)(cs & 0xFFFF);
        size_t blk = 0;
        for (;;) {
            // (the virtual offset of pos_u, as bam_chop_impl decides it)
            uint64_t voff;
            if (pos_u >= (int64_t)b->data.size()) {
                const size_t taken = b->blk_ustart.size();
                if (taken == 0) break;
                voff = (uint64_t)(b->blk_coff[taken - 1] + b->blk_csize[taken - 1]) << 16;
            } else {
                while (blk + 1 < b->blk_ustart.size() && pos_u >= b->blk_ustart[blk + 1]) ++blk;
                voff = ((uint64_t)b->blk_coff[blk] << 16) | (uint64_t)(pos_u - b->blk_ustart[blk]);
            }
            if (voff >= ce) break;
            if (!ensure(b, pos_u + 4)) {
                if (!g_bam_damaged) break;
                return bfail(VAPOR_E_ARG, std::string(who) + ": damaged BGZF block in " + b->path);
            }
            const int32_t bs = rd32(b->data.data() + pos_u);
            if (bs < 32 || bs > (1 << 29)) return bfail(VAPOR_E_ARG, std::string(who) + ": implausible record size in " + b->path);
            if (!ensure(b, pos_u + 4 + bs)) return bfail(VAPOR_E_ARG, std::string(who) + ": truncated record (or damaged block) in " + b->path);
            const uint8_t* r = b->data.data() + pos_u + 4;
            pos_u += 4 + bs;
            const int32_t ref_id = rd32(r), pos = rd32(r + 4);
            const int l_name = r[8];
            const int n_cig = r[12] | (r[13] << 8);
            const int32_t l_seq = rd32(r + 16);
            if (l_seq < 0 || 32 + (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)l_seq + 1) / 2 + (int64_t)l_seq > (int64_t)bs)
                return bfail(VAPOR_E_ARG, std::string(who) + ": record fields exceed the record in " + b->path);
            if (ref_id != tid || (int64_t)pos >= stop) {
                if (ref_id > tid || (ref_id == tid && (int64_t)pos >= stop)) break;
                continue;
            }
            if ((uint32_t)r[9] < b->min_mapq || (((uint32_t)r[14] | ((uint32_t)r[15] << 8)) & excl)) continue;
            const uint8_t* cig = r + 32 + l_name;
            const uint8_t* ops = cig;
            int32_t n_ops = n_cig;
            if (n_cig == 2) {
                const uint32_t o0 = (uint32_t)rd32(cig), o1 = (uint32_t)rd32(cig + 4);
                if ((o0 & 15u) == 4u && (int32_t)(o0 >> 4) == l_seq && (o1 & 15u) == 3u) {
                    int32_t cnt = 0;
                    const uint8_t* cg = find_cg(cig + 8 + (l_seq + 1) / 2 + l_seq, r + bs, &cnt);
                    if (cg) { ops = cg; n_ops = cnt; }
                }
            }
            // (a reader that needs more of the record - its FLAG, its aux fields - takes the record itself as well)
            if constexpr (std::is_invocable_v<PerRecord, int64_t, const uint8_t*, int32_t, const uint8_t*, int32_t>)
                rec((int64_t)pos, ops, n_ops, r, (int32_t)bs);
            else
                rec((int64_t)pos, ops, n_ops);
        }
    }
    return VAPOR_OK;
}

// Read depth of three consecutive intervals [b0, b1) [b1, b2) [b2, b3) of contig `tid`, 0-based half-open (`--depth`, DESIGN.md
// 4.19; vapor_amd/depth.py cover is the rule, bam_depth_kernel the device's form): bam_walk_records, and per passing record the overlap of every M, =
// and X operation with each interval - D and N move the reference cursor and cover nothing, a record without operations covers
// nothing.  A record at or behind b3 ends a chunk.
static int bam_depth_impl(vapor_bam* b, int32_t tid, const int64_t* bounds, int32_t n_chunks, const uint64_t* chunks, uint64_t* cov)
{
    if (!b || !bounds || !cov || n_chunks < 0 || (n_chunks && !chunks)) return bfail(VAPOR_E_ARG, "vapor_bam_depth: null argument");
    const int64_t b0 = bounds[0], b1 = bounds[1], b2 = bounds[2], b3 = bounds[3];
    if (b0 < 0 || b1 < b0 || b2 < b1 || b3 < b2 || b3 >= ((int64_t)1 << 31) || tid < 0)
        return bfail(VAPOR_E_ARG, "vapor_bam_depth: the bounds do not ascend from 0 to a BAM position, or the contig is none");
    cov[0] = cov[1] = cov[2] = 0;
    auto overlap = [](int64_t s, int64_t e, int64_t lo, int64_t hi) -> uint64_t {
        const int64_t a = std::max(s, lo), z = std::min(e, hi);
        return z > a ? (uint64_t)(z - a) : 0u;
    };
    return bam_walk_records(b, "vapor_bam_depth", tid, b3, n_chunks, chunks, [&](int64_t pos, const uint8_t* ops, int32_t n_ops) {
        int64_t cur = pos;
        for (int32_t t = 0; t < n_ops && cur < b3; ++t) {
            const uint32_t o = (uint32_t)rd32(ops + 4 * (size_t)t), code = o & 15u;
            const int64_t n = o >> 4;
            if (code == 0u || code == 7u || code == 8u) {
                cov[0] += overlap(cur, cur + n, b0, b1);
                cov[1] += overlap(cur, cur + n, b1, b2);
                cov[2] += overlap(cur, cur + n, b2, b3);
                cur += n;
            } else if (code == 2u || code == 3u) {
                cur += n;
            }
        }
    });
}

extern "C" int vapor_bam_depth(vapor_bam* b, int32_t tid, const int64_t* bounds, int32_t n_chunks, const uint64_t* chunks, uint64_t* cov)
{
    return bam_guarded("vapor_bam_depth", [&] { return bam_depth_impl(b, tid, bounds, n_chunks, chunks, cov); });
}

// Split-read and CIGAR evidence of one signature region (`--signatures`; vapor_amd/signature.py answer is the
// rule, bam_signature_kernel the device's form): bam_walk_records to w3, and per passing record its events - the leading clip
// from the first two operations, the trailing from the last two, a GAP per D or N and an INSOP per I at the cursor where the
// operation starts - counted at the region's targets, with the two histograms of offsets and their modes.  An empty window has
// no records.
// fields: w0, w3, x0, x1, tol, min_clip, nmin, nmax, mask (vapor_readplan.h SIG_FIELDS); out: six counts, off0, cnt0, off1, cnt1.
static int bam_signature_impl(vapor_bam* b, int32_t tid, const int64_t* fields, int32_t n_chunks, const uint64_t* chunks, int64_t* out)
{
    using namespace vapor_bamdev;
    if (!b || !fields || !out || n_chunks < 0 || (n_chunks && !chunks)) return bfail(VAPOR_E_ARG, "vapor_bam_signature: null argument");
    if (!vapor_readplan::sig_region_ok(tid, fields))
        return bfail(VAPOR_E_ARG, "vapor_bam_signature: the window does not ascend from 0 to a BAM position, the tolerance is not 0..255, "
                                  "the length bounds descend, or the contig is none");
    SigRegion R;
    vapor_readplan::sig_region_set(R, tid, fields, 0);
    const int64_t x[2] = {R.x0, R.x1}, tol = R.tol, width = 2 * tol + 1;
    std::vector<uint32_t> hist((size_t)(2 * width), 0u);
    int64_t cnt[6] = {0, 0, 0, 0, 0, 0};
    auto is_clip = [](uint32_t o) { return (o & 15u) == 4u || (o & 15u) == 5u; };
    const int rc = bam_walk_records(b, "vapor_bam_signature", tid, R.w3, R.w3 > R.w0 ? n_chunks : 0, chunks, [&](int64_t pos, const uint8_t* ops, int32_t n_ops) {
        if (n_ops <= 0) return;
        auto op = [&](int32_t t) { return (uint32_t)rd32(ops + 4 * (size_t)t); };
        const uint32_t o0 = op(0), o1 = n_ops >= 2 ? op(1) : 15u, ol = op(n_ops - 1), op2 = n_ops >= 2 ? op(n_ops - 2) : 15u;
        if (is_clip(o0) && (n_ops == 1 || (n_ops == 2 && is_clip(o1)))) return;     // all clips: neither event
        const int64_t lead = is_clip(o0) ? (int64_t)(o0 >> 4) + (is_clip(o1) ? (int64_t)(o1 >> 4) : 0) : 0;
        const int64_t trail = is_clip(ol) ? (int64_t)(ol >> 4) + (is_clip(op2) ? (int64_t)(op2 >> 4) : 0) : 0;
        int64_t cur = pos;
        for (int32_t t = 0; t < n_ops; ++t) {
            const uint32_t o = op(t), code = o & 15u;
            const int64_t n = o >> 4;
            if ((code == 2u || code == 3u) && (R.mask & SIG_GAP) && n >= R.nmin && n <= R.nmax) {
                const int64_t d0 = cur - x[0], d1 = cur + n - x[1];
                if (d0 >= -tol && d0 <= tol && d1 >= -tol && d1 <= tol) {
                    ++cnt[4];
                    ++hist[(size_t)(d0 + tol)];
                    ++hist[(size_t)(width + d1 + tol)];
                }
            }
            if (code == 1u && (R.mask & SIG_INSOP) && n >= R.nmin && n <= R.nmax && cur >= x[0] - tol && cur <= x[1] + tol) {
                ++cnt[5];
                if (cur - x[0] >= -tol && cur - x[0] <= tol) ++hist[(size_t)(cur - x[0] + tol)];
            }
            if (code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) cur += n;
        }
        for (int k = 0; k < 4; ++k) {
            if (!((R.mask >> k) & 1u)) continue;
            const int64_t have = (k & 1) ? trail : lead, d = ((k & 1) ? cur : pos) - x[k >> 1];
            if (have >= R.min_clip && d >= -tol && d <= tol) {
                ++cnt[k];
                ++hist[(size_t)((k >> 1) * width + d + tol)];
            }
        }
    });
    for (int k = 0; k < 10; ++k) out[k] = 0;
    if (rc != VAPOR_OK) return rc;
    for (int k = 0; k < 6; ++k) out[k] = cnt[k];
    for (int h = 0; h < 2; ++h) {
        // the mode: the largest count, then the smallest |offset|, then the negative offset
        int64_t best_off = 0, best = 0;
        for (int64_t off = -tol; off <= tol; ++off) {
            const int64_t c = hist[(size_t)(h * width + off + tol)];
            const int64_t a = off < 0 ? -off : off, ba = best_off < 0 ? -best_off : best_off;
            if (c > best || (c == best && c > 0 && (a < ba || (a == ba && off < best_off)))) { best = c; best_off = off; }
        }
        out[6 + 2 * h] = best ? best_off : 0;
        out[7 + 2 * h] = best;
    }
    return VAPOR_OK;
}

extern "C" int vapor_bam_signature(vapor_bam* b, int32_t tid, const int64_t* fields, int32_t n_chunks, const uint64_t* chunks, int64_t* out)
{
    return bam_guarded("vapor_bam_signature", [&] { return bam_signature_impl(b, tid, fields, n_chunks, chunks, out); });
}

// Alt and ref alignments of one support region (`--support`; vapor_amd/support.py answer is the rule,
// bam_support_kernel the device's form): bam_walk_records to w3, and per passing record - not per event - whether it carries a
// GAP or INSOP that 4.20 counts, whether a clip of it counts at either target, whether it reaches `flank` bases to either side
// of a target with no D, N or I of gmin bases in between, and whether it covers the target's base.  An empty window has no
// records.
// fields: the nine of bam_signature_impl, then flank and gmin (vapor_readplan.h SUP_FIELDS); out: alt_cg, alt_l, alt_r, ref_0,
// ref_1, cov_0, cov_1.
static int bam_support_impl(vapor_bam* b, int32_t tid, const int64_t* fields, int32_t n_chunks, const uint64_t* chunks, int64_t* out)
{
    using namespace vapor_bamdev;
    if (!b || !fields || !out || n_chunks < 0 || (n_chunks && !chunks)) return bfail(VAPOR_E_ARG, "vapor_bam_support: null argument");
    if (!vapor_readplan::sup_region_ok(tid, fields))
        return bfail(VAPOR_E_ARG, "vapor_bam_support: the window does not ascend from 0 to a BAM position, the tolerance is not 0..255, "
                                  "the length bounds descend, the flank is not 1..65535, the blocking length is below 1, or the contig is none");
    SupRegion R;
    vapor_readplan::sup_region_set(R, tid, fields, 0);
    const int64_t x[2] = {R.x0, R.x1}, tol = R.tol, F = R.flank, gmin = R.gmin;
    int64_t cnt[SUP_ANSWER_WORDS] = {0, 0, 0, 0, 0, 0, 0};
    auto is_clip = [](uint32_t o) { return (o & 15u) == 4u || (o & 15u) == 5u; };
    const int rc = bam_walk_records(b, "vapor_bam_support", tid, R.w3, R.w3 > R.w0 ? n_chunks : 0, chunks, [&](int64_t pos, const uint8_t* ops, int32_t n_ops) {
        if (n_ops <= 0) return;
        auto op = [&](int32_t t) { return (uint32_t)rd32(ops + 4 * (size_t)t); };
        const uint32_t o0 = op(0), o1 = n_ops >= 2 ? op(1) : 15u, ol = op(n_ops - 1), op2 = n_ops >= 2 ? op(n_ops - 2) : 15u;
        if (is_clip(o0) && (n_ops == 1 || (n_ops == 2 && is_clip(o1)))) return;     // all clips: no event, no base covered
        const int64_t lead = is_clip(o0) ? (int64_t)(o0 >> 4) + (is_clip(o1) ? (int64_t)(o1 >> 4) : 0) : 0;
        const int64_t trail = is_clip(ol) ? (int64_t)(ol >> 4) + (is_clip(op2) ? (int64_t)(op2 >> 4) : 0) : 0;
        bool cg = false, blocked[2] = {false, false};
        int64_t cur = pos;
        for (int32_t t = 0; t < n_ops; ++t) {
            const uint32_t o = op(t), code = o & 15u;
            const int64_t n = o >> 4;
            const bool gap = code == 2u || code == 3u, ins = code == 1u;
            if (gap && (R.mask & SIG_GAP) && n >= R.nmin && n <= R.nmax) {
                const int64_t d0 = cur - x[0], d1 = cur + n - x[1];
                if (d0 >= -tol && d0 <= tol && d1 >= -tol && d1 <= tol) cg = true;
            }
            if (ins && (R.mask & SIG_INSOP) && n >= R.nmin && n <= R.nmax && cur >= x[0] - tol && cur <= x[1] + tol) cg = true;
            if (n >= gmin)
                for (int k = 0; k < 2; ++k)
                    if ((gap && cur < x[k] + F && cur + n > x[k] - F) || (ins && cur >= x[k] - F && cur <= x[k] + F)) blocked[k] = true;
            if (code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) cur += n;
        }
        const int64_t q = cur;
        cnt[0] += cg;
        for (int k = 0; k < 2; ++k) {
            const int64_t dp = pos - x[k], dq = q - x[k];
            const bool clip = (((R.mask >> (2 * k)) & 1u) && lead >= R.min_clip && dp >= -tol && dp <= tol) ||
                              (((R.mask >> (2 * k + 1)) & 1u) && trail >= R.min_clip && dq >= -tol && dq <= tol);
            const bool span = pos <= x[k] - F && q >= x[k] + F && !blocked[k];
            cnt[1 + k] += clip && !cg;
            cnt[3 + k] += (R.mask & (k ? SUP_REF1 : SUP_REF0)) && span && !cg && !clip;
            cnt[5 + k] += pos <= x[k] && x[k] < q;
        }
    });
    for (int k = 0; k < SUP_ANSWER_WORDS; ++k) out[k] = 0;
    if (rc != VAPOR_OK) return rc;
    for (int k = 0; k < SUP_ANSWER_WORDS; ++k) out[k] = cnt[k];
    return VAPOR_OK;
}

extern "C" int vapor_bam_support(vapor_bam* b, int32_t tid, const int64_t* fields, int32_t n_chunks, const uint64_t* chunks, int64_t* out)
{
    return bam_guarded("vapor_bam_support", [&] { return bam_support_impl(b, tid, fields, n_chunks, chunks, out); });
}

// Split reads joined through their SA tags, one link region (`--links`; vapor_amd/links.py answer is the rule,
// bam_link_kernel the device's form): bam_walk_records to w3, and per passing record the clip event the region asks for - read as
// bam_signature_impl reads it - within tol of x; of such a clip record the entries of its SA value (vapor_sa.h), an entry below
// the handle's minimum MAPQ ignored; the first entry in text order that names the partner, holds the strand relation and lies
// within tol of y gives the record's offset.  A malformed aux area: what stood before the damage stands - the record has no
// entries.  An empty window has no records.
// fields: w0, w3, x, y, tol, min_clip, ev, pend, rel, name_off, name_len (vapor_readplan.h LINK_FIELDS); out: n_clip, n_split,
// n_link, the mode's offset and count.
static int bam_links_impl(vapor_bam* b, int32_t tid, const int64_t* fields, const uint8_t* names, int64_t names_len, int32_t n_chunks,
                          const uint64_t* chunks, int64_t* out)
{
    using namespace vapor_bamdev;
    if (!b || !fields || !out || names_len < 0 || (names_len && !names) || n_chunks < 0 || (n_chunks && !chunks))
        return bfail(VAPOR_E_ARG, "vapor_bam_links: null argument");
    if (!vapor_readplan::link_region_ok(tid, fields, names_len))
        return bfail(VAPOR_E_ARG, "vapor_bam_links: the window does not ascend from 0 to a BAM position, the tolerance is not 0..255, "
                                  "ev, pend or rel is not 0 or 1, the partner's name is empty or outside the names, or the contig is none");
    LinkRegion R;
    vapor_readplan::link_region_set(R, tid, fields, 0);
    const int64_t tol = R.tol, width = 2 * tol + 1;
    const bool want_r = R.bits & LINK_EV, use_b = R.bits & LINK_PEND, differ = R.bits & LINK_REL;
    const uint8_t* pname = names + R.name_off;
    std::vector<uint32_t> hist((size_t)width, 0u);
    int64_t n_clip = 0, n_split = 0, n_link = 0;
    auto is_clip = [](uint32_t o) { return (o & 15u) == 4u || (o & 15u) == 5u; };
    const int rc = bam_walk_records(b, "vapor_bam_links", tid, R.w3, R.w3 > R.w0 ? n_chunks : 0, chunks,
                                    [&](int64_t pos, const uint8_t* ops, int32_t n_ops, const uint8_t* r, int32_t bs) {
        if (n_ops <= 0) return;
        auto op = [&](int32_t t) { return (uint32_t)rd32(ops + 4 * (size_t)t); };
        const uint32_t o0 = op(0), o1 = n_ops >= 2 ? op(1) : 15u, ol = op(n_ops - 1), op2 = n_ops >= 2 ? op(n_ops - 2) : 15u;
        if (is_clip(o0) && (n_ops == 1 || (n_ops == 2 && is_clip(o1)))) return;     // all clips: neither event
        int64_t have, at;
        if (!want_r) {
            have = is_clip(o0) ? (int64_t)(o0 >> 4) + (is_clip(o1) ? (int64_t)(o1 >> 4) : 0) : 0;
            at = pos;
        } else {
            have = is_clip(ol) ? (int64_t)(ol >> 4) + (is_clip(op2) ? (int64_t)(op2 >> 4) : 0) : 0;
            at = pos;
            for (int32_t t = 0; t < n_ops; ++t) {
                const uint32_t o = op(t), code = o & 15u;
                if (code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) at += (int64_t)(o >> 4);
            }
        }
        const int64_t d = at - R.x;
        if (have < R.min_clip || d < -tol || d > tol) return;
        ++n_clip;
        const int l_name = r[8], n_cig = r[12] | (r[13] << 8);
        const int32_t l_seq = rd32(r + 16);
        const bool minus = (r[14] & 0x10u) != 0;
        const uint8_t* value = nullptr;
        size_t len = 0;
        if (vapor_sa::find_sa(r + 32 + l_name + 4 * (size_t)n_cig + ((size_t)l_seq + 1) / 2 + (size_t)l_seq, r + bs, &value, &len) != vapor_sa::FIND_VALUE) return;
        bool any = false, linked = false;
        int64_t off = 0;
        vapor_sa::for_each_piece(value, len, [&](bool ok, const vapor_sa::Entry& e) {
            if (!ok || e.mapq < b->min_mapq) return false;
            any = true;
            const int64_t dy = (use_b ? e.b : e.a) - R.y;
            if (e.name_len == R.name_len && !memcmp(e.name, pname, e.name_len) && ((e.minus != minus) == differ) && dy >= -tol && dy <= tol) {
                linked = true;
                off = dy;
                return true;
            }
            return false;
        });
        if (any) ++n_split;
        if (linked) {
            ++n_link;
            ++hist[(size_t)(off + tol)];
        }
    });
    for (int k = 0; k < LINK_ANSWER_WORDS; ++k) out[k] = 0;
    if (rc != VAPOR_OK) return rc;
    out[0] = n_clip; out[1] = n_split; out[2] = n_link;
    // the mode: the largest count, then the smallest |offset|, then the negative offset
    int64_t best_off = 0, best = 0;
    for (int64_t off = -tol; off <= tol; ++off) {
        const int64_t c = hist[(size_t)(off + tol)];
        const int64_t a = off < 0 ? -off : off, ba = best_off < 0 ? -best_off : best_off;
        if (c > best || (c == best && c > 0 && (a < ba || (a == ba && off < best_off)))) { best = c; best_off = off; }
    }
    out[3] = best ? best_off : 0;
    out[4] = best;
    return VAPOR_OK;
}

extern "C" int vapor_bam_links(vapor_bam* b, int32_t tid, const int64_t* fields, const uint8_t* names, int64_t names_len, int32_t n_chunks,
                               const uint64_t* chunks, int64_t* out)
{
    return bam_guarded("vapor_bam_links", [&] { return bam_links_impl(b, tid, fields, names, names_len, n_chunks, chunks, out); });
}

// chop_pacbio_read_by_pos (SF:339-354) over alignment records that are in memory already (a caller that holds its reads as
// objects - the synthetic worlds of the tests and benches, a reader of another format): the region rule of `samtools view`,
// the reference's `POS < start + 1`, the CIGAR walk to the window start (cigar2alignstart_by_pos, SF:309-337, over the CIGAR
// TEXT, as vapor_cigar2alignstart walks it: the walk ends where the reference cursor passes the window start, a few dozen
// operations into a long read's thousands, so nothing is parsed ahead of time), `miss_bp > flank / 2` and
// `len(read[q0:]) > end - start - miss_bp`, for n records in one call.  keep[r] = 1 and q0_miss[2r], q0_miss[2r+1] = offset
// into the read and miss_bp for the reads the reference keeps.  VAPOR_E_ARG for a record without CIGAR operation that
// reaches the walk (IndexError in the reference, SF:331).
extern "C" int vapor_chop_records(int32_t n, const int64_t* pos, const int64_t* ref_span, const char* const* cigar,
                                  const int64_t* seq_len, int64_t start, int64_t end, int64_t flank,
                                  int64_t* q0_miss, uint8_t* keep)
{
    if (n < 0 || (n && (!pos || !ref_span || !cigar || !seq_len || !q0_miss || !keep)))
        return bfail(VAPOR_E_ARG, "vapor_chop_records: null argument");
    for (int32_t r = 0; r < n; ++r) {
        keep[r] = 0;
        if (!(pos[r] <= end && pos[r] + ref_span[r] - 1 >= start)) continue;      // not in the region
        if (!(pos[r] < start + 1)) continue;
        int64_t q = 0, rr = pos[r], num = 0;
        bool have_n = false;
        char last = 0;
        for (const char* c = cigar[r] ? cigar[r] : ""; *c; ++c) {
            const char ch = *c;
            if (ch >= '0' && ch <= '9') { num = num * 10 + (ch - '0'); have_n = true; continue; }
            const bool op = ch == 'M' || ch == 'I' || ch == 'D' || ch == 'N' || ch == 'S' || ch == 'H' || ch == 'P' || ch == '=' || ch == 'X';
            if (op && have_n) {
                if (ch == 'S' || ch == 'I') q += num;
                else if (ch == 'M' || ch == '=') { q += num; rr += num; }
                else if (ch == 'D') rr += num;
                last = ch;
                if (rr > start - 1) break;
            }
            num = 0; have_n = false;           // any other character ends the number, as the regular expression would
        }
        if (!last) return bfail(VAPOR_E_ARG, "vapor_chop_records: record without CIGAR (the reference raises IndexError, SF:331)");
        const int64_t over = rr - start;
        int64_t q0, miss;
        if (last == 'M' || last == '=') { q0 = q - over; miss = 0; } else { q0 = q; miss = over; }
        if (2 * miss > flank) continue;                                    // miss_bp > flank_length / 2
        const int64_t want = end - start - miss;
        // len(seq[q0:]) as Python slices (a negative q0 counts from the end)
        const int64_t from = q0 < 0 ? std::max<int64_t>(seq_len[r] + q0, 0) : std::min(q0, seq_len[r]);
        if (!(seq_len[r] - from > want)) continue;
        keep[r] = 1;
        q0_miss[2 * r] = q0;
        q0_miss[2 * r + 1] = miss;
    }
    return VAPOR_OK;
}

// The right-anchored chop (`--both-ends`; not in the reference): vapor_chop_records of the records as the
// reverse-complemented contig holds them, in closed form.  An alignment qualifies when its last reference base (pos + the M, =
// and D operations - 1) is >= end; the walk goes from the far end of the CIGAR, the cursor moving left from that base, to the
// first operation after which it is <= end.  q1_miss[2r] = read bases to drop from the END of the read, q1_miss[2r + 1] = miss_bp
// counted from the window end; the kept read is the reverse complement of the end - start - miss_bp bases before the dropped
// ones.  A window shorter than its miss_bp keeps nothing here (callers leave such a window to the Python statement).
extern "C" int vapor_chop_records_right(int32_t n, const int64_t* pos, const int64_t* ref_span, const char* const* cigar,
                                        const int64_t* seq_len, int64_t start, int64_t end, int64_t flank,
                                        int64_t* q1_miss, uint8_t* keep)
{
    if (n < 0 || (n && (!pos || !ref_span || !cigar || !seq_len || !q1_miss || !keep)))
        return bfail(VAPOR_E_ARG, "vapor_chop_records_right: null argument");
    try {
        std::vector<std::pair<int64_t, char>> ops;
        for (int32_t r = 0; r < n; ++r) {
            keep[r] = 0;
            if (!(pos[r] <= end && pos[r] + ref_span[r] - 1 >= start)) continue;      // not in the region
            ops.clear();
            int64_t num = 0, span = 0;
            bool have_n = false;
            for (const char* c = cigar[r] ? cigar[r] : ""; *c; ++c) {
                const char ch = *c;
                if (ch >= '0' && ch <= '9') { num = num * 10 + (ch - '0'); have_n = true; continue; }
                const bool op = ch == 'M' || ch == 'I' || ch == 'D' || ch == 'N' || ch == 'S' || ch == 'H' || ch == 'P' || ch == '=' || ch == 'X';
                if (op && have_n) {
                    ops.emplace_back(num, ch);
                    if (ch == 'M' || ch == '=' || ch == 'D') span += num;
                }
                num = 0; have_n = false;
            }
            const int64_t last_ref = pos[r] + span - 1;
            if (!(last_ref >= end)) continue;
            if (ops.empty()) return bfail(VAPOR_E_ARG, "vapor_chop_records_right: record without CIGAR (the reference raises IndexError, SF:331)");
            int64_t q = 0, c = last_ref;
            char last = 0;
            for (size_t t = ops.size(); t-- > 0;) {
                const int64_t m = ops[t].first;
                last = ops[t].second;
                if (last == 'S' || last == 'I') q += m;
                else if (last == 'M' || last == '=') { q += m; c -= m; }
                else if (last == 'D') c -= m;
                if (c < end + 1) break;
            }
            const int64_t over = end - c;
            int64_t q1, miss;
            if (last == 'M' || last == '=') { q1 = q - over; miss = 0; } else { q1 = q; miss = over; }
            if (2 * miss > flank) continue;
            const int64_t want = end - start - miss;
            const int64_t head = std::max<int64_t>(seq_len[r] - q1, 0);
            if (want < 0 || q1 < 0 || !(head > want)) continue;
            keep[r] = 1;
            q1_miss[2 * r] = q1;
            q1_miss[2 * r + 1] = miss;
        }
    } catch (const std::bad_alloc&) {
        return bfail(VAPOR_E_NOMEM, "vapor_chop_records_right: out of memory");
    }
    return VAPOR_OK;
}

// chop_pacbio_read_by_pos (SF:339-354) and minimize_pacbio_read_list (SF:1091-1102: at most `max_keep` reads, smallest miss_bp
// first, input order inside one miss_bp value) for MANY regions in one call: region g looks at n_rec[g] records given as the
// arrays of vapor_chop_records (one pointer per region), keeps what that call keeps and, when there are more than max_keep,
// the first max_keep of them in a stable order by miss_bp.  kept_first[g] .. kept_first[g + 1] index rec_idx / q0 / miss
// (capacity max_keep per region); addr_out (may be NULL) receives seq_addr[g][record] for every kept read - where the caller
// keeps the records' sequences.  status[g] = 0, or VAPOR_E_ARG where a record without CIGAR reaches the walk (the reference
// raises IndexError there, SF:331: the caller lets that region take the reference-named route).
typedef int (*chop_records_fn)(int32_t, const int64_t*, const int64_t*, const char* const*, const int64_t*, int64_t, int64_t, int64_t,
                               int64_t*, uint8_t*);
static int chop_records_many_impl(chop_records_fn chop_one, int32_t n_regions, const int32_t* n_rec, const int64_t* const* pos,
                                  const int64_t* const* ref_span, const char* const* const* cigar,
                                  const int64_t* const* seq_len, const int64_t* start, const int64_t* end,
                                  const int64_t* flank, int32_t max_keep, int32_t* kept_first, int32_t* rec_idx,
                                  int64_t* q0, int64_t* miss, int32_t* status, const uint64_t* const* seq_addr,
                                  uint64_t* addr_out)
{
    if (n_regions < 0 || max_keep < 1 || (n_regions && (!n_rec || !pos || !ref_span || !cigar || !seq_len || !start || !end || !flank ||
                                                           !kept_first || !rec_idx || !q0 || !miss || !status)))
        return bfail(VAPOR_E_ARG, "vapor_chop_records_many: null argument");
    // every region into slots of its own (max_keep of them), on a few threads when there are many regions; then packed
    std::vector<int32_t> cnt((size_t)n_regions, 0), t_rec((size_t)n_regions * max_keep);
    std::vector<int64_t> t_q0((size_t)n_regions * max_keep), t_miss((size_t)n_regions * max_keep);
    auto work = [&](int32_t g0, int32_t g1) {
        std::vector<int64_t> qm;
        std::vector<uint8_t> keep;
        std::vector<int32_t> order;
        for (int32_t g = g0; g < g1; ++g) {
            status[g] = 0;
            const int32_t n = n_rec[g];
            if (n <= 0) continue;
            qm.resize((size_t)2 * n);
            keep.resize((size_t)n);
            if (chop_one(n, pos[g], ref_span[g], cigar[g], seq_len[g], start[g], end[g], flank[g], qm.data(), keep.data()) != VAPOR_OK) {
                status[g] = VAPOR_E_ARG;
                continue;
            }
            order.clear();
            for (int32_t r = 0; r < n; ++r)
                if (keep[(size_t)r]) order.push_back(r);
            vapor_readplan::keep_smallest_miss(order, max_keep, [&](int32_t r) { return qm[(size_t)2 * r + 1]; });
            int32_t c = 0;
            for (int32_t r : order) {
                const size_t o = (size_t)g * max_keep + (size_t)c++;
                t_rec[o] = r; t_q0[o] = qm[(size_t)2 * r]; t_miss[o] = qm[(size_t)2 * r + 1];
            }
            cnt[(size_t)g] = c;
        }
    };
    const int n_thr = n_regions >= 512 ? 4 : 1;
    if (n_thr == 1) {
        work(0, n_regions);
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < n_thr; ++t)
            th.emplace_back(work, (int32_t)((int64_t)n_regions * t / n_thr), (int32_t)((int64_t)n_regions * (t + 1) / n_thr));
        for (auto& x : th) x.join();
    }
    int32_t w = 0;
    for (int32_t g = 0; g < n_regions; ++g) {
        kept_first[g] = w;
        for (int32_t c = 0; c < cnt[(size_t)g]; ++c) {
            const size_t o = (size_t)g * max_keep + (size_t)c;
            rec_idx[w] = t_rec[o]; q0[w] = t_q0[o]; miss[w] = t_miss[o];
            if (addr_out) addr_out[w] = (seq_addr && seq_addr[g]) ? seq_addr[g][t_rec[o]] : 0;
            ++w;
        }
    }
    kept_first[n_regions] = w;
    return VAPOR_OK;
}

extern "C" int vapor_chop_records_many(int32_t n_regions, const int32_t* n_rec, const int64_t* const* pos,
                                       const int64_t* const* ref_span, const char* const* const* cigar,
                                       const int64_t* const* seq_len, const int64_t* start, const int64_t* end,
                                       const int64_t* flank, int32_t max_keep, int32_t* kept_first, int32_t* rec_idx,
                                       int64_t* q0, int64_t* miss, int32_t* status, const uint64_t* const* seq_addr,
                                       uint64_t* addr_out)
{
    return chop_records_many_impl(vapor_chop_records, n_regions, n_rec, pos, ref_span, cigar, seq_len, start, end, flank, max_keep, kept_first,
                                  rec_idx, q0, miss, status, seq_addr, addr_out);
}

// vapor_chop_records_many over the right-anchored chop (vapor_chop_records_right): q1[] = bases to drop from the read's end.
extern "C" int vapor_chop_records_right_many(int32_t n_regions, const int32_t* n_rec, const int64_t* const* pos,
                                             const int64_t* const* ref_span, const char* const* const* cigar,
                                             const int64_t* const* seq_len, const int64_t* start, const int64_t* end,
                                             const int64_t* flank, int32_t max_keep, int32_t* kept_first, int32_t* rec_idx,
                                             int64_t* q1, int64_t* miss, int32_t* status, const uint64_t* const* seq_addr,
                                             uint64_t* addr_out)
{
    return chop_records_many_impl(vapor_chop_records_right, n_regions, n_rec, pos, ref_span, cigar, seq_len, start, end, flank, max_keep,
                                  kept_first, rec_idx, q1, miss, status, seq_addr, addr_out);
}

// The row tails of a whole table in one call (no device): what result_organize_ins (SF:1219-1231) and
// gt_estimate_log_likelihood (SF:2054-2069) compute per locus from its read scores, minus the parts that are table lookups on
// the caller's side.  Per locus t with scores[off[t] .. off[t+1]):
//   n_pos[t]    = scores > 0 (GS = n_pos / n);  qs[t] = np.mean of those, summed as numpy's add.reduce sums a contiguous
//                 double array (pairwise: blocks of at most 128 with eight strided partial sums, SF:1225's np.mean)
//   n_nonpos[t] = scores that are not > 0 AFTER round(s, 2) - the l of log_likelihood_calcu (SF:2071-2077), which the
//                 reference reads back from the Rec string
//   rec         = ','.join(str(round(s, 2))): text[text_off[t] .. text_off[t+1]).  str(round(s, 2)) of a float is the
//                 correctly rounded two-decimal numeral without trailing zeros but with one decimal at least ("0.5", "-1.0",
//                 "-0.0"): round() rounds the exact binary value half-even through the shortest-string machinery, and below
//                 2^46 two doubles are less than 0.005 apart so no shorter numeral reads back as the same double.
//                 n_nonpos[t] = -1 instead where a score is not finite or is 1e13 and more in size: the caller formats that
//                 locus itself.
// VAPOR_E_OVERFLOW with text_off[n_loci] = bytes needed when text_cap is too small (16 bytes a score are always enough for
// |s| < 1e13).
namespace {
double pairwise_sum(const double* a, int64_t n)
{
    if (n < 8) {
        double r = 0.;          // (numpy starts from -0.0; adding it to the first value gives the same double except for an
        for (int64_t i = 0; i < n; ++i) r += a[i];     //  all-negative-zero list, which cannot be: these values are > 0)
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] += a[i + k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum(a, n2) + pairwise_sum(a + n2, n - n2);
}

// the numeral of round(x, 2) as Python prints it; returns its length, sets *positive to (rounded value > 0)
int two_decimals(double x, char* out, bool* positive)
{
    const double y = x * 100.;
    const double fl = std::floor(y);
    double cents;               // round(x, 2) * 100 as an integer-valued double (sign kept apart for -0.0)
    // x * 100 carries a relative error below 2^-53: away from a tie by more than that, the side it falls on is the exact one
    if (std::fabs((y - fl) - .5) > 1e-9 * (std::fabs(y) + 1.)) {
        cents = std::nearbyint(y);
    } else {
        char buf[40];
        std::snprintf(buf, sizeof buf, "%.2f", x);       // exact, half-even on the binary value
        cents = std::nearbyint(std::strtod(buf, nullptr) * 100.);
    }
    const bool neg = std::signbit(x);
    uint64_t c = (uint64_t)std::fabs(cents);
    *positive = !neg && c > 0;
    char tmp[32];
    int m = 0;
    const unsigned frac = (unsigned)(c % 100);
    c /= 100;
    do { tmp[m++] = (char)('0' + c % 10); c /= 10; } while (c);
    int len = 0;
    if (neg) out[len++] = '-';
    while (m) out[len++] = tmp[--m];
    out[len++] = '.';
    out[len++] = (char)('0' + frac / 10);
    if (frac % 10) out[len++] = (char)('0' + frac % 10);
    return len;
}
}   // namespace

extern "C" int vapor_row_tails(int32_t n_loci, const int64_t* off, const double* scores, double* qs, int32_t* n_pos,
                               int32_t* n_nonpos, char* text, int64_t text_cap, int64_t* text_off)
{
    if (n_loci < 0 || !off || !text_off || (n_loci && (!qs || !n_pos || !n_nonpos)) || text_cap < 0 || (text_cap && !text))
        return bfail(VAPOR_E_ARG, "vapor_row_tails: null argument");
    for (int32_t t = 0; t < n_loci; ++t)
        if (off[t + 1] < off[t] || off[t] < 0) return bfail(VAPOR_E_ARG, "vapor_row_tails: offsets must not decrease");
    if (n_loci && off[n_loci] > 0 && !scores) return bfail(VAPOR_E_ARG, "vapor_row_tails: null scores");
    try {
        std::vector<double> pos;
        int64_t w = 0;
        bool fits = true;
        for (int32_t t = 0; t < n_loci; ++t) {
            const double* s = scores + off[t];
            const int64_t n = off[t + 1] - off[t];
            text_off[t] = w;
            pos.clear();
            int32_t nonpos = 0;
            bool plain = true;
            for (int64_t i = 0; i < n; ++i) {
                if (s[i] > 0) pos.push_back(s[i]);
                if (!(std::fabs(s[i]) < 1e13)) { plain = false; continue; }      // (also NaN)
                char num[40];
                bool positive;
                const int len = two_decimals(s[i], num, &positive);
                nonpos += !positive;
                if (fits && w + len + 1 <= text_cap) {
                    if (i) text[w++] = ',';
                    std::memcpy(text + w, num, (size_t)len);
                    w += len;
                } else {
                    fits = false;
                    w += len + (i ? 1 : 0);
                }
            }
            n_pos[t] = (int32_t)pos.size();
            qs[t] = pos.empty() ? 0. : pairwise_sum(pos.data(), (int64_t)pos.size()) / (double)pos.size();
            n_nonpos[t] = plain ? nonpos : -1;
        }
        text_off[n_loci] = w;
        return fits ? VAPOR_OK : bfail(VAPOR_E_OVERFLOW, "vapor_row_tails: text buffer too small");
    } catch (const std::bad_alloc&) {
        return bfail(VAPOR_E_NOMEM, "vapor_row_tails: out of memory");
    }
}

// The wide route (vapor_wide_batch, vapor_clean_hits_wide) is device code in vapor_hip.hip, whose definitions take precedence
// over these weak ones in the library.  A build of this file without it - the CPU twin of the C ABI (oracle/, test
// infrastructure), which has no wide route - answers every call with VAPOR_E_ARG, so that it still exports the whole header.
extern "C" __attribute__((weak)) int vapor_wide_batch(vapor_ctx*, vapor_seqset*, int64_t, const vapor_pair*, int64_t*, int32_t*,
                                                      int64_t, int64_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_wide_batch: this build has no wide route");
}

extern "C" __attribute__((weak)) int vapor_clean_hits_wide(vapor_ctx*, int64_t, const int32_t*, const int64_t*, const uint32_t*,
                                                           int64_t*, uint8_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_clean_hits_wide: this build has no wide route");
}

// The any-k route (vapor_anyk_batch) is device code in vapor_hip.hip too; the CPU twin refuses it the same way.
extern "C" __attribute__((weak)) int vapor_anyk_batch(vapor_ctx*, vapor_seqset*, int64_t, const vapor_pair*, int64_t*, int32_t*,
                                                      int64_t, int64_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_anyk_batch: this build has no any-k route");
}

// `--realign`'s distances (vapor_realign_batch: realign_kernel) are device code in vapor_hip.hip as well and have no host route;
// the CPU twin exports the name and refuses every call, and Engine.realign does not call it there.
extern "C" __attribute__((weak)) int vapor_realign_batch(vapor_ctx*, vapor_seqset*, int64_t, const vapor_pair*, int32_t, int32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_realign_batch: this build has no realignment kernel");
}

// ... and so are `--realign-out`'s traces (vapor_realign_trace: realign_trace_kernel and traceback_kernel).
extern "C" __attribute__((weak)) int vapor_realign_trace(vapor_ctx*, vapor_seqset*, int64_t, const vapor_pair*, int32_t, int32_t, int32_t*,
                                                         uint32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_realign_trace: this build has no traceback kernel");
}

// ... and `--realign-polish`'s consensus (vapor_realign_polish: the four kernels of vapor_polish.h behind those two).
extern "C" __attribute__((weak)) int vapor_realign_polish(vapor_ctx*, vapor_seqset*, int64_t, const vapor_pair*, int32_t, int64_t, const int64_t*,
                                                          const int64_t*, int32_t*, uint8_t*, int32_t*, uint8_t*, uint32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_realign_polish: this build has no pileup kernels");
}

// ... and `--realign-revote`'s second vote on the polished allele (vapor_realign_revote: the three kernels of vapor_revote.h behind
// the polish's).
extern "C" __attribute__((weak)) int vapor_realign_revote(vapor_ctx*, vapor_seqset*, int64_t, const vapor_pair*, int32_t, int64_t, const int64_t*,
                                                          const int64_t*, int32_t*, uint8_t*, int32_t*, uint8_t*, uint32_t*, int64_t,
                                                          const vapor_pair*, const int64_t*, int32_t*, int32_t*, const int64_t*, uint8_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_realign_revote: this build has no re-vote kernels");
}

// ... and `--realign-junction`'s one-jump reading of a pair (vapor_realign_junction: the two kernels of vapor_junction.h).
extern "C" __attribute__((weak)) int vapor_realign_junction(vapor_ctx*, vapor_seqset*, int64_t, const vapor_pair*, int32_t, int32_t*, const int64_t*,
                                                            int32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_realign_junction: this build has no junction kernels");
}

// The reference windows of a bgzipped FASTA on the device (vapor_fasta_windows_device, vapor_fasta_last_stats) are device code in
// vapor_hip.hip as well; the CPU twin answers them with VAPOR_E_ARG, and the caller reads the windows on the host.
extern "C" __attribute__((weak)) int vapor_fasta_windows_device(vapor_ctx*, int, int32_t, const uint64_t*, const uint64_t*, uint8_t*, int64_t,
                                                                int64_t*, uint8_t*, int32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_fasta_windows_device: this build has no device FASTA reader");
}

extern "C" __attribute__((weak)) int vapor_fasta_last_stats(vapor_ctx*, double*, int32_t)
{
    return bfail(VAPOR_E_ARG, "vapor_fasta_last_stats: this build has no device FASTA reader");
}

// Breakpoint refinement's device step (vapor_plan_set_grid, vapor_plan_run_grid: grid_pick_kernel) is device code in vapor_hip.hip;
// the CPU twin refuses it, and the caller scores the candidates one by one (vapor_amd/refine.py).
extern "C" __attribute__((weak)) int vapor_plan_set_grid(vapor_plan*, int64_t, const int32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_plan_set_grid: this build has no refinement kernel");
}

extern "C" __attribute__((weak)) int vapor_plan_run_grid(vapor_plan*, int32_t*, double*, double*, int64_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_plan_run_grid: this build has no refinement kernel");
}

extern "C" __attribute__((weak)) int vapor_grid_pick(vapor_ctx*, int64_t, const int32_t*, const double*, const int32_t*, const double*,
                                                     int32_t*, double*, double*, int64_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_grid_pick: this build has no refinement kernel");
}

// The phased read extraction on the device (vapor_bam_chop_device_tagged: the tag walk of the chop kernel, bam_select_kernel) is
// device code in vapor_hip.hip; the CPU twin refuses it, and the caller's host readers select the groups (vapor_bam_chop_tagged).
extern "C" __attribute__((weak)) int vapor_bam_chop_device_tagged(vapor_ctx*, vapor_bam*, int32_t, const int32_t*, const int64_t*, const int64_t*,
                                                                  const int64_t*, const int32_t*, const uint64_t*, int32_t, int32_t*, uint64_t*,
                                                                  int64_t*, int64_t*, uint32_t*, int64_t*, int32_t*, int32_t*, vapor_bam_batch**)
{
    return bfail(VAPOR_E_ARG, "vapor_bam_chop_device_tagged: this build has no device reader");
}

// ... so is the one that haplotags the reads from phased SNVs (vapor_bam_chop_device_haplotag: bam_haplotag_kernel; the host
// readers take vapor_bam_chop_haplotag) ...
extern "C" __attribute__((weak)) int vapor_bam_chop_device_haplotag(vapor_ctx*, vapor_bam*, int32_t, const int32_t*, const int64_t*, const int64_t*,
                                                                    const int64_t*, const int32_t*, const uint64_t*, int32_t, int32_t*, uint64_t*,
                                                                    int64_t*, int64_t*, uint32_t*, int64_t*, int32_t*, int32_t*, vapor_bam_batch**,
                                                                    const int32_t*, const void*, const int32_t*, const int64_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_bam_chop_device_haplotag: this build has no device reader");
}

// ... and the name keys of a device batch (vapor_bam_batch_name_keys, `--dedup-qname`): no device reader, no batch.
extern "C" __attribute__((weak)) int vapor_bam_batch_name_keys(vapor_bam_batch*, int64_t, uint64_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_bam_batch_name_keys: this build has no device reader");
}

// ... and so is the right-anchored one (vapor_bam_chop_device_right: bam_chop_right_kernel).
extern "C" __attribute__((weak)) int vapor_bam_chop_device_right(vapor_ctx*, vapor_bam*, int32_t, const int32_t*, const int64_t*, const int64_t*,
                                                                 const int64_t*, const int32_t*, const uint64_t*, int32_t, int32_t*, uint64_t*,
                                                                 int64_t*, int64_t*, int32_t*, vapor_bam_batch**)
{
    return bfail(VAPOR_E_ARG, "vapor_bam_chop_device_right: this build has no device reader");
}

// ... and the read depth on the device (vapor_bam_depth_device: bam_depth_kernel; the host reader is vapor_bam_depth).
extern "C" __attribute__((weak)) int vapor_bam_depth_device(vapor_ctx*, vapor_bam*, int32_t, const int32_t*, const int64_t*, const int32_t*,
                                                            const uint64_t*, uint64_t*, int32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_bam_depth_device: this build has no device reader");
}

// ... and the signatures on the device (vapor_bam_signature_device: bam_signature_kernel; the host reader is vapor_bam_signature).
extern "C" __attribute__((weak)) int vapor_bam_signature_device(vapor_ctx*, vapor_bam*, int32_t, const int32_t*, const int64_t*, const int32_t*,
                                                                const uint64_t*, int64_t*, int32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_bam_signature_device: this build has no device reader");
}

// ... and the links on the device (vapor_bam_links_device: bam_link_kernel; the host reader is vapor_bam_links).
extern "C" __attribute__((weak)) int vapor_bam_links_device(vapor_ctx*, vapor_bam*, int32_t, const int32_t*, const int64_t*, const uint8_t*, int64_t,
                                                            const int32_t*, const uint64_t*, int64_t*, int32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_bam_links_device: this build has no device reader");
}

// ... and the support on the device (vapor_bam_support_device: bam_support_kernel; the host reader is vapor_bam_support).
extern "C" __attribute__((weak)) int vapor_bam_support_device(vapor_ctx*, vapor_bam*, int32_t, const int32_t*, const int64_t*, const int32_t*,
                                                              const uint64_t*, int64_t*, int32_t*)
{
    return bfail(VAPOR_E_ARG, "vapor_bam_support_device: this build has no device reader");
}
