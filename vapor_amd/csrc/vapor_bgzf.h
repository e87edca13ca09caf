// vapor_bgzf.h - the one statement of what a BGZF block is, for the host reader (vapor_bam.cpp) and the two device
// readers' host sides (vapor_hip.hip).  Plain C++17 without device code: the parser of a block's header and trailer, the walk over
// the blocks of a staged byte range, and on top of the walk the scans of the device readers (the spans of vapor_bam_chop_device*,
// the stretches of vapor_fasta_windows_device).  tools/bgzf_scan_check.cpp runs all of it on the host under the sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vapor_bgzf {

enum class Parse { BLOCK, NOT_BGZF, MORE };        // a whole block; not a BGZF block; the bytes given end before the block does

struct Header {
    int xlen = 0;                  // length of the gzip extra field
    int bsize = 0;                 // the whole block, header .. trailer (with MORE: set when the extra field was there, else 0)
    uint32_t crc = 0, isize = 0;   // the trailer: CRC-32 and size of the block's data
};

inline uint32_t le32(const uint8_t* t) { return (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24); }

// The block that starts at h, of which `avail` bytes are there; no byte behind them is read.  A block is the magic 1f 8b 08 with
// FLG.FEXTRA, an extra field that holds a BC subfield of SLEN 2 wholly inside it (the last one counts), bsize >= xlen + 20 (12
// bytes of header, the extra field, CRC32 and ISIZE: anything shorter is not a block) and isize <= 65536.
inline Parse parse_block(const uint8_t* h, size_t avail, Header& o)
{
    o = Header();
    if (avail < 18) return Parse::MORE;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return Parse::NOT_BGZF;
    o.xlen = h[10] | (h[11] << 8);
    if (12 + (size_t)o.xlen > avail) return Parse::MORE;
    int bsize = -1;
    for (int q = 0; q + 4 <= o.xlen;) {
        const uint8_t* e = h + 12 + q;
        const int slen = e[2] | (e[3] << 8);
        if (e[0] == 66 && e[1] == 67 && slen == 2 && q + 6 <= o.xlen) bsize = (e[4] | (e[5] << 8)) + 1;
        q += 4 + slen;
    }
    if (bsize < o.xlen + 20) return Parse::NOT_BGZF;       // (without BC as well)
    o.bsize = bsize;
    if ((size_t)bsize > avail) return Parse::MORE;
    o.crc = le32(h + bsize - 8);
    o.isize = le32(h + bsize - 4);
    return o.isize <= 65536u ? Parse::BLOCK : Parse::NOT_BGZF;
}

struct Block {                     // a whole block of a walk
    size_t pos;                    // where it starts in the walked range
    int xlen, bsize;
    uint32_t crc, isize;
    uint64_t u;                    // the data of the blocks before it in the walk
    size_t payload() const { return pos + 12 + (size_t)xlen; }         // its DEFLATE stream ...
    uint32_t c_len() const { return (uint32_t)(bsize - xlen - 20); }   // ... and that stream's length
};

enum class End { STOP, MORE, BAD };                // the stop rule said so; the bytes ran out; not BGZF, or the caller refused a block
struct Walked { End end; size_t pos; uint64_t u; };   // ... at this position of the range, behind this much data

// The whole blocks of base[0, n), which lie at `file_off` in the file: stop(file offset of the next block) is asked before each
// block, take(block) is handed each whole one and refuses it by returning false.
template <typename Stop, typename Take>
inline Walked walk(const uint8_t* base, size_t n, int64_t file_off, Stop stop, Take take)
{
    size_t p = 0;
    uint64_t u = 0;
    for (;;) {
        if (stop(file_off + (int64_t)p)) return {End::STOP, p, u};
        Header h;
        const Parse r = parse_block(base + p, n - p, h);
        if (r == Parse::MORE) return {End::MORE, p, u};
        if (r == Parse::NOT_BGZF || !take(Block{p, h.xlen, h.bsize, h.crc, h.isize, u})) return {End::BAD, p, u};
        u += h.isize;
        p += (size_t)h.bsize;
    }
}

// ---- vapor_bam_chop_device*: one index chunk of a region ---------------------------------------------------------------------
struct HostSpan {
    int32_t region;
    uint64_t cs, ce;               // the chunk's virtual offsets
    int64_t file_off;              // compressed range read from the file
    size_t want, got;
    size_t stage_off;              // ... into the pinned staging buffer here
    std::vector<Block> blks;       // the blocks that hold data (pos relative to the span's bytes, u to the span's data)
    uint64_t u_begin = 0, u_end = 0, u_total = 0;
    bool bad = false;              // not BGZF, a begin offset outside its block, 2 GB of data: the host route words the error
};
constexpr uint64_t SPAN_DATA_LIMIT = (uint64_t)1 << 31;     // (the device's offsets are 32-bit: BgzfBlk, BamSpan)

// the whole blocks of a span, through the block that holds the chunk's end
inline void scan_span(HostSpan& sp, const uint8_t* stage)
{
    const int64_t end_coff = (int64_t)(sp.ce >> 16);
    const uint32_t end_uoff = (uint32_t)(sp.ce & 0xFFFFu), b0 = (uint32_t)(sp.cs & 0xFFFFu);
    bool have_end = false;
    uint32_t first_usize = 0;      // (the first block in file order, empty or not, is the one `cs` names)
    const Walked w = walk(stage + sp.stage_off, sp.got, sp.file_off,
        [&](int64_t coff) { return coff > end_coff || (coff == end_coff && end_uoff == 0); },
        [&](const Block& b) {
            if (b.pos == 0) first_usize = b.isize;
            if (sp.file_off + (int64_t)b.pos == end_coff) { have_end = true; sp.u_end = b.u + std::min(end_uoff, b.isize); }
            if (b.isize == 0) return b.crc == 0;            // (the CRC-32 of no bytes)
            sp.blks.push_back(b);
            return true;
        });
    sp.u_total = w.u;
    if (!have_end) sp.u_end = w.u;                          // the chunk ends on a block boundary (or the file ends inside it)
    // the first record's offset must lie inside the first block
    sp.bad = w.end == End::BAD || b0 > first_usize || w.u >= SPAN_DATA_LIMIT;
    if (!sp.bad) sp.u_begin = b0;
}

// ---- vapor_fasta_windows_device: compressed bytes [c0, c_end) of the file, read at once; holds the blocks of its windows --------
struct FaStretch {
    int64_t c0 = 0, c_last = 0;    // first block; the last needed block starts at c_last (need_last) or ends there
    bool need_last = false;
    size_t want = 0, got = 0, stage_off = 0;
    std::vector<Block> blks;       // every block scanned, in file order, and behind them a sentinel: pos behind the last one, u = the stretch's size
    std::vector<uint32_t> gidx;    // ... the number of non-empty blocks before them in the call's block table
    bool cut = false;              // the scan stopped at a damaged or missing block: windows behind it are not found
    bool room = true;
    uint64_t arena_off = 0;
};

// what to read of the stretch's last block, from its first bytes: its BSIZE, or the 64 KB a block can be at most when they do not say
inline uint64_t last_block_size(const uint8_t* h, size_t avail)
{
    Header o;
    return parse_block(h, avail, o) != Parse::NOT_BGZF && o.bsize ? (uint64_t)o.bsize : 65536u;
}

inline void scan_stretch(FaStretch& s, const uint8_t* stage)
{
    const Walked w = walk(stage + s.stage_off, s.got, s.c0,
        [&](int64_t coff) { return coff > s.c_last || (coff == s.c_last && !s.need_last); },
        [&](const Block& b) {
            if (b.isize == 0 && b.crc != 0) return false;
            s.blks.push_back(b);
            return true;
        });
    s.cut = w.end != End::STOP;
    s.blks.push_back(Block{w.pos, 0, 0, 0, 0, w.u});
    s.gidx.assign(s.blks.size(), 0);
}

}   // namespace vapor_bgzf
