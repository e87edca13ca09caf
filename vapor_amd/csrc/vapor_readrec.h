// vapor_readrec.h - the records the device readers' host sides plan and their kernels read (vapor_bamdev.h, vapor_fasta.h): plain
// structs and constants, no HIP, as vapor_records.h holds the plan's.  Included by the two device headers and by vapor_readplan.h
// (the plan of a reader call, which a plain C++ compiler builds).
#pragma once
#include <stdint.h>

namespace vapor_bamdev {

struct BgzfBlk {          // 24 B
    uint32_t c_off;       // the block's DEFLATE payload in the batch's compressed bytes
    uint32_t c_len;
    uint32_t u_off;       // where its data goes in the arena
    uint32_t u_len;       // ISIZE
    uint32_t crc;         // CRC-32 of the data (the block's trailer)
    uint32_t pad;
};

// ---- the records of a region ----------------------------------------------------------------------------------------------
struct BamSpan {          // one index chunk of a region: its records start in arena[u_begin, u_end), its data ends at u_limit
    uint32_t u_begin, u_end, u_limit;
    uint32_t blk_first, blk_n;   // its blocks in the block table (their status decides whether the bytes can be read)
    uint32_t pad;
};
struct BamRegion {        // `samtools view bam tid:start-end` + chop_pacbio_read_by_pos(start, end, flank)
    int64_t start, end, flank;
    int32_t tid, span_first, span_n;
    int32_t pad;          // the read filter: exclude_flags | min_mapq << 16; 0 filters nothing
};
struct DepthRegion {      // `--depth`: three consecutive intervals [b0, b1) [b1, b2) [b2, b3) of a contig, 0-based half-open
    int64_t b[4];
    int32_t tid, span_first, span_n;
    uint32_t filter;      // the read filter as BamRegion::pad carries it, 0x704 already among the excluded flags
};
struct SigRegion {        // `--signatures`: the walk window [w0, w3) of a contig, two targets and what counts at them
    int64_t w0, w3, x0, x1;
    int32_t nmin, nmax;   // length bounds of GAP and INSOP, clamped to [-1, 2^28] (no operation is longer than 2^28 - 1)
    int32_t tid, span_first, span_n;
    uint32_t filter;      // the read filter as BamRegion::pad carries it, 0x704 already among the excluded flags
    int32_t tol, min_clip;    // 0..255; 1..2^30
    uint32_t mask;        // SIG_* bits
    int32_t pad;
};
struct LinkRegion {       // `--links`: the walk window [w0, w3) of a contig, a clip event at x and where its SA entry must lie
    int64_t w0, w3, x, y;
    int32_t tid, span_first, span_n;
    uint32_t filter;      // the read filter as BamRegion::pad carries it, 0x704 already among the excluded flags
    int32_t tol, min_clip;    // 0..255; 1..2^30
    uint32_t bits;        // LINK_EV: the event is RCLIP (else LCLIP), LINK_PEND: the entry's b is tested (else its a), LINK_REL: the strands differ
    uint32_t name_off, name_len;   // the partner contig's name in the call's name blob
    int32_t pad;
};
struct SupRegion {        // `--support`: a signature region, the flank a reference alignment must reach on either side of a target, the shortest D, N or I that blocks it
    int64_t w0, w3, x0, x1;
    int32_t nmin, nmax;   // as SigRegion's
    int32_t tid, span_first, span_n;
    uint32_t filter;      // the read filter as BamRegion::pad carries it, 0x704 already among the excluded flags
    int32_t tol, min_clip;    // 0..255; 1..2^30
    uint32_t mask;        // SIG_* bits, SUP_REF0, SUP_REF1
    int32_t flank, gmin;  // 1..65535; 1..2^28
    int32_t pad;
};
struct BamKept {          // a read the reference keeps: its packed bases at arena + sq_off, from base q0 on, miss_bp
    uint32_t sq_off;
    int32_t q0, miss, l_seq;
};
constexpr uint32_t DEPTH_EXCLUDE = 0x704u;   // what never counts towards depth: unmapped, secondary, QC-fail, duplicate (`samtools depth`)
// `--signatures`: the event kinds of a region's mask and of its six counts, the widest tolerance (the histograms of a region are
// 2 * (2 * SIG_TOL_MAX + 1) words of LDS), and the words of a region's answer: six counts, then offset and count of each mode
constexpr uint32_t SIG_LCLIP0 = 1u, SIG_RCLIP0 = 2u, SIG_LCLIP1 = 4u, SIG_RCLIP1 = 8u, SIG_GAP = 16u, SIG_INSOP = 32u;
constexpr int SIG_TOL_MAX = 255, SIG_HIST_WORDS = 2 * (2 * SIG_TOL_MAX + 1), SIG_ANSWER_WORDS = 10;
// `--links`: the bits of a region, its histogram (2 * tol + 1 words of LDS) and the words of its answer: n_clip, n_split, n_link,
// then offset and count of the mode
constexpr uint32_t LINK_EV = 1u, LINK_PEND = 2u, LINK_REL = 4u;
constexpr int LINK_HIST_WORDS = 2 * SIG_TOL_MAX + 1, LINK_ANSWER_WORDS = 5;
// `--support`: reference support is asked at x0 / at x1 (bits 6 and 7 of a region's mask, behind the six SIG_* bits), the widest
// flank, and the words of a region's answer: alt_cg, alt_l, alt_r, ref_0, ref_1, cov_0, cov_1
constexpr uint32_t SUP_REF0 = 64u, SUP_REF1 = 128u;
constexpr int SUP_FLANK_MAX = 65535, SUP_ANSWER_WORDS = 7;
constexpr int KEPT_CAP = 256;     // kept reads a region's slot holds (minimize_pacbio_read_list keeps 20 of them)
// status of a region: 0, or why the host route must do it
constexpr int REG_OK = 0, REG_BEYOND = 1, REG_MALFORMED = 2, REG_NO_CIGAR = 3, REG_KEPT_FULL = 4, REG_BLOCK = 5, REG_NEG_Q0 = 6, REG_NO_SEQ = 7;
constexpr int REG_PHASE_SETS = 8;  // (`--phase-vcf`) more phase sets among the region's sites than a wavefront tallies: set by the host, before anything is sent

// ---- haplotype tags (`--phased`) ----------------------------------------------------------------------------
struct BamTag {           // beside a region's BamKept entry, in an array of its own: the record's phase set and haplotype
    long long ps;         // value of the first PS field of integer type, PS_NONE without one
    int32_t hap, pad;     // value of the first HP field of integer type if it is 1 or 2, else 0
};
constexpr long long PS_NONE = (long long)0x8000000000000000ull;
struct BamPick {          // a read of a region's union of the three group lists (A, H1, H2), in record order
    uint32_t sq_off;
    int32_t q0, miss;
    uint32_t member;      // bits 0-2: in the list of A / H1 / H2; bits 8-15, 16-23, 24-31: its position in that list
};
struct BamPhase {         // a region's answer: its phase set P, whether any kept record is tagged, the size of the union
    long long ps;
    int32_t tagged, n_union;
};

// ---- haplotags from phased SNVs (`--phase-vcf`) --------------------------------------------------------------
struct BamOps {           // beside a region's BamKept entry, in an array of its own: where bam_haplotag_kernel finds the record
    uint32_t ops_off;     // its operations in the arena (the CIGAR, or the CG:B,I array of a long-CIGAR record)
    int32_t n_ops;
    int32_t pos;          // 0-based POS
    uint32_t sq_off;      // its packed bases
};
struct BamSite {          // a phased heterozygous SNV of a region, 8 B
    int32_t pos;          // 1-based
    uint8_t a1, a2;       // what haplotype 1 / 2 carries, BAM 4-bit codes
    uint8_t ps_idx, pad;  // its phase set: index into the region's table, below PHASE_SETS_CAP
};
struct BamSiteRange {     // a region's sites (in position order) and its table of phase-set values
    int32_t site_first, site_n, ps_first, ps_n;
};
constexpr int PHASE_SETS_CAP = 64;     // phase sets a wavefront tallies: lane p holds the two counts of phase set p

static_assert(sizeof(BgzfBlk) == 24 && sizeof(BamSpan) == 24 && sizeof(BamRegion) == 40 && sizeof(DepthRegion) == 48 && sizeof(SigRegion) == 72 && sizeof(LinkRegion) == 72 && sizeof(SupRegion) == 80 && sizeof(BamKept) == 16 && sizeof(BamTag) == 16 &&
              sizeof(BamPick) == 16 && sizeof(BamPhase) == 16 && sizeof(BamOps) == 16 && sizeof(BamSite) == 8 && sizeof(BamSiteRange) == 16,
              "the kernels index arrays of these, and the metadata block of a call is carved by their sizes");

}  // namespace vapor_bamdev

namespace vapor_fasta {

struct FastaWin {               // 32 B
    uint64_t a_beg, a_end;      // the window's raw bytes (newlines included) in the arena
    uint64_t t_off;             // its slot in the text buffer (a_end - a_beg bytes: the text is never longer)
    uint32_t blk_first, blk_n;  // its blocks in the block table
};
static_assert(sizeof(FastaWin) == 32, "fasta_window_kernel indexes an array of these");

// status of a window (include/vapor_hip.h: VAPOR_FASTA_*)
constexpr int WIN_OK = 0, WIN_BLOCK = 1, WIN_RANGE = 2, WIN_NON_ASCII = 3, WIN_ROOM = 4;

}  // namespace vapor_fasta
