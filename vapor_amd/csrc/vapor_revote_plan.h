// vapor_revote_plan.h - the host arithmetic of vapor_realign_revote, without HIP: the call-level checks the entry
// adds to vapor_realign_polish's, the record a vote pair travels as, what a locus adds to its group's device buffer - the own[]
// table, the byte staging of the spelt codes and the polished 4-bit plane, every piece on 16 bytes, charged to trace_budget through
// vapor_polish::plan_groups' `extra` - and the layouts of the outputs.  The kernels of vapor_revote.h read the same constants and
// records; tools/revote_check.cpp holds the functions to direct statements on the host under the sanitizers.
#pragma once

#include "vapor_polish_plan.h"

namespace vapor_revote {

// vout: four int32 a vote pair; lout: four int32 a locus
constexpr int VOUT = 4;
enum VoutField { V_D = 0, V_STATUS = 1, V_OFF2 = 2, V_M = 3 };
constexpr int LOUT = 4;
enum LoutField { L_STATUS = 0, L_PLEN = 1 };

// the most symbols the polished allele of a locus of len columns has: every column kept, and RMAX bases at every site it can keep
// (a site lies before a column q >= 1, so a locus has fewer sites than columns)
inline int64_t spelt_cap(int64_t len) { return len + (int64_t)vapor_polish::RMAX * (len < vapor_polish::MAX_SITES ? len : vapor_polish::MAX_SITES); }

// call-level checks of the vote pairs' table (ascending from 0 to n_votes) and of the spelt slots' (ascending from 0)
inline bool vfirst_ok(int64_t n_votes, int64_t n_loci, const int64_t* vfirst)
{
    if (n_votes < 0 || n_votes > vapor_realign::MAX_PAIRS || n_loci < 0 || !vfirst || vfirst[0] != 0) return false;
    for (int64_t g = 0; g < n_loci; ++g)
        if (vfirst[g + 1] < vfirst[g]) return false;
    return vfirst[n_loci] == n_votes;
}
inline bool spelt_off_ok(int64_t n_loci, const int64_t* spelt_off)
{
    if (n_loci < 0 || !spelt_off || spelt_off[0] != 0) return false;
    for (int64_t g = 0; g < n_loci; ++g)
        if (spelt_off[g + 1] < spelt_off[g]) return false;
    return true;
}
// whether a locus's spelt slot holds whatever its polished allele may be
inline bool slot_ok(int64_t slot_bytes, int64_t len) { return slot_bytes >= spelt_cap(len); }

// A vote pair as realign_onto_kernel takes it (24 B): the read's first x4 word and length, off2 in the called allele's columns,
// the locus among its group's loci.
struct VPair {
    uint64_t word1;
    int32_t n, off2;
    int32_t locus;
    int32_t status;            // 0, or VAPOR_E_ARG: the kernel writes {-1, status, 0, 0}
};
static_assert(sizeof(VPair) == 24, "VPair layout");

// the record of a vote pair: refused where vapor_realign_batch refuses it and where its seq2 is not the locus's allele
// (allele < 0: the locus has none)
template <typename LenOf, typename ChunkOf>
inline VPair vote_record(const vapor_pair& a, int32_t n_seqs, int64_t allele, int32_t locus, LenOf len_of, ChunkOf chunk_of)
{
    VPair r{0, 0, 0, locus, vapor_realign::pair_status(a, n_seqs, len_of)};
    if (!r.status && (allele < 0 || (int64_t)a.seq2 != allele)) r.status = VAPOR_E_ARG;
    if (r.status) return r;
    r.word1 = (uint64_t)chunk_of(a.seq1) * 4u;
    r.n = (int32_t)len_of(a.seq1);
    r.off2 = a.off2;
    return r;
}

// A locus as spell_kernel, spell_pack_kernel and realign_onto_kernel take it (48 B).  The three offsets are dwords from the start
// of the group's buffer.
struct VLocus {
    uint64_t word2;            // first x4 word of the called allele
    int64_t own_off;           // own[0 .. len]: int32, the polished position of column q's own symbol; own[len] = plen
    int64_t stage_off;         // the spelt codes, one a byte, in whole 32-byte chunks
    int64_t plane_off;         // the polished plane, in whole 32-symbol chunks of four words
    int32_t cap;               // spelt_cap(len): no symbol is written at or behind it
    int32_t status;            // not 0: the locus is not spelt, lout = {status, 0, 0, 0} (the polish's status, or no allele)
    int32_t short_slot;        // 1: spelt, but the caller's slot is too small - lout's status is VAPOR_E_ARG
    int32_t pad;
};
static_assert(sizeof(VLocus) == 48, "VLocus layout");

// dwords of a locus's three pieces, each a multiple of four (16 bytes).  The plane holds whole chunks up to the cap: RaReader
// (vapor_band_row.h) loads word k only while 8 k < plen <= cap, one word ahead included, so it stays inside.
inline int64_t chunks_of(int64_t len) { return (spelt_cap(len) + 31) / 32; }
inline int64_t own_words(int64_t len) { return vapor_polish::align4(len + 1); }
inline int64_t stage_words(int64_t len) { return 8 * chunks_of(len); }
inline int64_t plane_words(int64_t len) { return 4 * chunks_of(len); }
inline int64_t locus_extra(int64_t len) { return own_words(len) + stage_words(len) + plane_words(len); }

// Where the pieces of a group's loci stand: from `base` (the group's extra_off) on, the own[] tables of all its loci, then their
// stagings - one stretch, which the optional spelt output copies back at once -, then their planes.  lens[k] / extra[k]: the
// columns of the group's locus k and what it was charged (0: a locus that is not spelt has no pieces).  Returns the dwords used;
// stage_base: where the stagings start.
inline int64_t place(int64_t base, int64_t n, const int64_t* lens, const int64_t* extra, VLocus* out, int64_t& stage_base)
{
    int64_t at = base;
    for (int64_t k = 0; k < n; ++k) {
        out[k].own_off = at;
        if (extra[k]) at += own_words(lens[k]);
    }
    stage_base = at;
    for (int64_t k = 0; k < n; ++k) {
        out[k].stage_off = at;
        if (extra[k]) at += stage_words(lens[k]);
    }
    for (int64_t k = 0; k < n; ++k) {
        out[k].plane_off = at;
        if (extra[k]) at += plane_words(lens[k]);
    }
    return at - base;
}

}  // namespace vapor_revote
