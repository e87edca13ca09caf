// vapor_records.h - the records the host plans and the kernels read: plain structs and constants, no HIP.  Included by
// vapor_kernels.h (device code) and by vapor_planner.h (the host planner, which a plain C++ compiler builds).
#pragma once
#include <stdint.h>

namespace vapor {

// ------------------------------------------------------------------------------------------
// device-side records
// ------------------------------------------------------------------------------------------
struct SeqDesc {       // 32 B
    uint32_t chunk0;   // first 32-base chunk of this sequence in the planes
    int32_t len;
    int32_t n_exc;     // symbols outside upper-case ACGT
    int32_t n_invalid; // symbols outside invert_base's alphabet (after IUPAC folding)
    uint32_t asc0;     // first 32-byte chunk in the ASCII staging blob (pack only)
    uint32_t flags;
    int32_t n_nocomp;  // symbols complementary() would DROP (SF:471-478: anything outside ATGCN / atgcn); bytes only
    uint32_t pad;
};

#define VP_PAD_CHUNKS 3  // zeroed chunks after each sequence: window reads may run this far

// a segment of a derived sequence as derive_kernel reads it (vapor_kernels.h); vapor_seqset_plan.h writes the list
struct DSeg {          // 20 B: dst symbols [dst, dst + len) of the derived sequence = parent[off .. off + len), reversed and
    uint32_t chunk0;   // complemented when rc; chunk0 = the parent's first plane chunk
    int32_t off, len, dst;
    uint32_t rc;
};

struct DPair {         // 40 B
    int32_t seq1, seq2, off2, k;
    uint32_t flags, cap;
    int64_t hit_off;
    int32_t len1, len2;  // sequence lengths (the clean kernels need nothing else of the sequences)
};

struct DTask {         // 16 B: pairs task_pairs[first .. first + n_reads) of one launch, sorted by allele
    int32_t seq2, k, n_reads, first;
};

constexpr int MAX_READS_PER_TASK = 64;

// ---- shared joins: what remap_kernel reads (described with the kernel in vapor_kernels.h) ----
struct DMap {          // 16 B (host side: the interval maps of a (window, k) group before they are cut into the table below)
    int32_t lo, hi;    // k-mer starts of the shared sequence, inclusive
    int32_t base;      // position in the target at e == lo
    uint16_t flip;     // 1: reverse-complemented slice (j decreases with e, strands swap)
    uint16_t slot;     // which target of the share
};
// What the kernel reads is the same maps cut at each other's ends: boundaries B[0] = 0 < B[1] < ... < B[n_iv] over the k-mer
// starts of the shared sequence, and per elementary interval [B[t], B[t+1]) what a dot inside it becomes - for every target
// slot up to two ops (a tandem duplication's repeated stretch lies twice in its allele), each one word:
//     bit 0 valid, bit 1 flip, bits 2.. delta (signed):   j = e + delta,  or  j = delta - e with the strands swapped.
// A record looks its interval up once (binary search) and is then copied, shifted, under the ops of that interval; only a run
// that crosses a boundary is cut, interval by interval.
constexpr int REMAP_MAX_IV = 48;       // elementary intervals per share (the host shares no group with more)
constexpr int REMAP_OPS = 8;           // op words per interval: 4 target slots x 2 copies
struct DShare {        // 32 B
    int32_t dpair;     // the (read, T) pair the join ran
    int32_t iv_first;  // first word of this group's table in the maps buffer: B[0 .. n_iv], then n_iv x REMAP_OPS op words
    int32_t n_iv;
    int32_t target[4]; // pair index per slot, -1: this read has no pair against that allele
    int32_t pad;
};

struct DServe {        // 32 B per pair: what the clean workgroup of a pair served by a shared join needs to cut its records out
    int64_t hit_off;   // of the shared dot plot: the (read, T) pair's record slot ...
    uint32_t cap;
    int32_t dpair;     // ... its index (-1: this pair ran a join of its own),
    int32_t iv_first, n_iv;   // the group's table
    int32_t slot;      // and this pair's slot in it
    int32_t pad;
};

static_assert(sizeof(SeqDesc) == 32 && sizeof(DSeg) == 20 && sizeof(DPair) == 40 && sizeof(DTask) == 16 && sizeof(DMap) == 16 && sizeof(DShare) == 32 &&
              sizeof(DServe) == 32, "the sizes the comments state: the kernels index arrays of these");

}  // namespace vapor
