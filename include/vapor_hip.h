/*
 * vapor_hip.h - C ABI of libvapor_hip.so: VaPoR's recurrence-plot scoring path on MI355X.
 *
 * The reference has no FFI layer: its hot path is a set of module-level Python functions in
 * vapor_vali/Simple_function.pyx ("SF") that the `vapor` script star-imports
 * (vapor_vali/vapor:303,322,374,470).  Every entry point below names the reference routine(s)
 * it stands in for; the Python host code in vapor_amd/ keeps the reference's function names
 * and calls through this ABI with ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions: plain pointers and sizes; all buffers caller-allocated and never retained;
 * every function returns 0 or a negative VAPOR_E_* code (vapor_abi_version, vapor_build_flags, vapor_source_id, the two *_last_error
 * calls and vapor_crc32 return what their names say); vapor_last_error() gives a thread-local message (vapor_bam_last_error()
 * for the host helpers of the read extraction and the output table).  One host thread per context.  No exception crosses the
 * boundary.
 */
#ifndef VAPOR_HIP_H
#define VAPOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAPOR_ABI_VERSION 3
/* A developer build of the library (-DVAPOR_DEV_BUILD: timing stamps, A/B variants, non-default tuning constants)
 * reports VAPOR_ABI_VERSION + VAPOR_ABI_DEV_OFFSET and lists what it carries in vapor_build_flags(); the product
 * build reports VAPOR_ABI_VERSION and "".  A loader that accepts only VAPOR_ABI_VERSION can never run an
 * experimental library by accident. */
#define VAPOR_ABI_DEV_OFFSET 1000000

/* status codes */
#define VAPOR_OK 0
#define VAPOR_E_HIP (-1)       /* a HIP runtime call failed (message in vapor_last_error) */
#define VAPOR_E_OVERFLOW (-2)  /* caller-supplied output buffer too small; required size reported */
#define VAPOR_E_KEYERROR (-3)  /* a k-mer of seq1 holds a character invert_base lacks (SF:19-20, SF:1421) */
#define VAPOR_E_ARG (-4)       /* bad argument: index out of range, unsupported k, sequence too long */
#define VAPOR_E_NOMEM (-5)

#define VAPOR_MAX_SEQ_LEN 65535 /* positions are packed 16+16 bit on the device */
#define VAPOR_MAX_WIDE_SEQ_LEN 1048575 /* the wide route (vapor_wide_batch, vapor_clean_hits_wide): 2^20 - 1 */
#define VAPOR_MAX_ANY_K 64 /* the any-k route (vapor_anyk_batch): k from 1 to this */

typedef struct vapor_ctx vapor_ctx;
typedef struct vapor_seqset vapor_seqset;
typedef struct vapor_plan vapor_plan;

/* per-sequence upload flags */
#define VAPOR_SEQ_UPPER 1u /* apply str.upper() before packing (SF:183-184: abs_dis_m1b upper-cases ref and alt) */

/*
 * One dot plot: dotdata(k, seq1, seq2[off2:]) (SF:545-549 -> kmerhits SF:951-983), i.e. the
 * reference's call convention dotdata(window_size, read, allele[miss_bp:]) (SF:185-186,
 * 242-243, 278-279).  seq1/seq2 index a vapor_seqset.  k must be 10, 20, 30 or 40, the only
 * values window_size_refine can return (SF:2031-2041); vapor_anyk_batch takes 1 .. VAPOR_MAX_ANY_K.
 */
typedef struct vapor_pair {
    int32_t seq1;  /* read (the sequence whose k-mers are also searched reverse-complemented) */
    int32_t seq2;  /* allele window */
    int32_t off2;  /* miss_bp: seq2 is used from this offset on */
    int32_t k;
    uint32_t flags; /* VAPOR_PF_* */
} vapor_pair;

#define VAPOR_PF_C1 1u   /* clean_dotdata_diagnal_and_anti_diagnal (SF:432-448) -> ST_C1_* */
#define VAPOR_PF_C2 2u   /* the two-step cleaning of within_10Perc_m1b (SF:281-288) -> ST_C2_* */
#define VAPOR_PF_DIR 4u  /* with PF_C1: dis_to_diagnal_most_abundant_defined (SF:582-591) and
                            eu_dis_dir_calcu (SF:718-722) over the C1-kept dots -> ST_DIR_* */
#define VAPOR_PF_FORWARD 8u /* vapor_anyk_batch only: kmerhits(seq1, seq2, k, 1, inversions=False) - no reverse-complement keys,
                               no KeyError, symbols outside the folded alphabet compared byte for byte */

/* int64 statistics record per pair (VAPOR_STATS_STRIDE words) */
#define VAPOR_STATS_STRIDE 16
#define VAPOR_ST_N_HITS 0      /* len(dotdata) */
#define VAPOR_ST_FIRST_J 1     /* dotdata[0][0]  = smallest j, -1 if no hits (SF:187) */
#define VAPOR_ST_LAST_J 2      /* dotdata[-1][0] = largest j,  -1 if no hits */
#define VAPOR_ST_C1_KEPT 3     /* dots surviving C1 */
#define VAPOR_ST_C1_SUM_ABS 4  /* sum |j-i| over them: eu_dis_abs_calcu = this / C1_KEPT (SF:705-708) */
#define VAPOR_ST_C2_KEPT 5     /* dots surviving the diagonal step or the anti-diagonal step on the rest */
#define VAPOR_ST_C2_COUNT10 6  /* eu_dis_dots_within_10perc over them (SF:730-733) */
#define VAPOR_ST_N_DIAG 7      /* dots with j == i (qual_check_repetitive_region SF:1158-1160) */
#define VAPOR_ST_N_LOWER 8     /* dots with j > i  (SF:1162-1164) */
#define VAPOR_ST_C2_KEPT_DIAG 9 /* dots kept by the diagonal step alone */
#define VAPOR_ST_DIR_C2X 10     /* 2*c, c = the redefined diagonal intercept (a multiple of 0.5; 0 when not unique) */
#define VAPOR_ST_DIR_N 11       /* kept dots (x,y) = (j+c, i) with abs(x-y)/abs(x) > 0.1 (eu_dis_single_dot SF:710-716) */
#define VAPOR_ST_DIR_SUM2 12    /* 2 * sum(x - y) over them: eu_dis_dir_calcu = SUM2 / 2 / N, or 0.0001 when N == 0 */
#define VAPOR_ST_DIR_LISTS 13   /* number of longest sub-bins found (c is a median only when this is 1) */
#define VAPOR_ST_RECORDS_NEEDED 14 /* 0; on VAPOR_E_OVERFLOW the run records the pair produced (its slot was smaller) */
#define VAPOR_ST_STATUS 15     /* 0, or VAPOR_E_KEYERROR / VAPOR_E_ARG / VAPOR_E_OVERFLOW for this pair */

/* per-hit flag bits returned by vapor_plan_fetch_hits */
#define VAPOR_HF_C1_KEPT 1u
#define VAPOR_HF_C2_DIAG 2u
#define VAPOR_HF_C2_ANTI 4u

/* ---- context --------------------------------------------------------------------------- */
int vapor_abi_version(void);
const char* vapor_build_flags(void);
/* What the binary was built from: "<k>:<a>", k = sha256 (16 hex digits) over the kernel sources and the build recipe
 * (vapor_kernels.h, vapor_hip.hip, build.py: the id profiles/ cites), a = the same over every source file of the library.  The
 * loader compares it with the sources beside it and refuses a library that was built from other ones; "cpu-twin" for the
 * CPU twin, "unknown" for a build outside vapor_amd/build.py. */
const char* vapor_source_id(void);
const char* vapor_last_error(void);
int vapor_init(int device_ordinal, vapor_ctx** ctx);
int vapor_destroy(vapor_ctx* ctx);
/* tuning knobs: "reads_per_task" (at most this many pairs per join workgroup, <= 64), "join_tasks" (number of
 * join workgroups a launch is cut into; default = number of CUs), "join_align" (read at vapor_plan_create.  0: every run
 * takes the cost-balanced task table; 2: every run takes the window-aligned one - every task the reads of ONE allele, no table
 * built again by a neighbouring task, the tasks less even; 1, the default: blocking runs take the balanced table, an asynchronous
 * step the aligned one while a step of another plan of the context is in flight beside it and the planner's cost model sees
 * enough builds saved - the aligned table is made by the plan's first asynchronous step), "max_pair_cap" (largest record slot a pair may
 * grow to on an overflow rerun; beyond it the pair keeps VAPOR_E_OVERFLOW), "shared_join" (1, the default: a read scored
 * against a window and alleles derived from it - vapor_seqset_create_derived - is joined once for all of them; 0: one join per
 * pair), "remap_in_clean" (who cuts a served pair's records out of a shared dot plot.  1, the default: the workgroup that cleans
 * the pair when the plan's clean workgroups run in at most four rounds (a resident batch of a few thousand pairs), else a kernel
 * of its own before the cleaning, remap_kernel; 0: always that kernel; 2: always the clean workgroups), "clean_order" (1, the default: the clean kernel's workgroups - one per
 * pair - are dealt out longest pair first, so that the last round of a plan of a few rounds is made of its shortest pairs; 0: in
 * pair order), "clean_fit" (1, the default: after a plan's first blocking run the clean workgroups' LDS copy is sized for the
 * largest record count the pairs really have instead of the estimate made at vapor_plan_create - more workgroups per CU; 0: the
 * estimate stays), "stage_threads" (host threads that copy a
 * sequence set's bytes into the pinned staging buffer, default 3), "anyk_edit_pairs" (at least 1, default 2^31: the (allele k-mer,
 * key) distances one launch of vapor_anyk_batch's k > 40 pass may hold - a pair of n lookup entries is cut into launches of
 * max(4, anyk_edit_pairs / n rounded down to a multiple of 4) allele k-mers), "bam_cu_share" (0 .. 8: vapor_bam_chop_device's copies and kernels
 * go to a stream masked to that many eighths of the CUs - 0 and 8: the context's own stream, all CUs; a caller that scores several
 * batches at once on several contexts leaves CUs to the other contexts' kernels this way).  Results do not depend on any of them.
 * A test parameter: "pool_fill" (-1, the default: off; 0 .. 255: from now on every device or pinned block the context's pool hands
 * out, fresh or recycled, is filled with that byte over its whole capacity before the call that asked for it goes on, and so are
 * the staging buffers of vapor_seqset_create* - each fill ends in a host-side wait for the device, so calls are slow; any other
 * value is VAPOR_E_ARG).  No answer may depend on what a block held before: tests/test_gpu_pool_fill.py. */
int vapor_set_param(vapor_ctx* ctx, const char* name, int64_t value);

/* ---- sequences: ASCII in, packed bit planes resident in HBM ------------------------------ */
/*
 * Uploads n_seqs sequences (blob[off[s] .. off[s]+len[s])), folds IUPAC codes as key_modify
 * does (SF:908-949), optionally upper-cases, and packs them on the device into a 2-bit base
 * plane, a 1-bit "not A/C/G/T" plane and a 4-bit symbol plane.
 * seq_info[2*s] receives the number of symbols outside upper-case ACGT, seq_info[2*s+1] the
 * number outside invert_base's alphabet (such a seq1 raises KeyError in the reference).
 */
int vapor_seqset_create(vapor_ctx* ctx, int32_t n_seqs, const uint8_t* blob, const int64_t* off,
                        const int32_t* len, const uint8_t* flags, int32_t* seq_info,
                        vapor_seqset** set);
/* the same from one pointer per sequence (no concatenated copy on the caller's side): seq[s] points at len[s] bytes */
int vapor_seqset_create_ptrs(vapor_ctx* ctx, int32_t n_seqs, const uint8_t* const* seq, const int32_t* len,
                             const uint8_t* flags, int32_t* seq_info, vapor_seqset** out);
/*
 * Derived sequences: alleles the reference builds by string surgery on a window it has already read - a deletion's
 * ref_seq[:f] + ref_seq[-f:] (SF:1712), a tandem duplication's ref[:f] + mid + mid + ref[-f:] (SF:1755), an inversion's
 * ref[:f] + reverse(complementary(mid)) + ref[-f:] (SF:1907), an insertion's flank + ins_seq + flank (SF:1872), the block
 * structures of the complex types (SF:1557-1665), and the str.upper() twins of abs_dis_m1b (SF:183-184) - described instead of
 * uploaded: derived sequence d (index n_seqs + d of the set) is the concatenation of its segments
 * segs[seg_first[d] .. seg_first[d+1]), each a slice parent[off : off + len] of one of the n_seqs sequences given as bytes,
 * reverse-complemented when VAPOR_SEG_REVCOMP is set, the whole upper-cased when derived_flags[d] has VAPOR_SEQ_UPPER.  The
 * device assembles the bit planes from the parents' (derive_kernel); no byte of a derived sequence crosses the link.
 * complementary() DROPS every character outside ATGCN / atgcn (SF:471-478), which a descriptor cannot express: a
 * reverse-complemented segment whose parent holds such a character (an IUPAC code, an X) is refused with VAPOR_E_ARG and the
 * caller uploads that allele as bytes.  A derived sequence without VAPOR_SEQ_UPPER over a parent that was uploaded WITH it is
 * refused as well (the parent's planes hold the upper-cased text, not its bytes).  seq_info has 2 * (n_seqs + n_derived) entries.
 * A plan over such a set joins every read ONCE against a reference window and the alleles derived from it: the k-mers of a
 * derived allele are those of its parent's slices plus the few that span a junction or lie in inserted bytes, so one table
 * (the parent followed by those stretches) and one probe per read give the dots of all of them (remap_kernel).
 */
typedef struct vapor_segment {
    int32_t parent; /* 0 .. n_seqs-1 */
    int32_t off, len;
    uint32_t flags; /* VAPOR_SEG_* */
} vapor_segment;
#define VAPOR_SEG_REVCOMP 1u
#define VAPOR_MAX_SEGMENTS 16 /* per derived sequence */
int vapor_seqset_create_derived(vapor_ctx* ctx, int32_t n_seqs, const uint8_t* const* seq, const int32_t* len,
                                const uint8_t* flags, int32_t n_derived, const int32_t* seg_first, const vapor_segment* segs,
                                const uint8_t* derived_flags, int32_t* seq_info, vapor_seqset** out);
/* The packed planes of one sequence as they lie in HBM (for tests and callers that want to check a derived sequence against
 * the same text uploaded as bytes): ceil(len / 32) chunks, per chunk 2 words of the 2-bit plane into p2, 1 word of the
 * "not upper-case ACGT" plane into e1, 4 words of the 4-bit symbol plane into x4 (any of the three may be NULL). */
int vapor_seqset_planes(vapor_seqset* set, int32_t seq, uint32_t* p2, uint32_t* e1, uint32_t* x4);
int vapor_seqset_destroy(vapor_seqset* set);

/* ---- plans: a batch of dot plots resident on the device ---------------------------------- */
/* Validates and groups the pairs (reads sharing an allele window share its hash table),
 * uploads the descriptors and sizes the workspace.  The plan can be run any number of times. */
int vapor_plan_create(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs,
                      vapor_plan** plan);
int vapor_plan_destroy(vapor_plan* plan);
/*
 * The hot path: k-mer hash join (kmerhits SF:951-983), gap clustering and noise cleaning
 * (dis_cluster SF:551-564, dis_cluster_2 SF:566-580, SF:404-448) and the integer reductions
 * (SF:705-733, SF:1154-1171) for every pair.  stats: n_pairs * VAPOR_STATS_STRIDE int64.
 */
int vapor_plan_run(vapor_plan* plan, int64_t* stats);
/* device time of the kernels of the last vapor_plan_run, measured with HIP events on the
 * library's stream: ms[0] = join kernels (and remap_kernel where the plan runs it), ms[1] = clean kernels, ms[2] = whole run incl.
 * copies, ms[3] = number of join launches, ms[4] = number of retried pairs, ms[5] = finish kernel, ms[6] = pairs served by a shared
 * join, ms[7] = joins that serve them, ms[8] = clean workgroups per CU (what the staged records leave room for), ms[9] = 1 when
 * the clean workgroups cut the served pairs' records out of the shared dot plots themselves ("remap_in_clean"), ms[10] = join
 * tasks (workgroups) of the task table the last run took, ms[11] = allele tables that run built (per task: alleles x tiles;
 * "join_align").  n = how many of the twelve the caller wants. */
int vapor_plan_timings(vapor_plan* plan, double* ms, int32_t n);
/* run records the join of the last run wrote per pair (n_pairs int64): the device keeps runs of consecutive
 * dots (j+t, i+t) / (j-t, i+t) as one record; stats[0] stays the number of dots */
int vapor_plan_record_counts(vapor_plan* plan, int64_t* records);
/* algorithmic bytes of one run: sum over pairs of packed read + packed allele
 * + 8 B per hit + 128 B statistics record, using the hit counts of the last run */
int vapor_plan_algorithmic_bytes(vapor_plan* plan, int64_t* bytes, int64_t* cells);
/*
 * Hits of selected pairs after vapor_plan_run: hits_ji receives (j, i) int32 pairs in
 * unspecified order inside a pair (dotdata's list is these sorted by (j, i)), hit_flags one
 * VAPOR_HF_* byte per hit (may be NULL), hit_off[n_sel+1] the offsets.  VAPOR_E_OVERFLOW
 * with hit_off[n_sel] = required capacity if `capacity` (in hits) is too small.
 */
int vapor_plan_fetch_hits(vapor_plan* plan, int64_t n_sel, const int64_t* pair_idx,
                          int32_t* hits_ji, uint8_t* hit_flags, int64_t capacity, int64_t* hit_off);

/* ---- per-read scores and per-locus results on the device ------------------------------------ */
/*
 * One read of one locus and the dot plots that score it.  kind 1: abs_dis_m1b (SF:182-203) on pairs
 * (ref_a, alt_a); 2: within_10Perc_m1b (SF:277-294); 3: directed_dis_m1b_redefine_diagnal
 * (SF:241-257); 0: a deletion read - abs_dis_m1b on (ref_a, alt_a) and within_10Perc_m1b on
 * (ref_b, alt_b), the smaller score wins (SF:1718-1726).  len_ref / len_alt are the full allele
 * lengths the gates divide by, taken as given (they are not compared with the sequences) and at least 1: the
 * reference divides by zero at 0.  A scorer whose pair failed (word 15 of its record is not 0) scores nothing, so
 * the read is skipped - a deletion read keeps the score of its other scorer.  Reads must be sorted by locus.
 */
typedef struct vapor_read {
    int32_t ref_a, alt_a, ref_b, alt_b;
    int32_t kind, locus, len_ref, len_alt;
} vapor_read;

#define VAPOR_GT_TABLE_N 65
#define VAPOR_LOCUS_STRIDE 8 /* doubles per locus: QS, GS, GT (0 = 0/0, 1 = 0/1, 2 = 1/1), GQ, reads scored,
                                positive scores, scores that round to <= 0, reserved; all NaN but [4] = 0 for an 'NA' locus */
/* gt_table[(k * 65 + l) * 2 + {0,1}] = genotype index and quality for k scored reads of which l round to
 * <= 0 (gt_estimate_log_likelihood SF:2054-2069, evaluated by the host with the reference's float64 steps).
 * What a read is refused for and in which order, and what the device is handed: DESIGN.md 4.11-host (csrc/vapor_finish_plan.h). */
int vapor_plan_set_reads(vapor_plan* plan, int64_t n_reads, const vapor_read* reads, int64_t n_loci,
                         const double* gt_table);
/* join -> clean -> per-read scores (SF:1718-1726 etc.) -> result_organize_ins (SF:1219-1231) ->
 * genotype, all on the device.  d_loci_out: device buffer (may be NULL) filled on the library's stream
 * before it is synchronised; loci_out / read_scores: host copies (may be NULL; a skipped read is NaN).
 * Which path a run takes and when it is repeated: DESIGN.md 4.11-host. */
int vapor_plan_run_loci(vapor_plan* plan, void* d_loci_out, double* loci_out, double* read_scores);
/*
 * The same run without a host round trip per step.  vapor_plan_run_loci_async only enqueues join -> clean -> finish
 * (with 64 steps in flight it waits for them first; the plan must have run once through vapor_plan_run_loci, which
 * sizes the record slots); vapor_plan_sync waits, makes vapor_plan_timings report the averages over those steps,
 * copies the last step's records to loci_out (may be NULL) and returns VAPOR_E_OVERFLOW if a pair outgrew its slot
 * in one of them.
 * Streams: every plan keeps to one of two streams the context owns, dealt out in turn, so the steps of two plans in
 * flight overlap on the device (a caller that works through a sequence of batches gets this by keeping two plans
 * alive: the reference's loop over loci, vapor_vali/vapor:334-367, has no such stage).  The finish kernel of a step
 * goes to a third, high-priority stream: the plan's next join does not wait for it, its next clean kernels do, and
 * vapor_plan_then / vapor_plan_sync see it through the step's end event.  vapor_plan_then makes a
 * stream of the caller's wait, on the device, for the plan's most recently enqueued step (e.g. before a
 * collective that reads d_loci_out); vapor_plan_after makes the plan's next step wait for what the caller has
 * enqueued on its stream so far (before d_loci_out is overwritten).  vapor_set_stream makes the library enqueue
 * everything on the caller's HIP stream instead (NULL: back to its own streams).
 * What vapor_plan_run_loci_async refuses before it enqueues anything: DESIGN.md 4.11-host.
 */
int vapor_set_stream(vapor_ctx* ctx, void* hip_stream);
int vapor_plan_run_loci_async(vapor_plan* plan, void* d_loci_out);
int vapor_plan_then(vapor_plan* plan, void* hip_stream);
int vapor_plan_after(vapor_plan* plan, void* hip_stream);
int vapor_plan_sync(vapor_plan* plan, double* loci_out);

/* ---- breakpoint refinement: a grid of candidate breakpoints per locus (`--refine`) --------- */
/*
 * Not in the reference: a call whose breakpoints are tens of bases off is scored at a grid of candidate
 * breakpoints around it - one window, one set of reads, every candidate allele a derived sequence of the window - and the best
 * candidate is chosen on the device.  The plan's "loci" (vapor_plan_set_reads) are then the CANDIDATES; vapor_plan_set_grid says
 * which consecutive loci belong to one refined locus: group g = loci first_locus[g] .. first_locus[g + 1], 1 to
 * VAPOR_MAX_CANDIDATES of them, the first the call itself, all with the same number of reads (the group's reads, in one order);
 * first_locus[0] = 0 and first_locus[n_groups] = n_loci.  The rule (vapor_amd/refine.py, pick): a candidate is eligible when it
 * scored at least one read and at least as many as the group's first; among those the largest GS, then the largest QS, then the
 * lowest index; the first when none is eligible.  A NaN never beats a number.
 * vapor_plan_run_grid: vapor_plan_run_loci followed on the same stream, with no host step in between, by that choice
 * (grid_pick_kernel, one wavefront a group).  winner_idx[g] = the winner's index in its group; group_out[16 g ..] = the winner's
 * VAPOR_LOCUS_STRIDE doubles, then those of the group's first candidate; winner_scores[score_off[g] .. score_off[g + 1]) = the
 * winner's per-read scores (NaN: a skipped read); score_off (n_groups + 1 entries) is filled by the call.  Any of the four may
 * be NULL.  Only these cross the link, not the candidates' records and scores.
 * What vapor_plan_set_grid and vapor_grid_pick refuse a grid for and in which order, and the block the device is handed:
 * DESIGN.md 4.11-host (csrc/vapor_finish_plan.h).
 */
#define VAPOR_MAX_CANDIDATES 128 /* per group: one wavefront holds a group with two candidates per lane */
int vapor_plan_set_grid(vapor_plan* plan, int64_t n_groups, const int32_t* first_locus);
int vapor_plan_run_grid(vapor_plan* plan, int32_t* winner_idx, double* group_out, double* winner_scores, int64_t* score_off);
/* The same choice on the caller's own tables (host arrays in and out, one call): records = VAPOR_LOCUS_STRIDE doubles per
 * candidate, candidate c's per-read scores = read_scores[read_first[c] .. read_first[c + 1]) (read_first[0] = 0), the groups and
 * the four outputs as above. */
int vapor_grid_pick(vapor_ctx* ctx, int64_t n_groups, const int32_t* first_locus, const double* records, const int32_t* read_first,
                    const double* read_scores, int32_t* winner_idx, double* group_out, double* winner_scores, int64_t* score_off);

/* ---- one-shot conveniences over the above -------------------------------------------------- */
/* dotdata for a batch (create + run + fetch all + destroy). */
int vapor_dotplot_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs,
                        int32_t* hits_ji, int64_t hits_capacity, int64_t* hit_off, int64_t* stats);
/* statistics only (create + run + destroy). */
int vapor_score_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs,
                      int64_t* stats);
/* Integer part of window_size_refine's quality check (SF:2030-2046, SF:1154-1171): the self dot
 * plot dotdata(k, seq, seq) of each listed sequence; out[3*t..] = n_hits, n_diag, n_lower. */
int vapor_selfplot_qc(vapor_ctx* ctx, vapor_seqset* set, int32_t n, const int32_t* seq_idx,
                      const int32_t* k, int64_t* out);

/*
 * Cleaning and reductions on caller-supplied dot lists, for callers that hold an explicit
 * list the way clean_dotdata_diagnal_and_anti_diagnal (SF:432-448) and
 * clean_dotdata_diagnal_m1b / clean_dotdata_anti_diagnal_m1b (SF:404-430) are called:
 * list t is hits_ji[2*off[t] .. 2*off[t+1]) as (j, i) pairs, flags[t] VAPOR_PF_* (NULL = both).
 * stats as in vapor_plan_run; hit_flags (may be NULL) one VAPOR_HF_* byte per dot.
 */
int vapor_clean_hits(vapor_ctx* ctx, int64_t n_lists, const int32_t* hits_ji, const int64_t* off,
                     const uint32_t* flags, int64_t* stats, uint8_t* hit_flags);

/* ---- the wide route: sequences longer than VAPOR_MAX_SEQ_LEN ------------------------------- */
/*
 * The entry points above refuse a sequence longer than VAPOR_MAX_SEQ_LEN (their device records pack positions 16+16 bit).
 * These two take any pair they accept plus sequences up to VAPOR_MAX_WIDE_SEQ_LEN: one pair at a time, one dot per 8 bytes
 * (32-bit positions), the dot slot sized by a count pass, the cleaning's value bitmaps in HBM.  The results are those of the
 * narrow route for every pair both accept.
 *
 * vapor_wide_batch: the statistics record of every pair (as vapor_plan_run: VAPOR_ST_STATUS = VAPOR_E_ARG for a bad index,
 * an unsupported k or a sequence longer than VAPOR_MAX_WIDE_SEQ_LEN, VAPOR_E_KEYERROR as the reference raises it,
 * VAPOR_E_OVERFLOW for a pair with more than "max_pair_cap" dots - its count pass stops there, VAPOR_ST_RECORDS_NEEDED holds
 * the dots counted until then, more than the cap; the call itself
 * returns VAPOR_OK).  hits_ji (may be NULL) receives the dots of pair t as (j, i) int32 pairs at hit_off[t] .. hit_off[t+1]
 * in unspecified order inside a pair (dotdata's list is these sorted by (j, i)); hit_off (n_pairs + 1 entries, may be NULL
 * when hits_ji is) is always filled, and VAPOR_E_OVERFLOW is returned, with the statistics complete, when hit_off[n_pairs]
 * exceeds hits_capacity.
 * vapor_clean_hits_wide: vapor_clean_hits for lists whose coordinates lie in 0 .. VAPOR_MAX_WIDE_SEQ_LEN.
 */
int vapor_wide_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int64_t* stats,
                     int32_t* hits_ji, int64_t hits_capacity, int64_t* hit_off);
int vapor_clean_hits_wide(vapor_ctx* ctx, int64_t n_lists, const int32_t* hits_ji, const int64_t* off,
                          const uint32_t* flags, int64_t* stats, uint8_t* hit_flags);

/* ---- the any-k route: kmerhits at every k from 1 to VAPOR_MAX_ANY_K ------------------------- */
/*
 * kmerhits(seq1, seq2[off2:], k, 1, inversions) (SF:951-983) for any 1 <= k <= VAPOR_MAX_ANY_K, inversions unless the pair has
 * VAPOR_PF_FORWARD.  k <= 40: exact k-mer matches.  k > 40: the reference's edit-distance branch (SF:969-973) - allele k-mer j
 * matches every distinct read key (forward and, with inversions, reverse-complemented) within Levenshtein distance k / 10.
 * vapor_wide_batch's contract otherwise (sequences up to VAPOR_MAX_WIDE_SEQ_LEN, one pair at a time, the statistics record,
 * VAPOR_E_OVERFLOW past "max_pair_cap", hits_ji / hits_capacity / hit_off), except that the dots of a pair come in the
 * reference's list order: j ascending; for one j, k <= 40: the lookup list (i ascending, a k-mer equal to its own reverse
 * complement twice), k > 40: the keys in order of first insertion, each key's list in order.  A pair is refused with
 * VAPOR_E_ARG for k outside 1 .. VAPOR_MAX_ANY_K, and for VAPOR_PF_FORWARD over a derived sequence that holds a symbol outside
 * the folded alphabet (its bytes are not kept).  With inversions a seq1 of at least k symbols that holds a symbol outside
 * invert_base's alphabet is VAPOR_E_KEYERROR.
 */
int vapor_anyk_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int64_t* stats,
                     int32_t* hits_ji, int64_t hits_capacity, int64_t* hit_off);

/* ---- `--realign`: the banded edit distance of a read against an allele ------ */
/*
 * For every pair, with a = seq1 (n symbols) and b = seq2 from symbol off2 on (m symbols): the edit distance of a against b inside
 * the band |i - j| <= band, the start anchored at (0, 0), both ends free.  D[0][0] = 0; a cell (i, j) exists iff 0 <= i <= n,
 * 0 <= j <= m and |i - j| <= band; D[i][j] is the minimum over its existing predecessors of D[i-1][j-1] + (0 if a[i-1] matches
 * b[j-1] else 1), D[i-1][j] + 1 and D[i][j-1] + 1; d is the minimum of D over the existing cells of the last row (i = n) and of
 * the last column (j = m).  Symbols are the codes of the 4-bit plane: two match iff both are A, C, G or T in either case and the
 * same base - case never matters; N, an IUPAC code and any other byte match nothing, not even themselves.
 * out[2t] = d, out[2t + 1] = 0 for pair t; its k and flags are ignored.  A pair with a bad index, off2 outside 0 .. len(seq2)
 * or a sequence longer than VAPOR_MAX_SEQ_LEN gets out[2t] = -1 and out[2t + 1] = VAPOR_E_ARG, and the call still returns
 * VAPOR_OK.  The call itself returns VAPOR_E_ARG for a band outside 1 .. VAPOR_MAX_BAND or n_pairs < 0; n_pairs == 0 is
 * VAPOR_OK.  Any sequence set will do - bytes, derived sequences, the device-held BAM bases of vapor_seqset_create_mixed - since
 * only the 4-bit plane and the lengths are read.  One upload of the pair table, one launch (realign_kernel: one wavefront a
 * pair), one copy back, on the context's stream; the call returns when out is filled.  A library without a device (the CPU twin
 * of the tests, whose oracle/ sources do not get the entry) exports the name and refuses every call with VAPOR_E_ARG; there is no
 * host route: a caller without the kernel has no `--realign`.
 */
#define VAPOR_MAX_BAND 512
int vapor_realign_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band, int32_t* out);

/* ---- `--realign-out`: the alignment behind the distance --------------------- */
/*
 * For every pair, with a, n, b, m, the matrix D and d as vapor_realign_batch has them: one alignment of cost d, by a rule.
 * End cell: of the existing cells of the last row and of the last column whose D equals d, the one with the largest i, among
 * those the one with the largest j.  Walk from it back to (0, 0); at (i, j) take the diagonal predecessor if it exists and
 * D[i-1][j-1] + sub == D[i][j] (op '=' where the symbols match, 'X' where not), otherwise the vertical one if it exists and
 * D[i-1][j] + 1 == D[i][j] (op 'I': a read symbol against nothing), otherwise the horizontal one (op 'D': an allele symbol
 * skipped); row 0 is all horizontal.  The path reversed and run-length encoded is the pair's trace; the n - i_end read symbols
 * behind the end cell are soft-clipped and are no run.
 * head[8t ..] = {d, status, i_end, j_end, n_runs, 0, 0, 0}.  runs holds cap_runs words a pair; a run is len << 2 | op with op
 * 0 '=', 1 'X', 2 'I', 3 'D'; the runs of pair t are the LAST n_runs words of runs[t * cap_runs .. (t + 1) * cap_runs), in path
 * order, and what stands in front of them is unspecified.  A pair whose trace needs more than cap_runs runs gets status
 * VAPOR_E_OVERFLOW: its d, i_end and j_end are right, n_runs is the count it needs, its words are unspecified.  A pair that
 * vapor_realign_batch refuses gets d = -1 and status VAPOR_E_ARG here too, and the call still returns VAPOR_OK; d of every pair
 * is vapor_realign_batch's.  The call returns VAPOR_E_ARG where vapor_realign_batch does and for cap_runs < 1; n_pairs == 0 is
 * VAPOR_OK.  The forward pass keeps two bits a cell of the band: rows_walked * 256 bytes a pair up to band 288, twice that
 * above.  The pairs run in consecutive groups whose workspaces fit vapor_set_param(ctx, "trace_budget", bytes) - 512 MiB unless
 * set, never below the 64 MiB that hold the largest pair; a lower value is raised to that.  One upload, per group two kernels
 * (realign_trace_kernel, traceback_kernel: one wavefront a pair each), the copies back and one synchronisation, on the
 * context's stream.  A library without a device exports the name and refuses every call with VAPOR_E_ARG; there is no host route.
 */
int vapor_realign_trace(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band,
                        int32_t cap_runs, int32_t* head, uint32_t* runs);

/* ---- `--realign-polish`: the consensus of a locus's reads on its allele ------ */
/*
 * The pairs of locus g are first[g] .. first[g + 1] (n_loci + 1 ascending int64 from 0 to n_pairs); all of them name the same
 * seq2, the locus's allele of len symbols, whose columns 0 .. len - 1 are col_off[g] .. col_off[g + 1] of the call's columns
 * (n_loci + 1 ascending int64 from 0).  Every pair's trace (vapor_realign_trace's, with slots that always hold it) is walked
 * from (0, 0), the column of allele symbol j being off2 + j: a leading 'D' run is no coverage; an '=' or 'X' step adds 1 to the
 * column's counter A, C, G or T by the read symbol's base, O for a read symbol that is none; a later 'D' step adds 1 to Dl;
 * every covered column but the pair's first adds 1 to bcov; an 'I' run strictly inside the pair's coverage adds 1 to ins of
 * the column it lies before.  A column with cov = A + C + G + T + O + Dl >= 3 whose largest of A, C, G, T, Dl holds a strict
 * majority of cov is called as that (a base equal to the allele's is KEEP); a column q >= 1 with bcov >= 3 and 2 * ins > bcov is
 * an insertion site, the first 256 of a locus are kept, and position r < 64 of a site's text is the base most inserted there
 * (the smallest code on a tie) while more than half of bcov insert one.
 * stats[8g ..] = {status, pairs piled, columns with cov >= 3, substitutions, deletions, sites kept, inserted bases, sites
 * dropped}.  calls: one byte a column, 0 .. 3 a substituted base, 4 KEEP, 5 DELETE, bit 3 set when a kept site lies before the
 * column.  sites: 256 slots a locus of {column, bases}; ins: 64 bytes a slot, the inserted text in upper case, 0 behind it.
 * counts (may be NULL): eight uint32 a column, A C G T O Dl bcov ins.
 * A locus whose pairs name different seq2, whose columns are not its allele's length or one of whose pairs vapor_realign_batch
 * refuses gets status VAPOR_E_ARG; one whose trace workspace alone exceeds "trace_budget" VAPOR_E_NOMEM: zero statistics, every
 * column KEEP, the other loci are served.  A locus without pairs has status 0 and every column KEEP.  The call returns
 * VAPOR_E_ARG where vapor_realign_batch does, for tables that do not ascend from 0, a `first` that does not end at n_pairs and a
 * locus of more than VAPOR_MAX_SEQ_LEN columns; n_loci == 0 is VAPOR_OK.  Consecutive whole loci run in groups whose device
 * buffer - trace rows, run slots, counters and site tables - fits "trace_budget"; per group one clear and six kernels
 * (realign_trace_kernel, traceback_kernel, pileup_kernel, consensus_kernel, pileup_ins_kernel, insert_kernel) back to back, then
 * the copies back; one synchronisation a call.  Neither the trace rows nor the runs cross the link.  A library without a device
 * exports the name and refuses every call with VAPOR_E_ARG; there is no host route.
 */
int vapor_realign_polish(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band, int64_t n_loci,
                         const int64_t* first, const int64_t* col_off, int32_t* stats, uint8_t* calls, int32_t* sites, uint8_t* ins,
                         uint32_t* counts);

/* ---- `--realign-revote`: every read against the polished allele ------------- */
/*
 * vapor_realign_polish, and behind it, without a round trip, a second alignment.  The arguments up to `counts`, their results,
 * refusals and groups are vapor_realign_polish's, bit for bit.
 * Spelling, on plane codes (A C G T 0..3, a c g t 4..7, N / IUPAC 8, their lower case 9, other 15): the flagged columns of a locus
 * (call bit 3) are numbered k = 0, 1, .. in column order; for q ascending a flagged column emits the sites[k][1] bases of ins[k]
 * as codes 0..3, then every column emits its own symbol - KEEP the allele's code unchanged, a call 0..3 that code, DELETE nothing.
 * start(q) counts the symbols emitted before column q's inserted text, own(q) = start(q) + (sites[k][1] if q is flagged else 0),
 * own(len) = plen.
 * The vote pairs of locus g are votes[vfirst[g] .. vfirst[g + 1]) (n_loci + 1 ascending int64 from 0 to n_votes): seq1 the read,
 * seq2 the locus's allele (its pairs' seq2; for a locus without pairs that of its first vote pair vapor_realign_batch accepts
 * whose seq2 has the locus's columns), off2 in the called allele's columns.  A read starts in the polished allele at
 * off2' = own(off2); d_pol is vapor_realign_batch's d of the read against the polished symbols from off2' on, m' = plen - off2'.
 * vout[4 t ..] = {d_pol, status, off2', m'}; lout[4 g ..] = {vstatus, plen, 0, 0}.  vstatus is the polish status where that is
 * not 0 (and VAPOR_E_ARG for a locus that has no allele), with plen 0; VAPOR_E_ARG for plen > VAPOR_MAX_SEQ_LEN.  The vote pairs of
 * a locus whose vstatus is not 0 get {-1, vstatus, 0, 0}; a vote pair vapor_realign_batch would refuse, or whose seq2 is not the
 * locus's allele, gets {-1, VAPOR_E_ARG, 0, 0} while the others are served (off2 == len is legal: m' = 0).  A locus without vote
 * pairs is spelt all the same; n_votes == 0 is legal.
 * spelt (may be NULL): spelt_off holds n_loci + 1 ascending int64 from 0, and the plen codes of locus g are written one a byte
 * from spelt_off[g] on; a slot of fewer than len + 64 * min(256, len) bytes gives the locus vstatus VAPOR_E_ARG and writes
 * nothing, its polish part is served.
 * The call returns VAPOR_E_ARG where vapor_realign_polish does, for n_votes outside 0 .. 2^26, a vfirst that does not ascend from
 * 0 to n_votes and a spelt_off that does not ascend from 0.  Per locus the group's buffer also holds own[], one byte a spelt
 * symbol and the polished 4-bit plane, charged to "trace_budget"; per group three more kernels behind insert_kernel
 * (spell_kernel, spell_pack_kernel, realign_onto_kernel), still one synchronisation a call.  The polished allele never crosses
 * the link.  A library without a device exports the name and refuses every call with VAPOR_E_ARG; there is no host route.
 */
int vapor_realign_revote(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band, int64_t n_loci,
                         const int64_t* first, const int64_t* col_off, int32_t* stats, uint8_t* calls, int32_t* sites, uint8_t* ins,
                         uint32_t* counts, int64_t n_votes, const vapor_pair* votes, const int64_t* vfirst, int32_t* vout, int32_t* lout,
                         const int64_t* spelt_off, uint8_t* spelt);

/* ---- `--realign-junction`: the one jump between two sequences --------------- */
/*
 * Per pair: s = seq1 (ns symbols) and l = seq2 (nl symbols), ns <= nl, off2 == 0; symbols, matching, the band and D are
 * vapor_realign_batch's.  The row table T(s, l) has rows i = 0 .. ns: f(i) the minimum of D[i][j] over the existing cells of
 * row i (|i - j| <= band, 0 <= j <= nl; D of s[0:i] against l[0:j], anchored at (0, 0)), jf(i) the smallest j that attains it.
 * With F = T(s, l) and R = T(reversed s, reversed l), split row i has j1 = jf_F(i), j2 = nl - jf_R(ns - i) and
 * cost = f_F(i) + f_R(ns - i); it is valid iff j2 >= j1 (row 0 always is).  The junction is the valid row with the smallest
 * (cost, i): s is l with l[j1 : j2) skipped at row i, at `cost` further edits.
 * out[8 t ..] = {status, cost, i, j1, j2, f_F(i), f_R(ns - i), 0}.  rows may be NULL; otherwise row_off holds n_pairs + 1
 * ascending int64 from 0, and the ns + 1 rows of pair t are written from row row_off[t] on, four int32 a row:
 * {f_F, jf_F, f_R, jf_R}, each pass's two indexed by that pass's own row.  The rows of a refused pair are not written.
 * A bad index, a sequence longer than VAPOR_MAX_SEQ_LEN, off2 != 0, len(seq1) > len(seq2) or (rows given) a slot of fewer than
 * ns + 1 rows gives the pair status VAPOR_E_ARG and a record that is zero behind it; the other pairs are served.  The call
 * returns VAPOR_E_ARG where vapor_realign_batch does and for a row_off that does not ascend from 0, VAPOR_E_NOMEM when the pairs'
 * tables (16 (ns + 1) bytes each) exceed "trace_budget", VAPOR_OK for n_pairs == 0.  One upload, two launches
 * (junction_rows_kernel: a wavefront per pair and direction, the backward one reading both sequences from their last symbol;
 * junction_pick_kernel: a wavefront per pair), the copies back, one synchronisation.  A library without a device exports the
 * name and refuses every call with VAPOR_E_ARG; there is no host route.
 */
int vapor_realign_junction(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band, int32_t* out,
                           const int64_t* row_off, int32_t* rows);

/*
 * Host helper of the read extraction (cigar2alignstart_by_pos, SF:309-337; no device involved): walks the CIGAR of
 * an alignment starting at align_start until the reference cursor passes start-1; out[0] = offset into the read,
 * out[1] = miss_bp.  VAPOR_E_ARG if the CIGAR holds no operation (IndexError in the reference).
 */
int vapor_cigar2alignstart(const char* cigar, int64_t align_start, int64_t start, int64_t* out);
/* the same over a BAM record's binary CIGAR (n_ops words, length << 4 | operation code in "MIDNSHP=X" order) */
int vapor_cigar2alignstart_ops(const uint32_t* ops, int64_t n_ops, int64_t align_start, int64_t start, int64_t* out);

/*
 * Host helpers of the read extraction, no device involved: `samtools view bam chrom:start-end` piped into
 * chop_pacbio_read_by_pos (SF:339-354), which the reference runs as a process per locus, for one region of an open
 * BGZF/BAM file.  `chunks` are n_chunks (begin, end) virtual-offset pairs from the .bai index (the caller's lookup);
 * their blocks are inflated by a few host threads, the records of reference `tid` walked in file order, each CIGAR
 * walked in binary form to `start` (CG:B,I long CIGARs included), and the reads the reference would keep - alignment
 * start <= start, miss_bp <= flank / 2, more than end - start - miss_bp bases left - are written as ASCII:
 * read r is seq_out[meta[4r] .. + meta[4r+1]), meta[4r+2] = miss_bp, its name the C string at names_out + meta[4r+3].
 * VAPOR_E_OVERFLOW with need[0..2] = bytes of sequence, bytes of names and reads required when a buffer is too small.
 */
typedef struct vapor_bam vapor_bam;
int vapor_bam_open(const char* path, vapor_bam** bam);
int vapor_bam_close(vapor_bam* bam);
int vapor_bam_set_threads(vapor_bam* bam, int32_t n_threads);
/* Read filter of an open handle (`--min-mapq Q`, `--exclude-flags F`), Q = min_mapq and F = exclude_flags:
 * A record is *filtered* iff `MAPQ < Q` or `(FLAG & F) != 0` - this is `samtools view -q Q -F F`; MAPQ 255 passes every Q.
 * A filtered record is treated as if it were not in the file.  It is skipped after the checks every record gets (record size,
 * inner layout, contig and position order) and before the first decision about keeping it, so it sets no status, raises no
 * error and counts towards no limit; a malformed record is still malformed.  The setting is a property of the handle:
 * vapor_bam_chop, _tagged, _haplotag, _right and the four vapor_bam_chop_device* calls made with it apply it.  A new handle
 * has (0, 0), which filters nothing.  VAPOR_E_ARG outside 0 <= min_mapq <= 255, exclude_flags <= 65535. */
int vapor_bam_set_filter(vapor_bam* bam, int32_t min_mapq, uint32_t exclude_flags);
/* De-duplication of molecules by QNAME (`--dedup-qname`), a property of the open handle like the read filter.
 * Two records are the same molecule iff their name keys are equal: b_0 .. b_{n-1} the QNAME bytes without the NUL,
 * h = n + sum_i (b_i + 1) * M^(i+1) mod 2^64 with M = 0x9E3779B97F4A7C15, key = the splitmix64 finaliser of h (csrc/vapor_names.h).
 * Rule W: among the records a reader keeps for one region (after the read filter), those with one key leave exactly one - the
 * one with the smallest ((FLAG & 0x900) != 0, record order): the first that is neither secondary nor supplementary, else the
 * first.  A dropped record is treated as if it were not in the file: it counts towards no list, limit, group or phase set.
 * vapor_bam_chop, _tagged, _haplotag, _right apply the rule before they write their outputs (with buffers too small, `need` holds
 * the sizes before it); the four vapor_bam_chop_device* calls run bam_dedup_kernel behind their chop kernel.  A region with more
 * than 256 kept records before the rule still comes back for the host route.  on: 0 or 1, else VAPOR_E_ARG; a new handle has 0. */
int vapor_bam_set_dedup(vapor_bam* bam, int32_t on);
const char* vapor_bam_last_error(void);
int vapor_bam_chop(vapor_bam* bam, int32_t tid, int64_t start, int64_t end, int64_t flank, int32_t n_chunks,
                   const uint64_t* chunks, uint8_t* seq_out, int64_t seq_cap, char* names_out, int64_t names_cap,
                   int64_t* meta, int32_t max_reads, int32_t* n_reads, int64_t* need);
/*
 * The same with the haplotype tags of a haplotagged BAM (`--phased`; not in the reference, which reads nothing behind SEQ,
 * SF:339-354): six numbers per read in `meta` - read r is seq_out[meta[6r] .. + meta[6r+1]), meta[6r+2] = miss_bp, its name at
 * names_out + meta[6r+3], meta[6r+4] = hap, meta[6r+5] = ps.  hap = the value of the record's first HP aux field of integer
 * type (c C s S i I) if that is 1 or 2, else 0; ps = the value of its first PS aux field of integer type (I values up to
 * 2^32 - 1 exactly), INT64_MIN without one.  The aux walk ends at the first malformed field; what it found before stands.
 * minimize_pacbio_read_list (SF:1091-1102) is applied per group by the caller (vapor_amd/phase.py select).
 */
int vapor_bam_chop_tagged(vapor_bam* bam, int32_t tid, int64_t start, int64_t end, int64_t flank, int32_t n_chunks,
                          const uint64_t* chunks, uint8_t* seq_out, int64_t seq_cap, char* names_out, int64_t names_cap,
                          int64_t* meta, int32_t max_reads, int32_t* n_reads, int64_t* need);
/*
 * vapor_bam_chop_tagged for a file that is NOT haplotagged (`--phase-vcf`; not in the reference, which reads nothing behind SEQ,
 * SF:339-354): hap and ps of every kept read are made from the phased heterozygous SNVs of the locus, and the record's own HP /
 * PS fields are not read.  The n_sites sites of the locus - those of its contig within VAPOR_PHASE_REACH of [start, end] - come
 * in position order, none twice: site_pos (1-based), site_a1 / site_a2 = what haplotype 1 / 2 carries as a BAM 4-bit code
 * (A C G T = 1 2 4 8), site_ps = the site's phase set.  The record's operations (the CG:B,I array where it has the long-CIGAR
 * form) are walked with SAM's cursors, not cigar2alignstart_by_pos's: M = X advance reference and query, I S the query, D N the
 * reference, H P neither.  A site inside an M, = or X operation reads its base of SEQ: a1 is one vote for haplotype 1 in the
 * site's phase set, a2 one for haplotype 2, anything else none.  Among the phase sets with a vote the one with the most votes
 * decides (ties to the smallest value): hap = 1 or 2 by its majority; on a tie or without a vote hap = 0 and ps = INT64_MIN.
 * `meta` as in vapor_bam_chop_tagged; minimize_pacbio_read_list (SF:1091-1102) is the caller's, per group.
 */
#define VAPOR_PHASE_REACH 100000
int vapor_bam_chop_haplotag(vapor_bam* bam, int32_t tid, int64_t start, int64_t end, int64_t flank, int32_t n_chunks,
                            const uint64_t* chunks, uint8_t* seq_out, int64_t seq_cap, char* names_out, int64_t names_cap,
                            int64_t* meta, int32_t max_reads, int32_t* n_reads, int64_t* need, int32_t n_sites,
                            const int64_t* site_pos, const uint8_t* site_a1, const uint8_t* site_a2, const int64_t* site_ps);
/* vapor_bam_chop for the right-anchored reads of the window (vapor_bam_chop_device_right has the rule): the same outputs, every
 * read written as the reverse complement of its part that ends on the window end ("=ACMGRSVTWYHKDBN" complemented by reversing
 * the bits of a symbol's code), miss_bp counted from there. */
int vapor_bam_chop_right(vapor_bam* bam, int32_t tid, int64_t start, int64_t end, int64_t flank, int32_t n_chunks,
                         const uint64_t* chunks, uint8_t* seq_out, int64_t seq_cap, char* names_out, int64_t names_cap,
                         int64_t* meta, int32_t max_reads, int32_t* n_reads, int64_t* need);
/*
 * The read extraction of MANY regions on the DEVICE (vapor_amd/csrc/vapor_bamdev.h): what vapor_bam_chop does for one region on
 * host threads - and the reference as a `samtools view` process per locus piped into chop_pacbio_read_by_pos (SF:339-354) and
 * minimize_pacbio_read_list (SF:1091-1102) - for n_regions regions of the open file `bam` in one call.  Region g =
 * (tid[g], start[g], end[g], flank[g]); its .bai chunks are pairs chunk_first[g] .. chunk_first[g + 1] of `chunks` ((begin, end)
 * virtual offsets).  The host reads the chunks' BGZF blocks with positioned reads and sends them compressed; the device
 * inflates every block (one wavefront a block, CRC-32 checked against the block's trailer), walks the records of every region
 * (one wavefront a region) and keeps what the reference keeps.  Region g's kept reads - at most max_keep (<= 256), the
 * smallest miss_bp first, file order inside one value - are entries kept_first[g] .. kept_first[g + 1] of sq_addr (DEVICE
 * address of the record's packed bases, 4 bits each as BAM stores them), q0 (first base of the read's part) and miss (miss_bp);
 * the three have room for max_keep entries per region; the read is the end - start - miss_bp bases from q0 on
 * (vapor_seqset_create_mixed takes it as it lies).  status[g] = 0, or a positive code where the device leaves the region to
 * the host route (vapor_bam_chop, which also words the errors): a block whose Huffman code needs more table than the kernel
 * keeps, a damaged block, a record that runs past the chunk's blocks, a malformed record, a record without CIGAR, a read offset
 * before the record's first base, more than 256 kept reads.  `batch` owns the inflated data the addresses point into: destroy it
 * (vapor_bam_batch_destroy) after the sequence sets made from them.  One host thread per context, as everywhere.
 */
typedef struct vapor_bam_batch vapor_bam_batch;
int vapor_bam_chop_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* start,
                          const int64_t* end, const int64_t* flank, const int32_t* chunk_first, const uint64_t* chunks,
                          int32_t max_keep, int32_t* kept_first, uint64_t* sq_addr, int64_t* q0, int64_t* miss, int32_t* status,
                          vapor_bam_batch** batch);
int vapor_bam_batch_destroy(vapor_bam_batch* batch);
/* The name keys (vapor_bam_set_dedup) of the n entries that the vapor_bam_chop_device or vapor_bam_chop_device_right call which
 * made `batch` returned, in their order: n must be that call's kept_first[n_regions].  VAPOR_E_ARG for a batch made with a handle
 * that does not de-duplicate, for a batch of a _tagged / _haplotag call, and for another n. */
int vapor_bam_batch_name_keys(vapor_bam_batch* batch, int64_t n, uint64_t* keys);
/*
 * vapor_bam_chop_device for a haplotagged file (`--phased`; not in the reference, whose chop_pacbio_read_by_pos, SF:339-354,
 * reads nothing behind SEQ, and whose minimize_pacbio_read_list, SF:1091-1102, is applied here per group).  The chop kernel also
 * walks the aux fields of every record it keeps, once, for hap and ps (vapor_bam_chop_tagged has the rule; a CG:B,I array is
 * found in the same walk); a second kernel, one wavefront a region, then makes the region's answer on the device: P = the ps
 * most frequent among the kept records with hap != 0 (ties to the smallest value, "none" below every number); group A = all
 * kept records, H1 / H2 = those with hap == 1 / 2 and ps == P; a group's list = at most max_keep of it, record order when the
 * group has no more, else the smallest miss_bp first, record order inside one value.  What comes back is the union of the three
 * lists in record order: entries kept_first[g] .. kept_first[g + 1] of sq_addr, q0 and miss (as above) and `member` - bits 0-2:
 * the read is in the list of A / H1 / H2; bits 8-15, 16-23, 24-31: its position in that list.  The four arrays have room for
 * 3 * max_keep entries per region.  phase_set[g] = P (INT64_MIN: none), tagged[g] = 1 when a kept record has hap != 0.  status[g]
 * as above; a record whose aux area is malformed leaves its region to the host route.  A library without a device (the CPU
 * twin of the tests) does not have this entry: the caller's host readers select the groups.
 */
int vapor_bam_chop_device_tagged(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* start,
                                 const int64_t* end, const int64_t* flank, const int32_t* chunk_first, const uint64_t* chunks,
                                 int32_t max_keep, int32_t* kept_first, uint64_t* sq_addr, int64_t* q0, int64_t* miss,
                                 uint32_t* member, int64_t* phase_set, int32_t* tagged, int32_t* status, vapor_bam_batch** batch);
/*
 * vapor_bam_chop_device_tagged for a file that is not haplotagged (`--phase-vcf`; chop_pacbio_read_by_pos,
 * SF:339-354, and minimize_pacbio_read_list, SF:1091-1102, as there): the same answer, with hap and ps of every kept record made
 * on the device from the phased heterozygous SNVs of its region (vapor_bam_chop_haplotag has the rule) and the records' own HP /
 * PS fields not read.  The chop kernel stores the place of every kept record's operations; bam_haplotag_kernel, one wavefront a
 * kept record, walks them 64 a step against the region's sites and writes the tags the select kernel reads.  Region g's sites
 * are entries site_first[g] .. site_first[g + 1] of `sites`, in position order, 8 bytes each: int32 pos (1-based), uint8 a1,
 * uint8 a2 (BAM 4-bit codes), uint8 index of the site's phase set in the region's own table, uint8 0.  That table is entries
 * ps_first[g] .. ps_first[g + 1] of ps_values, at most VAPOR_PHASE_SETS_DEVICE of them: a region with more (or with an index
 * outside its table, or sites out of order) is left to the host route with a status of its own, as is every region the device
 * hands back for the reasons above.  A library without a device does not have this entry.
 */
#define VAPOR_PHASE_SETS_DEVICE 64
int vapor_bam_chop_device_haplotag(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* start,
                                   const int64_t* end, const int64_t* flank, const int32_t* chunk_first, const uint64_t* chunks,
                                   int32_t max_keep, int32_t* kept_first, uint64_t* sq_addr, int64_t* q0, int64_t* miss,
                                   uint32_t* member, int64_t* phase_set, int32_t* tagged, int32_t* status, vapor_bam_batch** batch,
                                   const int32_t* site_first, const void* sites, const int32_t* ps_first, const int64_t* ps_values);
/*
 * vapor_bam_chop_device for the RIGHT-anchored reads of every region (`--both-ends`; not in the reference): the
 * alignments whose last reference base (POS + the M, = and D operations - 1) is at or behind the window end, walked from the far
 * end of the CIGAR (CG:B,I arrays included) - chop_pacbio_read_by_pos (SF:339-354) of the records as the reverse-complemented
 * contig holds them.  Same arguments, statuses and selection (SF:1091-1102) as vapor_bam_chop_device, but q1[t] is the base of
 * read t that its reverse complement STARTS with and miss[t] counts from the window end: with src_kind 2,
 * vapor_seqset_create_mixed takes the read as the reverse complement of the end - start - miss[t] bases that end at q1[t].
 */
int vapor_bam_chop_device_right(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* start,
                                const int64_t* end, const int64_t* flank, const int32_t* chunk_first, const uint64_t* chunks,
                                int32_t max_keep, int32_t* kept_first, uint64_t* sq_addr, int64_t* q1, int64_t* miss,
                                int32_t* status, vapor_bam_batch** batch);
/*
 * Read depth (`--depth`; not in the reference).  A depth region is a contig and four bounds b0 <= b1 <= b2 <= b3,
 * 0-based: three consecutive half-open intervals [b0, b1) [b1, b2) [b2, b3), any of them empty.  A record counts iff it passes
 * the handle's read filter (vapor_bam_set_filter) with 0x704 - unmapped, secondary, QC-fail, duplicate - always among the
 * excluded flags; vapor_bam_set_dedup has no effect.  Of a counting record every M, = and X operation covers the reference bases
 * it spans; D and N move the reference cursor and cover nothing; I S H P do neither; a CG:B,I array replaces its two-operation
 * stand-in; a record without operations covers nothing.  cov[i] = the sum over those operations of their overlap with interval i.
 * vapor_bam_depth: one region on the host, `chunks` its .bai chunks (sorted and merged: a record is met once) as in
 * vapor_bam_chop; errors as there.  VAPOR_E_ARG for bounds that do not ascend from 0, b3 >= 2^31 or tid < 0.
 * vapor_bam_depth_device: n_regions regions in one call as vapor_bam_chop_device takes them (bounds: four a region, cov: three
 * a region) - their blocks inflated on the device, bam_depth_kernel, one wavefront a region.  status[g] = 0, or a positive code
 * of vapor_bam_chop_device's where the region is the host route's (its cov are 0 then).  Nothing stays on the device.
 */
int vapor_bam_depth(vapor_bam* bam, int32_t tid, const int64_t* bounds, int32_t n_chunks, const uint64_t* chunks, uint64_t* cov);
int vapor_bam_depth_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* bounds,
                           const int32_t* chunk_first, const uint64_t* chunks, uint64_t* cov, int32_t* status);
/*
 * Split-read and CIGAR evidence (`--signatures`; not in the reference).  A signature region is a contig and nine
 * fields: w0, w3 (the walk window [w0, w3), 0-based), x0, x1 (the two targets), tol (0..255), min_clip, nmin, nmax, mask.  A
 * record counts as for vapor_bam_depth (the handle's filter with 0x704 among the excluded flags; vapor_bam_set_dedup has no
 * effect; a CG:B,I array replaces its stand-in; a record without operations has no event).  Its events: LCLIP at POS when the S/H
 * operations among its first two sum to min_clip or more, RCLIP at its reference end likewise from its last two (a record of at
 * most two operations, all S/H, has neither); GAP(a, n) per D or N and INSOP(a, n) per I of length n at reference cursor a.
 * mask bit 0: LCLIP at x0, 1: RCLIP at x0, 2: LCLIP at x1, 3: RCLIP at x1 (|coordinate - x| <= tol), 4: GAP (nmin <= n <= nmax,
 * |a - x0| <= tol, |a + n - x1| <= tol), 5: INSOP (nmin <= n <= nmax, x0 - tol <= a <= x1 + tol).  out, ten a region: the six
 * counts, then offset and count of the mode of each target's histogram of offsets (largest count, then smallest |offset|, then
 * the negative one; 0 and 0 without an event).
 * vapor_bam_signature: one region on the host, `chunks` its .bai chunks as in vapor_bam_depth; errors as there.  VAPOR_E_ARG for
 * w0 < 0, w0 > w3, w3 >= 2^31, tol outside 0..255, nmin > nmax or tid < 0.
 * vapor_bam_signature_device: n_regions regions in one call as vapor_bam_depth_device takes them (regions: nine a region, out:
 * ten a region) - bam_signature_kernel, one wavefront a region.  status[g] = 0, or a positive code of vapor_bam_chop_device's
 * where the region is the host route's (its words are 0 then).  Nothing stays on the device.
 */
int vapor_bam_signature(vapor_bam* bam, int32_t tid, const int64_t* fields, int32_t n_chunks, const uint64_t* chunks, int64_t* out);
int vapor_bam_signature_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* regions,
                               const int32_t* chunk_first, const uint64_t* chunks, int64_t* out, int32_t* status);
/*
 * Split reads joined through their SA tags (`--links`; not in the reference).  A link region is a contig and
 * eleven fields: w0, w3 (the walk window [w0, w3), 0-based), x (the local target), y (the partner target), tol (0..255),
 * min_clip, ev (0: LCLIP, 1: RCLIP), pend (0: the entry's a, 1: its b), rel (0: the entry's strand is the record's, 1: it is the
 * other), name_off, name_len (the partner contig's name, bytes [name_off, name_off + name_len) of `names`, one blob for all the
 * regions of a call).  A record counts and has clip events as for vapor_bam_signature.  A clip record has event ev with
 * |coordinate - x| <= tol.  Its entries are the well-formed pieces of the value of its first aux field named SA, when that is of
 * type Z - rname,pos,strand,CIGAR,mapQ,NM; per piece, a = pos - 1, b = a + the lengths of M D N = X - with mapQ at or above the
 * handle's minimum MAPQ; an entry matches when its rname is the partner's name byte for byte, the strand relation holds and
 * |c - y| <= tol for c = a or b by pend.  out, five a region: n_clip, n_split (clip records with an entry), n_link (clip records
 * with a matching entry), then offset and count of the mode of the histogram of c - y of every linked record's first matching
 * entry (the tie rule of vapor_bam_signature).
 * vapor_bam_links: one region on the host, `chunks` its .bai chunks as in vapor_bam_depth; errors as there.  VAPOR_E_ARG for
 * w0 < 0, w0 > w3, w3 >= 2^31, tol outside 0..255, ev, pend or rel outside 0..1, an empty name or one outside `names`, tid < 0.
 * vapor_bam_links_device: n_regions regions in one call as vapor_bam_depth_device takes them (regions: eleven a region, out:
 * five a region) - bam_link_kernel, one wavefront a region; `names` is uploaded once.  status[g] = 0, or a positive code of
 * vapor_bam_chop_device's where the region is the host route's - a record whose aux area is malformed among them (its words are
 * 0 then).  Nothing stays on the device.
 */
int vapor_bam_links(vapor_bam* bam, int32_t tid, const int64_t* fields, const uint8_t* names, int64_t names_len, int32_t n_chunks,
                    const uint64_t* chunks, int64_t* out);
int vapor_bam_links_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* regions, const uint8_t* names,
                           int64_t names_len, const int32_t* chunk_first, const uint64_t* chunks, int64_t* out, int32_t* status);
/*
 * Alt and ref alignments per call (`--support`; not in the reference).  A support region is a contig and eleven
 * fields: the nine of a signature region with their meaning - w0, w3, x0, x1, tol, min_clip, nmin, nmax, mask - then flank (F,
 * 1..65535) and gmin (g, 1 or more); mask bit 6: reference support is asked at x0, bit 7: at x1.  A record counts and has events
 * as for vapor_bam_signature; every fact is per record.  With pos its 0-based start and q its reference end: cg - it has a GAP
 * or INSOP that vapor_bam_signature counts; clip_k (k = 0, 1) - it has a clip event that vapor_bam_signature counts at target k
 * (bits 2k, 2k + 1); blocked_k - a D or N of n >= g bases at cursor a with a < x_k + F and a + n > x_k - F, or an I of n >= g
 * bases at cursor a with x_k - F <= a <= x_k + F; span_k - pos <= x_k - F, q >= x_k + F and not blocked_k; cov_k - pos <= x_k < q.
 * out, seven a region: alt_cg (records with cg), alt_l (clip_0, not cg), alt_r (clip_1, not cg), ref_0 (bit 6, span_0, not cg, not
 * clip_0), ref_1 (bit 7, span_1, not cg, not clip_1), cov_0, cov_1 (whatever the mask).
 * vapor_bam_support: one region on the host, `chunks` its .bai chunks as in vapor_bam_depth; errors as there.  VAPOR_E_ARG for
 * what vapor_bam_signature refuses, flank outside 1..65535 or gmin < 1.
 * vapor_bam_support_device: n_regions regions in one call as vapor_bam_depth_device takes them (regions: eleven a region, out:
 * seven a region) - bam_support_kernel, one wavefront a region.  status[g] = 0, or a positive code of vapor_bam_chop_device's
 * where the region is the host route's (its words are 0 then).  Nothing stays on the device.
 */
int vapor_bam_support(vapor_bam* bam, int32_t tid, const int64_t* fields, int32_t n_chunks, const uint64_t* chunks, int64_t* out);
int vapor_bam_support_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* regions,
                             const int32_t* chunk_first, const uint64_t* chunks, int64_t* out, int32_t* status);
/* what the context's last vapor_bam_chop_device (or _tagged) did, for measurement (bench.py): out[0..6] = regions, BGZF blocks,
 * compressed bytes sent over the link, inflated bytes, the inflate kernel's duration between two events on its stream (ms), the
 * whole call (ms), bytes of kept reads and statuses copied back from the device */
int vapor_bam_last_stats(vapor_ctx* ctx, double* out, int32_t n);
/* the descriptor and the inflate-thread count of an open file (vapor_bam_chop_device reads with them) */
int vapor_bam_fileno(vapor_bam* bam);
int vapor_bam_threads(vapor_bam* bam);

/* Reference windows of a bgzipped FASTA on the device (the BGZF twin of `samtools faidx`, for a chunk of loci at once).  `fd` is
 * an open descriptor of the .fa.gz.  Window i is the raw FASTA text (newlines included) between the virtual offsets vbeg[i] and
 * vend[i] (compressed block offset << 16 | offset in the block's data), which the caller finds with the .fai and .gzi.  Every
 * distinct block is inflated once, however many windows hold it, and checked by its CRC-32.  The text of window i, without its
 * '\n' and '\r', is text[text_off[i] .. text_off[i + 1]) (text_off has n + 1 entries; text_cap bytes of room, the raw sizes'
 * sum always suffices); traits[i] = VAPOR_FASTA_TR_* bits of that text.  status[i] = 0, or a positive VAPOR_FASTA_* code where
 * the window is left to the host reader (its text is then empty): a damaged or non-BGZF block, offsets outside the blocks of
 * the file, a byte of 0x80 or more, no room (more than the call's block or text limits).  One host thread per context. */
#define VAPOR_FASTA_BLOCK 1
#define VAPOR_FASTA_RANGE 2
#define VAPOR_FASTA_NON_ASCII 3
#define VAPOR_FASTA_ROOM 4
#define VAPOR_FASTA_TR_LOWER 1            /* a byte in a-z */
#define VAPOR_FASTA_TR_NOT_ACGTN 2        /* a byte other than A C G T N */
#define VAPOR_FASTA_TR_NOT_ACGTN_ANY_CASE 4   /* a byte other than A C G T N a c g t n */
#define VAPOR_FASTA_TR_HIGH 8             /* a byte of 0x80 or more */
int vapor_fasta_windows_device(vapor_ctx* ctx, int fd, int32_t n, const uint64_t* vbeg, const uint64_t* vend, uint8_t* text,
                               int64_t text_cap, int64_t* text_off, uint8_t* traits, int32_t* status);
/* what the context's last vapor_fasta_windows_device did: out[0..5] = windows, distinct blocks inflated, compressed bytes read
 * and sent, inflated bytes, both kernels between two events on their stream (ms), the whole call (ms) */
int vapor_fasta_last_stats(vapor_ctx* ctx, double* out, int32_t n);
/*
 * vapor_seqset_create_derived for a set some of whose sequences are on the device already: src_kind[i] = 1 says seq[i] is the
 * DEVICE address of BAM-packed bases (4 bits a base, "=ACMGRSVTWYHKDBN", the first base of a byte in its high half) inside the
 * data of a live vapor_bam_batch of this context, and the sequence is the len[i] bases from base src_first[i] on; src_kind[i] = 0
 * (or src_kind == NULL): bytes on the host, as vapor_seqset_create_derived takes them.  Only the host bytes cross the link.
 * src_kind[i] = 2: a device source like 1, taken reverse complemented - the sequence is the complement (a symbol's 4-bit code
 * with its bits reversed: = and N stay) of base src_first[i], then of src_first[i] - 1, ... for len[i] bases
 * (len[i] <= src_first[i] + 1).
 * VAPOR_E_ARG for a device source that does not lie inside a live batch.
 */
int vapor_seqset_create_mixed(vapor_ctx* ctx, int32_t n_seqs, const uint8_t* const* seq, const int32_t* len, const uint8_t* flags,
                              const uint8_t* src_kind, const int64_t* src_first, int32_t n_derived, const int32_t* seg_first,
                              const vapor_segment* segs, const uint8_t* derived_flags, int32_t* seq_info, vapor_seqset** set);
/*
 * chop_pacbio_read_by_pos (SF:339-354) over n alignment records the caller holds in memory (no file, no device):
 * pos 1-based leftmost aligned base, ref_span the reference bases a record is taken to cover (the region rule of
 * `samtools view`), cigar[r] the record's CIGAR as text (a C string, walked only as far as the window start), seq_len the
 * read lengths.  keep[r] = 1 and q0_miss[2r], q0_miss[2r+1] = offset into the read and miss_bp for the reads the reference
 * would keep (POS < start + 1, miss_bp <= flank / 2, more than end - start - miss_bp bases from the offset on); the caller
 * slices.  VAPOR_E_ARG for a record without CIGAR operation (IndexError in the reference, SF:331).
 */
int vapor_chop_records(int32_t n, const int64_t* pos, const int64_t* ref_span, const char* const* cigar,
                       const int64_t* seq_len, int64_t start, int64_t end, int64_t flank, int64_t* q0_miss, uint8_t* keep);
/*
 * chop_pacbio_read_by_pos (SF:339-354) followed by minimize_pacbio_read_list (SF:1091-1102: at most max_keep reads, the smallest
 * miss_bp first, input order inside one miss_bp value) for MANY regions in one call (host, no device) - the read selection of a
 * whole batch of loci, which the reference runs as a samtools process and two Python loops per locus.  Region g looks at
 * n_rec[g] records given as vapor_chop_records' arrays (pos[g], ref_span[g], cigar[g], seq_len[g]: one pointer per region);
 * its kept reads are entries kept_first[g] .. kept_first[g + 1] of rec_idx (index into the region's records), q0 (offset into
 * the read) and miss (miss_bp); the three have room for max_keep entries per region.  addr_out (may be NULL, same room)
 * receives seq_addr[g][record] per kept read: the address of that record's sequence where the caller keeps it.  status[g] = VAPOR_E_ARG for a region
 * with a record without CIGAR operation (IndexError in the reference, SF:331), else 0.
 */
int vapor_chop_records_many(int32_t n_regions, const int32_t* n_rec, const int64_t* const* pos, const int64_t* const* ref_span,
                            const char* const* const* cigar, const int64_t* const* seq_len, const int64_t* start,
                            const int64_t* end, const int64_t* flank, int32_t max_keep, int32_t* kept_first, int32_t* rec_idx,
                            int64_t* q0, int64_t* miss, int32_t* status, const uint64_t* const* seq_addr, uint64_t* addr_out);
/*
 * The right-anchored forms of the two calls above (vapor_bam_chop_device_right has the rule): q1_miss[2r] / q1[] = the number of
 * bases to drop from the END of the read, miss_bp counted from the window end; the kept read is the reverse complement of the
 * end - start - miss_bp bases before the dropped ones.  The whole CIGAR text of a qualifying record is read.
 */
int vapor_chop_records_right(int32_t n, const int64_t* pos, const int64_t* ref_span, const char* const* cigar,
                             const int64_t* seq_len, int64_t start, int64_t end, int64_t flank, int64_t* q1_miss, uint8_t* keep);
int vapor_chop_records_right_many(int32_t n_regions, const int32_t* n_rec, const int64_t* const* pos, const int64_t* const* ref_span,
                                  const char* const* const* cigar, const int64_t* const* seq_len, const int64_t* start,
                                  const int64_t* end, const int64_t* flank, int32_t max_keep, int32_t* kept_first, int32_t* rec_idx,
                                  int64_t* q1, int64_t* miss, int32_t* status, const uint64_t* const* seq_addr, uint64_t* addr_out);
/*
 * The row tails of a whole output table in one call (host, no device): per locus t with read scores
 * scores[off[t] .. off[t+1]) what result_organize_ins (SF:1219-1231) and gt_estimate_log_likelihood (SF:2054-2069, reading
 * the rounded Rec string back, SF:2056) derive from them - n_pos[t] = scores > 0, qs[t] = their np.mean (numpy's pairwise
 * summation order; 0 when none), n_nonpos[t] = scores not > 0 after round(s, 2), and Rec = ','.join(str(round(s, 2))) as
 * text[text_off[t] .. text_off[t+1]) (ASCII, no terminator).  n_nonpos[t] = -1 where a score is not finite or at least 1e13
 * in size: the caller formats that locus itself.  VAPOR_E_OVERFLOW with text_off[n_loci] = bytes needed when text_cap is too
 * small.  Replaces the per-locus round -> str -> join -> split -> float of the reference's writer (SF:1229, 2056).
 */
int vapor_row_tails(int32_t n_loci, const int64_t* off, const double* scores, double* qs, int32_t* n_pos, int32_t* n_nonpos,
                    char* text, int64_t text_cap, int64_t* text_off);
/*
 * The block decoder of vapor_bam_chop by itself (host, no device): a raw DEFLATE stream (RFC 1951; the payload of a BGZF
 * block) of in_n bytes into exactly out_n bytes.  VAPOR_E_ARG for anything that is not such a stream (truncated, damaged,
 * another size); it reads and writes nothing outside the two buffers.  Replaces the inflate inside `samtools view`
 * (SF:342 runs it as a process per locus).
 */
int vapor_inflate_raw(const uint8_t* in, int64_t in_n, uint8_t* out, int64_t out_n);
/*
 * The CRC-32 (gzip polynomial) every inflated BGZF block is checked against its trailer with (host, no device), by itself:
 * carry-less-multiply folding where the CPU has it, table lookups for the rest and - tables_only != 0 - for everything.
 * 0 for an empty buffer.  Replaces the check inside `samtools view` (htslib verifies each block, SF:342 runs it per locus).
 */
uint32_t vapor_crc32(const uint8_t* data, int64_t n, int32_t tables_only);

#ifdef __cplusplus
}
#endif
#endif /* VAPOR_HIP_H */
