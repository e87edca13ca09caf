// vapor_hip.hip - host side of libvapor_hip.so: the C ABI declared in include/vapor_hip.h.
//
// Build (see vapor_amd/build.py):
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -shared -Iinclude vapor_amd/csrc/vapor_hip.hip
//
// Everything the GPU touches is resident in HBM between calls: a vapor_seqset holds the packed
// bit planes, a vapor_plan holds pair/task descriptors, the hit workspace and the statistics.
#include "vapor_kernels.h"
#include "vapor_wide.h"
#include "vapor_anyk.h"
#include "vapor_realign.h"
#include "vapor_realign_trace.h"
#include "vapor_polish.h"
#include "vapor_revote.h"
#include "vapor_polish_call.h"
#include "vapor_seqset_plan.h"
#include "vapor_junction.h"
#include "vapor_bamdev.h"
#include "vapor_bgzf.h"
#include "vapor_fasta.h"
#include "vapor_refine.h"
#include "vapor_finish_plan.h"
#include "vapor_planner.h"
#include "vapor_readplan.h"
#include "vapor_pool.h"
#include "vapor_hip.h"

#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <type_traits>
#include <array>
#include <atomic>
#include <chrono>
#include <vector>

using namespace vapor;

static thread_local std::string g_err;

static int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}
// a refusal of the plan headers (a code, and the message without the entry's name) as the entry's status
static int refused(const std::string& entry, const vapor_image::Refusal& no) { return fail(no.code, entry + ": " + no.msg); }

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(VAPOR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

// ------------------------------------------------------------------------------------------
// Device and pinned-host blocks are recycled inside a context: a caller that works through a sequence of batches
// creates and destroys a sequence set and a plan per batch, and a dozen hipMalloc / hipHostMalloc / hipFree calls per
// batch cost more than the batch's kernels.  Freed blocks go to a per-context free list (by capacity) and are handed
// out again to requests of similar size; vapor_destroy releases them.  A set or plan that outlives its context
// frees its blocks directly.  Who gives a block back, and when it may: see CallScope / Block below the pool's functions.
// The pool's policy - rounding, the window a free block serves, the caching limits, the test fill - is vapor_pool.h's.
using vapor_pool::BlockPool;
static std::mutex g_live_m;
static std::set<const void*> g_live_ctx;

struct vapor_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;          // the stream vapor_init created (vapor_set_stream may replace `stream`)
    // vapor_plan_run_loci_async: every plan keeps to one of two library-owned streams ("lanes"), dealt out in turn, so
    // that the steps of two plans in flight overlap (the join owns every CU's LDS while it runs; the clean and finish
    // kernels of the other plan fill the CUs it has not reached or has already left).  A caller's stream
    // (vapor_set_stream) replaces both.
    hipStream_t lane[2] = {nullptr, nullptr};
    hipStream_t fin[2] = {nullptr, nullptr};   // per lane: the stream its plans' finish kernels go to (highest priority)
    unsigned lane_rr = 0;
    vapor_plan* lane_plan[2] = {nullptr, nullptr};   // per lane: the plan whose asynchronous step was enqueued last (join_table_for_async)
    bool user_stream = false;
    // staging for vapor_seqset_create*, kept between calls (pinned allocations are slow): ASCII chunks + chunk map
    uint8_t* h_stage = nullptr;
    uint8_t* d_stage = nullptr;
    size_t stage_cap = 0;
    // the genotype table of vapor_plan_set_reads, kept on the device while callers keep passing the same one
    std::vector<double> h_gt;
    double* d_gt = nullptr;
    int reads_per_task = MAX_READS_PER_TASK;   // upper bound on pairs per join task
    int n_cus = 256;
    int join_tasks = 256;                      // join tasks aimed for per launch (cost-balanced ranges): one per CU
    int join_align = 1;                        // which task table a run takes: 0 the cost-balanced one, 2 the window-aligned one, 1 by run (join_table_for_async)
    int64_t max_pair_cap = (int64_t)1 << 28;
    bool shared_join = true;                   // reads scored against a window and alleles derived from it: one join for all
    int remap_in_clean = 1;                    // ... and the clean workgroup of a target cuts its records out of the shared plot (0: remap_kernel)
    int clean_order = 1;                       // 1: the clean workgroups are dealt out longest pair first (clean_order); 0: in pair order
    int clean_fit = 1;                         // 1: after a blocking run the clean kernel's LDS copy is sized for the records the pairs really hold
    int64_t trace_budget = vapor_trace::BUDGET_DEFAULT;      // bytes of vapor_realign_trace's workspace (never below BUDGET_FLOOR)
    int64_t anyk_edit_pairs = ANYK_EDIT_PAIRS;  // (query, key) distances one launch of the any-k route's edit pass may hold (dots_plan::edit_cut)
    int stage_threads = 3;                     // host threads that copy a large upload into the pinned staging buffer (measured:
                                               // two to four are as fast as it gets, more are slower - tools/upload_sweep.py)
    bool attrs_set = false;
    // vapor_bam_chop_device: the CRC combination constants on the device, and the arenas of the batches that are alive
    // (vapor_seqset_create_mixed takes packed bases by device address: only addresses inside one of these are followed)
    uint32_t* d_crc_pow = nullptr;
    std::map<const uint8_t*, size_t> arenas;
    // the stream the extraction's copies and kernels go to: the context's own, or (parameter bam_cu_share = s of 8) one masked to
    // s eighths of the CUs, so that the kernels other contexts' threads launch meanwhile (packing, joins, cleaning) find CUs whose
    // LDS is not held by twenty inflating wavefronts (cli.py sets it when it scores several chunks at once: 25.5-26.8 k -> 27.5-30.5 k
    // loci/s from files at 5 of 8, profiles/r05_bamdev.txt)
    hipStream_t bam_stream = nullptr;
    int bam_stream_share = 0;                  // the share bam_stream was made for
    int bam_cu_share = 0;
    hipEvent_t bam_ev[2] = {nullptr, nullptr}; // around the inflate launch of the last vapor_bam_chop_device (vapor_bam_last_stats)
    double bam_stats[7] = {0, 0, 0, 0, 0, 0, 0};  // regions, blocks, compressed bytes, inflated bytes, inflate ms, whole call ms, bytes copied back
    hipEvent_t fasta_ev[2] = {nullptr, nullptr};   // around the kernels of the last vapor_fasta_windows_device (vapor_fasta_last_stats)
    double fasta_stats[6] = {0, 0, 0, 0, 0, 0};    // windows, distinct blocks, compressed bytes, inflated bytes, kernels ms, whole call ms
    BlockPool pool;
};

static bool ctx_alive(const vapor_ctx* c)
{
    std::lock_guard<std::mutex> g(g_live_m);
    return g_live_ctx.count(c) != 0;
}

// one host thread per context (include/vapor_hip.h), so the lists themselves need no lock
static hipError_t pool_alloc(vapor_ctx* c, void** out, size_t bytes, bool host)
{
    return (hipError_t)vapor_pool::take(
        c->pool, out, bytes, host,
        [](void** o, size_t cap, bool h) { return (int)(h ? hipHostMalloc(o, cap) : hipMalloc(o, cap)); },
        // (parameter pool_fill: the library's streams do not wait for the null stream, and the block may be used on any of them -
        // the fill is over when the device is idle)
        [](void* p, size_t cap, bool h, int byte) {
            if (h) { memset(p, byte, cap); return 0; }
            const hipError_t e = hipMemset(p, byte, cap);
            return (int)(e != hipSuccess ? e : hipDeviceSynchronize());
        });
}
static hipError_t dmalloc(vapor_ctx* c, void** out, size_t bytes) { return pool_alloc(c, out, bytes, false); }
static hipError_t hmalloc(vapor_ctx* c, void** out, size_t bytes) { return pool_alloc(c, out, bytes, true); }

static void pool_free(vapor_ctx* c, void* p, bool host)
{
    if (!p) return;
    vapor_pool::give(c && ctx_alive(c) ? &c->pool : nullptr, p, host, [](void* q, bool h) {
        if (h) (void)hipHostFree(q); else (void)hipFree(q);
    });
}
static void dfree(vapor_ctx* c, void* p) { pool_free(c, p, false); }
static void hfree(vapor_ctx* c, void* p) { pool_free(c, p, true); }

// Who gives a block back.  An object that outlives the call that made it (vapor_seqset, vapor_plan, vapor_bam_batch) owns its
// members and releases them in its destroy function; a create function that fails half-way hands the half-built object to
// that function by scope (Building<>).  A block whose life ends with the call that took it is a Block of that call's
// CallScope.  The rule, for every route: no block returns to the pool while work this call enqueued may still read or write
// it, and no host buffer that an enqueued copy reads or fills dies first.  A call that succeeds ends in a
// hipStreamSynchronize of its own and says so (settled()): unwinding adds nothing there.  A call that leaves early - a HIPCHK
// that fails, a refusal, an exception - has its stream synchronised by the first owner that unwinds.  So a function declares
// the host buffers that its copies use before its owners (which unwind first).  HIPCHK is the only check macro: with every
// owner on the stack, returning at once is always right.
struct CallScope {
    vapor_ctx* ctx;
    hipStream_t st;                            // the stream this call enqueues on
    bool pending = true;                       // work may be in flight (assumed until the call says otherwise)
    CallScope(vapor_ctx* c, hipStream_t s) : ctx(c), st(s) {}
    void settled() { pending = false; }        // the caller has just synchronised `st` and enqueues nothing more
    void settle()
    {
        if (pending) (void)hipStreamSynchronize(st);
        pending = false;
    }
};

// A device (or pinned host) block from the context's pool, given back when the handle goes out of scope.
template <typename T = uint8_t, bool HOST = false>
struct Block {
    CallScope* sc = nullptr;
    T* p = nullptr;
    size_t cap = 0;
    Block() = default;                         // (an array's element: its owner sets `sc`)
    explicit Block(CallScope& s) : sc(&s) {}
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    ~Block()
    {
        if (!p) return;
        sc->settle();
        pool_free(sc->ctx, p, HOST);
    }
    // Grow-only, the contents are not kept.  A block that grows goes back to the pool at once, without a synchronisation: the
    // caller grows a block only when nothing it has enqueued since its last synchronisation touches it.
    hipError_t ensure(size_t bytes)
    {
        if (cap >= bytes) return hipSuccess;
        pool_free(sc->ctx, p, HOST);
        p = nullptr;
        cap = 0;
        const hipError_t e = pool_alloc(sc->ctx, (void**)&p, bytes, HOST);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    operator T*() const { return p; }
};
template <typename T = uint8_t> using HostBlock = Block<T, true>;

// The deleter of a half-built set, plan or batch: std::unique_ptr<T, Building<T, destroy>> until the create function releases it.
template <typename T, int (*DESTROY)(T*)>
struct Building {
    CallScope* sc;
    void operator()(T* o) const
    {
        sc->settle();
        DESTROY(o);
    }
};

struct vapor_seqset {
    vapor_ctx* ctx = nullptr;
    int device = 0;                // kept here: the set may be destroyed after its context
    int32_t n = 0;                 // sequences the caller sees: n_lit given as bytes, then the derived ones
    int32_t n_lit = 0;
    std::vector<SeqDesc> h;        // host copy (with device-computed counts); hidden shared sequences behind the caller's
    SeqDesc* d_seqs = nullptr;
    uint32_t *d_p2 = nullptr, *d_e1 = nullptr, *d_x4 = nullptr;
    size_t plane_chunks = 0;
    std::vector<std::vector<HSeg>> derived;     // per derived sequence (index - n_lit)
    std::vector<ShareGroup> groups;
    std::vector<int32_t> group_of, slot_of;     // per caller-visible sequence: its group (-1: none) and slot in it
    // the bytes of the sequences given as bytes that hold a symbol outside invert_base's alphabet (the 4-bit plane keeps one
    // code for all of them; vapor_anyk_batch's forward pairs compare them byte for byte): sequence i at d_raw + raw_off[i], -1: none
    uint8_t* d_raw = nullptr;
    std::vector<int64_t> raw_off;
};

namespace fp = vapor::finish_plan;

// A plan's finishing state (vapor_finish_plan.h): the read table and the grid described over it, each the
// device's copy of its upload image, the blocks the kernels write, the counts and what the host keeps.  Members of the plan:
// release() gives the blocks back when a new table comes and in the plan's destroy function.
struct ReadTables {
    fp::ReadImage im;
    int64_t n_reads = 0, n_loci = 0;
    uint8_t* d_image = nullptr;           // reads | locus_first
    double* d_gt = nullptr;
    bool own_gt = false;                  // false: the context's cached table
    double* d_read_scores = nullptr;
    double* d_loci = nullptr;
    std::vector<int32_t> h_locus_first;   // host copy of d_locus_first()
    bool set() const { return d_image != nullptr; }
    const DRead* d_reads() const { return reinterpret_cast<const DRead*>(im.reads.in(d_image)); }
    const int32_t* d_locus_first() const { return im.locus_first.in(d_image); }
    void release(vapor_ctx* ctx)
    {
        dfree(ctx, d_image);
        if (own_gt) dfree(ctx, d_gt);
        dfree(ctx, d_read_scores);
        dfree(ctx, d_loci);
        *this = ReadTables();
    }
};
struct GridTables {                       // groups of consecutive loci, each one locus's candidates (grid_pick_kernel)
    fp::GridImage im;
    int64_t n_groups = 0, n_scores = 0;
    uint8_t* d_image = nullptr;           // first_locus | score_off | winner_idx
    double* d_group_out = nullptr;        // a group record a group
    double* d_winner_scores = nullptr;
    std::vector<int32_t> score_off;       // per group: its first slot among the winners' scores
    void release(vapor_ctx* ctx)
    {
        dfree(ctx, d_image);
        dfree(ctx, d_group_out);
        dfree(ctx, d_winner_scores);
        *this = GridTables();
    }
};

struct vapor_plan : PlanLayout {   // the layout the planner made (vapor_planner.h) and what the device holds of it
    vapor_ctx* ctx = nullptr;
    int device = 0;                // kept here: the plan may be destroyed after its context
    vapor_seqset* set = nullptr;
    int64_t n_pairs = 0;
    std::vector<int64_t> last_stats;
    int hcap_want = 4096;
    bool hcap_measured = false;                // hcap_want is the largest record count a blocking run saw (else: an estimate)
    int64_t total_cap = 0;
    DPair* d_pairs = nullptr;
    DTask* d_tasks = nullptr;
    DTask* d_atasks = nullptr;              // the window-aligned table (`atasks`), NULL when the plan was made with join_align 0
    int join_align = 0;                     // the context's parameter when the plan was made
    PlanParams params{};                    // ... and what the planner read of the context then
    bool aligned_made = false;              // join_align 1: `atasks` exists (made and uploaded by the first asynchronous step)
    int last_table = 0;                     // the table the last run took: 0 `tasks`, 1 `atasks`
    int32_t* d_task_pairs = nullptr;
    unsigned long long* d_hits = nullptr;   // run records (VREC_*), hp[].cap slots per pair
    uint8_t* d_hflags = nullptr;            // one flag byte per record
    unsigned long long* d_nhits = nullptr;
    long long* d_stats = nullptr;
    long long* h_stats = nullptr;  // pinned
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_f[2] = {nullptr, nullptr};
    // vapor_plan_run_loci_async: one set of four events per step in flight, summed by vapor_plan_sync
    std::vector<std::array<hipEvent_t, 4>> ring;
    int ring_n = 0;
    bool overflow_final = false;               // some pair overflows even at max_pair_cap: do not retry again
    double acc_ms[4] = {0, 0, 0, 0};           // join, clean, finish, total of the steps already folded in
    int64_t acc_n = 0;
    double* h_loci = nullptr;                  // pinned copy of the per-locus records of the last async step
    hipEvent_t ev_t0 = nullptr;
    hipStream_t lane = nullptr;                // the stream this plan's asynchronous steps are enqueued on
    int lane_ix = -1;                          // ... as an index into the context's lanes
    hipStream_t fin = nullptr;                 // ... and the one their finish kernels go to (NULL: the lane itself)
    hipEvent_t ev_clean = nullptr;             // the clean kernels of the last enqueued step are done (lane -> fin)
    hipEvent_t ev_fin = nullptr;               // its finish kernel is done (fin -> lane: the next step's clean kernels wait for it)
    bool have_fin = false;
    hipEvent_t ev_last = nullptr;              // end of the most recently enqueued asynchronous step
    hipEvent_t ev_after = nullptr;             // vapor_plan_after: the next step waits for it
    bool have_last = false, have_after = false;
    double t_join = 0, t_clean = 0, t_total = 0;
    int n_retried = 0;
    bool ran = false;
    bool flags_valid = false;                  // the last run wrote the per-record flag bytes (vapor_plan_fetch_hits hands them out)
    ReadTables reads;                     // optional per-read / per-locus finishing on the device (vapor_plan_set_reads)
    GridTables grid;                      // breakpoint refinement (vapor_plan_set_grid)
    unsigned int* d_overflow = nullptr;   // [0] pairs whose slot overflowed, [1] length of d_big_list
    int32_t* d_big_list = nullptr;        // pairs with more dots than clean_kernel stages in LDS
    unsigned int* h_overflow = nullptr;   // pinned, two counters: pairs that overflowed their slot, pairs left to clean_big_kernel
    bool big_known = false;               // a blocking run has reported how many pairs clean_kernel leaves to clean_big_kernel
    unsigned int n_big = 0;
    double t_finish = 0;
    // shared joins (remap_kernel): pairs n_pairs .. n_pairs + n_dpairs - 1 of hp are the (read, shared sequence) pairs the
    // join runs instead of the pairs they serve
    int64_t n_dpairs = 0;                      // shares.size()
    DShare* d_shares = nullptr;
    int32_t* d_maps = nullptr;                 // `tables`
    DServe* d_serve = nullptr;
    int32_t* d_clean_order = nullptr;          // the pairs in the order their clean workgroups are dealt out (longest first)
};

// ------------------------------------------------------------------------------------------
// A developer build (-DVAPOR_DEV_BUILD: timing stamps, tools/ab.py variants, non-default tuning constants) says so in
// both: the product loader accepts VAPOR_ABI_VERSION only, and vapor_build_flags() lists what the build carries.
#ifdef VAPOR_DEV_BUILD
extern "C" int vapor_abi_version(void) { return VAPOR_ABI_VERSION + VAPOR_ABI_DEV_OFFSET; }
#define VP_STR2(x) #x
#define VP_STR(x) VP_STR2(x)
extern "C" const char* vapor_build_flags(void)
{
    return "dev"
#ifdef VAPOR_PHASE_TIMING
           ",phase_timing"
#endif
#ifdef VAPOR_BLOCK_TIMING
           ",block_timing"
#endif
#ifdef VAPOR_AB
           ",ab=" VP_STR(VAPOR_AB)
#endif
           ",jq_fast_slack=" VP_STR(VAPOR_JQ_FAST_SLACK) ",clean_threads=" VP_STR(VAPOR_CLEAN_THREADS) ",build_cost_x8=" VP_STR(VAPOR_BUILD_COST_X8);
}
#else
extern "C" int vapor_abi_version(void) { return VAPOR_ABI_VERSION; }
extern "C" const char* vapor_build_flags(void) { return ""; }
#endif
extern "C" const char* vapor_last_error(void) { return g_err.c_str(); }
// what this binary was built from (vapor_amd/build.py: sha256 of the kernel sources ':' sha256 of every source file); the
// marker in front lets the build read it out of the file without loading it
#ifndef VAPOR_SOURCE_ID
#define VAPOR_SOURCE_ID "unknown"
#endif
static const char g_source_id[] = "VAPOR_SOURCE_ID=" VAPOR_SOURCE_ID;
extern "C" const char* vapor_source_id(void) { return g_source_id + 16; }

#define JOIN_DYN_LDS(BPS) 0            // the join's LDS is a static array of the kernel

extern "C" int vapor_init(int device_ordinal, vapor_ctx** out)
{
    if (!out) return fail(VAPOR_E_ARG, "vapor_init: null out pointer");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device_ordinal < 0 || device_ordinal >= n)
        return fail(VAPOR_E_ARG, "vapor_init: no such device ordinal");
    HIPCHK(hipSetDevice(device_ordinal));
    vapor_ctx* c = new (std::nothrow) vapor_ctx();
    if (!c) return fail(VAPOR_E_NOMEM, "vapor_init: out of memory");
    c->device = device_ordinal;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0) {
            c->n_cus = prop.multiProcessorCount;
            // a join workgroup fills a CU's LDS (or, in the two-per-CU experiment geometry, half of it)
            c->join_tasks = prop.multiProcessorCount * (JoinCfg::THREADS <= 768 ? 2 : 1);
        }
    }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(VAPOR_E_HIP, hipGetErrorString(e)); }
    for (const void* k : {reinterpret_cast<const void*>(&clean_kernel<4>), reinterpret_cast<const void*>(&clean_kernel<8>),
                          reinterpret_cast<const void*>(&clean_kernel<CLEAN_PER_MAX>), reinterpret_cast<const void*>(&clean_big_kernel)})
        if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CLEAN_LDS_DYNAMIC_MAX);
    if (e != hipSuccess) { (void)hipStreamDestroy(c->stream); delete c; return fail(VAPOR_E_HIP, std::string("hipFuncSetAttribute(clean): ") + hipGetErrorString(e)); }
    c->own_stream = c->stream;
    { std::lock_guard<std::mutex> g(g_live_m); g_live_ctx.insert(c); }
    *out = c;
    return VAPOR_OK;
}

extern "C" int vapor_destroy(vapor_ctx* c)
{
    if (!c) return VAPOR_OK;
    (void)hipSetDevice(c->device);
    { std::lock_guard<std::mutex> g(g_live_m); g_live_ctx.erase(c); }
    (void)hipDeviceSynchronize();
    for (auto& b : c->pool.free_dev) (void)hipFree(b.second);
    for (auto& b : c->pool.free_host) (void)hipHostFree(b.second);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    for (hipStream_t l : c->lane)
        if (l) (void)hipStreamDestroy(l);
    for (hipStream_t l : c->fin)
        if (l) (void)hipStreamDestroy(l);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->d_stage) (void)hipFree(c->d_stage);
    if (c->d_gt) (void)hipFree(c->d_gt);
    if (c->d_crc_pow) (void)hipFree(c->d_crc_pow);
    if (c->bam_stream) (void)hipStreamDestroy(c->bam_stream);
    for (hipEvent_t e : c->bam_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->fasta_ev)
        if (e) (void)hipEventDestroy(e);
    delete c;
    return VAPOR_OK;
}

extern "C" int vapor_set_param(vapor_ctx* c, const char* name, int64_t v)
{
    if (!c || !name) return fail(VAPOR_E_ARG, "vapor_set_param: null argument");
    if (!strcmp(name, "reads_per_task")) {
        if (v < 1 || v > MAX_READS_PER_TASK) return fail(VAPOR_E_ARG, "reads_per_task out of range");
        c->reads_per_task = (int)v;
        return VAPOR_OK;
    }
    if (!strcmp(name, "bam_cu_share")) {
        if (v < 0 || v > 8) return fail(VAPOR_E_ARG, "bam_cu_share out of range (0 .. 8 eighths of the CUs; 0 and 8: all)");
        c->bam_cu_share = (int)(v == 8 ? 0 : v);
        return VAPOR_OK;
    }
    if (!strcmp(name, "join_tasks")) {
        if (v < 1) return fail(VAPOR_E_ARG, "join_tasks out of range");
        c->join_tasks = (int)v;
        return VAPOR_OK;
    }
    if (!strcmp(name, "join_align")) {
        if (v < 0 || v > 2) return fail(VAPOR_E_ARG, "vapor_set_param: join_align is 0, 1 or 2");
        c->join_align = (int)v;
        return VAPOR_OK;
    }
    if (!strcmp(name, "max_pair_cap")) {
        if (v < 1) return fail(VAPOR_E_ARG, "max_pair_cap out of range");
        c->max_pair_cap = v;
        return VAPOR_OK;
    }
    if (!strcmp(name, "shared_join")) {
        c->shared_join = v != 0;
        return VAPOR_OK;
    }
    if (!strcmp(name, "remap_in_clean")) {
        if (v < 0 || v > 2) return fail(VAPOR_E_ARG, "vapor_set_param: remap_in_clean is 0, 1 or 2");
        c->remap_in_clean = (int)v;
        return VAPOR_OK;
    }
    if (!strcmp(name, "clean_order")) {
        c->clean_order = v != 0 ? 1 : 0;
        return VAPOR_OK;
    }
    if (!strcmp(name, "clean_fit")) {
        c->clean_fit = v != 0;
        return VAPOR_OK;
    }
    if (!strcmp(name, "trace_budget")) {
        c->trace_budget = vapor_trace::budget_of(v);       // (a lower value is raised to the floor that always holds one pair)
        return VAPOR_OK;
    }
    if (!strcmp(name, "anyk_edit_pairs")) {
        if (v < 1) return fail(VAPOR_E_ARG, "anyk_edit_pairs out of range");
        c->anyk_edit_pairs = v;
        return VAPOR_OK;
    }
    if (!strcmp(name, "stage_threads")) {
        if (v < 1 || v > 64) return fail(VAPOR_E_ARG, "stage_threads out of range");
        c->stage_threads = (int)v;
        return VAPOR_OK;
    }
    if (!strcmp(name, "pool_fill")) {
        if (!vapor_pool::valid_fill(v)) return fail(VAPOR_E_ARG, "vapor_set_param: pool_fill is -1 (off) or a byte, 0 .. 255");
        c->pool.fill = (int)v;
        return VAPOR_OK;
    }
    return fail(VAPOR_E_ARG, std::string("unknown parameter ") + name);
}

// ------------------------------------------------------------------------------------------
extern "C" int vapor_seqset_destroy(vapor_seqset* s)
{
    if (!s) return VAPOR_OK;
    (void)hipSetDevice(s->device);
    dfree(s->ctx, s->d_seqs);
    dfree(s->ctx, s->d_p2);
    dfree(s->ctx, s->d_e1);
    dfree(s->ctx, s->d_x4);
    dfree(s->ctx, s->d_raw);
    delete s;
    return VAPOR_OK;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// vapor_seqset_create*: the four entries state their call, and everything that is arithmetic - the refusals in their order, where
// every sequence lies in the planes, the staging buffer's tables and what is written into them, the threaded staging, what follows
// the counts - is vapor_seqset_plan.h's.  Here: the staging buffer kept in the context and grown on demand, the set's blocks, the
// copies, bam_expand_kernel / pack_kernel / derive_kernel, the copy back and the synchronisation.
static int seqset_create_impl(vapor_ctx* ctx, const vapor_seqset_plan::Call& call, int32_t* seq_info, vapor_seqset** out)
{
    namespace sp = vapor_seqset_plan;
    // (vapor_seqset_create_mixed takes packed bases by device address: only addresses inside the arena of a live batch are followed)
    const auto in_live_batch = [ctx](const uint8_t* a, const uint8_t* b) {
        auto it = ctx->arenas.upper_bound(a);
        if (it == ctx->arenas.begin()) return false;
        --it;
        return b < it->first + it->second;
    };
    if (const sp::Refusal no = sp::check_args(call, in_live_batch)) return fail(no.code, no.msg);
    HIPCHK(hipSetDevice(ctx->device));
    const bool dbg_t = getenv("VAPOR_DEBUG_UPLOAD") != nullptr;
    double tq[6] = {now_ms(), 0, 0, 0, 0, 0};
    sp::Layout L;                              // (the copies read and fill its descriptors: declared before the owners)
    CallScope sc(ctx, ctx->stream);
    std::unique_ptr<vapor_seqset, Building<vapor_seqset, vapor_seqset_destroy>> s(new (std::nothrow) vapor_seqset(), {&sc});
    if (!s) return fail(VAPOR_E_NOMEM, "out of memory");
    s->ctx = ctx;
    s->device = ctx->device;
    if (const sp::Refusal no = L.build(call, ctx->shared_join)) return fail(no.code, no.msg);
    s->n = L.n;
    s->n_lit = L.n_lit;
    s->plane_chunks = L.plane_chunks;
    const int32_t n_seqs = L.n_lit;
    const size_t n_asc = L.n_asc, pl = L.plane_chunks, desc_bytes = sizeof(SeqDesc) * L.h.size();
    tq[1] = now_ms();
    const sp::Staging st(call, L);
    if (st.need > ctx->stage_cap) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
        if (ctx->d_stage) (void)hipFree(ctx->d_stage);
        ctx->h_stage = nullptr; ctx->d_stage = nullptr; ctx->stage_cap = 0;
        const size_t cap = st.need + st.need / 4;
        HIPCHK(hipHostMalloc((void**)&ctx->h_stage, cap));
        HIPCHK(hipMalloc((void**)&ctx->d_stage, cap));
        ctx->stage_cap = cap;
    }
    uint8_t *const h_stage = ctx->h_stage, *const d_stage = ctx->d_stage;
    if (ctx->pool.fill != vapor_pool::FILL_OFF && ctx->stage_cap) {
        // (parameter pool_fill: the staging buffers are no pool blocks and are never fresh after the first upload)
        HIPCHK(hipStreamSynchronize(ctx->stream));
        memset(h_stage, ctx->pool.fill, ctx->stage_cap);
        HIPCHK(hipMemset(d_stage, ctx->pool.fill, ctx->stage_cap));
        HIPCHK(hipDeviceSynchronize());
    }
    HIPCHK(dmalloc(ctx, (void**)&s->d_seqs, desc_bytes));
    HIPCHK(dmalloc(ctx, (void**)&s->d_p2, pl * 2 * sizeof(uint32_t)));
    HIPCHK(dmalloc(ctx, (void**)&s->d_e1, pl * sizeof(uint32_t)));
    HIPCHK(dmalloc(ctx, (void**)&s->d_x4, pl * 4 * sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(s->d_p2, 0, pl * 2 * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync(s->d_e1, 0, pl * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync(s->d_x4, 0, pl * 4 * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemcpyAsync(s->d_seqs, L.h.data(), desc_bytes, hipMemcpyHostToDevice, ctx->stream));
    tq[2] = now_ms();
    // the copy into the pinned staging buffer is the largest part of an upload (a core moves ~8 GB/s, the link 50): the literals
    // are split over a few host threads when there is enough to copy
    const int n_thr = st.sliced ? ctx->stage_threads : 1;
    if (L.mixed) {
        // (the device holds some literals already, 4 bits a base: bam_expand_kernel writes their part of the ASCII layout)
        sp::stage_range(call, L, st, h_stage, 0, n_seqs);
        sp::fill_sources(call, st, h_stage);
        if (st.host_end) HIPCHK(hipMemcpyAsync(d_stage, h_stage, st.host_end * 32, hipMemcpyHostToDevice, ctx->stream));
        if (n_asc) HIPCHK(hipMemcpyAsync(st.map.in(d_stage), st.map.in(h_stage), st.map.bytes(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(st.src.in(d_stage), st.src.in(h_stage), st.mix_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (n_asc) {
            hipLaunchKernelGGL(vapor_bamdev::bam_expand_kernel, dim3((unsigned)((n_asc + 255) / 256)), dim3(256), 0, ctx->stream, st.asc.in(d_stage),
                               st.map.in(d_stage), (uint32_t)n_asc, reinterpret_cast<const uint32_t*>(s->d_seqs), st.src.in(d_stage), st.first.in(d_stage));
            HIPCHK(hipGetLastError());
        }
    } else if (n_thr == 1) {
        sp::stage_range(call, L, st, h_stage, 0, n_seqs);
        if (n_asc) HIPCHK(hipMemcpyAsync(d_stage, h_stage, st.asc.bytes() + st.map.bytes(), hipMemcpyHostToDevice, ctx->stream));
    } else {
        hipError_t err = hipSuccess;
        sp::stage_sliced(call, L, st, h_stage, n_thr, [&](size_t c0, size_t c1) {
            if (err == hipSuccess) err = hipMemcpyAsync(d_stage + c0 * 32, h_stage + c0 * 32, (c1 - c0) * 32, hipMemcpyHostToDevice, ctx->stream);
        });
        HIPCHK(err);
        HIPCHK(hipMemcpyAsync(st.map.in(d_stage), st.map.in(h_stage), st.map.bytes(), hipMemcpyHostToDevice, ctx->stream));
    }
    tq[3] = now_ms();
    if (n_asc) {
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((n_asc + 255) / 256)), dim3(256), 0, ctx->stream, st.asc.in(d_stage), s->d_seqs, n_seqs,
                           st.map.in(d_stage), (uint32_t)n_asc, s->d_p2, s->d_e1, s->d_x4);
        HIPCHK(hipGetLastError());
    }
    if (L.der_chunks) {
        sp::fill_derived(L, st, h_stage);
        HIPCHK(hipMemcpyAsync(st.segs.in(d_stage), st.segs.in(h_stage), st.der_bytes, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(derive_kernel, dim3((unsigned)((L.der_chunks + 255) / 256)), dim3(256), 0, ctx->stream, s->d_seqs, st.der_map.in(d_stage),
                           (uint32_t)L.der_chunks, st.seg_first.in(d_stage), st.segs.in(d_stage), n_seqs, s->d_p2, s->d_e1, s->d_x4);
        HIPCHK(hipGetLastError());
    }
    tq[4] = now_ms();
    HIPCHK(hipMemcpyAsync(L.h.data(), s->d_seqs, desc_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    tq[5] = now_ms();
    if (dbg_t) fprintf(stderr, "seqset: layout+groups %.3f  alloc+memset %.3f  stage+h2d %.3f  launches %.3f  sync %.3f ms\n", tq[1] - tq[0], tq[2] - tq[1], tq[3] - tq[2], tq[4] - tq[3], tq[5] - tq[4]);
    if (const sp::Refusal no = sp::revcomp_refusal(L)) return fail(no.code, no.msg);
    // keep the bytes of the sequences with symbols outside the alphabet (rare) before the staging buffer is reused
    if (const size_t raw_bytes = sp::raw_layout(L, s->raw_off)) {
        HIPCHK(dmalloc(ctx, (void**)&s->d_raw, raw_bytes));
        for (int32_t i = 0; i < n_seqs; ++i)
            if (s->raw_off[i] >= 0 && L.h[i].len)
                HIPCHK(hipMemcpyAsync(s->d_raw + s->raw_off[i], st.asc.in(d_stage) + (size_t)L.h[i].asc0 * 32, (size_t)L.h[i].len,
                                      hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    sp::fill_seq_info(L, seq_info);
    s->h = std::move(L.h);
    s->derived = std::move(L.derived);
    s->groups = std::move(L.groups);
    s->group_of = std::move(L.group_of);
    s->slot_of = std::move(L.slot_of);
    *out = s.release();
    return VAPOR_OK;
}

extern "C" int vapor_seqset_create(vapor_ctx* ctx, int32_t n_seqs, const uint8_t* blob, const int64_t* off,
                                   const int32_t* len, const uint8_t* flags, int32_t* seq_info, vapor_seqset** out)
{
    return seqset_create_impl(ctx, {vapor_seqset_plan::BLOB, ctx && out, n_seqs, blob, off, nullptr, len, flags, nullptr, nullptr, 0, nullptr, nullptr, nullptr},
                              seq_info, out);
}

extern "C" int vapor_seqset_create_ptrs(vapor_ctx* ctx, int32_t n_seqs, const uint8_t* const* seq, const int32_t* len,
                                        const uint8_t* flags, int32_t* seq_info, vapor_seqset** out)
{
    return seqset_create_impl(ctx, {vapor_seqset_plan::PTRS, ctx && out, n_seqs, nullptr, nullptr, seq, len, flags, nullptr, nullptr, 0, nullptr, nullptr, nullptr},
                              seq_info, out);
}

extern "C" int vapor_seqset_create_derived(vapor_ctx* ctx, int32_t n_seqs, const uint8_t* const* seq, const int32_t* len,
                                           const uint8_t* flags, int32_t n_derived, const int32_t* seg_first,
                                           const vapor_segment* segs, const uint8_t* derived_flags, int32_t* seq_info,
                                           vapor_seqset** out)
{
    return seqset_create_impl(ctx, {vapor_seqset_plan::DERIVED, ctx && out, n_seqs, nullptr, nullptr, seq, len, flags, nullptr, nullptr, n_derived, seg_first, segs,
                                    derived_flags}, seq_info, out);
}

// vapor_seqset_create_derived with sequences whose bases are on the device already (vapor_bam_chop_device's reads): src_kind[i] = 1
// says seq[i] is the DEVICE address of BAM-packed bases (4 bits each, high nibble first) inside the arena of a live batch of this
// context and src_first[i] the first base; len[i] bases from there are the sequence.  0: bytes on the host, as ever.
extern "C" int vapor_seqset_create_mixed(vapor_ctx* ctx, int32_t n_seqs, const uint8_t* const* seq, const int32_t* len,
                                         const uint8_t* flags, const uint8_t* src_kind, const int64_t* src_first,
                                         int32_t n_derived, const int32_t* seg_first, const vapor_segment* segs,
                                         const uint8_t* derived_flags, int32_t* seq_info, vapor_seqset** out)
{
    return seqset_create_impl(ctx, {vapor_seqset_plan::MIXED, ctx && out, n_seqs, nullptr, nullptr, seq, len, flags, src_kind, src_first, n_derived, seg_first, segs,
                                    derived_flags}, seq_info, out);
}

extern "C" int vapor_seqset_planes(vapor_seqset* s, int32_t seq, uint32_t* p2, uint32_t* e1, uint32_t* x4)
{
    if (!s || seq < 0 || seq >= s->n) return fail(VAPOR_E_ARG, "vapor_seqset_planes: no such sequence");
    HIPCHK(hipSetDevice(s->device));
    const SeqDesc& d = s->h[(size_t)seq];
    const size_t ch = ((size_t)d.len + 31) / 32;
    if (!ch) return VAPOR_OK;
    if (p2) HIPCHK(hipMemcpy(p2, s->d_p2 + (size_t)d.chunk0 * 2, ch * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (e1) HIPCHK(hipMemcpy(e1, s->d_e1 + (size_t)d.chunk0, ch * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (x4) HIPCHK(hipMemcpy(x4, s->d_x4 + (size_t)d.chunk0 * 4, ch * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
// Read extraction on the device (vapor_bamdev.h): the host side reads the regions' BGZF blocks as they lie in the file, lays
// out where every block's data goes, sends the compressed bytes and runs the kernels.
// ------------------------------------------------------------------------------------------
extern "C" int vapor_bam_fileno(vapor_bam* b);
extern "C" int vapor_bam_threads(vapor_bam* b);
extern "C" uint32_t vapor_bam_filter_word(vapor_bam* b);      // the handle's read filter as BamRegion::pad carries it (vapor_bam.cpp)
extern "C" int vapor_bam_dedup_on(vapor_bam* b);              // whether the handle de-duplicates by QNAME (vapor_bam_set_dedup, vapor_bam.cpp)

struct vapor_bam_batch {
    vapor_ctx* ctx = nullptr;
    int device = 0;
    uint8_t* d_arena = nullptr;
    size_t arena_bytes = 0;
    // `--dedup-qname`: the name keys of the entries a plain or right-anchored call returned, in their order
    bool has_keys = false;
    std::vector<uint64_t> name_keys;
};

extern "C" int vapor_bam_batch_destroy(vapor_bam_batch* b)
{
    if (!b) return VAPOR_OK;
    if (b->d_arena) {
        (void)hipSetDevice(b->device);
        if (b->ctx && ctx_alive(b->ctx)) {
            // (kernels that read the arena - bam_expand_kernel of a set made from it - are on the context's stream)
            (void)hipStreamSynchronize(b->ctx->stream);
            b->ctx->arenas.erase(b->d_arena);
        }
        dfree(b->ctx, b->d_arena);
    }
    delete b;
    return VAPOR_OK;
}

// the CRC combination constants bgzf_inflate_kernel multiplies its lanes' slice CRCs by, on the device once per context
static hipError_t crc_pow_on_device(vapor_ctx* ctx)
{
    if (ctx->d_crc_pow) return hipSuccess;
    // x^(8 * 1024 * (63 - l)) mod P, l = 0 .. 63 (bit 31 = x^0): what lane l's slice CRC is multiplied by
    uint32_t pw[64];
    auto mul = [](uint32_t a, uint32_t b) {
        uint32_t m = 1u << 31, p = 0;
        for (int i = 0; i < 32; ++i) { if (a & m) p ^= b; m >>= 1; b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1; }
        return p;
    };
    for (int l = 0; l < 64; ++l) {
        uint64_t e = (uint64_t)8 * 1024 * (uint64_t)(63 - l);
        uint32_t r = 0x80000000u, b = 0x40000000u;
        while (e) { if (e & 1) r = mul(r, b); b = mul(b, b); e >>= 1; }
        pw[l] = r;
    }
    uint32_t* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, sizeof pw);
    if (e != hipSuccess) return e;
    e = hipMemcpy(d, pw, sizeof pw, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return e; }
    ctx->d_crc_pow = d;
    return hipSuccess;
}

// The inflate stage of the two device readers (vapor_bam_chop_device*, vapor_fasta_windows_device): the file's bytes read into a
// pinned block, one metadata block (vapor_readplan.h carves it) that holds the BgzfBlk list, both sent on the call's stream, bgzf_inflate_kernel.
// Its blocks are Blocks of the call's CallScope, so they go back to the pool as every other block of the call does.
struct InflateStage {
    CallScope& sc;
    HostBlock<> h_comp, h_meta;
    Block<> d_comp, d_meta;
    size_t stage_bytes = 0;
    explicit InflateStage(CallScope& s) : sc(s), h_comp(s), h_meta(s), d_comp(s), d_meta(s) {}
    hipError_t begin(size_t bytes) { stage_bytes = bytes; return h_comp.ensure(std::max<size_t>(bytes, 64)); }     // room for the call's compressed bytes
    // file bytes [file_off, file_off + want) to h_comp + stage_off; how many there were
    size_t read(int fd, size_t stage_off, size_t want, int64_t file_off) const
    {
        size_t got = 0;
        while (got < want) {
            const ssize_t r = pread(fd, h_comp + stage_off + got, want - got, (off_t)(file_off + (int64_t)got));
            if (r <= 0) break;
            got += (size_t)r;
        }
        return got;
    }
    int alloc(size_t h_meta_bytes, size_t d_meta_bytes)
    {
        HIPCHK(h_meta.ensure(h_meta_bytes));
        HIPCHK(d_meta.ensure(d_meta_bytes));
        HIPCHK(d_comp.ensure(std::max<size_t>(stage_bytes, 64)));
        HIPCHK(crc_pow_on_device(sc.ctx));
        return VAPOR_OK;
    }
    // On sc.st: the compressed bytes and the first in_bytes of the metadata (the tables the call's plan filled in, the n_blks blocks
    // of d_blks among them) go to the device, ev[0], the blocks inflate to `arena`, their statuses to d_blk_status.  The caller
    // records ev[1] where its timing ends.
    // (t_comp: the developer's timing - the stream is synchronised behind the first copy and the clock written there)
    int run(size_t n_blks, size_t in_bytes, const vapor_bamdev::BgzfBlk* d_blks, int32_t* d_blk_status, uint8_t* arena, hipEvent_t* ev, double* t_comp = nullptr)
    {
        using namespace vapor_bamdev;
        if (!ev[0]) { HIPCHK(hipEventCreate(&ev[0])); HIPCHK(hipEventCreate(&ev[1])); }
        if (stage_bytes) HIPCHK(hipMemcpyAsync(d_comp, h_comp, stage_bytes, hipMemcpyHostToDevice, sc.st));
        if (t_comp) { HIPCHK(hipStreamSynchronize(sc.st)); *t_comp = now_ms(); }
        HIPCHK(hipMemcpyAsync(d_meta, h_meta, in_bytes, hipMemcpyHostToDevice, sc.st));
        HIPCHK(hipEventRecord(ev[0], sc.st));
        if (n_blks) {
            hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)((n_blks + INFLATE_WAVES - 1) / INFLATE_WAVES)), dim3(64 * INFLATE_WAVES), 0, sc.st, d_comp,
                               d_blks, (int)n_blks, arena, sc.ctx->d_crc_pow, d_blk_status);
            HIPCHK(hipGetLastError());
        }
        return VAPOR_OK;
    }
};

// No exception crosses the C boundary (a thread that could not start, a vector that could not grow, ...).
template <typename F>
static int guarded(const char* name, F body)
{
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(VAPOR_E_NOMEM, std::string(name) + ": out of memory");
    } catch (const std::exception& e) {
        return fail(VAPOR_E_ARG, std::string(name) + ": " + e.what());
    }
}

// The stream the chop kernels run on: the context's own, or - a share of the CUs set aside for them - a CU-masked one, made again
// when the share changes.
static hipStream_t bam_stream_of(vapor_ctx* ctx)
{
    const char* sh = getenv("VAPOR_BAM_CU_SHARE");            // (experiments: overrides the parameter)
    const int share = ctx->user_stream ? 0 : (sh ? atoi(sh) : ctx->bam_cu_share);
    if (share != ctx->bam_stream_share) {
        if (ctx->bam_stream) { (void)hipStreamSynchronize(ctx->bam_stream); (void)hipStreamDestroy(ctx->bam_stream); ctx->bam_stream = nullptr; }
        ctx->bam_stream_share = share;
        if (share >= 1 && share <= 7) {
            // (CU i of the mask's enumeration is on in s of every 8: every XCD keeps CUs of both kinds)
            std::vector<uint32_t> mask((size_t)(ctx->n_cus + 31) / 32, 0u);
            for (int i = 0; i < ctx->n_cus; ++i)
                if (i % 8 < share) mask[(size_t)i / 32] |= 1u << (i % 32);
            if (hipExtStreamCreateWithCUMask(&ctx->bam_stream, (uint32_t)mask.size(), mask.data()) != hipSuccess) ctx->bam_stream = nullptr;
        }
    }
    return ctx->bam_stream ? ctx->bam_stream : ctx->stream;
}

#ifdef VBD_TIMING
// (developer builds) the shader clocks bgzf_inflate_kernel left where the blocks' compressed bytes were
static int dump_inflate_timing(const uint8_t* d_comp, size_t stage_bytes, const std::vector<vapor_bamdev::BgzfBlk>& blks)
{
    std::vector<uint8_t> back(stage_bytes);
    HIPCHK(hipMemcpy(back.data(), d_comp, stage_bytes, hipMemcpyDeviceToHost));
    double sum[13] = {0};
    size_t cnt = 0;
    for (const vapor_bamdev::BgzfBlk& k : blks) {
        if (k.c_len < 128) continue;
        const long long* d = reinterpret_cast<const long long*>(back.data() + ((k.c_off + 7u) & ~7u));
        for (int t = 0; t < 13; ++t) sum[t] += (double)d[t];
        ++cnt;
    }
    fprintf(stderr, "  per block (shader clocks, mean of %zu): top-up %.0f  decode %.0f (tables %.0f)  matches %.0f  crc %.0f  all %.0f\n"
                    "  counts: fast literal steps %.0f, fast general symbols %.0f, careful symbols %.0f, matches %.0f (fills %.0f), batches %.0f; clocks in the fast loop's general symbols %.0f\n", cnt,
            sum[0] / cnt, sum[1] / cnt, sum[2] / cnt, sum[3] / cnt, sum[4] / cnt, sum[5] / cnt, sum[6] / cnt, sum[10] / cnt, sum[7] / cnt, sum[8] / cnt,
            sum[11] / cnt, sum[9] / cnt, sum[12] / cnt);
    return VAPOR_OK;
}
#endif

// The read and the scan of a device reader call's spans, a few threads: every span's file range into the staging block, its BGZF
// blocks listed (vapor_bgzf::scan_span).  A span whose block list cannot be held is marked bad: its region goes the host route.
static void read_and_scan(InflateStage& stage, int fd, vapor_bam* bam, std::vector<vapor_readplan::HostSpan>& spans)
{
    const int n_thr = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(vapor_bam_threads(bam), 1) * 2, spans.size() / 8 + 1));
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t i = next.fetch_add(1, std::memory_order_relaxed);
            if (i >= spans.size()) break;
            vapor_readplan::HostSpan& sp = spans[i];
            sp.got = stage.read(fd, sp.stage_off, sp.want, sp.file_off);
            try {
                vapor_bgzf::scan_span(sp, stage.h_comp);
            } catch (const std::exception&) {       // (out of memory for the block list: the region goes the host route)
                sp.blks.clear();
                sp.bad = true;
            }
        }
    };
    if (n_thr <= 1) {
        work();
    } else {
        std::vector<std::thread> th;
        for (int t = 1; t < n_thr; ++t) th.emplace_back(work);
        work();
        for (auto& x : th) x.join();
    }
}

// The four vapor_bam_chop_device* entries (vapor_readplan.h ChopMode).  TAGGED: the tagged chop kernel, the select kernel behind it
// on the same stream, and only the regions' compact unions and phase sets copied back.  HAPLOTAG: the tags the select kernel reads
// come from bam_haplotag_kernel, which runs between the two.
static int bam_chop_device_impl(vapor_ctx* ctx, vapor_bam* bam, vapor_readplan::ChopCall call, const vapor_readplan::ChopOut& o, vapor_bam_batch** out)
{
    using namespace vapor_bamdev;
    using namespace vapor_readplan;
    if (!ctx || !bam || !out) return fail(VAPOR_E_ARG, "vapor_bam_chop_device: bad argument");
    if (const Refusal r = check_args(call, o)) return fail(r.code, r.msg);
    const int fd = vapor_bam_fileno(bam);
    if (fd < 0) return fail(VAPOR_E_ARG, "vapor_bam_chop_device: the file is not open");
    call.filter_word = vapor_bam_filter_word(bam);
    call.dedup = vapor_bam_dedup_on(bam) != 0;
    const int32_t n_regions = call.n_regions;
    const bool phased = call.phased(), haplo = call.haplo();
    HIPCHK(hipSetDevice(ctx->device));
    *out = nullptr;
    const bool dbg_t = getenv("VAPOR_DEBUG_BAMDEV") != nullptr;
    double tq[8] = {now_ms(), 0, 0, 0, 0, 0, 0, 0};
    return guarded("vapor_bam_chop_device", [&]() -> int {
        // ---- what to read ---------------------------------------------------------------------------------------------------
        SpanPlan plan;
        if (const Refusal r = plan_spans(call, o.status, plan)) return fail(r.code, r.msg);
        std::vector<HostSpan>& spans = plan.spans;
        // (what the call holds while it runs goes back to the context's pool on every way out, an exception's included; the batch
        // survives a successful return only)
        CallScope sc(ctx, ctx->stream);
        std::unique_ptr<vapor_bam_batch, Building<vapor_bam_batch, vapor_bam_batch_destroy>> B(new vapor_bam_batch(), {&sc});
        B->ctx = ctx;
        B->device = ctx->device;
        InflateStage stage(sc);
        HIPCHK(stage.begin(plan.stage_bytes));
        // ---- read and scan, a few threads -------------------------------------------------------------------------------------
        read_and_scan(stage, fd, bam, spans);
        tq[1] = now_ms();
        // ---- layout of the arena and the tables -------------------------------------------------------------------------------
        ChopLayout L;
        if (const Refusal r = layout(call, plan, o.status, L)) return fail(r.code, r.msg);
        const ChopMeta& M = L.meta;
        const size_t n_blks = L.blks.size();
        if (const int rc = stage.alloc(M.host_bytes(), M.bytes)) return rc;
        HIPCHK(dmalloc(ctx, (void**)&B->d_arena, L.arena + 64));
        B->arena_bytes = L.arena + 64;
        ctx->arenas[B->d_arena] = B->arena_bytes;
        uint8_t *const h_meta = stage.h_meta, *const d_meta = stage.d_meta;
        M.fill(h_meta, call, L, o.status);
        const hipStream_t st = sc.st = bam_stream_of(ctx);
        tq[2] = now_ms();
        if (const int rc = stage.run(n_blks, M.in_bytes, M.blks.in(d_meta), M.blk_status.in(d_meta), B->d_arena, ctx->bam_ev, dbg_t ? &tq[3] : nullptr)) return rc;
        HIPCHK(hipEventRecord(ctx->bam_ev[1], st));
        if (dbg_t) { HIPCHK(hipStreamSynchronize(st)); tq[4] = now_ms(); }
        if (n_regions) {
            // the chop kernel of the call: plain, right-anchored, or (phased) the tagged one with the select kernel behind it
            auto chop = [&](auto kernel, auto... tags) {
                hipLaunchKernelGGL(kernel, dim3((unsigned)n_regions), dim3(64), 0, st, B->d_arena, M.regs.in(d_meta), M.spans.in(d_meta), M.blk_status.in(d_meta),
                                   (int)n_regions, M.kept.in(d_meta), M.n_kept.in(d_meta), M.reg_status.in(d_meta), tags...);
            };
            if (haplo) chop(bam_chop_ops_kernel, M.ops.in(d_meta));
            else if (phased) chop(bam_chop_tagged_kernel, M.tags.in(d_meta));
            else chop(call.mode == ChopMode::RIGHT ? bam_chop_right_kernel : bam_chop_kernel);
            HIPCHK(hipGetLastError());
            if (call.dedup) {
                // one record of a molecule per region (rule W), before anything looks at the kept entries
                hipLaunchKernelGGL(bam_dedup_kernel, dim3((unsigned)n_regions), dim3(64), 0, st, B->d_arena, M.regs.in(d_meta), M.spans.in(d_meta), (int)n_regions,
                                   M.kept.in(d_meta), M.n_kept.in(d_meta), M.reg_status.in(d_meta), phased && !haplo ? M.tags.in(d_meta) : (BamTag*)nullptr,
                                   haplo ? M.ops.in(d_meta) : (BamOps*)nullptr, M.keys.in(d_meta));
                HIPCHK(hipGetLastError());
            }
            if (haplo) {
                // the tags of the kept records from the region's phased sites: a wavefront a (region, slot)
                hipLaunchKernelGGL(bam_haplotag_kernel, dim3((unsigned)n_regions * (unsigned)(KEPT_CAP / HAPLOTAG_WAVES)), dim3(64 * HAPLOTAG_WAVES), 0, st,
                                   B->d_arena, M.kept.in(d_meta), M.ops.in(d_meta), M.n_kept.in(d_meta), M.reg_status.in(d_meta), (int)n_regions,
                                   M.site_ranges.in(d_meta), M.sites.in(d_meta), M.ps_values.in(d_meta), M.tags.in(d_meta));
                HIPCHK(hipGetLastError());
            }
            if (phased) {
                hipLaunchKernelGGL(bam_select_kernel, dim3((unsigned)n_regions), dim3(64), 0, st, M.kept.in(d_meta), M.tags.in(d_meta), M.n_kept.in(d_meta),
                                   M.reg_status.in(d_meta), (int)n_regions, (int)call.max_keep, M.picks.in(d_meta), M.phases.in(d_meta));
                HIPCHK(hipGetLastError());
            }
        }
        // (counts and statuses first; the kept reads of a region are read where its count says)
        HIPCHK(hipMemcpyAsync(M.back(h_meta), M.back(d_meta), M.back_bytes(), hipMemcpyDeviceToHost, st));
        ctx->bam_stats[6] = (double)M.back_bytes();
        HIPCHK(hipStreamSynchronize(st));
        tq[5] = now_ms();
        {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ctx->bam_ev[0], ctx->bam_ev[1]) != hipSuccess) ms = 0.f;
            ctx->bam_stats[0] = n_regions; ctx->bam_stats[1] = (double)n_blks; ctx->bam_stats[2] = (double)plan.stage_bytes;
            ctx->bam_stats[3] = (double)L.arena; ctx->bam_stats[4] = ms; ctx->bam_stats[5] = tq[5] - tq[0];
        }
        if (dbg_t)
            fprintf(stderr, "bam_chop_device: %d regions, %zu blocks, %.1f MB compressed -> %.1f MB; read+scan %.2f  layout+alloc %.2f  h2d %.2f  inflate %.2f  chop+d2h %.2f ms\n",
                    n_regions, n_blks, plan.stage_bytes / 1e6, L.arena / 1e6, tq[1] - tq[0], tq[2] - tq[1], tq[3] - tq[2], tq[4] - tq[3], tq[5] - tq[4]);
#ifdef VBD_TIMING
        if (dbg_t && n_blks)
            if (const int rc = dump_inflate_timing(stage.d_comp, plan.stage_bytes, L.blks)) return rc;
#endif
        B->has_keys = call.dedup && !phased;
        collect(call, M, h_meta, (uint64_t)reinterpret_cast<uintptr_t>(B->d_arena), o, B->name_keys);
        sc.settled();
        *out = B.release();
        return VAPOR_OK;
    });
}

// the caller's region arrays and answer arrays of the four entries, as bam_chop_device_impl takes them
static vapor_readplan::ChopCall chop_call(vapor_readplan::ChopMode mode, int32_t n_regions, const int32_t* tid, const int64_t* start, const int64_t* end,
                                          const int64_t* flank, const int32_t* chunk_first, const uint64_t* chunks, int32_t max_keep)
{
    vapor_readplan::ChopCall c;
    c.n_regions = n_regions; c.tid = tid; c.start = start; c.end = end; c.flank = flank; c.chunk_first = chunk_first; c.chunks = chunks;
    c.max_keep = max_keep; c.mode = mode;
    return c;
}

extern "C" int vapor_bam_chop_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* start,
                                     const int64_t* end, const int64_t* flank, const int32_t* chunk_first, const uint64_t* chunks,
                                     int32_t max_keep, int32_t* kept_first, uint64_t* sq_addr, int64_t* q0, int64_t* miss,
                                     int32_t* status, vapor_bam_batch** out)
{
    using namespace vapor_readplan;
    return bam_chop_device_impl(ctx, bam, chop_call(ChopMode::PLAIN, n_regions, tid, start, end, flank, chunk_first, chunks, max_keep),
                                ChopOut{kept_first, sq_addr, q0, miss, status}, out);
}

// The name keys (`--dedup-qname`; vapor_names.h name_key) of the n entries the call that made the batch returned, in
// their order: n = kept_first[n_regions].  VAPOR_E_ARG for a batch of a handle without the option, of a tagged / haplotag call
// (their unions are made on the device, and no caller needs their keys) and for another n.
extern "C" int vapor_bam_batch_name_keys(vapor_bam_batch* b, int64_t n, uint64_t* keys)
{
    if (!b || !b->has_keys || n != (int64_t)b->name_keys.size() || (n && !keys))
        return fail(VAPOR_E_ARG, "vapor_bam_batch_name_keys: no keys in this batch, or another count");
    if (n) memcpy(keys, b->name_keys.data(), sizeof(uint64_t) * (size_t)n);
    return VAPOR_OK;
}

// vapor_bam_chop_device for the right-anchored reads of every region (`--both-ends`, DESIGN.md 4.14: bam_chop_right_kernel).
// q1[t] = the base of read t its reverse complement starts with: with src_kind 2, vapor_seqset_create_mixed takes the read as
// the reverse complement of the end - start - miss[t] bases that end there.
extern "C" int vapor_bam_chop_device_right(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* start,
                                           const int64_t* end, const int64_t* flank, const int32_t* chunk_first, const uint64_t* chunks,
                                           int32_t max_keep, int32_t* kept_first, uint64_t* sq_addr, int64_t* q1, int64_t* miss,
                                           int32_t* status, vapor_bam_batch** out)
{
    using namespace vapor_readplan;
    return bam_chop_device_impl(ctx, bam, chop_call(ChopMode::RIGHT, n_regions, tid, start, end, flank, chunk_first, chunks, max_keep),
                                ChopOut{kept_first, sq_addr, q1, miss, status}, out);
}

extern "C" int vapor_bam_chop_device_tagged(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* start,
                                            const int64_t* end, const int64_t* flank, const int32_t* chunk_first, const uint64_t* chunks,
                                            int32_t max_keep, int32_t* kept_first, uint64_t* sq_addr, int64_t* q0, int64_t* miss,
                                            uint32_t* member, int64_t* phase_set, int32_t* tagged, int32_t* status, vapor_bam_batch** out)
{
    using namespace vapor_readplan;
    if (!member) return fail(VAPOR_E_ARG, "vapor_bam_chop_device_tagged: bad argument");
    return bam_chop_device_impl(ctx, bam, chop_call(ChopMode::TAGGED, n_regions, tid, start, end, flank, chunk_first, chunks, max_keep),
                                ChopOut{kept_first, sq_addr, q0, miss, status, member, phase_set, tagged}, out);
}

// vapor_bam_chop_device_tagged with the tags made on the device from phased SNVs (`--phase-vcf`): bam_chop_ops_kernel,
// bam_haplotag_kernel, bam_select_kernel on one stream.
extern "C" int vapor_bam_chop_device_haplotag(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* start,
                                              const int64_t* end, const int64_t* flank, const int32_t* chunk_first, const uint64_t* chunks,
                                              int32_t max_keep, int32_t* kept_first, uint64_t* sq_addr, int64_t* q0, int64_t* miss,
                                              uint32_t* member, int64_t* phase_set, int32_t* tagged, int32_t* status, vapor_bam_batch** out,
                                              const int32_t* site_first, const void* sites, const int32_t* ps_first, const int64_t* ps_values)
{
    using namespace vapor_readplan;
    if (!member) return fail(VAPOR_E_ARG, "vapor_bam_chop_device_haplotag: bad argument");
    ChopCall c = chop_call(ChopMode::HAPLOTAG, n_regions, tid, start, end, flank, chunk_first, chunks, max_keep);
    c.site_first = site_first; c.sites = static_cast<const vapor_bamdev::BamSite*>(sites); c.ps_first = ps_first; c.ps_values = ps_values;
    return bam_chop_device_impl(ctx, bam, c, ChopOut{kept_first, sq_addr, q0, miss, status, member, phase_set, tagged}, out);
}

// The evidence of many regions of an open BAM file (`--depth`, `--signatures`, `--links`, `--support`): what
// bam_chop_device_impl does up to the inflate launch - the regions' chunks staged, scanned, laid out in the arena, inflated with
// CRC - then the call's kernel, one wavefront a region (launch(stream, arena, meta, the device's block)), and one copy back.  The
// arena is a block of the call: nothing stays on the device, and there is no batch.  The statistics of the chop call
// (vapor_bam_last_stats) are left alone.  `who` is the entry's name in its errors; the plan is the call's in vapor_readplan.h.
template <typename Layout, typename Call, typename Out, typename Launch>
static int bam_evidence_device(vapor_ctx* ctx, vapor_bam* bam, const char* who, Call& call, Out* out, int32_t* status, Launch launch)
{
    using namespace vapor_readplan;
    if (!ctx || !bam) return fail(VAPOR_E_ARG, std::string(who) + ": bad argument");
    if (const Refusal r = check_args(call, out, status)) return fail(r.code, r.msg);
    const int fd = vapor_bam_fileno(bam);
    if (fd < 0) return fail(VAPOR_E_ARG, std::string(who) + ": the file is not open");
    call.filter_word = depth_filter_word(vapor_bam_filter_word(bam));
    HIPCHK(hipSetDevice(ctx->device));
    return guarded(who, [&]() -> int {
        SpanPlan plan;
        if (const Refusal r = plan_spans(call, status, plan)) return fail(r.code, r.msg);
        CallScope sc(ctx, ctx->stream);
        InflateStage stage(sc);
        Block<> d_arena(sc);
        HIPCHK(stage.begin(plan.stage_bytes));
        read_and_scan(stage, fd, bam, plan.spans);
        Layout L;
        if (const Refusal r = layout(call, plan, status, L)) return fail(r.code, r.msg);
        const typename Layout::Meta& M = L.meta;
        if (const int rc = stage.alloc(M.bytes, M.bytes)) return rc;
        HIPCHK(d_arena.ensure(L.arena + 64));
        uint8_t *const h_meta = stage.h_meta, *const d_meta = stage.d_meta;
        L.fill(h_meta);
        const hipStream_t st = sc.st = bam_stream_of(ctx);
        if (const int rc = stage.run(L.blks.size(), M.in_bytes, M.blks.in(d_meta), M.blk_status.in(d_meta), d_arena, ctx->bam_ev)) return rc;
        if (call.n_regions) {
            launch(st, (const uint8_t*)d_arena, M, d_meta);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(M.back(h_meta), M.back(d_meta), M.back_bytes(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        sc.settled();
        collect(call, M, h_meta, out, status);
        return VAPOR_OK;
    });
}

// bam_depth_kernel: three 64-bit sums a region
extern "C" int vapor_bam_depth_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* bounds,
                                      const int32_t* chunk_first, const uint64_t* chunks, uint64_t* cov, int32_t* status)
{
    using namespace vapor_bamdev;
    vapor_readplan::DepthCall call;
    call.n_regions = n_regions; call.tid = tid; call.bounds = bounds; call.chunk_first = chunk_first; call.chunks = chunks;
    return bam_evidence_device<vapor_readplan::DepthLayout>(ctx, bam, "vapor_bam_depth_device", call, cov, status,
                                                            [&](hipStream_t st, const uint8_t* arena, const auto& M, uint8_t* d_meta) {
        hipLaunchKernelGGL(bam_depth_kernel, dim3((unsigned)n_regions), dim3(64), 0, st, arena, M.regs.in(d_meta), M.spans.in(d_meta), M.blk_status.in(d_meta),
                           (int)n_regions, reinterpret_cast<unsigned long long*>(M.ans.in(d_meta)), M.reg_status.in(d_meta));
    });
}

// bam_signature_kernel: SIG_ANSWER_WORDS words a region
extern "C" int vapor_bam_signature_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* regions,
                                          const int32_t* chunk_first, const uint64_t* chunks, int64_t* out, int32_t* status)
{
    using namespace vapor_bamdev;
    vapor_readplan::SigCall call;
    call.n_regions = n_regions; call.tid = tid; call.regions = regions; call.chunk_first = chunk_first; call.chunks = chunks;
    return bam_evidence_device<vapor_readplan::SigLayout>(ctx, bam, "vapor_bam_signature_device", call, out, status,
                                                          [&](hipStream_t st, const uint8_t* arena, const auto& M, uint8_t* d_meta) {
        hipLaunchKernelGGL(bam_signature_kernel, dim3((unsigned)n_regions), dim3(64), 0, st, arena, M.regs.in(d_meta), M.spans.in(d_meta), M.blk_status.in(d_meta),
                           (int)n_regions, M.ans.in(d_meta), M.reg_status.in(d_meta));
    });
}

// bam_link_kernel: LINK_ANSWER_WORDS words a region; the partner names go up once, inside the call's metadata block
extern "C" int vapor_bam_links_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* regions, const uint8_t* names,
                                      int64_t names_len, const int32_t* chunk_first, const uint64_t* chunks, int64_t* out, int32_t* status)
{
    using namespace vapor_bamdev;
    vapor_readplan::LinkCall call;
    call.n_regions = n_regions; call.tid = tid; call.regions = regions; call.names = names; call.names_len = names_len;
    call.chunk_first = chunk_first; call.chunks = chunks;
    return bam_evidence_device<vapor_readplan::LinkLayout>(ctx, bam, "vapor_bam_links_device", call, out, status,
                                                           [&](hipStream_t st, const uint8_t* arena, const auto& M, uint8_t* d_meta) {
        hipLaunchKernelGGL(bam_link_kernel, dim3((unsigned)n_regions), dim3(64), 0, st, arena, M.regs.in(d_meta), M.spans.in(d_meta), M.blk_status.in(d_meta),
                           M.names.in(d_meta), (uint32_t)names_len, (int)n_regions, M.ans.in(d_meta), M.reg_status.in(d_meta));
    });
}

// bam_support_kernel: SUP_ANSWER_WORDS counts a region
extern "C" int vapor_bam_support_device(vapor_ctx* ctx, vapor_bam* bam, int32_t n_regions, const int32_t* tid, const int64_t* regions,
                                        const int32_t* chunk_first, const uint64_t* chunks, int64_t* out, int32_t* status)
{
    using namespace vapor_bamdev;
    vapor_readplan::SupCall call;
    call.n_regions = n_regions; call.tid = tid; call.regions = regions; call.chunk_first = chunk_first; call.chunks = chunks;
    return bam_evidence_device<vapor_readplan::SupLayout>(ctx, bam, "vapor_bam_support_device", call, out, status,
                                                          [&](hipStream_t st, const uint8_t* arena, const auto& M, uint8_t* d_meta) {
        hipLaunchKernelGGL(bam_support_kernel, dim3((unsigned)n_regions), dim3(64), 0, st, arena, M.regs.in(d_meta), M.spans.in(d_meta), M.blk_status.in(d_meta),
                           (int)n_regions, M.ans.in(d_meta), M.reg_status.in(d_meta));
    });
}

// what the context's last vapor_bam_chop_device did: regions, blocks, compressed bytes sent, inflated bytes, the inflate kernel's
// duration between two events on its stream (ms), the whole call on the host's clock (ms)
extern "C" int vapor_bam_last_stats(vapor_ctx* ctx, double* out, int32_t n)
{
    if (!ctx || !out || n < 0) return fail(VAPOR_E_ARG, "vapor_bam_last_stats: null argument");
    for (int32_t i = 0; i < n && i < 7; ++i) out[i] = ctx->bam_stats[i];
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
// Reference windows from a bgzipped FASTA on the device (vapor_fasta.h).  The windows' virtual-offset ranges are sorted and the
// ranges that share a block or touch are read as one stretch of the file, so that every distinct block is read, sent and
// inflated once however many windows hold it.  Sizes and offsets are 64-bit throughout; a stretch whose data would pass the
// arena's limit leaves its windows to the host (VAPOR_FASTA_ROOM).  Everything runs on the context's own stream and is
// synchronised before the call's blocks go back to the pool (BlockPool: no block is handed back while a kernel may read it).
// ------------------------------------------------------------------------------------------
extern "C" int vapor_fasta_windows_device(vapor_ctx* ctx, int fd, int32_t n, const uint64_t* vbeg, const uint64_t* vend, uint8_t* text,
                                          int64_t text_cap, int64_t* text_off, uint8_t* traits, int32_t* status)
{
    using namespace vapor_bamdev;
    using namespace vapor_fasta;
    using namespace vapor_readplan;
    if (!ctx || fd < 0 || n < 0 || text_cap < 0 || !text_off || (n && (!vbeg || !vend || !traits || !status)) || (text_cap && !text))
        return fail(VAPOR_E_ARG, "vapor_fasta_windows_device: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    const double t0 = now_ms();
    return guarded("vapor_fasta_windows_device", [&]() -> int {
        // ---- what to read: the windows in file order, merged into stretches ---------------------------------------------------
        const FastaCall call{n, vbeg, vend, text_cap};
        StretchPlan plan;
        plan_stretches(call, status, traits, plan);
        stage_stretches(plan, [&](int64_t file_off, uint8_t* h) { return (size_t)std::max<ssize_t>(pread(fd, h, 64, (off_t)file_off), 0); });
        CallScope sc(ctx, ctx->stream);
        InflateStage stage(sc);
        HostBlock<> h_text(sc);
        Block<> d_arena(sc), d_text(sc);
        HIPCHK(stage.begin((size_t)plan.stage_bytes));
        // ---- read and scan the stretches --------------------------------------------------------------------------------------
        uint64_t read_bytes = 0;
        for (FaStretch& s : plan.sts) {
            if (!s.room) continue;
            s.got = stage.read(fd, s.stage_off, s.want, s.c0);
            read_bytes += s.got;
            vapor_bgzf::scan_stretch(s, stage.h_comp);
        }
        // ---- layout: the arena, the block table, the windows, the metadata block ----------------------------------------------
        FastaLayout L;
        layout_arena(plan, L);
        place_windows(call, plan, status, L);
        const FastaMeta M(n, L.blks.size());
        if (const int rc = stage.alloc(M.bytes, M.bytes)) return rc;
        HIPCHK(d_arena.ensure((size_t)L.arena + 64));
        HIPCHK(d_text.ensure((size_t)std::max<uint64_t>(L.slots, 64)));
        HIPCHK(h_text.ensure((size_t)std::max<uint64_t>(L.slots, 64)));
        uint8_t *const h_meta = stage.h_meta, *const d_meta = stage.d_meta;
        M.fill(h_meta, L, status, n);
        // ---- the device: copies, two kernels, the answers back -----------------------------------------------------------------
        hipStream_t st = ctx->stream;
        if (const int rc = stage.run(L.blks.size(), M.in_bytes, M.blks.in(d_meta), M.blk_status.in(d_meta), d_arena, ctx->fasta_ev)) return rc;
        if (n) {
            hipLaunchKernelGGL(fasta_window_kernel, dim3((unsigned)(((size_t)n + WIN_WAVES - 1) / WIN_WAVES)), dim3(64 * WIN_WAVES), 0, st, d_arena,
                               M.wins.in(d_meta), (int)n, M.blk_status.in(d_meta), d_text, M.text_len.in(d_meta), M.traits.in(d_meta), M.status.in(d_meta));
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ctx->fasta_ev[1], st));
        HIPCHK(hipMemcpyAsync(M.back(h_meta), M.back(d_meta), M.back_bytes(), hipMemcpyDeviceToHost, st));
        if (L.slots) HIPCHK(hipMemcpyAsync(h_text, d_text, (size_t)L.slots, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        sc.settled();
        // ---- the texts, one after the other ------------------------------------------------------------------------------------
        gather_texts(n, M, h_meta, h_text, L.wins, text, text_off, traits, status);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->fasta_ev[0], ctx->fasta_ev[1]) != hipSuccess) ms = 0.f;
        ctx->fasta_stats[0] = n; ctx->fasta_stats[1] = (double)L.blks.size(); ctx->fasta_stats[2] = (double)read_bytes;
        ctx->fasta_stats[3] = (double)L.arena; ctx->fasta_stats[4] = ms; ctx->fasta_stats[5] = now_ms() - t0;
        return VAPOR_OK;
    });
}

// what the context's last vapor_fasta_windows_device did: windows, distinct blocks inflated, compressed bytes read and sent,
// inflated bytes, the two kernels between two events on the stream (ms), the whole call on the host's clock (ms)
extern "C" int vapor_fasta_last_stats(vapor_ctx* ctx, double* out, int32_t n)
{
    if (!ctx || !out || n < 0) return fail(VAPOR_E_ARG, "vapor_fasta_last_stats: null argument");
    for (int32_t i = 0; i < n && i < 6; ++i) out[i] = ctx->fasta_stats[i];
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
static void plan_free_device(vapor_plan* p)
{
    dfree(p->ctx, p->d_pairs); p->d_pairs = nullptr;
    dfree(p->ctx, p->d_tasks); p->d_tasks = nullptr;
    dfree(p->ctx, p->d_atasks); p->d_atasks = nullptr;
    dfree(p->ctx, p->d_task_pairs); p->d_task_pairs = nullptr;
    dfree(p->ctx, p->d_hits); p->d_hits = nullptr;
    dfree(p->ctx, p->d_hflags); p->d_hflags = nullptr;
    dfree(p->ctx, p->d_nhits); p->d_nhits = nullptr;
    dfree(p->ctx, p->d_stats); p->d_stats = nullptr;
    p->reads.release(p->ctx);
    dfree(p->ctx, p->d_shares); p->d_shares = nullptr;
    dfree(p->ctx, p->d_maps); p->d_maps = nullptr;
    dfree(p->ctx, p->d_serve); p->d_serve = nullptr;
    dfree(p->ctx, p->d_clean_order); p->d_clean_order = nullptr;
    p->grid.release(p->ctx);
}

extern "C" int vapor_plan_destroy(vapor_plan* p)
{
    if (!p) return VAPOR_OK;
    (void)hipSetDevice(p->device);
    if (p->ring_n > 0 && p->lane && ctx_alive(p->ctx)) {                                       // steps in flight use the blocks
        (void)hipStreamSynchronize(p->lane);
        if (p->fin) (void)hipStreamSynchronize(p->fin);
    }
    if (ctx_alive(p->ctx))
        for (auto& q : p->ctx->lane_plan)
            if (q == p) q = nullptr;
    plan_free_device(p);
    hfree(p->ctx, p->h_stats);
    hfree(p->ctx, p->h_overflow);
    dfree(p->ctx, p->d_overflow);
    dfree(p->ctx, p->d_big_list);
    for (auto& e : p->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& r : p->ring)
        for (auto& e : r)
            if (e) (void)hipEventDestroy(e);
    hfree(p->ctx, p->h_loci);
    for (auto& e : p->ev_f)
        if (e) (void)hipEventDestroy(e);
    if (p->ev_t0) (void)hipEventDestroy(p->ev_t0);
    if (p->ev_last) (void)hipEventDestroy(p->ev_last);
    if (p->ev_clean) (void)hipEventDestroy(p->ev_clean);
    if (p->ev_fin) (void)hipEventDestroy(p->ev_fin);
    if (p->ev_after) (void)hipEventDestroy(p->ev_after);
    delete p;
    return VAPOR_OK;
}

// lays out the hit workspace from hp[].cap (clean_plan::lay_slots) and (re)allocates it
static int plan_alloc_hits(vapor_plan* p)
{
    const int64_t tot = clean_plan::lay_slots(p->hp, p->serve);
    HIPCHK(hipStreamSynchronize(p->ctx->stream));      // (a rerun: nothing may still read the old slots when they are reused)
    dfree(p->ctx, p->d_hits); p->d_hits = nullptr;
    dfree(p->ctx, p->d_hflags); p->d_hflags = nullptr;
    HIPCHK(dmalloc(p->ctx, (void**)&p->d_hits, (size_t)tot * sizeof(unsigned long long)));
    HIPCHK(dmalloc(p->ctx, (void**)&p->d_hflags, (size_t)tot));
    p->total_cap = tot;
    HIPCHK(hipMemcpyAsync(p->d_pairs, p->hp.data(), sizeof(DPair) * p->hp.size(), hipMemcpyHostToDevice, p->ctx->stream));
    if (p->n_dpairs)                                    // the served pairs' view of the shared dot plots' slots
        HIPCHK(hipMemcpyAsync(p->d_serve, p->serve.data(), sizeof(DServe) * p->serve.size(), hipMemcpyHostToDevice, p->ctx->stream));
    return VAPOR_OK;
}

extern "C" int vapor_plan_create(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs,
                                 vapor_plan** out)
{
    if (!ctx || !set || !out || n_pairs < 0 || (n_pairs && !pairs))
        return fail(VAPOR_E_ARG, "vapor_plan_create: null argument");
    if (n_pairs > 0x7FFFFFF0LL) return fail(VAPOR_E_ARG, "too many pairs");
    HIPCHK(hipSetDevice(ctx->device));
    CallScope sc(ctx, ctx->stream);
    std::unique_ptr<vapor_plan, Building<vapor_plan, vapor_plan_destroy>> p(new (std::nothrow) vapor_plan(), {&sc});
    if (!p) return fail(VAPOR_E_NOMEM, "out of memory");
    p->ctx = ctx;
    p->device = ctx->device;
    p->set = set;
    p->n_pairs = n_pairs;
    // (join_align 1: the aligned table is made by the plan's first asynchronous step, join_table_for_async - a plan that is only ever
    // run blocking, a pipeline chunk's, does not pay for it: 2.8 ms of host time on 40 000 joins)
    p->params = PlanParams{ctx->reads_per_task, ctx->join_tasks, ctx->max_pair_cap, ctx->shared_join,
                           tile_pos<JoinCfg, 2>(), tile_pos<JoinCfg, 4>(), ctx->join_align == 2};
    static_cast<PlanLayout&>(*p) = plan_layout(p->params,
                                               SetView{set->h, set->n, set->n_lit, set->derived, set->groups, set->group_of, set->slot_of},
                                               n_pairs, pairs);
    p->join_align = ctx->join_align;
    // (join_align 2: the aligned table is the plan's only one - blocking runs, asynchronous steps and vapor_debug_plan_tasks see it)
    if (p->join_align == 2) { p->tasks = p->atasks; p->launches = p->alaunches; p->model[0] = p->model[1]; }
    p->hcap_want = (int)std::min<int64_t>(p->hwant, CLEAN_HCAP_MAX);
    p->n_dpairs = (int64_t)p->shares.size();
    HIPCHK(dmalloc(ctx, (void**)&p->d_pairs, sizeof(DPair) * p->hp.size()));
    HIPCHK(dmalloc(ctx, (void**)&p->d_tasks, sizeof(DTask) * std::max<size_t>(p->tasks.size(), 1)));
    HIPCHK(dmalloc(ctx, (void**)&p->d_task_pairs, sizeof(int32_t) * std::max<size_t>(p->task_pairs.size(), 1)));
    HIPCHK(dmalloc(ctx, (void**)&p->d_nhits, sizeof(unsigned long long) * p->hp.size()));
    HIPCHK(hipMemsetAsync(p->d_nhits, 0, sizeof(unsigned long long) * p->hp.size(), ctx->stream));
    HIPCHK(dmalloc(ctx, (void**)&p->d_stats, sizeof(long long) * 16 * p->hp.size()));
    HIPCHK(hmalloc(ctx, (void**)&p->h_stats, sizeof(long long) * 16 * p->hp.size()));
    HIPCHK(dmalloc(ctx, (void**)&p->d_overflow, 4 * sizeof(unsigned int)));
    HIPCHK(hipMemsetAsync(p->d_overflow, 0, 4 * sizeof(unsigned int), ctx->stream));
    HIPCHK(dmalloc(ctx, (void**)&p->d_big_list, sizeof(int32_t) * p->hp.size()));
    HIPCHK(hmalloc(ctx, (void**)&p->h_overflow, 2 * sizeof(unsigned int)));
    if (p->n_dpairs) {
        HIPCHK(dmalloc(ctx, (void**)&p->d_shares, sizeof(DShare) * p->shares.size()));
        HIPCHK(dmalloc(ctx, (void**)&p->d_maps, sizeof(int32_t) * std::max<size_t>(p->tables.size(), 1)));
        HIPCHK(dmalloc(ctx, (void**)&p->d_serve, sizeof(DServe) * p->serve.size()));
        HIPCHK(hipMemcpyAsync(p->d_shares, p->shares.data(), sizeof(DShare) * p->shares.size(), hipMemcpyHostToDevice, ctx->stream));
        if (!p->tables.empty())
            HIPCHK(hipMemcpyAsync(p->d_maps, p->tables.data(), sizeof(int32_t) * p->tables.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    // (a plan of many rounds of clean workgroups has no tail worth ordering for - cfg3's 62 rounds gain nothing - and sorting
    // 80 000 pairs costs a pipeline chunk's plan 3-4 ms: the order is made for plans of up to eight rounds)
    if (ctx->clean_order && n_pairs > 1 && n_pairs <= (int64_t)8 * CLEAN_PER_CU_MAX * ctx->n_cus) {
        HIPCHK(dmalloc(ctx, (void**)&p->d_clean_order, sizeof(int32_t) * (size_t)n_pairs));
        const std::vector<int32_t> ord = clean_order(*p, n_pairs);
        HIPCHK(hipMemcpy(p->d_clean_order, ord.data(), sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice));
    }
    for (auto& e : p->ev) HIPCHK(hipEventCreate(&e));
    for (auto& e : p->ev_f) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventCreate(&p->ev_t0));
    // (the copies read the plan's own vectors: a plan that fails here is destroyed after its stream is synchronised)
    if (!p->tasks.empty())
        HIPCHK(hipMemcpyAsync(p->d_tasks, p->tasks.data(), sizeof(DTask) * p->tasks.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!p->task_pairs.empty())
        HIPCHK(hipMemcpyAsync(p->d_task_pairs, p->task_pairs.data(), sizeof(int32_t) * p->task_pairs.size(), hipMemcpyHostToDevice, ctx->stream));
    if (const int rc = plan_alloc_hits(p.get())) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    p->last_stats.assign((size_t)n_pairs * 16, 0);
    *out = p.release();
    return VAPOR_OK;
}

template <int BPS, int K>
static void launch_join(vapor_plan* p, const Launch& L, const DTask* d_tasks, bool first, hipStream_t st)
{
    const vapor_seqset* s = p->set;
    if (BPS == 2 && L.exc == 1)
        hipLaunchKernelGGL((join_kernel<JoinCfg, BPS, K, (BPS == 2 ? 1 : 0)>), dim3((unsigned)L.n_tasks), dim3(JoinCfg::THREADS), JOIN_DYN_LDS(BPS),
                           st, s->d_seqs, s->d_p2, s->d_e1, s->d_x4, p->d_pairs, d_tasks + L.task_begin,
                           p->d_task_pairs, p->d_hits, p->d_nhits, first ? p->d_overflow : (unsigned int*)nullptr);
    else if (BPS == 2 && L.exc == 2)
        hipLaunchKernelGGL((join_kernel<JoinCfg, BPS, K, (BPS == 2 ? 2 : 0)>), dim3((unsigned)L.n_tasks), dim3(JoinCfg::THREADS), JOIN_DYN_LDS(BPS),
                           st, s->d_seqs, s->d_p2, s->d_e1, s->d_x4, p->d_pairs, d_tasks + L.task_begin,
                           p->d_task_pairs, p->d_hits, p->d_nhits, first ? p->d_overflow : (unsigned int*)nullptr);
    else
        hipLaunchKernelGGL((join_kernel<JoinCfg, BPS, K, 0>), dim3((unsigned)L.n_tasks), dim3(JoinCfg::THREADS), JOIN_DYN_LDS(BPS),
                           st, s->d_seqs, s->d_p2, s->d_e1, s->d_x4, p->d_pairs, d_tasks + L.task_begin,
                           p->d_task_pairs, p->d_hits, p->d_nhits, first ? p->d_overflow : (unsigned int*)nullptr);
}

// The clean launch: vapor_clean_plan.h says how many records a workgroup stages, how its LDS is carved, which compiled width the
// value range takes and who cuts the served pairs' records; here are the launches and a developer build's overrides.
template <typename... A>
static void launch_clean(int range_words_cap, unsigned grid, size_t lds, hipStream_t st, A... a)
{
    const int per = clean_plan::width(range_words_cap);
    if (per == 4) hipLaunchKernelGGL(clean_kernel<4>, dim3(grid), dim3(CLEAN_THREADS), lds, st, a...);
    else if (per == 8) hipLaunchKernelGGL(clean_kernel<8>, dim3(grid), dim3(CLEAN_THREADS), lds, st, a...);
    else hipLaunchKernelGGL(clean_kernel<CLEAN_PER_MAX>, dim3(grid), dim3(CLEAN_THREADS), lds, st, a...);
}

static clean_plan::Geom clean_geom(int range_words_cap, int want, bool exact = false)
{
    clean_plan::Geom g = clean_plan::geom(range_words_cap, want, exact);
#ifdef VAPOR_DEV_BUILD
    const char* dual = getenv("VAPOR_DEV_CLEAN_DUAL");               // experiment: the layout, whatever it costs in residency
    if (dual) g = clean_plan::geom_for(range_words_cap, want, atoi(dual) != 0, exact);
    if (const char* e = getenv("VAPOR_DEV_HCAP")) g = clean_plan::Geom{atoi(e) & ~3, 1, dual ? g.dual : true};   // experiment: records staged per pair
#endif
    return g;
}
static clean_plan::Geom clean_geom(const vapor_plan* p) { return clean_geom(p->range_words_cap, p->hcap_want, p->hcap_measured); }

static bool remap_in_clean(const vapor_plan* p, const clean_plan::Geom& cg)
{
    return clean_plan::remap_in_clean(p->ctx->remap_in_clean, p->n_dpairs, p->n_pairs, cg.per_cu, p->ctx->n_cus);
}

static void launch_clean_big(int64_t n_pairs, int rw, hipStream_t st, const DPair* pairs, const unsigned long long* n_hits,
                             const unsigned long long* hits, uint8_t* hflags, long long* stats, const unsigned int* overflow, const int32_t* big_list)
{
    const clean_plan::Layout big = clean_plan::big_layout(rw);
    hipLaunchKernelGGL(clean_big_kernel, dim3((unsigned)std::min<int64_t>(n_pairs, CLEAN_BIG_GRID)), dim3(CLEAN_THREADS), big.big_bytes(), st,
                       pairs, n_hits, hits, hflags, stats, rw, big.groups_cap, overflow, big_list);
}

static int async_fold(vapor_plan* p);

// Which task table an asynchronous step takes under join_align 1.  Blocking runs always take the cost-balanced table: there one
// plan's latency is what the caller waits for, and the aligned table's dearer tasks are that latency.  The same holds for the
// asynchronous steps of ONE plan, which lie behind each other on its stream (cfg2, one plan: 0.1679-0.1694 -> 0.1733-0.1744 ms a
// pass with the aligned table, join 0.079 -> 0.084), so a step takes the aligned table only while a step of another plan is in
// flight on the context's other lane (by the host's books: it has enqueued steps nobody has waited for yet) - then the CUs the
// fewer or shorter join tasks leave go to that plan's clean workgroups.
// Measured with two plans in flight, join_align 0 against 2, five alternating runs each on one box, no two ranges overlapping
// (profiles/join_align.txt), beside what the planner's cost units (TableModel) say of the two tables:
//   cfg2   0.1241-0.1248 -> 0.1223-0.1230 ms   300 -> 250 builds   sum of the tasks -3.0 %   dearest task +9.5 %
//   cfg3   3.210-3.219   -> 3.172-3.178        1700 -> 1000        -1.7 %                    -25 %  (1 000 tasks of 40 reads for 768 of 52)
//   small  0.7772-0.7795 -> 0.7670-0.7695      2671 -> 2000        -2.5 %                    -57 %  (2 000 tasks)
// The aligned table won on all three, so the sweep gives no shape where it loses with two plans in flight; the two thresholds
// are the edges of what was measured, not of what wins: a saving of at least 1.5 % of the tasks' sum (cfg3's 1.7 % is the
// smallest that was seen to pay; below it the model sees less than a run can tell from noise) and a dearest task at most 10 %
// dearer than the balanced table's (cfg2's 9.5 % is the dearest that was seen to pay).  Between and beyond these shapes the rule
// is a guess - a plan whose aligned tasks are 20 % dearer for 5 % fewer builds may well win and is turned down.
constexpr int JOIN_ALIGN_MIN_SAVING_PM = 15;       // per mille of the balanced table's sum
constexpr int JOIN_ALIGN_MAX_DEARER_PCT = 10;
static bool join_align_pays(const TableModel& bal, const TableModel& ali)
{
    return ali.n_tasks > 0 && (bal.sum - ali.sum) * 1000 >= bal.sum * JOIN_ALIGN_MIN_SAVING_PM && ali.path * 100 <= bal.path * (100 + JOIN_ALIGN_MAX_DEARER_PCT);
}
static int join_table_for_async(vapor_plan* p, hipStream_t st, int* table)
{
    *table = 0;
    if (p->join_align != 1) return VAPOR_OK;                   // (0 and 2: the plan has one table)
    const vapor_ctx* c = p->ctx;
    if (c->user_stream || p->lane_ix < 0) return VAPOR_OK;     // (one stream for every plan: nothing runs beside this step)
    // a step of another plan in flight beside this one, by the host's own books: the plan enqueued last on the other lane has
    // steps that no vapor_plan_sync or blocking run has waited for yet (no question to the device: the same calls take the same tables)
    const vapor_plan* o = c->lane_plan[1 - p->lane_ix];
    if (!o || o == p || o->ring_n <= 0) return VAPOR_OK;
    if (!p->aligned_made) {
        const vapor_seqset* s = p->set;
        plan_aligned(p->params, SetView{s->h, s->n, s->n_lit, s->derived, s->groups, s->group_of, s->slot_of}, p);
        p->aligned_made = true;
        if (!p->atasks.empty() && join_align_pays(p->model[0], p->model[1])) {
            // (on the step's own stream, in front of its join; `atasks` lives as long as the plan)
            HIPCHK(dmalloc(p->ctx, (void**)&p->d_atasks, sizeof(DTask) * p->atasks.size()));
            HIPCHK(hipMemcpyAsync(p->d_atasks, p->atasks.data(), sizeof(DTask) * p->atasks.size(), hipMemcpyHostToDevice, st));
        }
    }
    if (p->d_atasks) *table = 1;                               // (else: the model does not see the aligned table pay)
    return VAPOR_OK;
}

// keep_flags: the clean kernel writes the per-record flag bytes beside the pairs' records - what vapor_plan_fetch_hits hands out;
// the device-finished path (vapor_plan_run_loci*) needs the statistics only and leaves that pass out.
// `table`: the join's task table, 0 the plan's own (`tasks`), 1 the window-aligned one beside it (`atasks`, join_align 1).  The
// tables cut the same sorted pair list and a pair lies whole inside one task of either, so what a pair's records are does not
// depend on the table (tests/test_gpu_join_align.py holds the library to that).
static int plan_run_once(vapor_plan* p, int table, bool fetch_stats = true, hipEvent_t* evs = nullptr, hipStream_t on = nullptr, bool skip_big = false,
                         hipEvent_t before_clean = nullptr, bool keep_flags = true)
{
    vapor_ctx* c = p->ctx;
    hipStream_t st = on ? on : c->stream;
    hipEvent_t* ev = evs ? evs : p->ev;
    if (table == 1 && !p->d_atasks) table = 0;
    const std::vector<Launch>& launches = table == 1 ? p->alaunches : p->launches;
    const DTask* d_tasks = table == 1 ? p->d_atasks : p->d_tasks;
    p->last_table = table;
    // no memsets in the steady state: the pair counts are stored whole by the join, the clean kernels' two
    // counters are cleared by the first join launch
    if (launches.empty()) HIPCHK(hipMemsetAsync(p->d_overflow, 0, 2 * sizeof(unsigned int), st));
    HIPCHK(hipEventRecord(ev[0], st));       // start of the run and of the join
    bool first = true;
    for (const Launch& L : launches) {
        if (L.bps == 2) {
            if (L.k == 10) launch_join<2, 10>(p, L, d_tasks, first, st);
            else if (L.k == 20) launch_join<2, 20>(p, L, d_tasks, first, st);
            else if (L.k == 30) launch_join<2, 30>(p, L, d_tasks, first, st);
            else launch_join<2, 40>(p, L, d_tasks, first, st);
        } else {
            if (L.k == 10) launch_join<4, 10>(p, L, d_tasks, first, st);
            else if (L.k == 20) launch_join<4, 20>(p, L, d_tasks, first, st);
            else if (L.k == 30) launch_join<4, 30>(p, L, d_tasks, first, st);
            else launch_join<4, 40>(p, L, d_tasks, first, st);
        }
        first = false;
        HIPCHK(hipGetLastError());
    }
    const clean_plan::Geom cg = clean_geom(p);
    const bool in_clean = remap_in_clean(p, cg);
#if defined(VAPOR_AB) && VAPOR_AB == 3               /* (developer variant 3: the shared joins without their remap) */
    if (false) {
#else
    if (p->n_dpairs && !in_clean) {
#endif
        hipLaunchKernelGGL(remap_kernel, dim3((unsigned)p->n_dpairs), dim3(256), 0, st, (const DPair*)p->d_pairs, (const DShare*)p->d_shares,
                           (const int32_t*)p->d_maps, p->d_hits, p->d_nhits, p->d_overflow);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ev[1], st));
    // (the clean kernels overwrite the statistics the previous step's finish kernel reads on its own stream)
    if (before_clean) HIPCHK(hipStreamWaitEvent(st, before_clean, 0));
    if (p->n_pairs > 0) {
        const clean_plan::Layout lay = clean_plan::staged_layout(p->range_words_cap, cg.hcap, cg.dual);
        size_t lds = clean_plan::launch_bytes(lay, in_clean);
#ifdef VAPOR_DEV_BUILD
        if (const char* e = getenv("VAPOR_DEV_CLEAN_PAD")) lds += (size_t)atoi(e);   // experiment: fewer workgroups per CU
#endif
        launch_clean(p->range_words_cap, (unsigned)p->n_pairs, lds, st,
                     (const DPair*)p->d_pairs, (const int32_t*)p->d_clean_order, p->d_nhits,
                     p->d_hits, p->d_hflags, p->d_stats, p->range_words_cap,
                     lay.groups_cap, lay.hcap, p->d_overflow, p->d_big_list, skip_big ? 0 : 1, cg.dual ? 1 : 0,
                     in_clean ? (const DServe*)p->d_serve : (const DServe*)nullptr, (const int32_t*)p->d_maps, keep_flags ? 1 : 0);
        HIPCHK(hipGetLastError());
        p->flags_valid = keep_flags;
        // (clean_big_kernel needs a CU with free LDS like any other clean workgroup: behind another plan's join it sits
        // on the stream until that join is over even with nothing to do, and holds back the finish kernel and the
        // plan's next step with it - so an asynchronous step leaves it out when the plan's blocking run left it no pair)
        if (!skip_big) {
            launch_clean_big(p->n_pairs, p->range_words_cap, st, p->d_pairs, p->d_nhits, p->d_hits, p->d_hflags, p->d_stats, p->d_overflow, p->d_big_list);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipEventRecord(ev[2], st));
    if (p->n_pairs > 0 && fetch_stats)
        HIPCHK(hipMemcpyAsync(p->h_stats, p->d_stats, sizeof(long long) * 16 * (size_t)p->n_pairs, hipMemcpyDeviceToHost, st));
    if (!fetch_stats) return VAPOR_OK;          // device-side finishing: the statistics stay in HBM
    HIPCHK(hipEventRecord(ev[3], st));
    HIPCHK(hipStreamSynchronize(st));
    float a = 0, b = 0, t = 0;
    HIPCHK(hipEventElapsedTime(&a, ev[0], ev[1]));
    HIPCHK(hipEventElapsedTime(&b, ev[1], ev[2]));
    HIPCHK(hipEventElapsedTime(&t, ev[0], ev[3]));
    p->t_join = a; p->t_clean = b; p->t_total = t;
    return VAPOR_OK;
}

extern "C" int vapor_plan_run(vapor_plan* p, int64_t* stats)
{
    if (!p || (p->n_pairs && !stats)) return fail(VAPOR_E_ARG, "vapor_plan_run: null argument");
    HIPCHK(hipSetDevice(p->ctx->device));
    if (p->ring_n > 0) {                        // asynchronous steps in flight share the workspace: let them finish
        int rc0 = async_fold(p);
        if (rc0 != VAPOR_OK) return rc0;
    }
    p->n_retried = 0;
    // The shared dot plots' packed counters, fetched after every run.  The copy of the LAST run serves what follows the loop too:
    // the loop ends either where nothing grew, or after the third run's plan_alloc_hits, which allocates the record slots anew and
    // uploads pair records - no kernel runs and nothing writes d_nhits between that copy and the end of the loop.
    std::vector<unsigned long long> plots((size_t)p->n_dpairs);
    for (int attempt = 0; attempt < 3; ++attempt) {
        int rc = plan_run_once(p, 0);
        if (rc != VAPOR_OK) return rc;
        if (p->n_dpairs)
            HIPCHK(hipMemcpy(plots.data(), p->d_nhits + p->n_pairs, sizeof(unsigned long long) * plots.size(), hipMemcpyDeviceToHost));
        // pairs and plots whose record count exceeded their slot: enlarge to the exact count and rerun
        const int64_t grow = clean_plan::grow_slots(p->h_stats, p->n_pairs, plots, p->ctx->max_pair_cap, p->hp);
        if (!grow) break;
        p->n_retried += (int)grow;
        rc = plan_alloc_hits(p);
        if (rc != VAPOR_OK) return rc;
    }
    if (p->ctx->clean_fit && p->n_pairs > 0) {
        // the clean kernel's geometry from what the pairs really hold (clean_plan::measured_want)
        std::vector<unsigned long long> cnt((size_t)p->n_pairs);
        HIPCHK(hipMemcpy(cnt.data(), p->d_nhits, sizeof(unsigned long long) * cnt.size(), hipMemcpyDeviceToHost));
        if (const int want = clean_plan::measured_want(cnt, p->status)) {
            p->hcap_want = want;
            p->hcap_measured = true;
        }
    }
    clean_plan::refuse_truncated_plots(plots, p->hp, p->n_pairs, p->shares, p->status);
    clean_plan::mask_refused(p->h_stats, p->status, p->n_pairs);
    memcpy(p->last_stats.data(), p->h_stats, sizeof(int64_t) * 16 * (size_t)p->n_pairs);
    memcpy(stats, p->h_stats, sizeof(int64_t) * 16 * (size_t)p->n_pairs);
    p->ran = true;
    return VAPOR_OK;
}

extern "C" int vapor_plan_timings(vapor_plan* p, double* ms, int32_t n)
{
    if (!p || !ms) return fail(VAPOR_E_ARG, "vapor_plan_timings: null argument");
    const clean_plan::Geom cg = clean_geom(p);
    const TableModel& tm = p->model[p->last_table];
    double v[12] = {p->t_join, p->t_clean, p->t_total, (double)p->launches.size(), (double)p->n_retried, p->t_finish,
                    (double)p->n_served, (double)p->n_dpairs, (double)cg.per_cu, remap_in_clean(p, cg) ? 1.0 : 0.0,
                    (double)tm.n_tasks, (double)tm.builds};
    for (int i = 0; i < n && i < 12; ++i) ms[i] = v[i];
    return VAPOR_OK;
}

extern "C" int vapor_plan_record_counts(vapor_plan* p, int64_t* records)
{
    if (!p || !records) return fail(VAPOR_E_ARG, "vapor_plan_record_counts: null argument");
    if (!p->ran) return fail(VAPOR_E_ARG, "vapor_plan_record_counts: plan has not been run");
    HIPCHK(hipSetDevice(p->ctx->device));
    std::vector<unsigned long long> cnt((size_t)std::max<int64_t>(p->n_pairs, 1));
    HIPCHK(hipMemcpy(cnt.data(), p->d_nhits, sizeof(unsigned long long) * (size_t)p->n_pairs, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < p->n_pairs; ++i) records[i] = (int64_t)(uint32_t)cnt[i];
    return VAPOR_OK;
}

extern "C" int vapor_plan_algorithmic_bytes(vapor_plan* p, int64_t* bytes, int64_t* cells)
{
    if (!p || !bytes || !cells) return fail(VAPOR_E_ARG, "null argument");
    int64_t b = 0, c = 0;
    for (int64_t i = 0; i < p->n_pairs; ++i) {
        if (p->status[i] != 0) continue;
        int64_t n1 = p->set->h[p->hp[i].seq1].len;
        int64_t n2 = std::max<int64_t>(0, (int64_t)p->set->h[p->hp[i].seq2].len - p->hp[i].off2);
        int64_t nh = p->ran ? p->last_stats[16 * i] : 0;
        b += (3 * n1 + 7) / 8 + (3 * n2 + 7) / 8 + 8 * nh + 128;
        c += n1 * n2;
    }
    *bytes = b;
    *cells = c;
    return VAPOR_OK;
}

extern "C" int vapor_plan_fetch_hits(vapor_plan* p, int64_t n_sel, const int64_t* pair_idx, int32_t* hits_ji,
                                     uint8_t* hit_flags, int64_t capacity, int64_t* hit_off)
{
    if (!p || n_sel < 0 || (n_sel && (!pair_idx || !hit_off))) return fail(VAPOR_E_ARG, "vapor_plan_fetch_hits: null argument");
    if (!p->ran) return fail(VAPOR_E_ARG, "vapor_plan_fetch_hits: plan has not been run");
    HIPCHK(hipSetDevice(p->ctx->device));
    if (hit_flags && (!p->flags_valid || p->ring_n > 0)) {
        // the last pass was a device-finished one (vapor_plan_run_loci*), which writes no per-record flags: run once more, with them
        int rc0 = vapor_plan_run(p, p->last_stats.data());
        if (rc0 != VAPOR_OK) return rc0;
    }
    std::vector<long long> off((size_t)n_sel + 1, 0), sel((size_t)std::max<int64_t>(n_sel, 1), 0);
    for (int64_t q = 0; q < n_sel; ++q) {
        int64_t i = pair_idx[q];
        if (i < 0 || i >= p->n_pairs) return fail(VAPOR_E_ARG, "pair index out of range");
        sel[q] = i;
        int64_t n = (p->last_stats[16 * i + 15] == 0) ? p->last_stats[16 * i] : 0;
        off[q + 1] = off[q] + n;
    }
    for (int64_t q = 0; q <= n_sel; ++q) hit_off[q] = off[q];
    if (off[n_sel] > capacity) return fail(VAPOR_E_OVERFLOW, "hit buffer too small");
    if (n_sel == 0 || off[n_sel] == 0) return VAPOR_OK;
    if (!hits_ji) return fail(VAPOR_E_ARG, "null hit buffer");
    // record counts of the selected pairs (the low half of the join's packed counters)
    std::vector<unsigned long long> cnt((size_t)p->n_pairs);
    HIPCHK(hipMemcpy(cnt.data(), p->d_nhits, sizeof(unsigned long long) * cnt.size(), hipMemcpyDeviceToHost));
    std::vector<long long> nrec((size_t)n_sel, 0);
    for (int64_t q = 0; q < n_sel; ++q)
        if (off[q + 1] > off[q]) nrec[q] = (long long)(uint32_t)cnt[sel[q]];
    hipStream_t st = p->ctx->stream;
    CallScope sc(p->ctx, st);
    Block<long long> d_sel(sc), d_off(sc), d_nrec(sc);
    Block<int32_t> d_ji(sc);
    Block<uint8_t> d_fl(sc);
    HIPCHK(d_sel.ensure(sizeof(long long) * sel.size()));
    HIPCHK(d_off.ensure(sizeof(long long) * off.size()));
    HIPCHK(d_nrec.ensure(sizeof(long long) * nrec.size()));
    HIPCHK(d_ji.ensure(sizeof(int32_t) * 2 * (size_t)off[n_sel]));
    if (hit_flags) HIPCHK(d_fl.ensure((size_t)off[n_sel]));
    HIPCHK(hipMemcpyAsync(d_sel, sel.data(), sizeof(long long) * sel.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_off, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_nrec, nrec.data(), sizeof(long long) * nrec.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)n_sel), dim3(256), 0, st, p->d_pairs, d_sel.p, d_off.p, d_nrec.p, p->d_hits,
                       p->d_hflags, d_ji.p, d_fl.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hits_ji, d_ji, sizeof(int32_t) * 2 * (size_t)off[n_sel], hipMemcpyDeviceToHost, st));
    if (hit_flags) HIPCHK(hipMemcpyAsync(hit_flags, d_fl, (size_t)off[n_sel], hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    sc.settled();
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" int vapor_score_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs,
                                 int64_t* stats)
{
    vapor_plan* p = nullptr;
    int rc = vapor_plan_create(ctx, set, n_pairs, pairs, &p);
    if (rc != VAPOR_OK) return rc;
    rc = vapor_plan_run(p, stats);
    vapor_plan_destroy(p);
    return rc;
}

extern "C" int vapor_dotplot_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs,
                                   int32_t* hits_ji, int64_t hits_capacity, int64_t* hit_off, int64_t* stats)
{
    if (!hit_off) return fail(VAPOR_E_ARG, "vapor_dotplot_batch: null hit_off");
    vapor_plan* p = nullptr;
    int rc = vapor_plan_create(ctx, set, n_pairs, pairs, &p);
    if (rc != VAPOR_OK) return rc;
    std::vector<int64_t> st((size_t)std::max<int64_t>(n_pairs, 1) * 16);
    rc = vapor_plan_run(p, st.data());
    if (rc == VAPOR_OK) {
        std::vector<int64_t> idx((size_t)n_pairs);
        std::iota(idx.begin(), idx.end(), 0);
        rc = vapor_plan_fetch_hits(p, n_pairs, idx.data(), hits_ji, nullptr, hits_capacity, hit_off);
        if (stats) memcpy(stats, st.data(), sizeof(int64_t) * 16 * (size_t)n_pairs);
    }
    vapor_plan_destroy(p);
    return rc;
}

extern "C" int vapor_selfplot_qc(vapor_ctx* ctx, vapor_seqset* set, int32_t n, const int32_t* seq_idx, const int32_t* k,
                                 int64_t* out)
{
    if (n < 0 || (n && (!seq_idx || !k || !out))) return fail(VAPOR_E_ARG, "vapor_selfplot_qc: null argument");
    std::vector<vapor_pair> pr((size_t)n);
    for (int32_t t = 0; t < n; ++t) pr[t] = vapor_pair{seq_idx[t], seq_idx[t], 0, k[t], 0u};
    std::vector<int64_t> st((size_t)std::max(n, 1) * 16);
    int rc = vapor_score_batch(ctx, set, n, pr.data(), st.data());
    if (rc != VAPOR_OK) return rc;
    for (int32_t t = 0; t < n; ++t) {
        if (st[16 * t + 15] != 0) return fail((int)st[16 * t + 15], "vapor_selfplot_qc: pair failed");
        out[3 * t] = st[16 * t];
        out[3 * t + 1] = st[16 * t + 7];
        out[3 * t + 2] = st[16 * t + 8];
    }
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
// Cleaning and reductions on caller-supplied hit lists: what clean_dotdata_diagnal_and_anti_diagnal
// (SF:432-448), clean_dotdata_diagnal_m1b / clean_dotdata_anti_diagnal_m1b (SF:404-430) and the
// eu_dis_* reductions do when handed an explicit dot list instead of a fresh dotdata() result.
// (the refusals of the two list entries and the packing of the narrow one: clean_plan::lists_check, clean_plan::ListPack)
extern "C" int vapor_clean_hits(vapor_ctx* ctx, int64_t n_lists, const int32_t* hits_ji, const int64_t* off,
                                const uint32_t* flags, int64_t* stats, uint8_t* hit_flags)
{
    if (const auto no = clean_plan::lists_check(ctx != nullptr, n_lists, hits_ji, off, stats, VAPOR_MAX_SEQ_LEN, -1)) return refused("vapor_clean_hits", no);
    if (n_lists == 0) return VAPOR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t tot = off[n_lists];
    const clean_plan::ListPack L(n_lists, hits_ji, off, flags);
    const int rw = L.rw;
    std::vector<uint8_t> fl(hit_flags && tot ? L.packed.size() : 0);
    hipStream_t st = ctx->stream;
    CallScope sc(ctx, st);
    Block<DPair> d_dp(sc);
    Block<unsigned long long> d_nh(sc), d_hits(sc);
    Block<unsigned int> d_ov(sc);
    Block<int32_t> d_big(sc);
    Block<uint8_t> d_fl(sc);
    Block<long long> d_st(sc);
    HIPCHK(d_ov.ensure(4 * sizeof(unsigned int)));
    HIPCHK(d_big.ensure(sizeof(int32_t) * L.dp.size()));
    HIPCHK(d_dp.ensure(sizeof(DPair) * L.dp.size()));
    HIPCHK(d_nh.ensure(sizeof(unsigned long long) * L.counts.size()));
    HIPCHK(d_hits.ensure(sizeof(unsigned long long) * L.packed.size()));
    HIPCHK(d_fl.ensure(L.packed.size()));
    HIPCHK(d_st.ensure(sizeof(long long) * 16 * (size_t)n_lists));
    HIPCHK(hipMemsetAsync(d_ov, 0, 4 * sizeof(unsigned int), st));
    HIPCHK(hipMemcpyAsync(d_dp, L.dp.data(), sizeof(DPair) * L.dp.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_nh, L.counts.data(), sizeof(unsigned long long) * L.counts.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_hits, L.packed.data(), sizeof(unsigned long long) * L.packed.size(), hipMemcpyHostToDevice, st));
    const clean_plan::Geom cg = clean_geom(rw, clean_plan::LISTS_WANT);
    const clean_plan::Layout lay = clean_plan::staged_layout(rw, cg.hcap, cg.dual);
    launch_clean(rw, (unsigned)n_lists, clean_plan::launch_bytes(lay, false), st, (const DPair*)d_dp, (const int32_t*)nullptr,
                 d_nh.p, d_hits.p, d_fl.p, d_st.p, rw,
                 lay.groups_cap, lay.hcap, d_ov.p, d_big.p, 1, cg.dual ? 1 : 0,
                 (const DServe*)nullptr, (const int32_t*)nullptr, 1);
    HIPCHK(hipGetLastError());
    launch_clean_big(n_lists, rw, st, d_dp.p, d_nh.p, d_hits.p, d_fl.p, d_st.p, d_ov.p, d_big.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(stats, d_st, sizeof(long long) * 16 * (size_t)n_lists, hipMemcpyDeviceToHost, st));
    if (!fl.empty()) HIPCHK(hipMemcpyAsync(fl.data(), d_fl, fl.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    sc.settled();
    for (int64_t t = 0; !fl.empty() && t < n_lists; ++t) memcpy(hit_flags + off[t], fl.data() + L.poff[t], (size_t)(off[t + 1] - off[t]));
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
// The explicit-dot routes: the wide route (vapor_wide.h; sequences up to VAPOR_MAX_WIDE_SEQ_LEN, explicit dots with 32-bit
// positions) and the any-k route (vapor_anyk.h), one pair at a time.  Their host plan - refusals, sizes, schedules, records - is
// vapor_dots_plan.h's; here: ensure, memset, the launches, the copies and the synchronisations.  The narrow
// entry points above keep their limit and their refusals.
namespace dp = vapor::dots_plan;
static_assert(dp::SKIP_C2D == HF_C2D && sizeof(int2) == 8 && sizeof(int4) == 16, "what vapor_dots_plan.h states without HIP");

namespace {

template <typename Slot, int N>
struct DotBufs {                   // an owner's blocks by slot (vapor_dots_plan.h), each grown to the largest pair so far (Block::ensure)
    Block<> p[N];
    explicit DotBufs(CallScope& sc) { for (auto& q : p) q.sc = &sc; }
    hipError_t ensure(Slot b, size_t bytes) { return p[b].ensure(std::max(bytes, dp::BLOCK_FLOOR)); }
    template <typename T> T* at(Slot b) const { return reinterpret_cast<T*>(p[b].p); }
};
using SharedBufs = DotBufs<dp::SharedSlot, dp::N_SHARED>;
using WideBufs = DotBufs<dp::WideSlot, dp::N_WIDE>;
using AnykBufs = DotBufs<dp::AnykSlot, dp::N_ANYK>;

// Cleaning and reductions of the n > 0 dots in b.DOTS (coordinates i <= maxi, j <= maxj), enqueued on st; the results land in
// b.ACC, which the caller has initialised.
hipError_t wide_clean(SharedBufs& b, hipStream_t st, int n, int maxi, int maxj, uint32_t flags)
{
    const dp::Cleaning c = dp::cleaning(flags);
    const dp::Scratch s = dp::scratch(maxi, maxj);
    hipError_t e = b.ensure(dp::SCR, s.bytes);
    if (e != hipSuccess) return e;
    const int2* dots = b.at<int2>(dp::DOTS);
    uint8_t* fl = b.at<uint8_t>(dp::FL);
    WideAcc* acc = b.at<WideAcc>(dp::ACC);
    uint32_t *cnt = b.at<uint32_t>(dp::SCR), *gid = cnt + s.R, *gsize = gid + s.R;
    const dim3 grid(dp::grid(n)), block(dp::THREADS);
    for (int t = 0; t < c.n_passes; ++t) {
        const dp::ClusterPass& q = c.pass[t];
        if ((e = hipMemsetAsync(cnt, 0, s.axis_bytes(), st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(gsize, 0, s.axis_bytes(), st)) != hipSuccess) return e;
        hipLaunchKernelGGL(wide_hist_kernel, grid, block, 0, st, dots, (const uint8_t*)fl, n, q.axis, s.shift, q.skip, cnt);
        hipLaunchKernelGGL(wide_group_kernel, dim3(1), dim3(WIDE_SCAN_THREADS), 0, st, (const uint32_t*)cnt, s.R, gid, gsize, acc, q.slot);
        hipLaunchKernelGGL(wide_flag_kernel, grid, block, 0, st, dots, fl, n, q.mode, s.shift, flags, (const uint32_t*)gid, (const uint32_t*)gsize,
                           (const WideAcc*)acc);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (c.zero_flags && (e = hipMemsetAsync(fl, 0, (size_t)n, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(wide_reduce_kernel, grid, block, 0, st, dots, fl, n, acc);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (c.dir) {
        if ((e = hipMemsetAsync(cnt, 0, s.axis_bytes(), st)) != hipSuccess) return e;
        hipLaunchKernelGGL(wide_dir_kernel, dim3(1), dim3(WIDE_SCAN_THREADS), 0, st, dots, (const uint8_t*)fl, n, acc, cnt);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

// The per-pair loop of the explicit-dot routes (vapor_wide_batch, vapor_anyk_batch).  A Route supplies three things:
//   admit(view, a)                   the status the pair gets before any device work, 0 to go on (dots_plan::admit_wide / admit_anyk);
//   count(a, s1, s2, shape, &at)     enqueues the count pass and says where on the device the number of dots will stand;
//   emit(a, shape)                   enqueues the dots into b.DOTS.
// The loop owns everything else: the accumulator, the read-back of the total, the pair that outgrows the dot bound, DOTS / FL,
// the cleaning, the copies out and hit_off.  Two synchronisations per scored pair, one for a pair without k-mers.
template <typename Route>
static int dot_pairs(const std::string& who, vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int64_t* stats,
              int32_t* hits_ji, int64_t hits_capacity, int64_t* hit_off)
{
    if (const auto no = dp::call_refusal(dp::Call{dp::BATCH, ctx && set, n_pairs, stats, hits_ji, hit_off, pairs, hits_capacity, 0})) return refused(who, no);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CallScope sc(ctx, st);
    const WideAcc init = dp::acc_init();
    WideAcc res;
    long long total = 0;
    const int64_t cap = dp::dots_cap(ctx->max_pair_cap);
    const dp::SetView view{set->n, set->h.data(), set->raw_off.data(), set->raw_off.size()};
    SharedBufs b(sc);
    Route route(sc, b, set, cap);
    HIPCHK(b.ensure(dp::ACC, sizeof(WideAcc)));
    HIPCHK(route.prepare());
    dp::Capacity room(hits_ji != nullptr, hits_capacity, hit_off);
    for (int64_t t = 0; t < n_pairs; ++t) {
        const vapor_pair& a = pairs[t];
        int64_t* s = stats + 16 * t;
        int64_t n = 0;
        if (const int code = Route::admit(view, a)) {
            dp::record_refused(code, s);
        } else {
            const SeqDesc& s1 = set->h[a.seq1];
            const SeqDesc& s2 = set->h[a.seq2];
            const dp::Shape sh = dp::shape(s1, s2, a);
            HIPCHK(hipMemcpyAsync(b.p[dp::ACC], &init, sizeof(WideAcc), hipMemcpyHostToDevice, st));
            if (sh.kmers()) {
                const long long* d_total = nullptr;
                HIPCHK(route.count(a, s1, s2, sh, &d_total));
                HIPCHK(hipMemcpyAsync(&total, d_total, sizeof(long long), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                if (total > cap) {
                    dp::record_overflowed(total, s);
                    room.close(t, 0);
                    continue;
                }
                n = total;
                HIPCHK(b.ensure(dp::DOTS, sizeof(int2) * (size_t)n));
                HIPCHK(b.ensure(dp::FL, (size_t)n));
                if (n) {
                    HIPCHK(route.emit(a, sh));
                    HIPCHK(wide_clean(b, st, (int)n, sh.nk1 - 1, sh.nk2 - 1, a.flags));
                }
            }
            HIPCHK(hipMemcpyAsync(&res, b.p[dp::ACC], sizeof(WideAcc), hipMemcpyDeviceToHost, st));
            if (room.fits(n)) HIPCHK(hipMemcpyAsync(hits_ji + 2 * room.running, b.p[dp::DOTS], sizeof(int2) * (size_t)n, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            dp::record_folded(res, n, a.flags, s);
        }
        room.close(t, n);
    }
    sc.settled();              // (every pair ended in a synchronisation, a refused one enqueued nothing)
    if (room.overflowed()) return fail(VAPOR_E_OVERFLOW, who + ": hits_capacity too small (hit_off[n_pairs] holds the count needed)");
    return VAPOR_OK;
}

namespace {
struct WideRoute {
    SharedBufs& b;
    WideBufs w;
    hipStream_t st;
    const vapor_seqset* set;
    const unsigned long long cap;                          // the dot bound: the count pass stops booking beyond it
    const uint32_t *x4_1 = nullptr, *x4_2 = nullptr;       // of the pair being counted, for its emit pass
    dp::WideJoin j{};
    WideRoute(CallScope& sc, SharedBufs& bufs, const vapor_seqset* s, int64_t dots_cap)
        : b(bufs), w(sc), st(sc.st), set(s), cap((unsigned long long)dots_cap) {}
    hipError_t prepare() { return w.ensure(dp::WIDE_BOOKED, sizeof(unsigned long long)); }
    static int admit(const dp::SetView& v, const vapor_pair& a) { return dp::admit_wide(v, a); }
    template <int K>
    void join(const vapor_pair& a, const dp::Shape& sh, bool emit)
    {
        const WKey<K>* keys = w.at<const WKey<K>>(dp::WIDE_KEYS);
        const int32_t *head = w.at<int32_t>(dp::WIDE_HEAD), *next = w.at<int32_t>(dp::WIDE_NEXT);
        const dim3 block(dp::THREADS);
        if (!emit) {
            hipLaunchKernelGGL(wide_table_kernel<K>, dim3(j.table_grid), block, 0, st, x4_1, sh.nk1, w.at<WKey<K>>(dp::WIDE_KEYS),
                               w.at<int32_t>(dp::WIDE_HEAD), w.at<int32_t>(dp::WIDE_NEXT), j.mask);
            hipLaunchKernelGGL((wide_probe_kernel<K, false>), dim3(j.probe_grid), block, 0, st, x4_2, a.off2, sh.nk2, keys, head, next, j.mask,
                               w.at<uint32_t>(dp::WIDE_CNT), (const long long*)nullptr, (int2*)nullptr, w.at<unsigned long long>(dp::WIDE_BOOKED), cap);
            hipLaunchKernelGGL(wide_scan_kernel, dim3(j.scan_grid), dim3(WIDE_SCAN_THREADS), 0, st, (const uint32_t*)w.at<uint32_t>(dp::WIDE_CNT), sh.nk2,
                               w.at<long long>(dp::WIDE_OFF));
        } else {
            hipLaunchKernelGGL((wide_probe_kernel<K, true>), dim3(j.probe_grid), block, 0, st, x4_2, a.off2, sh.nk2, keys, head, next, j.mask,
                               (uint32_t*)nullptr, (const long long*)w.at<long long>(dp::WIDE_OFF), b.at<int2>(dp::DOTS), (unsigned long long*)nullptr, cap);
        }
    }
    hipError_t join(const vapor_pair& a, const dp::Shape& sh, bool emit)
    {
        switch (a.k) {
        case 10: join<10>(a, sh, emit); break;
        case 20: join<20>(a, sh, emit); break;
        case 30: join<30>(a, sh, emit); break;
        default: join<40>(a, sh, emit); break;
        }
        return hipGetLastError();
    }
    hipError_t count(const vapor_pair& a, const SeqDesc& s1, const SeqDesc& s2, const dp::Shape& sh, const long long** d_total)
    {
        j = dp::wide_join(a.k, sh.nk1, sh.nk2);
        hipError_t e;
        if ((e = w.ensure(dp::WIDE_KEYS, j.keys)) != hipSuccess) return e;
        if ((e = w.ensure(dp::WIDE_HEAD, j.heads)) != hipSuccess) return e;
        if ((e = w.ensure(dp::WIDE_NEXT, j.nexts)) != hipSuccess) return e;
        if ((e = w.ensure(dp::WIDE_CNT, j.counts)) != hipSuccess) return e;
        if ((e = w.ensure(dp::WIDE_OFF, j.offsets)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(w.p[dp::WIDE_HEAD], 0xFF, j.heads, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(w.p[dp::WIDE_BOOKED], 0, sizeof(unsigned long long), st)) != hipSuccess) return e;
        x4_1 = set->d_x4 + (size_t)s1.chunk0 * 4;
        x4_2 = set->d_x4 + (size_t)s2.chunk0 * 4;
        *d_total = w.at<long long>(dp::WIDE_OFF) + sh.nk2;
        return join(a, sh, false);
    }
    hipError_t emit(const vapor_pair& a, const dp::Shape& sh) { return join(a, sh, true); }
};
}  // namespace

extern "C" int vapor_wide_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int64_t* stats,
                                int32_t* hits_ji, int64_t hits_capacity, int64_t* hit_off)
{
    return dot_pairs<WideRoute>("vapor_wide_batch", ctx, set, n_pairs, pairs, stats, hits_ji, hits_capacity, hit_off);
}

extern "C" int vapor_clean_hits_wide(vapor_ctx* ctx, int64_t n_lists, const int32_t* hits_ji, const int64_t* off,
                                     const uint32_t* flags, int64_t* stats, uint8_t* hit_flags)
{
    if (const auto no = dp::call_refusal(dp::Call{dp::LISTS, ctx != nullptr, n_lists, stats, hits_ji, off, nullptr, 0, ctx ? ctx->max_pair_cap : 0}))
        return refused("vapor_clean_hits_wide", no);
    if (n_lists == 0) return VAPOR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CallScope sc(ctx, st);
    const WideAcc init = dp::acc_init();
    WideAcc res;
    SharedBufs b(sc);
    HIPCHK(b.ensure(dp::ACC, sizeof(WideAcc)));
    for (int64_t t = 0; t < n_lists; ++t) {
        const int64_t n = off[t + 1] - off[t];
        const uint32_t f = flags ? flags[t] : dp::LIST_FLAGS;
        const dp::Extent x = dp::extent(hits_ji, off[t], off[t + 1]);
        HIPCHK(hipMemcpyAsync(b.p[dp::ACC], &init, sizeof(WideAcc), hipMemcpyHostToDevice, st));
        if (n) {
            HIPCHK(b.ensure(dp::DOTS, sizeof(int2) * (size_t)n));
            HIPCHK(b.ensure(dp::FL, (size_t)n));
            HIPCHK(hipMemcpyAsync(b.p[dp::DOTS], hits_ji + 2 * off[t], sizeof(int2) * (size_t)n, hipMemcpyHostToDevice, st));
            HIPCHK(wide_clean(b, st, (int)n, x.mi, x.mj, f));
        }
        HIPCHK(hipMemcpyAsync(&res, b.p[dp::ACC], sizeof(WideAcc), hipMemcpyDeviceToHost, st));
        if (hit_flags && n) HIPCHK(hipMemcpyAsync(hit_flags + off[t], b.p[dp::FL], (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        dp::record_folded(res, n, f, stats + 16 * t);
    }
    sc.settled();
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
// The any-k route (vapor_anyk.h): kmerhits at every k from 1 to VAPOR_MAX_ANY_K, dots in the reference's order, the statistics
// from the wide route's cleaning.
namespace {
struct AnykRoute {
    SharedBufs& b;
    AnykBufs x;
    hipStream_t st;
    const vapor_seqset* set;
    const long long edit_pairs;                    // the context's "anyk_edit_pairs"
    AnykSrc src{};                                 // of the pair being counted, for its emit pass
    dp::AnykPass p{};
    AnykRoute(CallScope& sc, SharedBufs& bufs, const vapor_seqset* s, int64_t) : b(bufs), x(sc), st(sc.st), set(s), edit_pairs(sc.ctx->anyk_edit_pairs) {}
    hipError_t prepare() { return hipSuccess; }
    static int admit(const dp::SetView& v, const vapor_pair& a) { return dp::admit_anyk(v, a); }
    // the bytes the set kept of sequence q (it holds a symbol outside the alphabet), or null
    const uint8_t* raw(int32_t q) const
    {
        return set->h[q].n_invalid > 0 && (size_t)q < set->raw_off.size() && set->raw_off[q] >= 0 ? set->d_raw + set->raw_off[q] : nullptr;
    }
    // the edit-distance pass over the allele k-mers, one launch per range of the cut
    template <bool EMIT>
    void edit(int nk2, uint32_t* cnt, const long long* off, int2* dots)
    {
        const dp::EditCut c = dp::edit_cut(p.n, nk2, edit_pairs);
        for (int t = 0; t < c.launches(); ++t)
            hipLaunchKernelGGL((anyk_edit_kernel<EMIT>), dim3(c.grid(t)), dim3(64 * ANYK_EDIT_WAVES), 0, st, src, x.at<const uint32_t>(dp::ANYK_IDX),
                               (const int4*)x.at<int4>(dp::ANYK_KEYS), (const long long*)(x.at<long long>(dp::ANYK_RANK) + p.n), c.j0(t), c.j1(t), cnt, off, dots);
    }
    // the pair's symbol bytes, sorted entries and per-j counts: enqueued on st, the number of dots at x.OFF[nk2]
    hipError_t count(const vapor_pair& a, const SeqDesc& s1, const SeqDesc& s2, const dp::Shape& sh, const long long** d_total)
    {
        const bool inv = !dp::forward_only(a);
        p = dp::anyk_pass(a.k, inv, s1.len, sh);
        const dp::Symbols& y = p.sym;
        hipError_t e;
        for (int q = 0; q < dp::N_ANYK; ++q)
            if (p.bytes[q] && (e = x.ensure((dp::AnykSlot)q, p.bytes[q])) != hipSuccess) return e;
        uint8_t* sym = x.at<uint8_t>(dp::ANYK_SYM);
        const uint32_t* x4_1 = set->d_x4 + (size_t)s1.chunk0 * 4;
        const uint32_t* x4_2 = set->d_x4 + (size_t)s2.chunk0 * 4;
        const dim3 block(dp::THREADS);
        // (without inversions a symbol outside the alphabet is compared byte for byte; with them one of seq1 is refused, and one of
        // seq2 matches nothing: it stays 0xFF)
        hipLaunchKernelGGL(anyk_sym_kernel, dim3(dp::grid(s1.len)), block, 0, st, x4_1, inv ? (const uint8_t*)nullptr : raw(a.seq1), (int)(s1.flags & 1u), 0,
                           s1.len, sym + y.s1, inv ? sym + y.r1 : (uint8_t*)nullptr);
        hipLaunchKernelGGL(anyk_sym_kernel, dim3(dp::grid(sh.n2)), block, 0, st, x4_2, inv ? (const uint8_t*)nullptr : raw(a.seq2), (int)(s2.flags & 1u), a.off2,
                           sh.n2, sym + y.s2, (uint8_t*)nullptr);
        src = AnykSrc{sym + y.s1, sym + y.r1, sym + y.s2, s1.len, a.k, inv ? 1 : 0};
        uint32_t* idx = x.at<uint32_t>(dp::ANYK_IDX);
        hipLaunchKernelGGL(anyk_iota_kernel, dim3(p.iota_grid), block, 0, st, idx, p.n, p.np);
        for (const dp::SortStep& s : dp::sort_schedule(p.np)) {
            if (s.local) hipLaunchKernelGGL(anyk_sort_local_kernel, dim3(p.tile_grid), block, 0, st, src, idx, s.full, s.kk);
            else hipLaunchKernelGGL(anyk_sort_global_kernel, dim3(p.stride_grid), block, 0, st, src, idx, p.np, s.kk, s.jj);
        }
        uint32_t* cnt = x.at<uint32_t>(dp::ANYK_CNT);
        if (p.exact) {
            hipLaunchKernelGGL(anyk_probe_kernel, dim3(p.allele_grid), block, 0, st, src, (const uint32_t*)idx, p.n, sh.nk2, cnt, x.at<uint32_t>(dp::ANYK_FIRST));
        } else {
            uint32_t* isf = x.at<uint32_t>(dp::ANYK_ISF);
            long long* rank = x.at<long long>(dp::ANYK_RANK);
            if ((e = hipMemsetAsync(isf, 0, p.bytes[dp::ANYK_ISF], st)) != hipSuccess) return e;
            hipLaunchKernelGGL(anyk_group_kernel, dim3(p.entry_grid), block, 0, st, src, (const uint32_t*)idx, p.n, isf, x.at<int2>(dp::ANYK_RUN));
            hipLaunchKernelGGL(wide_scan_kernel, dim3(1), dim3(WIDE_SCAN_THREADS), 0, st, (const uint32_t*)isf, p.n, rank);
            hipLaunchKernelGGL(anyk_rank_kernel, dim3(p.entry_grid), block, 0, st, p.n, (const uint32_t*)isf, (const long long*)rank,
                               (const int2*)x.at<int2>(dp::ANYK_RUN), x.at<int4>(dp::ANYK_KEYS));
            edit<false>(sh.nk2, cnt, nullptr, nullptr);
        }
        hipLaunchKernelGGL(wide_scan_kernel, dim3(1), dim3(WIDE_SCAN_THREADS), 0, st, (const uint32_t*)cnt, sh.nk2, x.at<long long>(dp::ANYK_OFF));
        *d_total = x.at<long long>(dp::ANYK_OFF) + sh.nk2;
        return hipGetLastError();
    }
    hipError_t emit(const vapor_pair&, const dp::Shape& sh)
    {
        const long long* off = x.at<const long long>(dp::ANYK_OFF);
        int2* dots = b.at<int2>(dp::DOTS);
        if (p.exact)
            hipLaunchKernelGGL(anyk_emit_kernel, dim3(p.allele_grid), dim3(dp::THREADS), 0, st, src, x.at<const uint32_t>(dp::ANYK_IDX), sh.nk2,
                               (const uint32_t*)x.at<uint32_t>(dp::ANYK_CNT), (const uint32_t*)x.at<uint32_t>(dp::ANYK_FIRST), off, dots);
        else
            edit<true>(sh.nk2, nullptr, off, dots);
        return hipGetLastError();
    }
};
}  // namespace

extern "C" int vapor_anyk_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int64_t* stats,
                                int32_t* hits_ji, int64_t hits_capacity, int64_t* hit_off)
{
    return dot_pairs<AnykRoute>("vapor_anyk_batch", ctx, set, n_pairs, pairs, stats, hits_ji, hits_capacity, hit_off);
}

// ------------------------------------------------------------------------------------------
// `--realign` (vapor_realign.h): the banded edit distance of every pair, one wavefront a pair.  The checks, the pair records and
// the geometry are vapor_realign_plan.h's; here: one upload of the records, one launch, one copy back.
//
// What the four realign entries share.  The compiled lane width of a band, as a constant: f(std::integral_constant<int, S>) for
// the S of vapor_realign::WIDTHS the band takes (a band out of range, which every entry has refused, would take the widest).
template <int K = 0, typename F>
static void with_lane_width(int32_t band, F&& f)
{
    namespace ra = vapor_realign;
    if constexpr (K + 1 < ra::N_WIDTHS) {
        if (ra::lane_width(band) != ra::WIDTHS[K]) return with_lane_width<K + 1>(band, f);
    }
    f(std::integral_constant<int, ra::WIDTHS[K]>{});
}

// the set as the plan headers take it: its sequences, and the length and first chunk of sequence s
static auto seqs_of(const vapor_seqset* set)
{
    return vapor_polish_call::seqs(set->n, [set](int32_t s) { return set->h[(size_t)s].len; }, [set](int32_t s) { return set->h[(size_t)s].chunk0; });
}

// the records of a call's pairs over the set: vapor_realign::RPair, or vapor_junction::JPair
template <typename Rec>
static std::vector<Rec> pair_records(const vapor_seqset* set, const vapor_pair* pairs, int64_t n_pairs)
{
    const auto s = seqs_of(set);
    std::vector<Rec> recs((size_t)n_pairs);
    for (int64_t t = 0; t < n_pairs; ++t) {
        if constexpr (std::is_same_v<Rec, vapor_junction::JPair>) recs[(size_t)t] = vapor_junction::pair_record(pairs[t], s.n, s.len_of, s.chunk_of);
        else recs[(size_t)t] = vapor_realign::pair_record(pairs[t], s.n, s.len_of, s.chunk_of);
    }
    return recs;
}

// the refusals of every entry, in their order; args_ok: the pointers a call with pairs needs are there
static int realign_refusal(const char* entry, const vapor_ctx* ctx, const vapor_seqset* set, int64_t n_pairs, bool args_ok, int32_t band)
{
    if (const auto no = vapor_polish_call::realign_args(ctx && set, n_pairs, args_ok, band)) return refused(entry, no);
    return VAPOR_OK;
}

template <int S>
static void realign_launch(hipStream_t st, const uint32_t* x4, const vapor_realign::RPair* d_pairs, int64_t n_pairs, int32_t band, int32_t* d_out)
{
    hipLaunchKernelGGL((realign_kernel<S>), dim3((unsigned)vapor_realign::grid_of(n_pairs)), dim3(64 * vapor_realign::WAVES), 0, st, x4, d_pairs,
                       (long long)n_pairs, (int)band, d_out);
}

extern "C" int vapor_realign_batch(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band, int32_t* out)
{
    namespace ra = vapor_realign;
    if (const int no = realign_refusal("vapor_realign_batch", ctx, set, n_pairs, pairs && out, band)) return no;
    if (n_pairs == 0) return VAPOR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const std::vector<ra::RPair> recs = pair_records<ra::RPair>(set, pairs, n_pairs);      // (the upload reads it: declared before the owners, which unwind first)
    CallScope sc(ctx, st);
    Block<ra::RPair> d_pairs(sc);
    Block<int32_t> d_out(sc);
    HIPCHK(d_pairs.ensure(sizeof(ra::RPair) * (size_t)n_pairs));
    HIPCHK(d_out.ensure(sizeof(int32_t) * 2 * (size_t)n_pairs));
    HIPCHK(hipMemcpyAsync(d_pairs.p, recs.data(), sizeof(ra::RPair) * (size_t)n_pairs, hipMemcpyHostToDevice, st));
    with_lane_width(band, [&](auto S) { realign_launch<S()>(st, set->d_x4, d_pairs, n_pairs, band, d_out); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out.p, sizeof(int32_t) * 2 * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    sc.settled();
    return VAPOR_OK;
}

// `--realign-out` (vapor_realign_trace.h): the alignment behind every pair's distance.  The pair records are
// vapor_realign_plan.h's, the groups, the workspace and the head vapor_trace_plan.h's; here: one upload (records and workspace
// offsets), per group the forward pass and the traceback back to back on one workspace, the copies back and one synchronisation.
template <int S>
static void realign_trace_launch(hipStream_t st, const uint32_t* x4, const vapor_realign::RPair* d_pairs, const uint64_t* d_off, int64_t t0,
                                 int64_t count, int32_t band, uint32_t* d_ws, int32_t cap_runs, int32_t* d_head, uint32_t* d_runs)
{
    const dim3 grid((unsigned)vapor_realign::grid_of(count)), block(64 * vapor_realign::WAVES);
    hipLaunchKernelGGL((realign_trace_kernel<S>), grid, block, 0, st, x4, d_pairs, d_off, (long long)t0, (long long)count, (int)band, d_ws, d_head);
    hipLaunchKernelGGL((traceback_kernel<S>), grid, block, 0, st, d_pairs, d_off, (long long)t0, (long long)count, (int)band,
                       (const uint32_t*)d_ws, (int)cap_runs, d_head, d_runs);
}

extern "C" int vapor_realign_trace(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band, int32_t cap_runs,
                                   int32_t* head, uint32_t* runs)
{
    namespace ra = vapor_realign;
    namespace tr = vapor_trace;
    if (const int no = realign_refusal("vapor_realign_trace", ctx, set, n_pairs, pairs && head && runs, band)) return no;
    if (!tr::cap_ok(cap_runs)) return fail(VAPOR_E_ARG, "vapor_realign_trace: cap_runs below 1");
    if (n_pairs == 0) return VAPOR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int S = ra::lane_width(band);
    const size_t np = (size_t)n_pairs;
    const std::vector<ra::RPair> recs = pair_records<ra::RPair>(set, pairs, n_pairs);
    std::vector<int64_t> first;
    std::vector<uint64_t> off;
    vapor_image::Table<ra::RPair> t_recs;                        // the upload image: the records, then the workspace offsets
    vapor_image::Table<uint64_t> t_off;
    vapor_image::Carve carve;
    carve.take(t_recs, np);
    carve.take(t_off, np);
    std::vector<uint8_t> up(carve.off);                                // (the upload reads it: declared before the owners)
    CallScope sc(ctx, st);
    Block<uint8_t> d_up(sc);
    Block<uint32_t> d_ws(sc);
    Block<int32_t> d_head(sc);
    Block<uint32_t> d_runs(sc);
    const int64_t ws_words = tr::plan_groups(recs.data(), n_pairs, band, S, ctx->trace_budget, first, off);
    t_recs.fill(up, recs);
    t_off.fill(up, off);
    HIPCHK(d_up.ensure(up.size()));
    HIPCHK(d_ws.ensure(sizeof(uint32_t) * (size_t)std::max<int64_t>(ws_words, 64)));
    HIPCHK(d_head.ensure(sizeof(int32_t) * tr::HEAD * np));
    HIPCHK(d_runs.ensure(sizeof(uint32_t) * np * (size_t)cap_runs));
    HIPCHK(hipMemcpyAsync(d_up.p, up.data(), up.size(), hipMemcpyHostToDevice, st));
    const ra::RPair* d_pairs = t_recs.in(d_up.p);
    const uint64_t* d_off = t_off.in(d_up.p);
    for (size_t g = 0; g + 1 < first.size(); ++g) {
        const int64_t t0 = first[g], count = first[g + 1] - t0;
        if (count == 0) continue;
        with_lane_width(band, [&](auto W) { realign_trace_launch<W()>(st, set->d_x4, d_pairs, d_off, t0, count, band, d_ws, cap_runs, d_head, d_runs); });
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(head, d_head.p, sizeof(int32_t) * tr::HEAD * np, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(runs, d_runs.p, sizeof(uint32_t) * np * (size_t)cap_runs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    sc.settled();
    return VAPOR_OK;
}

// `--realign-polish` (vapor_polish.h): the consensus of every locus's pairs on its allele.  The checks, the groups
// and the layout of a group's buffer are vapor_polish_plan.h's, and the call's plan - every record, every offset, the upload image
// and the dealing of the spelt bytes - is vapor_polish_call.h's; here: one upload (pair records, workspace offsets, the locus
// records, the pairs' loci), per group one clear of its tables, the forward pass, the traceback into run slots that stay on the
// device, the four kernels and the copies back; one synchronisation at the end.
//
// `--realign-revote` (vapor_revote.h) is the same call with three more kernels a group behind insert_kernel: `rv`
// names the vote pairs and the outputs of vapor_realign_revote, null for the polish alone, which launches what it always did.
// The extra checks, the vote pair's record and the pieces a locus adds to its group's buffer are vapor_revote_plan.h's.
using vapor_polish_call::RevoteArgs;

template <int S>
static void realign_onto_launch(hipStream_t st, const uint32_t* x4, const vapor_revote::VPair* d_votes, const vapor_revote::VLocus* d_vloci,
                                const uint32_t* d_buf, const int32_t* d_lout, int64_t n_votes, int32_t band, int32_t* d_vout)
{
    hipLaunchKernelGGL((realign_onto_kernel<S>), dim3((unsigned)vapor_realign::grid_of(n_votes)), dim3(64 * vapor_realign::WAVES), 0, st, x4,
                       d_votes, d_vloci, d_buf, d_lout, (long long)n_votes, (int)band, d_vout);
}

static int polish_call(const std::string& entry, vapor_ctx* ctx, vapor_seqset* set, const vapor_polish_call::Call& c)
{
    namespace ra = vapor_realign;
    namespace tr = vapor_trace;
    namespace pp = vapor_polish;
    namespace vr = vapor_revote;
    bool nothing = false;
    if (const auto no = vapor_polish_call::check_args(c, nothing)) return refused(entry, no);
    if (nothing) return VAPOR_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const RevoteArgs* rv = c.rv;
    const int64_t* col_off = c.col_off;
    const int32_t band = c.band;
    const size_t np = (size_t)c.n_pairs, nl = (size_t)c.n_loci, nv = rv ? (size_t)rv->n_votes : 0;
    const vapor_polish_call::Plan plan(c, seqs_of(set), ctx->trace_budget);     // (the upload reads its image: declared before the owners)
    std::vector<uint32_t> staged((size_t)plan.staged_words);                   // (the copies back write it: declared before the owners)
    const std::vector<pp::Group>& groups = plan.groups;
    CallScope sc(ctx, st);
    Block<uint8_t> d_up(sc);
    Block<uint32_t> d_buf(sc);
    Block<int32_t> d_head(sc);
    Block<int32_t> d_vout(sc), d_lout(sc);
    if (rv) {
        HIPCHK(d_vout.ensure(sizeof(int32_t) * vr::VOUT * std::max<size_t>(nv, 1)));
        HIPCHK(d_lout.ensure(sizeof(int32_t) * vr::LOUT * nl));
    }
    HIPCHK(d_up.ensure(plan.image.size()));
    HIPCHK(d_buf.ensure(sizeof(uint32_t) * (size_t)std::max<int64_t>(plan.most, 64)));
    HIPCHK(d_head.ensure(sizeof(int32_t) * tr::HEAD * std::max<size_t>(np, 1)));
    HIPCHK(hipMemcpyAsync(d_up.p, plan.image.data(), plan.image.size(), hipMemcpyHostToDevice, st));
    const ra::RPair* d_pairs = plan.t_recs.in(d_up.p);
    const uint64_t* d_off = plan.t_off.in(d_up.p);
    const pp::PLocus* d_loci = plan.t_loci.in(d_up.p);
    const int32_t* d_pl = plan.t_pair_locus.in(d_up.p);
    const vr::VLocus* d_vloci = plan.t_vloci.in(d_up.p);
    const vr::VPair* d_votes = plan.t_vrecs.in(d_up.p);
    for (const pp::Group& gr : groups) {
        const int64_t count = gr.pair1 - gr.pair0, gl = gr.locus1 - gr.locus0;
        uint32_t* const b = d_buf.p;
        uint32_t* const g_counts = b + gr.counts_off;
        uint32_t* const g_slot = b + gr.slot_off;
        uint8_t* const g_calls = reinterpret_cast<uint8_t*>(b + gr.calls_off);
        int32_t* const g_stats = reinterpret_cast<int32_t*>(b + gr.stats_off);
        int32_t* const g_sites = reinterpret_cast<int32_t*>(b + gr.sites_off);
        uint8_t* const g_ins = reinterpret_cast<uint8_t*>(b + gr.ins_off);
        uint32_t* const g_insb = b + gr.insb_off;
        HIPCHK(hipMemsetAsync(b + gr.zero_off, 0, sizeof(uint32_t) * (size_t)(gr.words - gr.zero_off), st));
        const ra::RPair* gp = d_pairs + gr.pair0;
        const pp::PLocus* gloc = d_loci + gr.locus0;
        const int32_t* gpl = d_pl + gr.pair0;
        int32_t* ghead = d_head.p + tr::HEAD * gr.pair0;
        const int32_t cap_runs = (int32_t)gr.cap_runs;
        if (count > 0) {
            const uint64_t* goff = d_off + gr.pair0;
            uint32_t* g_runs = b + gr.runs_off;
            with_lane_width(band, [&](auto W) { realign_trace_launch<W()>(st, set->d_x4, gp, goff, 0, count, band, b, cap_runs, ghead, g_runs); });
            HIPCHK(hipGetLastError());
            const dim3 grid((unsigned)ra::grid_of(count)), block(64 * ra::WAVES);
            hipLaunchKernelGGL(pileup_kernel, grid, block, 0, st, (const uint32_t*)set->d_x4, gp, gpl, gloc, (long long)count, (const int32_t*)ghead,
                               (const uint32_t*)g_runs, (int)cap_runs, g_counts);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(consensus_kernel, dim3((unsigned)gl), dim3(CONSENSUS_THREADS), 0, st, (const uint32_t*)set->d_x4, gloc,
                           (const uint32_t*)g_counts, g_slot, g_calls, g_stats, g_sites);
        HIPCHK(hipGetLastError());
        if (count > 0) {
            const dim3 grid((unsigned)ra::grid_of(count)), block(64 * ra::WAVES);
            hipLaunchKernelGGL(pileup_ins_kernel, grid, block, 0, st, (const uint32_t*)set->d_x4, gp, gpl, gloc, (long long)count,
                               (const int32_t*)ghead, (const uint32_t*)(b + gr.runs_off), (int)cap_runs, (const uint32_t*)g_slot, g_insb);
            HIPCHK(hipGetLastError());
            const long long n_slots = (long long)gl * pp::MAX_SITES;
            hipLaunchKernelGGL(insert_kernel, dim3((unsigned)ra::grid_of(n_slots)), block, 0, st, gloc, n_slots, (const uint32_t*)g_counts,
                               (const uint32_t*)g_insb, g_stats, g_sites, g_ins);
            HIPCHK(hipGetLastError());
        }
        if (rv) {
            const size_t k = (size_t)(&gr - groups.data());
            const vr::VLocus* gvl = d_vloci + gr.locus0;
            int32_t* glout = d_lout.p + vr::LOUT * gr.locus0;
            hipLaunchKernelGGL(spell_kernel, dim3((unsigned)gl), dim3(CONSENSUS_THREADS), 0, st, (const uint32_t*)set->d_x4, gloc, gvl,
                               (const uint8_t*)g_calls, (const int32_t*)g_sites, (const uint8_t*)g_ins, b, glout);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(spell_pack_kernel, dim3((unsigned)gl), dim3(CONSENSUS_THREADS), 0, st, gvl, b, (const int32_t*)glout);
            HIPCHK(hipGetLastError());
            const int64_t v0 = rv->vfirst[gr.locus0], n_gv = rv->vfirst[gr.locus1] - v0;
            if (n_gv > 0) {
                with_lane_width(band, [&](auto W) {
                    realign_onto_launch<W()>(st, set->d_x4, d_votes + v0, gvl, b, glout, n_gv, band, d_vout.p + vr::VOUT * v0);
                });
                HIPCHK(hipGetLastError());
            }
            if (rv->spelt && plan.stage_words[k])
                HIPCHK(hipMemcpyAsync(staged.data() + plan.stage_host[k], b + plan.stage_base[k], sizeof(uint32_t) * (size_t)plan.stage_words[k],
                                      hipMemcpyDeviceToHost, st));
        }
        const size_t c0 = (size_t)col_off[gr.locus0], l0 = (size_t)gr.locus0;
        if (gr.cols) HIPCHK(hipMemcpyAsync(c.calls + c0, g_calls, (size_t)gr.cols, hipMemcpyDeviceToHost, st));
        if (gr.cols && c.counts)
            HIPCHK(hipMemcpyAsync(c.counts + pp::COUNTERS * c0, g_counts, sizeof(uint32_t) * pp::COUNTERS * (size_t)gr.cols, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(c.stats + pp::STATS * l0, g_stats, sizeof(int32_t) * pp::STATS * (size_t)gl, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(c.sites + pp::SITE_WORDS * l0, g_sites, sizeof(int32_t) * pp::SITE_WORDS * (size_t)gl, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(c.ins + 4 * pp::INS_WORDS * l0, g_ins, 4 * (size_t)pp::INS_WORDS * (size_t)gl, hipMemcpyDeviceToHost, st));
    }
    if (rv) {
        if (nv) HIPCHK(hipMemcpyAsync(rv->vout, d_vout.p, sizeof(int32_t) * vr::VOUT * nv, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(rv->lout, d_lout.p, sizeof(int32_t) * vr::LOUT * nl, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    sc.settled();
    if (rv) plan.deal_spelt(staged.data(), rv->lout, rv->spelt_off, rv->spelt);
    return VAPOR_OK;
}

extern "C" int vapor_realign_polish(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band, int64_t n_loci,
                                    const int64_t* first, const int64_t* col_off, int32_t* stats, uint8_t* calls, int32_t* sites, uint8_t* ins,
                                    uint32_t* counts)
{
    return polish_call("vapor_realign_polish", ctx, set, {ctx && set, n_pairs, pairs, band, n_loci, first, col_off, stats, calls, sites, ins, counts, nullptr});
}

extern "C" int vapor_realign_revote(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band, int64_t n_loci,
                                    const int64_t* first, const int64_t* col_off, int32_t* stats, uint8_t* calls, int32_t* sites, uint8_t* ins,
                                    uint32_t* counts, int64_t n_votes, const vapor_pair* votes, const int64_t* vfirst, int32_t* vout, int32_t* lout,
                                    const int64_t* spelt_off, uint8_t* spelt)
{
    const RevoteArgs rv{n_votes, votes, vfirst, vout, lout, spelt_off, spelt};
    return polish_call("vapor_realign_revote", ctx, set, {ctx && set, n_pairs, pairs, band, n_loci, first, col_off, stats, calls, sites, ins, counts, &rv});
}

// `--realign-junction` (vapor_junction.h): the one jump between the two sequences of every pair.  The checks, the
// pair records and the workspace are vapor_junction_plan.h's; here: one upload of the records, the two launches back to back, the
// copies back - the rows through one staging buffer, dealt to the caller's slots on the host - and one synchronisation.
template <int S>
static void junction_launch(hipStream_t st, const uint32_t* x4, const vapor_junction::JPair* d_pairs, int64_t n_pairs, int32_t band, int32_t* d_ws,
                            int32_t* d_out)
{
    namespace vj = vapor_junction;
    const dim3 block(64 * vapor_realign::WAVES);
    hipLaunchKernelGGL((junction_rows_kernel<S>), dim3((unsigned)vj::rows_grid(n_pairs)), block, 0, st, x4, d_pairs, (long long)vj::tasks_of(n_pairs),
                       (int)band, d_ws);
    hipLaunchKernelGGL(junction_pick_kernel, dim3((unsigned)vj::pick_grid(n_pairs)), block, 0, st, d_pairs, (long long)n_pairs, (const int32_t*)d_ws,
                       d_out);
}

extern "C" int vapor_realign_junction(vapor_ctx* ctx, vapor_seqset* set, int64_t n_pairs, const vapor_pair* pairs, int32_t band, int32_t* out,
                                      const int64_t* row_off, int32_t* rows)
{
    namespace ra = vapor_realign;
    namespace vj = vapor_junction;
    if (const int no = realign_refusal("vapor_realign_junction", ctx, set, n_pairs, pairs && out, band)) return no;
    if (rows && !vj::row_off_ok(n_pairs, row_off)) return fail(VAPOR_E_ARG, "vapor_realign_junction: row_off must ascend from 0");
    if (n_pairs == 0) return VAPOR_OK;
    const size_t np = (size_t)n_pairs;
    std::vector<vj::JPair> recs = pair_records<vj::JPair>(set, pairs, n_pairs);    // (the upload reads it: declared before the owners, which unwind first)
    for (int64_t t = 0; rows && t < n_pairs; ++t)
        if (!vj::slot_holds(recs[(size_t)t], row_off, t)) recs[(size_t)t] = vj::JPair{0, 0, 0, 0, VAPOR_E_ARG, 0, 0};
    const int64_t n_rows = vj::lay_out(recs.data(), n_pairs);
    if (!vj::fits(n_rows, ctx->trace_budget)) return fail(VAPOR_E_NOMEM, "vapor_realign_junction: the pairs' row tables exceed trace_budget");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t ws_bytes = sizeof(int32_t) * vj::ROW * (size_t)n_rows;
    std::vector<int32_t> staged(rows ? vj::ROW * (size_t)n_rows : 0);
    CallScope sc(ctx, st);
    Block<vj::JPair> d_pairs(sc);
    Block<int32_t> d_ws(sc);
    Block<int32_t> d_out(sc);
    HIPCHK(d_pairs.ensure(sizeof(vj::JPair) * np));
    HIPCHK(d_ws.ensure(std::max<size_t>(ws_bytes, 64)));
    HIPCHK(d_out.ensure(sizeof(int32_t) * vj::OUT * np));
    HIPCHK(hipMemcpyAsync(d_pairs.p, recs.data(), sizeof(vj::JPair) * np, hipMemcpyHostToDevice, st));
    with_lane_width(band, [&](auto S) { junction_launch<S()>(st, set->d_x4, d_pairs, n_pairs, band, d_ws, d_out); });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out.p, sizeof(int32_t) * vj::OUT * np, hipMemcpyDeviceToHost, st));
    if (rows && n_rows) HIPCHK(hipMemcpyAsync(staged.data(), d_ws.p, ws_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    sc.settled();
    if (rows)
        for (int64_t t = 0; t < n_pairs; ++t) {
            const vj::JPair& r = recs[(size_t)t];
            if (!r.status)
                memcpy(rows + vj::ROW * row_off[t], staged.data() + vj::ROW * r.row0, sizeof(int32_t) * vj::ROW * (size_t)vj::pair_rows(r.ns));
        }
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
// per-read scores and per-locus summaries on the device, and the breakpoint grid over them.  What a call is refused for, the
// upload images and every size are vapor_finish_plan.h's.
extern "C" int vapor_plan_set_reads(vapor_plan* p, int64_t n_reads, const vapor_read* reads, int64_t n_loci,
                                    const double* gt_table)
{
    if (!p || n_reads < 0 || n_loci < 0 || (n_reads && !reads) || !gt_table)
        return fail(VAPOR_E_ARG, "vapor_plan_set_reads: null argument");
    static_assert(sizeof(vapor_read) == sizeof(DRead), "vapor_read layout");
    HIPCHK(hipSetDevice(p->ctx->device));
    std::vector<int32_t> first;
    std::vector<uint8_t> image;
    fp::ReadImage im;
    if (const fp::Refusal no = fp::read_table(n_reads, reads, n_loci, p->n_pairs, first, im, image)) return fail(no.code, no.msg);
    ReadTables& t = p->reads;
    t.release(p->ctx);
    t.im = im;
    HIPCHK(dmalloc(p->ctx, (void**)&t.d_image, im.bytes));
    HIPCHK(dmalloc(p->ctx, (void**)&t.d_read_scores, im.score_bytes));
    HIPCHK(dmalloc(p->ctx, (void**)&t.d_loci, im.loci_bytes));
    HIPCHK(hipMemcpy(t.d_image, image.data(), image.size(), hipMemcpyHostToDevice));
    // the genotype table is the same for every plan of a run: uploaded once per context, again only for a different one
    {
        vapor_ctx* c = p->ctx;
        const size_t gt_bytes = sizeof(double) * fp::GT_ENTRIES;
        if (!c->d_gt) {
            HIPCHK(hipMalloc((void**)&c->d_gt, gt_bytes));
            HIPCHK(hipMemcpy(c->d_gt, gt_table, gt_bytes, hipMemcpyHostToDevice));
            c->h_gt.assign(gt_table, gt_table + fp::GT_ENTRIES);
        }
        if (memcmp(c->h_gt.data(), gt_table, gt_bytes) == 0) {
            t.d_gt = c->d_gt;
        } else {
            HIPCHK(dmalloc(c, (void**)&t.d_gt, gt_bytes));
            t.own_gt = true;
            HIPCHK(hipMemcpy(t.d_gt, gt_table, gt_bytes, hipMemcpyHostToDevice));
        }
    }
    t.n_reads = n_reads;
    t.n_loci = n_loci;
    t.h_locus_first = std::move(first);
    // (a grid described for an earlier read table does not describe this one)
    p->grid.release(p->ctx);
    return VAPOR_OK;
}

extern "C" int vapor_plan_set_grid(vapor_plan* p, int64_t n_groups, const int32_t* first_locus)
{
    if (!p || n_groups < 0 || !first_locus) return fail(VAPOR_E_ARG, "vapor_plan_set_grid: null argument");
    if (!p->reads.set()) return fail(VAPOR_E_ARG, "vapor_plan_set_grid: call vapor_plan_set_reads first");
    HIPCHK(hipSetDevice(p->ctx->device));
    std::vector<int32_t> off;
    if (const fp::Refusal no = fp::grid_check(n_groups, first_locus, p->reads.n_loci, p->reads.h_locus_first.data(), off))
        return fail(no.code, no.msg);
    GridTables& g = p->grid;
    g.release(p->ctx);
    if (n_groups == 0) return VAPOR_OK;
    g.im = fp::GridImage((size_t)n_groups, off.back(), 0);
    const std::vector<uint8_t> image = g.im.filled(first_locus, off, nullptr);
    HIPCHK(dmalloc(p->ctx, (void**)&g.d_image, g.im.bytes));
    HIPCHK(dmalloc(p->ctx, (void**)&g.d_group_out, g.im.group_bytes));
    HIPCHK(dmalloc(p->ctx, (void**)&g.d_winner_scores, g.im.winner_bytes));
    HIPCHK(hipMemcpy(g.d_image, image.data(), image.size(), hipMemcpyHostToDevice));
    g.n_scores = off.back();
    g.score_off = std::move(off);
    g.n_groups = n_groups;
    return VAPOR_OK;
}

// finish_kernel over a read table, a workgroup a locus: the per-read scores into the table's block, the locus records to d_out and,
// where h_copy is given (pinned host memory), there as well
static int launch_finish(hipStream_t st, const ReadTables& t, const long long* d_stats, double* d_out, double* h_copy)
{
    if (t.n_loci <= 0) return VAPOR_OK;
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)t.n_loci), dim3(64), 0, st, t.d_reads(), t.d_locus_first(), d_stats, t.d_gt,
                       t.d_read_scores, d_out, h_copy);
    HIPCHK(hipGetLastError());
    return VAPOR_OK;
}

// grid_pick_kernel, a workgroup a group, and what of its answers the caller wants on the host
struct GridOut { int32_t* winner_idx; double* group_out; double* winner_scores; };     // host arrays, each may be null
struct GridView {
    const fp::GridImage& im;
    uint8_t* d_image;
    size_t n_scores;
    const double* d_records;                   // the candidates' locus records
    const int32_t* d_read_first;               // ... and read ranges
    const double* d_read_scores;
    double *d_group_out, *d_winner_scores;
};
static int launch_grid_pick(hipStream_t st, const GridView& v, const GridOut& o)
{
    int32_t* d_idx = v.im.winner_idx.in(v.d_image);
    hipLaunchKernelGGL(grid_pick_kernel, dim3((unsigned)v.im.winner_idx.n), dim3(64), 0, st, v.d_records, v.im.first_locus.in(v.d_image),
                       v.d_read_first, v.d_read_scores, v.im.score_off.in(v.d_image), d_idx, v.d_group_out, v.d_winner_scores);
    HIPCHK(hipGetLastError());
    if (o.winner_idx) HIPCHK(hipMemcpyAsync(o.winner_idx, d_idx, v.im.winner_idx.bytes(), hipMemcpyDeviceToHost, st));
    if (o.group_out) HIPCHK(hipMemcpyAsync(o.group_out, v.d_group_out, v.im.group_bytes, hipMemcpyDeviceToHost, st));
    if (o.winner_scores && v.n_scores)
        HIPCHK(hipMemcpyAsync(o.winner_scores, v.d_winner_scores, sizeof(double) * v.n_scores, hipMemcpyDeviceToHost, st));
    return VAPOR_OK;
}

// join -> clean -> finish (-> the choice among each group's candidates when the plan has a grid) on the device; the per-pair
// statistics stay in HBM.  grid_out: where vapor_plan_run_grid wants the choice, or null.
static int run_loci_impl(vapor_plan* p, void* d_loci_out, double* loci_out, double* read_scores, const GridOut* grid_out)
{
    HIPCHK(hipSetDevice(p->ctx->device));
    if (p->ring_n > 0) {
        int rc0 = async_fold(p);
        if (rc0 != VAPOR_OK) return rc0;
    }
    hipStream_t st = p->ctx->stream;
    const ReadTables& t = p->reads;
    bool host_status = fp::any_status(p->status.data(), p->n_pairs);
    int rc;
    const bool light = fp::light_run(p->ran, host_status);
    if (!light) {
        // first run, or pairs the host marked as failed: full path once (statistics to the host, slots grown)
        rc = vapor_plan_run(p, p->last_stats.data());
        if (rc != VAPOR_OK) return rc;
        // (the run itself may have given pairs a host-side status: the targets of a shared dot plot beyond max_pair_cap)
        host_status = host_status || fp::any_status(p->status.data(), p->n_pairs);
    } else {
        rc = plan_run_once(p, 0, false, nullptr, nullptr, false, nullptr, false);
        if (rc != VAPOR_OK) return rc;
    }
    if (fp::reupload_statuses(light, host_status))
        HIPCHK(hipMemcpyAsync(p->d_stats, p->h_stats, sizeof(long long) * fp::STATS_WORDS * (size_t)p->n_pairs, hipMemcpyHostToDevice, st));
    hipEvent_t e1 = p->ev_f[1];                  // the finish kernel starts where the clean kernels end (ev[2])
    double* d_out = d_loci_out ? static_cast<double*>(d_loci_out) : t.d_loci;
    if ((rc = launch_finish(st, t, p->d_stats, d_out, nullptr)) != VAPOR_OK) return rc;
    HIPCHK(hipEventRecord(e1, st));
    const GridTables& g = p->grid;
    if (g.n_groups > 0 && t.n_loci > 0) {
        // behind the finish kernel on its stream (no host step in between)
        const GridView v{g.im, g.d_image, (size_t)g.n_scores, d_out, t.d_locus_first(), t.d_read_scores,
                         g.d_group_out, g.d_winner_scores};
        if ((rc = launch_grid_pick(st, v, grid_out ? *grid_out : GridOut{})) != VAPOR_OK) return rc;
    }
    // only the overflow count has to come back (after the finish kernel, so that nothing sits between the kernels)
    HIPCHK(hipMemcpyAsync(p->h_overflow, p->d_overflow, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (loci_out && t.n_loci)
        HIPCHK(hipMemcpyAsync(loci_out, d_out, sizeof(double) * fp::LOCUS_DOUBLES * (size_t)t.n_loci, hipMemcpyDeviceToHost, st));
    if (read_scores && t.n_reads)
        HIPCHK(hipMemcpyAsync(read_scores, t.d_read_scores, sizeof(double) * (size_t)t.n_reads, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (fp::repeat_full(light, *p->h_overflow != 0, p->overflow_final)) {
        // some pair outgrew its record slot on this run: the full path resizes, then the whole run once more.  A pair that still
        // overflows (its slot would pass max_pair_cap) keeps VAPOR_E_OVERFLOW in its statistics: overflow_final, no further repeat
        rc = vapor_plan_run(p, p->last_stats.data());
        if (rc != VAPOR_OK) return rc;
        if (fp::still_overflows(p->last_stats.data(), p->n_pairs)) p->overflow_final = true;
        return run_loci_impl(p, d_loci_out, loci_out, read_scores, grid_out);
    }
    p->big_known = true;
    p->n_big = p->h_overflow[1];
    float f = 0, a = 0, b = 0, tt = 0;
    HIPCHK(hipEventElapsedTime(&f, p->ev[2], e1));
    p->t_finish = f;
    if (hipEventElapsedTime(&a, p->ev[0], p->ev[1]) == hipSuccess && hipEventElapsedTime(&b, p->ev[1], p->ev[2]) == hipSuccess &&
        hipEventElapsedTime(&tt, p->ev[0], e1) == hipSuccess) {
        p->t_join = a; p->t_clean = b; p->t_total = tt;
    }
    return VAPOR_OK;
}

// d_loci_out (device pointer, n_loci * VAPOR_LOCUS_STRIDE doubles, may be NULL) receives a copy on the library's stream before it
// is synchronised; loci_out / read_scores (host, may be NULL) receive host copies.
extern "C" int vapor_plan_run_loci(vapor_plan* p, void* d_loci_out, double* loci_out, double* read_scores)
{
    if (!p) return fail(VAPOR_E_ARG, "vapor_plan_run_loci: null plan");
    if (!p->reads.set()) return fail(VAPOR_E_ARG, "vapor_plan_run_loci: call vapor_plan_set_reads first");
    return run_loci_impl(p, d_loci_out, loci_out, read_scores, nullptr);
}

// vapor_plan_run_loci with the choice among each group's candidates handed out: per group the winner's index among its candidates,
// a group record (the winner's locus record, candidate 0's), and the winner's per-read scores (group g's at score_off[g] ..
// score_off[g + 1]; a skipped read is NaN).  Only these cross the link.
extern "C" int vapor_plan_run_grid(vapor_plan* p, int32_t* winner_idx, double* group_out, double* winner_scores, int64_t* score_off)
{
    if (!p) return fail(VAPOR_E_ARG, "vapor_plan_run_grid: null plan");
    if (p->grid.n_groups <= 0 || !p->grid.d_image) return fail(VAPOR_E_ARG, "vapor_plan_run_grid: call vapor_plan_set_grid first");
    if (score_off) std::copy(p->grid.score_off.begin(), p->grid.score_off.end(), score_off);
    const GridOut out{winner_idx, group_out, winner_scores};
    return run_loci_impl(p, nullptr, nullptr, nullptr, &out);
}

// grid_pick_kernel on the caller's tables (records and scores computed elsewhere; the tests' hand-made ones): one call, host
// arrays in and out.
extern "C" int vapor_grid_pick(vapor_ctx* ctx, int64_t n_groups, const int32_t* first_locus, const double* records,
                               const int32_t* read_first, const double* read_scores, int32_t* winner_idx, double* group_out,
                               double* winner_scores, int64_t* score_off)
{
    if (!ctx || n_groups < 0 || !first_locus || !records || !read_first) return fail(VAPOR_E_ARG, "vapor_grid_pick: null argument");
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<int32_t> off;
    if (const fp::Refusal no = fp::pick_check(n_groups, first_locus, read_first, off)) return fail(no.code, no.msg);
    if (score_off) std::copy(off.begin(), off.end(), score_off);
    if (n_groups == 0) return VAPOR_OK;
    const size_t nl = (size_t)first_locus[n_groups], nr = (size_t)read_first[nl], nw = (size_t)off.back();
    if (const fp::Refusal no = fp::pick_scores_check(nr, read_scores)) return fail(no.code, no.msg);
    const fp::GridImage im((size_t)n_groups, off.back(), nl + 1);
    const std::vector<uint8_t> image = im.filled(first_locus, off, read_first);
    const size_t rec_bytes = sizeof(double) * fp::LOCUS_DOUBLES * nl;
    hipStream_t st = ctx->stream;
    CallScope sc(ctx, st);
    Block<uint8_t> d_image(sc);
    Block<double> d_rec(sc), d_sc(sc), d_out(sc), d_win(sc);
    HIPCHK(d_image.ensure(im.bytes));
    HIPCHK(d_rec.ensure(rec_bytes));
    HIPCHK(d_sc.ensure(sizeof(double) * std::max<size_t>(nr, 1)));
    HIPCHK(d_out.ensure(im.group_bytes));
    HIPCHK(d_win.ensure(im.winner_bytes));
    HIPCHK(hipMemcpyAsync(d_image, image.data(), image.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_rec, records, rec_bytes, hipMemcpyHostToDevice, st));
    if (nr) HIPCHK(hipMemcpyAsync(d_sc, read_scores, sizeof(double) * nr, hipMemcpyHostToDevice, st));
    const GridView v{im, d_image.p, nw, d_rec.p, im.read_first.in(d_image.p), d_sc.p, d_out.p, d_win.p};
    if (const int rc = launch_grid_pick(st, v, GridOut{winner_idx, group_out, winner_scores})) return rc;
    HIPCHK(hipStreamSynchronize(st));
    sc.settled();
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
// Host helper of the read extraction: cigar2alignstart_by_pos, SF:309-337.  Walks the CIGAR until the
// reference cursor passes start-1; out[0] = offset into the read, out[1] = miss_bp.  S/I/M/= advance the read,
// M/=/D the reference, N/H/P/X nothing (as in the reference).  VAPOR_E_ARG when the CIGAR holds no operation
// (the reference raises IndexError there).
extern "C" int vapor_cigar2alignstart(const char* cigar, int64_t align_start, int64_t start, int64_t* out)
{
    if (!cigar || !out) return fail(VAPOR_E_ARG, "vapor_cigar2alignstart: null argument");
    int64_t q = 0, r = align_start, n = 0;
    bool have_n = false;
    char last = 0;
    for (const char* c = cigar; *c; ++c) {
        const char ch = *c;
        if (ch >= '0' && ch <= '9') { n = n * 10 + (ch - '0'); have_n = true; continue; }
        const bool op = ch == 'M' || ch == 'I' || ch == 'D' || ch == 'N' || ch == 'S' || ch == 'H' || ch == 'P' || ch == '=' || ch == 'X';
        if (op && have_n) {
            if (ch == 'S' || ch == 'I') q += n;
            else if (ch == 'M' || ch == '=') { q += n; r += n; }
            else if (ch == 'D') r += n;
            last = ch;
            if (r > start - 1) break;
        }
        n = 0; have_n = false;             // any other character ends the number, as the regular expression would
    }
    if (!last) return fail(VAPOR_E_ARG, "vapor_cigar2alignstart: no CIGAR operation");
    const int64_t over = r - start;
    if (last == 'M' || last == '=') { out[0] = q - over; out[1] = 0; }
    else { out[0] = q; out[1] = over; }
    return VAPOR_OK;
}

// The same walk over a BAM record's binary CIGAR (uint32 per operation: length << 4 | code, codes "MIDNSHP=X"), so that
// the in-process BAM reader neither formats nor re-parses CIGAR text (thousands of operations per long read).
extern "C" int vapor_cigar2alignstart_ops(const uint32_t* ops, int64_t n_ops, int64_t align_start, int64_t start, int64_t* out)
{
    if (!out || (n_ops > 0 && !ops)) return fail(VAPOR_E_ARG, "vapor_cigar2alignstart_ops: null argument");
    if (n_ops <= 0) return fail(VAPOR_E_ARG, "vapor_cigar2alignstart_ops: no CIGAR operation");
    int64_t q = 0, r = align_start;
    uint32_t last = 0;
    for (int64_t t = 0; t < n_ops; ++t) {
        const int64_t n = ops[t] >> 4;
        last = ops[t] & 15u;
        if (last == 4u || last == 1u) q += n;                    // S, I
        else if (last == 0u || last == 7u) { q += n; r += n; }   // M, =
        else if (last == 2u) r += n;                             // D
        if (r > start - 1) break;
    }
    const int64_t over = r - start;
    if (last == 0u || last == 7u) { out[0] = q - over; out[1] = 0; }
    else { out[0] = q; out[1] = over; }
    return VAPOR_OK;
}

// ------------------------------------------------------------------------------------------
// The same run without a host round trip per step: enqueue only, vapor_plan_sync() waits and reports.
constexpr int ASYNC_RING = 64;

extern "C" int vapor_set_stream(vapor_ctx* c, void* hip_stream)
{
    if (!c) return fail(VAPOR_E_ARG, "vapor_set_stream: null context");
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    c->user_stream = hip_stream != nullptr;
    return VAPOR_OK;
}

// the stream a plan's asynchronous steps go to: the caller's if one is set, else the plan's lane (dealt out on first use)
static int plan_lane(vapor_plan* p, hipStream_t* out)
{
    vapor_ctx* c = p->ctx;
    if (c->user_stream) { *out = c->stream; return VAPOR_OK; }
    if (!p->lane) {
        const unsigned l = c->lane_rr++ & 1u;
        if (!c->lane[l]) HIPCHK(hipStreamCreateWithFlags(&c->lane[l], hipStreamNonBlocking));
        if (!c->fin[l]) {
            int lo = 0, hi = 0;                  // (numerically lowest = highest priority)
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
                hipStreamCreateWithPriority(&c->fin[l], hipStreamNonBlocking, hi) != hipSuccess) {
                (void)hipGetLastError();
                c->fin[l] = nullptr;
                HIPCHK(hipStreamCreateWithFlags(&c->fin[l], hipStreamNonBlocking));   // no priorities here: an ordinary stream
            }
        }
        p->lane = c->lane[l];
        p->lane_ix = (int)l;
        p->fin = c->fin[l];
    }
    *out = p->lane;
    return VAPOR_OK;
}

// waits for the steps in flight and adds their event times to the accumulators
static int async_fold(vapor_plan* p)
{
    hipStream_t st = nullptr;
    int rc = plan_lane(p, &st);
    if (rc != VAPOR_OK) return rc;
    // (the plan's own streams as well when the caller has switched streams with steps in flight)
    if (p->lane && p->lane != st) HIPCHK(hipStreamSynchronize(p->lane));
    HIPCHK(hipStreamSynchronize(st));
    if (p->fin && p->fin != st) HIPCHK(hipStreamSynchronize(p->fin));
    for (int i = 0; i < p->ring_n; ++i) {
        float x = 0;
        hipEvent_t* ev = p->ring[(size_t)i].data();
        HIPCHK(hipEventElapsedTime(&x, ev[0], ev[1])); p->acc_ms[0] += x;
        HIPCHK(hipEventElapsedTime(&x, ev[1], ev[2])); p->acc_ms[1] += x;
        HIPCHK(hipEventElapsedTime(&x, ev[2], ev[3])); p->acc_ms[2] += x;
        HIPCHK(hipEventElapsedTime(&x, ev[0], ev[3])); p->acc_ms[3] += x;
    }
    p->acc_n += p->ring_n;
    p->ring_n = 0;
    return VAPOR_OK;
}

extern "C" int vapor_plan_run_loci_async(vapor_plan* p, void* d_loci_out)
{
    if (!p) return fail(VAPOR_E_ARG, "vapor_plan_run_loci_async: null plan");
    if (const fp::Refusal no = fp::async_refusal(p->reads.set(), p->ran, p->status.data(), p->n_pairs)) return fail(no.code, no.msg);
    HIPCHK(hipSetDevice(p->ctx->device));
    if (p->ring_n >= ASYNC_RING) {              // every event set is in use: wait for those steps, keep their times
        int rc0 = async_fold(p);
        if (rc0 != VAPOR_OK) return rc0;
    }
    hipStream_t st = nullptr;
    int rc = plan_lane(p, &st);
    if (rc != VAPOR_OK) return rc;
    if (p->ring.empty()) {
        p->ring.resize(ASYNC_RING);
        for (auto& r : p->ring)
            for (auto& e : r) { e = nullptr; HIPCHK(hipEventCreate(&e)); }
        HIPCHK(hmalloc(p->ctx, (void**)&p->h_loci, p->reads.im.loci_bytes));
        HIPCHK(hipEventCreateWithFlags(&p->ev_last, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&p->ev_clean, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&p->ev_fin, hipEventDisableTiming));
    }
    // The finish kernel goes to a stream of its own (highest priority): as a kernel it needs a CU with 56 free registers
    // per SIMD, which another plan's join (4 waves x 120) does not leave, so behind the clean kernels on the plan's
    // stream it held back the plan's next join until that other join was over (7 % of cfg2's rate).  On its own stream
    // it takes the first CU a join workgroup leaves; the next step's clean kernels wait for it, its join does not.
    hipStream_t fs = (p->fin && !p->ctx->user_stream) ? p->fin : st;
    if (p->have_after) {                        // vapor_plan_after: what the caller enqueued elsewhere comes first
        HIPCHK(hipStreamWaitEvent(fs, p->ev_after, 0));   // (it is the finish kernel that overwrites the records)
        p->have_after = false;
    }
    // the sticky overflow counter reports on the asynchronous steps since the last vapor_plan_sync: what a blocking
    // run counted before it resized the slots is not theirs
    if (p->ring_n == 0 && p->acc_n == 0) HIPCHK(hipMemsetAsync(p->d_overflow + 2, 0, sizeof(unsigned int), st));
    hipEvent_t* ev = p->ring[(size_t)p->ring_n].data();
    int table = 0;
    rc = join_table_for_async(p, st, &table);
    if (rc != VAPOR_OK) return rc;
    rc = plan_run_once(p, table, false, ev, st, p->big_known && p->n_big == 0, (fs != st && p->have_fin) ? p->ev_fin : nullptr, false);
    if (rc != VAPOR_OK) return rc;
    double* d_out = d_loci_out ? static_cast<double*>(d_loci_out) : p->reads.d_loci;
    if (fs != st) {
        HIPCHK(hipEventRecord(p->ev_clean, st));
        HIPCHK(hipStreamWaitEvent(fs, p->ev_clean, 0));
    }
    // (the finish kernel writes the pinned host copy itself: no copy kernel behind it)
    if ((rc = launch_finish(fs, p->reads, p->d_stats, d_out, p->h_loci)) != VAPOR_OK) return rc;
    HIPCHK(hipEventRecord(ev[3], fs));
    HIPCHK(hipEventRecord(p->ev_last, fs));
    if (fs != st) {
        HIPCHK(hipEventRecord(p->ev_fin, fs));
        p->have_fin = true;
    }
    p->have_last = true;
    if (!p->ctx->user_stream && p->lane_ix >= 0) p->ctx->lane_plan[p->lane_ix] = p;
    ++p->ring_n;
    return VAPOR_OK;
}

// Ordering against a stream of the caller's without a host round trip (e.g. a framework's collective on its own
// stream): vapor_plan_then makes `hip_stream` wait for the plan's most recently enqueued step (so the caller can read
// d_loci_out there), vapor_plan_after makes the plan's NEXT step wait for everything enqueued on `hip_stream` so far
// (so that step does not overwrite d_loci_out under the caller's feet).
extern "C" int vapor_plan_then(vapor_plan* p, void* hip_stream)
{
    if (!p) return fail(VAPOR_E_ARG, "vapor_plan_then: null plan");
    if (!p->have_last) return VAPOR_OK;
    HIPCHK(hipSetDevice(p->ctx->device));
    HIPCHK(hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), p->ev_last, 0));
    return VAPOR_OK;
}

extern "C" int vapor_plan_after(vapor_plan* p, void* hip_stream)
{
    if (!p) return fail(VAPOR_E_ARG, "vapor_plan_after: null plan");
    HIPCHK(hipSetDevice(p->ctx->device));
    if (!p->ev_after) HIPCHK(hipEventCreateWithFlags(&p->ev_after, hipEventDisableTiming));
    HIPCHK(hipEventRecord(p->ev_after, static_cast<hipStream_t>(hip_stream)));
    p->have_after = true;
    return VAPOR_OK;
}

// waits for the steps in flight; timings() then reports their averages; loci_out (may be NULL) receives the
// records of the last step.  VAPOR_E_OVERFLOW if a pair outgrew its slot in one of them (run vapor_plan_run_loci).
extern "C" int vapor_plan_sync(vapor_plan* p, double* loci_out)
{
    if (!p) return fail(VAPOR_E_ARG, "vapor_plan_sync: null plan");
    HIPCHK(hipSetDevice(p->ctx->device));
    const int had = p->ring_n;
    int rc0 = async_fold(p);
    if (rc0 != VAPOR_OK) return rc0;
    if (p->acc_n > 0) {
        p->t_join = (float)(p->acc_ms[0] / p->acc_n); p->t_clean = (float)(p->acc_ms[1] / p->acc_n);
        p->t_finish = (float)(p->acc_ms[2] / p->acc_n); p->t_total = (float)(p->acc_ms[3] / p->acc_n);
        if (loci_out && p->reads.n_loci && (had > 0 || p->h_loci))
            memcpy(loci_out, p->h_loci, sizeof(double) * fp::LOCUS_DOUBLES * (size_t)p->reads.n_loci);
    }
    p->acc_ms[0] = p->acc_ms[1] = p->acc_ms[2] = p->acc_ms[3] = 0;
    p->acc_n = 0;
    unsigned int sticky = 0;
    HIPCHK(hipMemcpy(&sticky, p->d_overflow + 2, sizeof(unsigned int), hipMemcpyDeviceToHost));
    if (sticky) {
        HIPCHK(hipMemset(p->d_overflow + 2, 0, sizeof(unsigned int)));
        return fail(VAPOR_E_OVERFLOW, "a pair outgrew its record slot during the asynchronous steps; run vapor_plan_run_loci (it resizes)" +
                    std::string(p->big_known ? "" : " [no blocking run has counted the pairs left to clean_big_kernel]") +
                    " [pairs left to clean_big_kernel on the last blocking run: " + std::to_string(p->n_big) + "]");
    }
    return VAPOR_OK;
}

#if defined(VAPOR_PHASE_TIMING) || defined(VAPOR_BLOCK_TIMING)
extern "C" int vapor_debug_block_ticks(double* out, int32_t n)
{
    std::vector<unsigned long long> h(4096);
    if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(vapor::g_block_ticks), sizeof(unsigned long long) * 4096) != hipSuccess) return -1;
    for (int x = 0; x < n && x < 4096; ++x) out[x] = (double)h[(size_t)x];
    return 0;
}
#endif
#if defined(VAPOR_PHASE_TIMING) || defined(VAPOR_BLOCK_TIMING)
extern "C" int vapor_debug_block_info(double* info, double* phase, int32_t n)
{
    std::vector<unsigned long long> h(4096 * 4), ph(4096 * 8), z(4096 * 8, 0ULL);
    if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(vapor::g_block_info), sizeof(unsigned long long) * 4096 * 4) != hipSuccess) return -1;
    for (int x = 0; x < n * 4 && x < 4096 * 4; ++x) info[x] = (double)h[(size_t)x];
#ifdef VAPOR_PHASE_TIMING
    if (hipMemcpyFromSymbol(ph.data(), HIP_SYMBOL(vapor::g_block_phase), sizeof(unsigned long long) * 4096 * 8) != hipSuccess) return -1;
    for (int x = 0; x < n * 8 && x < 4096 * 8; ++x) phase[x] = (double)ph[(size_t)x];
    if (hipMemcpyToSymbol(HIP_SYMBOL(vapor::g_block_phase), z.data(), sizeof(unsigned long long) * 4096 * 8) != hipSuccess) return -1;
#endif
    return 0;
}
// developer build only: the join tasks of a plan (first index into the sorted pair list, pairs in the task) and
// the sorted pair list itself
extern "C" int vapor_debug_plan_tasks(vapor_plan* p, int32_t* first, int32_t* n_reads, int32_t cap, int32_t* order, int32_t order_cap)
{
    if (!p) return -1;
    const int n = (int)p->tasks.size();
    for (int x = 0; x < n && x < cap; ++x) { first[x] = p->tasks[(size_t)x].first; n_reads[x] = p->tasks[(size_t)x].n_reads; }
    for (int x = 0; x < (int)p->task_pairs.size() && x < order_cap; ++x) order[x] = p->task_pairs[(size_t)x];
    return n;
}
#endif
#ifdef VAPOR_PHASE_TIMING
// developer build only: read (and clear) the per-phase tick sums
extern "C" int vapor_debug_phases(double* out, int32_t n)
{
    unsigned long long h[64];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(vapor::g_phase), sizeof(h)) != hipSuccess) return -1;
    for (int x = 0; x < n && x < 64; ++x) out[x] = (double)h[x];
    memset(h, 0, sizeof(h));
    if (hipMemcpyToSymbol(HIP_SYMBOL(vapor::g_phase), h, sizeof(h)) != hipSuccess) return -1;
    return 0;
}
#endif
