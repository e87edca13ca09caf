// dots_plan_check.cpp - the host side of the explicit-dot routes (vapor_amd/csrc/vapor_dots_plan.h) held to direct statements of its
// rules, as a program of its own under the address and undefined-behaviour sanitizers (tests/test_dots_plan_cpu.py builds and runs
// it; no HIP, no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc
//       tools/dots_plan_check.cpp -o dots_plan_check && ./dots_plan_check dots_plan.json
// The argument is tests/golden/dots_plan.json.gz, unpacked: what the formulas answered before they moved into the header
// (tools/dots_plan_fixture.cpp).
#include "vapor_dots_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

using namespace vapor;
namespace dp = vapor::dots_plan;

static int g_bad = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            if (++g_bad <= 20) {                            \
                std::printf("FAILED %s: ", #cond);          \
                std::printf(__VA_ARGS__);                   \
                std::printf("\n");                          \
            }                                               \
        }                                                   \
    } while (0)

// ------------------------------------------------------------------------------------------
// refusals
// ------------------------------------------------------------------------------------------
// the set of the cases: 0 good, 1 good, 2 a symbol outside the alphabet with its bytes kept, 3 too long, 4 too long and such a
// symbol, 5 such a symbol and no bytes (a derived sequence behind the kept ones), 6 such a symbol and too short for a k-mer
enum { GOOD1, GOOD2, BAD_KEPT, LONG, LONG_BAD, BAD_NO_BYTES, SHORT_BAD, N_SEQ };
struct World {
    SeqDesc h[N_SEQ + 1] = {};                     // (one hidden sequence behind the caller's: not a valid index)
    int64_t raw_off[5] = {-1, -1, 0, -1, 112};
    dp::SetView view() const { return dp::SetView{N_SEQ, h, raw_off, 5}; }
    World()
    {
        const int len[N_SEQ] = {100, 300, 100, VAPOR_MAX_WIDE_SEQ_LEN + 1, VAPOR_MAX_WIDE_SEQ_LEN + 1, 100, 5};
        const int bad[N_SEQ] = {0, 0, 2, 0, 1, 1, 1};
        for (int i = 0; i < N_SEQ; ++i) { h[i].len = len[i]; h[i].n_invalid = bad[i]; }
        h[N_SEQ].len = 100;
    }
};

// the order of each route's rules and the status each gives, written out: what include/vapor_hip.h promises
struct Want { dp::Rule rule; int code; };
static const std::vector<Want> WIDE_ORDER = {{dp::INDICES, -4}, {dp::OFF2, -4}, {dp::K_WIDE, -4}, {dp::LENGTH, -4}, {dp::KEY_ERROR, -3}};
static const std::vector<Want> ANYK_INV_ORDER = {{dp::INDICES, -4}, {dp::OFF2, -4}, {dp::K_ANY, -4}, {dp::LENGTH, -4}, {dp::KEY_ERROR, -3}};
static const std::vector<Want> ANYK_FWD_ORDER = {{dp::INDICES, -4}, {dp::OFF2, -4}, {dp::K_ANY, -4}, {dp::LENGTH, -4}, {dp::NO_BYTES, -4}};

// a pair that breaks exactly the rules of `mask` (bits by dp::Rule) where the sequences can be read at all
static vapor_pair breaking(unsigned mask, bool forward, int variant)
{
    auto has = [&](dp::Rule r) { return (mask >> r) & 1u; };
    vapor_pair a{GOOD1, GOOD2, 0, 10, forward ? VAPOR_PF_FORWARD | 3u : 3u};
    if (has(dp::KEY_ERROR)) a.seq1 = has(dp::LENGTH) ? LONG_BAD : BAD_KEPT;
    else if (has(dp::LENGTH)) { if (variant && !has(dp::NO_BYTES)) a.seq2 = LONG; else a.seq1 = LONG; }
    if (has(dp::NO_BYTES)) { if (variant && !has(dp::LENGTH)) a.seq1 = BAD_NO_BYTES; else a.seq2 = BAD_NO_BYTES; }
    if (has(dp::OFF2)) a.off2 = variant ? INT32_MIN : -1;
    if (has(dp::K_WIDE)) a.k = variant ? 15 : 50;
    if (has(dp::K_ANY)) a.k = variant ? 0 : VAPOR_MAX_ANY_K + 1;
    if (has(dp::INDICES)) {
        if (has(dp::NO_BYTES) || has(dp::LENGTH)) a.seq1 = variant ? -1 : N_SEQ;       // (N_SEQ: the hidden sequence)
        else a.seq2 = variant ? -1 : N_SEQ;
    }
    return a;
}

static int check_route(const char* name, const std::vector<Want>& order, const dp::Step* steps, int n_steps, bool forward,
                       int (*admit)(const dp::SetView&, const vapor_pair&))
{
    const World w;
    const dp::SetView v = w.view();
    int n = 0;
    CHECK((int)order.size() <= n_steps, "%s: %d steps", name, n_steps);
    for (int variant = 0; variant < 2; ++variant) {
        const vapor_pair good = breaking(0u, forward, variant);
        CHECK(admit(v, good) == 0 && dp::first_broken(steps, n_steps, v, good, !forward) == -1, "%s: a good pair", name);
        ++n;
        for (size_t r1 = 0; r1 < order.size(); ++r1) {
            const vapor_pair one = breaking(1u << order[r1].rule, forward, variant);
            CHECK(admit(v, one) == order[r1].code, "%s rule %zu alone: %d", name, r1, admit(v, one));
            const int at = dp::first_broken(steps, n_steps, v, one, !forward);
            CHECK(at >= 0 && steps[at].rule == order[r1].rule, "%s rule %zu alone: step %d", name, r1, at);
            // alone: no other rule of the route is broken by that pair (where the sequences can be read)
            for (size_t r2 = 0; r2 < order.size(); ++r2)
                if (r2 != r1 && order[r1].rule != dp::INDICES) CHECK(!dp::broken(order[r2].rule, v, one, !forward), "%s rule %zu alone breaks rule %zu", name, r1, r2);
            ++n;
            for (size_t r2 = r1 + 1; r2 < order.size(); ++r2) {
                const vapor_pair two = breaking((1u << order[r1].rule) | (1u << order[r2].rule), forward, variant);
                if (order[r1].rule != dp::INDICES)
                    CHECK(dp::broken(order[r1].rule, v, two, !forward) && dp::broken(order[r2].rule, v, two, !forward), "%s rules %zu and %zu: both broken", name, r1, r2);
                const int at2 = dp::first_broken(steps, n_steps, v, two, !forward);
                CHECK(admit(v, two) == order[r1].code && at2 >= 0 && steps[at2].rule == order[r1].rule, "%s rules %zu and %zu: %d at step %d", name, r1, r2,
                      admit(v, two), at2);
                ++n;
            }
        }
    }
    return n;
}

static void check_refusals()
{
    int n = check_route("wide", WIDE_ORDER, dp::WIDE_STEPS, dp::N_WIDE_STEPS, false, dp::admit_wide);
    n += check_route("any-k", ANYK_INV_ORDER, dp::ANYK_STEPS, dp::N_ANYK_STEPS, false, dp::admit_anyk);
    n += check_route("any-k forward", ANYK_FWD_ORDER, dp::ANYK_STEPS, dp::N_ANYK_STEPS, true, dp::admit_anyk);
    const World w;
    const dp::SetView v = w.view();
    // what is no refusal: a symbol outside the alphabet in a read too short for a k-mer, or in seq2; forward, one whose bytes were
    // kept; with inversions, one whose bytes were not; every k of each route and none of the other's
    CHECK(dp::admit_wide(v, vapor_pair{SHORT_BAD, GOOD1, 0, 10, 3u}) == 0 && dp::admit_anyk(v, vapor_pair{SHORT_BAD, GOOD1, 0, 10, 3u}) == 0, "no k-mer, no key error");
    CHECK(dp::admit_wide(v, vapor_pair{GOOD1, BAD_KEPT, 0, 10, 3u}) == 0 && dp::admit_anyk(v, vapor_pair{GOOD1, BAD_NO_BYTES, 0, 10, 3u}) == 0, "seq2 raises nothing");
    CHECK(dp::admit_anyk(v, vapor_pair{BAD_KEPT, BAD_KEPT, 0, 10, VAPOR_PF_FORWARD}) == 0, "forward over kept bytes");
    CHECK(dp::admit_anyk(v, vapor_pair{SHORT_BAD, GOOD1, 0, 10, VAPOR_PF_FORWARD}) == -4, "forward: bytes beyond the kept table");
    CHECK(dp::admit_wide(v, vapor_pair{GOOD1, GOOD2, 1 << 30, 10, 3u}) == 0, "off2 behind the allele");
    for (int k = -1; k <= 70; ++k) {
        CHECK((dp::admit_wide(v, vapor_pair{GOOD1, GOOD2, 0, k, 3u}) == 0) == (k == 10 || k == 20 || k == 30 || k == 40), "wide k %d", k);
        CHECK((dp::admit_anyk(v, vapor_pair{GOOD1, GOOD2, 0, k, 3u}) == 0) == (k >= 1 && k <= 64), "any k %d", k);
    }
    n += 5;

    // the calls
    auto says = [](const dp::Refusal& r, const char* msg) { return msg ? r.code == VAPOR_E_ARG && r.msg && !std::strcmp(r.msg, msg) : (r.code == 0 && !r); };
    const vapor_pair pr[2] = {};
    const int64_t st[32] = {0};
    int64_t ho[3] = {0};
    const int32_t ji[8] = {1, 2, 3, 4, VAPOR_MAX_WIDE_SEQ_LEN, 0, 7, 7};
    const dp::Call ok{dp::BATCH, true, 2, st, ji, ho, pr, 4, 0};
    int nc = 0;
    auto batch = [&](auto change, const char* msg, const char* what) {
        dp::Call c = ok;
        change(c);
        CHECK(says(dp::call_refusal(c), msg), "batch call: %s", what);
        ++nc;
    };
    batch([](dp::Call&) {}, nullptr, "a good call");
    batch([](dp::Call& c) { c.handles = false; }, "null argument", "no context or no set");
    batch([](dp::Call& c) { c.n = -1; }, "null argument", "a negative count");
    batch([](dp::Call& c) { c.pairs = nullptr; }, "null argument", "no pairs");
    batch([](dp::Call& c) { c.stats = nullptr; }, "null argument", "no statistics");
    batch([](dp::Call& c) { c.off = nullptr; }, "null argument", "dots wanted without hit_off");
    batch([](dp::Call& c) { c.hits_capacity = -1; }, "null argument", "a negative capacity");
    batch([](dp::Call& c) { c.hits_ji = nullptr; c.off = nullptr; c.hits_capacity = 0; }, nullptr, "no dots wanted");
    batch([](dp::Call& c) { c.n = 0; c.pairs = nullptr; c.stats = nullptr; }, nullptr, "no pairs at all");
    const int64_t off[] = {0, 2, 3}, longer[] = {0, 3, 3}, back[] = {0, 2, 1}, huge[] = {0, (int64_t)1 << 31};
    const dp::Call lists{dp::LISTS, true, 2, st, ji, off, nullptr, 0, 2};
    auto list = [&](auto change, const char* msg, const char* what) {
        dp::Call c = lists;
        change(c);
        CHECK(says(dp::call_refusal(c), msg), "list call: %s", what);
        ++nc;
    };
    list([](dp::Call&) {}, nullptr, "two good lists, a coordinate at the route's limit");
    list([](dp::Call& c) { c.handles = false; }, "null argument", "no context");
    list([](dp::Call& c) { c.stats = nullptr; }, "null argument", "no statistics");
    list([](dp::Call& c) { c.hits_ji = nullptr; }, "null hit list", "no dots");
    list([&](dp::Call& c) { c.off = longer; }, "bad list offsets", "a list above max_pair_cap");
    list([&](dp::Call& c) { c.off = longer; c.max_pair_cap = 3; }, nullptr, "a list at max_pair_cap");
    list([&](dp::Call& c) { c.off = back; }, "bad list offsets", "offsets that decrease");
    // (a list beyond the dot bound is refused by its offsets, before a dot of it is read, whatever max_pair_cap says)
    list([&](dp::Call& c) { c.n = 1; c.off = huge; c.max_pair_cap = INT64_MAX; }, "bad list offsets", "a list of 2^31 dots");
    const int32_t far[8] = {1, 2, 3, 4, VAPOR_MAX_WIDE_SEQ_LEN + 1, 0, 7, 7};
    list([&](dp::Call& c) { c.hits_ji = far; }, "coordinate out of range", "a coordinate above the route's");
    list([](dp::Call& c) { c.n = 0; c.off = nullptr; c.stats = nullptr; c.hits_ji = nullptr; }, nullptr, "no lists");
    std::printf("refusals: %d pairs in order, %d calls\n", n, nc);
}

// ------------------------------------------------------------------------------------------
// shapes and the wide join
// ------------------------------------------------------------------------------------------
static void check_hash()
{
    SeqDesc s1{}, s2{};
    s1.len = 100; s2.len = 300;
    const dp::Shape a = dp::shape(s1, s2, vapor_pair{0, 1, 0, 10, 0u}), b = dp::shape(s1, s2, vapor_pair{0, 1, 291, 10, 0u}), c = dp::shape(s1, s2, vapor_pair{0, 1, 292, 10, 0u}),
                    d = dp::shape(s1, s2, vapor_pair{0, 1, INT32_MAX, 64, 0u}), e = dp::shape(s1, s2, vapor_pair{0, 1, 0, 64, 0u}),
                    f = dp::shape(s1, s2, vapor_pair{0, 1, 0, 100, 0u}), g = dp::shape(s1, s2, vapor_pair{0, 1, 0, 101, 0u});
    CHECK(a.nk1 == 91 && a.nk2 == 291 && a.n2 == 300 && a.kmers(), "100 x 300 at k 10");
    CHECK(b.nk2 == 0 && b.n2 == 9 && !b.kmers() && c.nk2 == -1 && c.n2 == 8, "an allele of nine and of eight symbols");
    CHECK(d.n2 == 0 && d.nk2 == -63 && !d.kmers() && e.nk1 == 37 && e.kmers(), "off2 behind the allele; k 64");
    CHECK(f.nk1 == 1 && f.kmers() && g.nk1 == 0 && !g.kmers(), "a read of exactly one k-mer, and of none");

    std::mt19937 rng(5);
    long long n = 0;
    auto at = [&](int nk1) {
        const int k = 10 * (1 + (int)(rng() % 4)), nk2 = 1 + (int)(rng() % 100000);
        const dp::WideJoin w = dp::wide_join(k, nk1, nk2);
        const int64_t ne = 2 * (int64_t)nk1;
        CHECK(w.ne == ne && w.H && (w.H & (w.H - 1)) == 0 && w.mask == w.H - 1, "nk1 %d: H %u", nk1, w.H);
        CHECK(2 * ne <= (int64_t)w.H && ((int64_t)w.H < 4 * ne || (nk1 == 1 && w.H == 4)), "nk1 %d: %lld entries in %u buckets", nk1, (long long)ne, w.H);
        CHECK(w.heads == 4 * (size_t)w.H && w.nexts == 4 * (size_t)ne && w.counts == 4 * (size_t)nk2 && w.offsets == 8 * ((size_t)nk2 + 1), "nk1 %d: bytes", nk1);
        CHECK((int64_t)w.table_grid * 256 >= ne && ((int64_t)w.table_grid - 1) * 256 < ne && (int64_t)w.probe_grid * 256 >= nk2 && ((int64_t)w.probe_grid - 1) * 256 < nk2 &&
                  w.scan_grid == 1, "nk1 %d: grids", nk1);
        ++n;
    };
    for (int nk1 = 1; nk1 <= 5000; ++nk1) at(nk1);
    for (int t = 0; t < 5000; ++t) at(1 + (int)(rng() % (1u << 20)));
    at(1 << 20);
    CHECK(dp::wide_join(10, 1, 1).H == 4 && dp::wide_join(10, 128, 1).H == 512 && dp::wide_join(10, 129, 1).H == 1024, "the edges at 1, 128 and 129 k-mers");
    CHECK(dp::wide_key_bytes(10) == 8 && dp::wide_key_bytes(20) == 12 && dp::wide_key_bytes(30) == 16 && dp::wide_key_bytes(40) == 20, "key bytes");
    CHECK(dp::wide_join(10, 91, 7).keys == 1456 && dp::wide_join(20, 91, 7).keys == 2184 && dp::wide_join(30, 91, 7).keys == 2912 && dp::wide_join(40, 91, 7).keys == 3640, "key bytes of 182 entries");
    CHECK(dp::grid(0) == 0 && dp::grid(1) == 1 && dp::grid(256) == 1 && dp::grid(257) == 2 && dp::THREADS == 256 && dp::BLOCK_FLOOR == 256, "grids");
    std::printf("hash table: %lld sizes\n", n);
}

// ------------------------------------------------------------------------------------------
// the any-k pass
// ------------------------------------------------------------------------------------------
static void check_sort()
{
    static_assert(ANYK_TILE == 512 && ANYK_EDIT_WAVES == 4 && ANYK_EXACT_MAX_K == 40 && ANYK_EDIT_PAIRS == (1ll << 31), "the constants");
    // the size: the smallest power of two that holds the entries, a tile at least
    for (int n = 0; n <= (1 << 21); ++n) {
        const int np = dp::sort_size(n);
        if (!(np >= 512 && (np & (np - 1)) == 0 && np >= n && (np == 512 || np / 2 < n))) CHECK(false, "%d entries sorted in %d", n, np);
    }
    // the schedule: the compare-exchange stages it performs, (merge size, stride), are those of the bitonic network of np elements -
    // every merge size 2 .. np, every stride from half of it down to 1 - with every stride of 512 and more a launch of its own
    int n_sizes = 0;
    for (int np = 512; np <= (1 << 21); np <<= 1, ++n_sizes) {
        const std::vector<dp::SortStep> s = dp::sort_schedule(np);
        std::vector<std::pair<int, int>> did, want;
        for (int size = 2; size <= np; size <<= 1)
            for (int jj = size / 2; jj > 0; jj >>= 1) want.push_back({size, jj});
        int n_global = 0;
        for (const dp::SortStep& x : s) {
            if (x.local && x.full) {
                for (int size = 2; size <= 512; size <<= 1)
                    for (int jj = size / 2; jj > 0; jj >>= 1) did.push_back({size, jj});
            } else if (x.local) {
                for (int jj = 256; jj > 0; jj >>= 1) did.push_back({x.kk, jj});
            } else {
                CHECK(x.jj >= 512 && x.jj < x.kk, "np %d: a global step of stride %d in merge %d", np, x.jj, x.kk);
                did.push_back({x.kk, x.jj});
                ++n_global;
            }
        }
        CHECK(did == want, "np %d: %zu stages, the network has %zu", np, did.size(), want.size());
        CHECK(s.front().local && s.front().full == 1 && s.back().local, "np %d: the ends", np);
        if (np == 512) CHECK(s.size() == 1 && n_global == 0, "one tile: %zu launches", s.size());
    }
    // and it sorts: the schedule run on the host, tile by tile as the kernels do it
    std::mt19937 rng(9);
    for (int np : {512, 1024, 4096, 16384}) {
        std::vector<uint32_t> v((size_t)np);
        for (auto& x : v) x = rng() % 1000;
        auto exchange = [&](int lo, int jj, int size) {
            const bool up = (lo & size) == 0;
            if ((v[(size_t)lo + jj] < v[(size_t)lo]) == up) std::swap(v[(size_t)lo], v[(size_t)lo + jj]);
        };
        for (const dp::SortStep& x : dp::sort_schedule(np)) {
            if (!x.local) {
                for (int q = 0; q < np / 2; ++q) exchange(2 * q - (q & (x.jj - 1)), x.jj, x.kk);
                continue;
            }
            for (int size = x.full ? 2 : x.kk; size <= (x.full ? 512 : x.kk); size <<= 1)
                for (int jj = std::min(size, 512) >> 1; jj > 0; jj >>= 1)
                    for (int q = 0; q < np / 2; ++q) exchange(2 * q - (q & (jj - 1)), jj, size);
        }
        CHECK(std::is_sorted(v.begin(), v.end()), "np %d: not sorted", np);
    }
    // a 10 kb read with inversions
    SeqDesc s1{}, s2{};
    s1.len = 10000; s2.len = 20000;
    const vapor_pair a{0, 1, 0, 10, 3u};
    const dp::AnykPass p = dp::anyk_pass(10, true, s1.len, dp::shape(s1, s2, a));
    CHECK(p.n == 19982 && p.np == 32768 && dp::sort_schedule(p.np).size() == 28, "a 10 kb read: %d entries, %zu launches", p.n, dp::sort_schedule(p.np).size());
    CHECK(p.exact && p.bytes[dp::ANYK_IDX] == 131072 && p.bytes[dp::ANYK_CNT] == 4 * 19991 && p.bytes[dp::ANYK_FIRST] == 4 * 19991 && p.bytes[dp::ANYK_OFF] == 8 * 19992 &&
              !p.bytes[dp::ANYK_ISF] && !p.bytes[dp::ANYK_RUN] && !p.bytes[dp::ANYK_RANK] && !p.bytes[dp::ANYK_KEYS] && p.bytes[dp::ANYK_SYM] == p.sym.bytes, "the exact branch's blocks");
    CHECK(p.iota_grid == 128 && p.tile_grid == 64 && p.stride_grid == 64 && p.entry_grid == 79 && p.allele_grid == 79, "the grids");
    const dp::AnykPass q = dp::anyk_pass(41, false, s1.len, dp::shape(s1, s2, vapor_pair{0, 1, 0, 41, VAPOR_PF_FORWARD}));
    CHECK(!q.exact && q.n == 9960 && q.np == 16384 && q.bytes[dp::ANYK_ISF] == 4 * 9960 && q.bytes[dp::ANYK_RUN] == 8 * 9960 && q.bytes[dp::ANYK_RANK] == 8 * 9961 &&
              q.bytes[dp::ANYK_KEYS] == 16 * 9960 && !q.bytes[dp::ANYK_FIRST] && q.bytes[dp::ANYK_CNT] == 4 * 19960, "the edit branch's blocks");
    std::printf("sort schedule: %d sizes are the bitonic network, 10 kb in 28 launches\n", n_sizes);
}

static void check_symbols()
{
    std::vector<int> lens;
    for (int n = 0; n <= 100; ++n) lens.push_back(n);
    for (int m = 112; m <= 4096; m += 16)
        for (int d = -1; d <= 1; ++d) lens.push_back(m + d);
    long long n = 0;
    for (int len1 : lens)
        for (int n2 : lens)
            for (int inv = 0; inv < 2; ++inv, ++n) {
                const dp::Symbols y = dp::symbols(len1, n2, inv != 0);
                // the strings in their order, each [start, start + length); the next one (or the end) at least 16 bytes behind
                std::vector<std::pair<size_t, size_t>> str = {{y.s1, (size_t)len1}};
                if (inv) str.push_back({y.r1, (size_t)len1});
                str.push_back({y.s2, (size_t)n2});
                bool ok = y.s1 == 0;
                for (size_t t = 0; t < str.size(); ++t) {
                    const size_t next = t + 1 < str.size() ? str[t + 1].first : y.bytes;
                    ok = ok && str[t].first % 16 == 0 && str[t].first + str[t].second + 16 <= next;
                }
                if (!ok || y.bytes % 16) CHECK(false, "%d and %d symbols, inversions %d: %zu, %zu, %zu of %zu", len1, n2, inv, y.s1, y.r1, y.s2, y.bytes);
            }
    CHECK(dp::symbols(0, 0, false).bytes == 32 && dp::symbols(100, 300, true).s2 == 256 && dp::symbols(100, 300, true).bytes == 576 && dp::symbols(16, 1, false).s2 == 32, "literals");
    std::printf("symbol layout: %lld layouts, strings disjoint, on 16 bytes, 16 bytes behind each\n", n);
}

static void check_edit_cut()
{
    const int ns[] = {1, 2, 3, 250, 251, 252, 253, 1000, 399902, 1 << 21};
    const int nk2s[] = {1, 3, 4, 5, 63, 64, 65, 351, 12151, 1 << 20};
    const long long caps[] = {1, 3, 4, 1008, 2016, 16128, 1ll << 20, 1ll << 31, (1ll << 31) + 1, 1ll << 40, INT64_MAX};
    long long n = 0;
    for (int en : ns)
        for (int nk2 : nk2s)
            for (long long cap : caps) {
                const dp::EditCut c = dp::edit_cut(en, nk2, cap);
                CHECK(c.per >= 4 && c.per % 4 == 0 && (c.per == 4 || c.per <= cap / en), "n %d, %lld pairs: %lld a launch", en, cap, c.per);
                if (c.per > 4) CHECK(c.per > cap / en - 4, "n %d, %lld pairs: %lld a launch is not the most", en, cap, c.per);
                int at = 0;
                bool ok = c.launches() >= 1;
                for (int t = 0; t < c.launches(); ++t) {
                    ok = ok && c.j0(t) == at && c.j1(t) > at && c.j1(t) <= nk2;
                    if (t + 1 < c.launches()) ok = ok && c.j1(t) - c.j0(t) == c.per;
                    ok = ok && (long long)c.grid(t) * 4 >= c.j1(t) - c.j0(t) && ((long long)c.grid(t) - 1) * 4 < c.j1(t) - c.j0(t);
                    at = c.j1(t);
                    if (!ok || t > 4) break;      // (the first launches; the last one below)
                }
                const int last = c.launches() - 1;
                ok = ok && c.j1(last) == nk2 && c.j0(last) < nk2 && (last == 0 || c.j0(last) == c.j1(last - 1)) && c.j0(last) == (long long)last * c.per;
                if (c.launches() <= 6) ok = ok && at == nk2;
                CHECK(ok, "n %d, nk2 %d, %lld pairs: the ranges do not tile", en, nk2, cap);
                ++n;
            }
    CHECK(dp::edit_cut(1, 0, 1).launches() == 0 && dp::edit_cut(0, 5, 1ll << 31).per == (1ll << 31), "no allele k-mer; no entry");
    // what the designs state: the read of 200 000 symbols at the shipped size, and 252 per for per in 4, 8, 64
    const dp::EditCut big = dp::edit_cut(399902, 12151, ANYK_EDIT_PAIRS);
    CHECK(big.per == 5368 && big.launches() == 3 && big.j0(2) == 10736 && big.j1(2) == 12151 && big.grid(0) == 1342 && big.grid(2) == 354, "200 000 symbols: %lld a launch, %d launches", big.per, big.launches());
    for (int per : {4, 8, 64})
        for (int en : {251, 252}) {
            const dp::EditCut c = dp::edit_cut(en, 351, 252ll * per);
            CHECK(c.per == per && c.launches() == (351 + per - 1) / per, "252 x %d over %d entries: %lld a launch", per, en, c.per);
        }
    CHECK(dp::edit_cut(252, 351, 252 * 4).launches() == 88 && dp::edit_cut(252, 351, 252 * 8).launches() == 44 && dp::edit_cut(252, 351, 252 * 64).launches() == 6, "launch counts");
    std::printf("edit cut: %lld cuts tile their allele, 200 000 symbols in 3 launches\n", n);
}

// ------------------------------------------------------------------------------------------
// the cleaning, the records, the capacity protocol, the dot bound
// ------------------------------------------------------------------------------------------
static void check_cleaning()
{
    struct Row { int n_passes; dp::ClusterPass pass[3]; bool zero, dir; };
    const dp::ClusterPass D{0, 0u, 0, 0}, A1{1, 0u, 1, 1}, A2{1, 2u, 2, 2}, none{0, 0u, 0, 0};
    const Row rows[8] = {{0, {none, none, none}, true, false}, {2, {D, A1, none}, false, false}, {2, {D, A2, none}, false, false}, {3, {D, A1, A2}, false, false},
                         {0, {none, none, none}, true, false}, {2, {D, A1, none}, false, true},  {2, {D, A2, none}, false, false}, {3, {D, A1, A2}, false, true}};
    for (uint32_t f = 0; f < 16; ++f) {      // (bit 3, VAPOR_PF_FORWARD, changes nothing)
        const dp::Cleaning c = dp::cleaning(f);
        const Row& r = rows[f & 7u];
        bool same = c.n_passes == r.n_passes && c.zero_flags == r.zero && c.dir == r.dir && dp::wants_dir(f) == r.dir;
        for (int t = 0; t < r.n_passes; ++t)
            same = same && c.pass[t].axis == r.pass[t].axis && c.pass[t].skip == r.pass[t].skip && c.pass[t].slot == r.pass[t].slot && c.pass[t].mode == r.pass[t].mode;
        CHECK(same, "flags %u", f);
    }
    const dp::Scratch a = dp::scratch(0, 0), b = dp::scratch(1, 0), c = dp::scratch(0, 1), d = dp::scratch(VAPOR_MAX_WIDE_SEQ_LEN, VAPOR_MAX_WIDE_SEQ_LEN);
    CHECK(a.R == 1 && a.shift == 0 && a.bytes == 12 && a.axis_bytes() == 4, "one value");
    CHECK(b.R == 2 && b.shift == 0 && b.bytes == 24 && c.R == 2 && c.shift == 1 && c.bytes == 24, "two values");
    // the cap: every i + j and i - j + shift below 2^21, three words a value: the 24 MiB of DESIGN.md 4.9
    CHECK(d.R == 2097151 && d.shift == 1048575 && d.bytes == 25165812 && d.axis_bytes() * 3 == d.bytes, "the cap: %d values, %zu bytes", d.R, d.bytes);
    CHECK((size_t)3 * 4 * ((size_t)1 << 21) == (size_t)24 << 20 && d.bytes <= ((size_t)24 << 20) && d.bytes + 12 == ((size_t)24 << 20), "24 MiB");
    const int32_t ji[] = {5, 1, 2, 9, 7, 7, 0, 0};
    const dp::Extent all = dp::extent(ji, 0, 4), mid = dp::extent(ji, 1, 2), empty = dp::extent(ji, 2, 2);
    CHECK(all.mj == 7 && all.mi == 9 && mid.mj == 2 && mid.mi == 9 && empty.mi == 0 && empty.mj == 0 && dp::LIST_FLAGS == 3u, "the extent of a list");
    std::printf("cleaning: 8 flag values, the scratch at 4 extents\n");
}

static void check_records()
{
    const WideAcc z = dp::acc_init();
    CHECK(sizeof(WideAcc) == 112 && z.min_j == 2147483647 && z.max_j == -1 && z.kd_lo == 2147483647 && z.kd_hi == -2147483647, "the first accumulator");
    CHECK(!z.n_diag && !z.n_lower && !z.c1_kept && !z.c1_sum_abs && !z.c2_kept && !z.c2_count10 && !z.c2_kept_diag && !z.dir_sum2 && !z.dir_c2x && !z.dir_n && !z.dir_lists &&
              !z.max_group[0] && !z.max_group[1] && !z.max_group[2] && !z.max_group[3], "and its zeros");
    auto is = [](const int64_t* st, std::vector<int64_t> want) { return std::vector<int64_t>(st, st + 16) == want; };
    int64_t st[17];
    st[16] = 77;
    for (int t = 0; t < 16; ++t) st[t] = 99;
    dp::record_refused(VAPOR_E_KEYERROR, st);
    CHECK(is(st, {0, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -3}), "a refused pair");
    for (int t = 0; t < 16; ++t) st[t] = 99;
    dp::record_overflowed(((int64_t)1 << 28) + 4096, st);
    CHECK(is(st, {268439552, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 268439552, -2}), "a pair beyond the bound");
    WideAcc a = z;
    a.n_diag = 7; a.n_lower = 8; a.c1_kept = 3; a.c1_sum_abs = 4; a.c2_kept = 5; a.c2_count10 = 6; a.c2_kept_diag = 9;
    a.dir_sum2 = -12; a.min_j = 1; a.max_j = 2; a.dir_c2x = 10; a.dir_n = 11; a.dir_lists = 13; a.max_group[0] = 50;
    for (uint32_t f = 0; f < 16; ++f) {
        for (int t = 0; t < 16; ++t) st[t] = 99;
        dp::record_folded(a, 40, f, st);
        const bool dir = (f & 1u) && (f & 4u);
        CHECK(is(st, {40, 1, 2, 3, 4, 5, 6, 7, 8, 9, dir ? 10 : 0, dir ? 11 : 0, dir ? -12 : 0, dir ? 13 : 0, 0, 0}), "a scored pair under flags %u", f);
        for (int t = 0; t < 16; ++t) st[t] = 99;
        dp::record_folded(z, 0, f, st);
        CHECK(is(st, {0, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}), "no dots under flags %u", f);
    }
    CHECK(st[16] == 77, "a record is 16 words");
    std::printf("records: refused, overflowed and folded equal their literals\n");
}

static void check_capacity()
{
    // test_batch_state's three capacities over made-up counts: a pair without dots and a refused one among them
    const int64_t counts[] = {5, 0, 7, 0, 3}, need = 15;
    struct Run { int64_t cap; bool over; std::vector<int> copied; };
    const Run runs[] = {{need - 1, true, {1, 0, 1, 0, 0}}, {5, true, {1, 0, 0, 0, 0}}, {need, false, {1, 0, 1, 0, 1}}};
    for (const Run& r : runs) {
        int64_t off[6] = {-7, -7, -7, -7, -7, -7};
        dp::Capacity room(true, r.cap, off);
        CHECK(off[0] == 0, "hit_off[0]");
        int64_t at = 0;
        for (int t = 0; t < 5; ++t) {
            CHECK(room.fits(counts[t]) == (r.copied[(size_t)t] != 0) && room.running == at, "capacity %lld, pair %d", (long long)r.cap, t);
            if (room.fits(counts[t])) CHECK(room.running + counts[t] <= r.cap, "capacity %lld, pair %d written beyond it", (long long)r.cap, t);
            room.close(t, counts[t]);
            at += counts[t];
        }
        CHECK(room.overflowed() == r.over && off[1] == 5 && off[2] == 5 && off[3] == 12 && off[4] == 12 && off[5] == need, "capacity %lld: the end", (long long)r.cap);
    }
    int64_t off[3] = {-7, -7, -7};
    dp::Capacity stats_only(false, 0, off), nothing(false, 0, nullptr);
    CHECK(!stats_only.fits(4) && !nothing.fits(4), "no dots wanted");
    stats_only.close(0, 4); stats_only.close(1, 0); nothing.close(0, 4);
    CHECK(off[0] == 0 && off[1] == 4 && off[2] == 4 && !stats_only.overflowed() && !nothing.overflowed() && nothing.running == 4, "hit_off without hits_ji; neither");
    std::printf("capacity protocol: 3 capacities\n");

    CHECK(dp::dots_cap(1) == 1 && dp::dots_cap((int64_t)1 << 28) == ((int64_t)1 << 28) && dp::dots_cap(2147483647) == 2147483647 && dp::dots_cap((int64_t)1 << 31) == 2147483647 &&
              dp::dots_cap(INT64_MAX) == 2147483647, "the dot bound");
    // every count the routes hand a kernel as an int is at most the bound
    CHECK((int)dp::dots_cap(INT64_MAX) == 2147483647 && sizeof(int) == 4, "an int holds it");
    std::printf("dot bound: 5 values\n");
}

// ------------------------------------------------------------------------------------------
// every integer of the file behind "rows", eight a row (tools/dots_plan_fixture.cpp)
// ------------------------------------------------------------------------------------------
static void check_fixture(const char* path)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { CHECK(false, "cannot open %s", path); return; }
    std::string text;
    char buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
    std::fclose(f);
    const size_t rows = text.find("\"rows\"");
    CHECK(rows != std::string::npos, "no rows in %s", path);
    std::vector<long long> v;
    for (size_t at = rows == std::string::npos ? text.size() : rows; at < text.size();) {
        if (text[at] >= '0' && text[at] <= '9') {
            char* end = nullptr;
            v.push_back(std::strtoll(text.c_str() + at, &end, 10));
            at = (size_t)(end - text.c_str());
        } else ++at;
    }
    CHECK(v.size() % 8 == 0 && v.size() >= 8 * 3000, "%zu numbers", v.size());
    size_t n = 0, per_family[5] = {0, 0, 0, 0, 0};
    for (size_t t = 0; t + 8 <= v.size(); t += 8, ++n) {
        const long long fam = v[t], a = v[t + 1], b = v[t + 2], c = v[t + 3];
        long long got[4] = {0, 0, 0, 0};
        if (fam == 0) {
            const dp::WideJoin w = dp::wide_join((int)b, (int)a, 1);
            got[0] = w.H; got[1] = (long long)w.keys; got[2] = w.ne;
        } else if (fam == 1) {
            got[0] = dp::sort_size((int)a); got[1] = (long long)dp::sort_schedule((int)got[0]).size();
        } else if (fam == 2) {
            const dp::EditCut e = dp::edit_cut((int)a, (int)b, c);
            got[0] = e.per; got[1] = e.launches();
        } else if (fam == 3) {
            const dp::Symbols y = dp::symbols((int)a, (int)b, c != 0);
            got[0] = (long long)y.r1; got[1] = (long long)y.s2; got[2] = (long long)y.bytes;
        } else if (fam == 4) {
            const dp::Scratch s = dp::scratch((int)a, (int)b);
            got[0] = s.R; got[1] = s.shift; got[2] = (long long)s.bytes;
        } else {
            CHECK(false, "family %lld", fam);
            continue;
        }
        ++per_family[fam];
        CHECK(got[0] == v[t + 4] && got[1] == v[t + 5] && got[2] == v[t + 6] && got[3] == v[t + 7], "family %lld at (%lld, %lld, %lld): %lld, %lld, %lld", fam, a, b, c,
              got[0], got[1], got[2]);
    }
    for (size_t fam = 0; fam < 5; ++fam) CHECK(per_family[fam] >= 500, "family %zu: %zu points", fam, per_family[fam]);
    std::printf("fixture: %zu points equal what the formulas answered before\n", n);
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::printf("usage: dots_plan_check dots_plan.json\n"); return 2; }
    check_refusals();
    check_hash();
    check_sort();
    check_symbols();
    check_edit_cut();
    check_cleaning();
    check_records();
    check_capacity();
    check_fixture(argv[1]);
    if (g_bad) { std::printf("dots_plan_check: %d statements FAILED\n", g_bad); return 1; }
    std::printf("dots_plan_check: all equal\n");
    return 0;
}
