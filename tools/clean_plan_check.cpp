// clean_plan_check.cpp - the host side of a clean launch (vapor_amd/csrc/vapor_clean_plan.h) held to direct statements of its rules, as
// a program of its own under the address and undefined-behaviour sanitizers (tests/test_clean_plan_cpu.py builds and runs it; no HIP,
// no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc
//       tools/clean_plan_check.cpp -o clean_plan_check && ./clean_plan_check clean_geom.json
// The argument is tests/golden/clean_geom.json.gz, unpacked: what the formulas answered before they moved into the header.
#include "vapor_clean_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

using namespace vapor;
namespace cp = vapor::clean_plan;

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

static const int WANTS[] = {4, 64, 1024, 4096, 8192};

// regions of one allocation, in words: each [lo, hi); they ascend, do not overlap and end inside `words`
struct Region { const char* name; long long lo, hi; };
static bool ordered_inside(const std::vector<Region>& r, long long words)
{
    long long at = 0;
    for (const Region& g : r) {
        if (g.lo < at || g.hi < g.lo) return false;
        at = g.hi;
    }
    return at <= words;
}

static void check_layout()
{
    static_assert(CLEAN_THREADS != 256 || (CLEAN_PER_MAX == 16 && CLEAN_WAVES == 4), "the constants at 256 threads");
    static_assert(CLEAN_RANGE_WORDS_MAX == 4096 && CLEAN_HCAP_MAX == 8192 && CLEAN_BIG_GRID == 1024, "the constants");
    static_assert(CLEAN_LDS_PER_CU == 163840 && CLEAN_STATIC_LDS_ROOM == 512, "the LDS budget");
    long long n = 0, n_big = 0;
    size_t largest = 0, largest_big = 0;
    for (int rw = 1; rw <= CLEAN_RANGE_WORDS_MAX; ++rw) {
        for (int dual = 0; dual < 2; ++dual) {
            std::set<int> hcaps = {0, 4, 8, 16, 64, 252, 1024, 4096, 8188, 8192};
            for (int w : WANTS)
                for (int e = 0; e < 2; ++e) hcaps.insert(cp::geom_for(rw, w, dual != 0, e != 0).hcap);
            for (int hcap : hcaps) {
                const cp::Layout L = cp::staged_layout(rw, hcap, dual != 0);
                const long long words = (long long)(L.staged_bytes() / 4), half = (rw + 1) / 2;
                const long long counters16 = (L.groups_cap + 1) / 2, median = rw * 32 / 100 + 8;
                CHECK(L.staged_bytes() % 4 == 0 && L.range_words_cap == rw && L.hcap == hcap, "rw %d hcap %d", rw, hcap);
                // the 16-bit counters hold one group per staged record (or as many as the value range has) ...
                CHECK(L.groups_cap >= std::min(rw * 32 / 10 + 8, std::max(hcap, 1)), "rw %d hcap %d: %d counters", rw, hcap, L.groups_cap);
                std::vector<Region> r = {{"bitmap", L.bitmap(), L.bitmap() + rw}, {"ranks", L.ranks(), L.ranks() + half}};
                if (dual) {
                    r.push_back({"bitmap2", L.bitmap2(), L.bitmap2() + rw});
                    r.push_back({"ranks2", L.ranks2(), L.ranks2() + half});
                }
                // ... and the median's per-value counters, 32 bit each, lie in the same region
                r.push_back({"counters", L.counters(), L.counters() + std::max(counters16, median)});
                r.push_back({"records", L.records(), L.records() + 2LL * hcap});
                CHECK(ordered_inside(r, words), "rw %d hcap %d dual %d: regions overlap or leave %lld words", rw, hcap, dual, words);
                CHECK(L.bitmap() == 0 && L.records() % 2 == 0, "rw %d hcap %d dual %d: records at word %d", rw, hcap, dual, L.records());
                CHECK(L.staged_bytes() <= CLEAN_LDS_DYNAMIC_MAX && L.staged_bytes() <= 160 * 1024, "rw %d hcap %d dual %d: %zu bytes", rw, hcap, dual, L.staged_bytes());
                largest = std::max(largest, L.staged_bytes());
                ++n;
            }
        }
        const cp::Layout B = cp::big_layout(rw);
        CHECK(B.groups_cap == rw * 32 / 10 + 8 && !B.dual && B.hcap == 0, "rw %d: big layout", rw);
        CHECK(ordered_inside({{"bitmap", B.bitmap(), B.bitmap() + rw}, {"ranks", B.ranks(), B.ranks() + (rw + 1) / 2},
                              {"counters", B.counters(), B.counters() + std::max(B.groups_cap, rw * 32 / 100 + 8)}}, (long long)(B.big_bytes() / 4)),
              "rw %d: big regions", rw);
        CHECK(B.big_bytes() <= CLEAN_LDS_DYNAMIC_MAX, "rw %d: big %zu bytes", rw, B.big_bytes());
        largest_big = std::max(largest_big, B.big_bytes());
        ++n_big;
    }
    CHECK(largest == 131144 && largest_big == 77100, "largest allocations %zu, %zu", largest, largest_big);
    std::printf("layout: %lld staged and %lld streamed layouts, regions ordered, disjoint and inside the allocation\n", n, n_big);
}

static void check_geometry_literals()
{
    struct Row { int len1, len2, rw, want, seq_hcap, seq_cu, dual_hcap, dual_cu; bool dual; size_t bytes; int groups_lds; size_t big; };
    const Row rows[] = {{10000, 20000, 938, 1573, 1572, 7, 1492, 6, false, 21424, 1572, 17728},
                        {15000, 20000, 1094, 2264, 2264, 5, 2264, 4, false, 29280, 2264, 20660},
                        {30000, 40000, 2188, 5480, 5480, 2, 5456, 2, true, 80888, 5456, 41228},
                        {100, 100, 7, 1024, 1024, 8, 1024, 8, true, 8416, 30, 228},
                        {65535, 65535, 4096, 8192, 8192, 1, 8192, 1, true, 131144, 8192, 77100}};
    int n = 0;
    for (const Row& r : rows) {
        CHECK((r.len1 + r.len2 + 2 + 31) / 32 == r.rw, "%d x %d", r.len1, r.len2);
        const cp::Geom s = cp::geom_for(r.rw, r.want, false), d = cp::geom_for(r.rw, r.want, true), g = cp::geom(r.rw, r.want);
        CHECK(s.hcap == r.seq_hcap && s.per_cu == r.seq_cu && !s.dual, "%d x %d sequential: %d, %d", r.len1, r.len2, s.hcap, s.per_cu);
        CHECK(d.hcap == r.dual_hcap && d.per_cu == r.dual_cu && d.dual, "%d x %d dual: %d, %d", r.len1, r.len2, d.hcap, d.per_cu);
        CHECK(g.dual == r.dual && g.hcap == (r.dual ? d : s).hcap && g.per_cu == (r.dual ? d : s).per_cu, "%d x %d chosen", r.len1, r.len2);
        const cp::Layout L = cp::staged_layout(r.rw, g.hcap, g.dual);
        CHECK(L.staged_bytes() == r.bytes && L.groups_cap == r.groups_lds && cp::groups_lds(r.rw, g.hcap) == r.groups_lds, "%d x %d: %zu bytes, %d counters",
              r.len1, r.len2, L.staged_bytes(), L.groups_cap);
        CHECK(cp::big_layout(r.rw).big_bytes() == r.big, "%d x %d: big %zu", r.len1, r.len2, cp::big_layout(r.rw).big_bytes());
        ++n;
    }
    // a measured want at the 10 kb x 20 kb shape: eight workgroups per CU up to 1372 records, seven from 1376
    for (int w = 4; w <= 1600; w += 4) {
        const cp::Geom g = cp::geom(938, w, true);
        CHECK(g.hcap == w && g.per_cu == (w <= 1372 ? 8 : w <= 1600 ? 7 : 0), "rw 938 exact %d: %d per CU", w, g.per_cu);
    }
    {
        const cp::Geom g = cp::geom(4096, cp::LISTS_WANT);
        CHECK(cp::LISTS_WANT == 4096 && !g.dual && g.per_cu == 2 && g.hcap == 4096, "the list route at rw 4096: %d, %d", g.per_cu, g.hcap);
    }
    size_t smallest = ~(size_t)0, smallest_served = ~(size_t)0;
    for (int rw = 1; rw <= CLEAN_RANGE_WORDS_MAX; ++rw)
        for (int w : WANTS)
            for (int e = 0; e < 2; ++e) {
                const cp::Geom g = cp::geom(rw, w, e != 0);
                CHECK(g.per_cu >= 1 && g.per_cu <= 8 && g.hcap >= 0 && g.hcap % 4 == 0 && g.hcap <= std::min(w, 8192), "rw %d want %d: %d, %d", rw, w, g.hcap, g.per_cu);
                if ((w == 1024 || w == 8192) && !e) CHECK(g.hcap > 0, "rw %d estimated want %d stages nothing", rw, w);
                const cp::Layout L = cp::staged_layout(rw, g.hcap, g.dual);
                smallest = std::min(smallest, cp::launch_bytes(L, false));
                smallest_served = std::min(smallest_served, cp::launch_bytes(L, true));
                CHECK(cp::launch_bytes(L, false) == L.staged_bytes() && cp::launch_bytes(L, true) == std::max<size_t>(L.staged_bytes(), 640), "rw %d want %d: floor", rw, w);
                // the floor costs no residency: eight workgroups of it are far below a CU's LDS
                CHECK(cp::launch_bytes(L, true) == L.staged_bytes() || (640 + 512) * 8 <= 160 * 1024, "floor and residency");
            }
    CHECK(cp::staged_layout(7, 4, true).staged_bytes() == 232, "rw 7, hcap 4, dual: %zu", cp::staged_layout(7, 4, true).staged_bytes());
    CHECK(smallest == 152 && smallest_served == 640 && REMAP_SCRATCH_BYTES == 640, "smallest %zu, served %zu", smallest, smallest_served);
    // what remap_for_target addresses: 3 counters, REMAP_MAX_IV + 2 boundaries, 2 * REMAP_MAX_IV op words
    CHECK(REMAP_BOUNDS_WORD == 4 && REMAP_OPS_WORD == 64 && REMAP_MAX_IV == 48, "the scratch words");
    CHECK(3 <= REMAP_BOUNDS_WORD && REMAP_BOUNDS_WORD + REMAP_MAX_IV + 2 <= REMAP_OPS_WORD && (size_t)(REMAP_OPS_WORD + 2 * REMAP_MAX_IV) * 4 <= REMAP_SCRATCH_BYTES,
          "the scratch regions");
    std::printf("geometry: %d shapes, the measured edge and the smallest allocation equal their literals\n", n);
}

// every integer of the file behind "rows", eight a row: rw, want, exact -> hcap, per_cu, dual, bytes, groups_lds
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
    CHECK(v.size() % 8 == 0 && v.size() >= 8 * 2000, "%zu numbers", v.size());
    size_t n = 0;
    for (size_t t = 0; t + 8 <= v.size(); t += 8, ++n) {
        const int rw = (int)v[t], want = (int)v[t + 1];
        const bool exact = v[t + 2] != 0;
        const cp::Geom g = cp::geom(rw, want, exact);
        const cp::Layout L = cp::staged_layout(rw, g.hcap, g.dual);
        CHECK(g.hcap == v[t + 3] && g.per_cu == v[t + 4] && (g.dual ? 1 : 0) == v[t + 5] && (long long)L.staged_bytes() == v[t + 6] && L.groups_cap == v[t + 7],
              "rw %d want %d exact %d: %d, %d, %d, %zu, %d", rw, want, (int)exact, g.hcap, g.per_cu, (int)g.dual, L.staged_bytes(), L.groups_cap);
    }
    std::printf("fixture: %zu points equal what the formulas answered before\n", n);
}

static void check_width_rounds_slots()
{
    static_assert(CLEAN_N_WIDTHS == 3 && CLEAN_WIDTHS[0] == 4 && CLEAN_WIDTHS[1] == 8 && CLEAN_WIDTHS[2] == CLEAN_PER_MAX, "the compiled widths");
    int n = 0;
    for (int rw = 1; rw <= CLEAN_RANGE_WORDS_MAX; ++rw, ++n) {
        const int w = cp::width(rw);
        CHECK(w * CLEAN_THREADS >= rw, "rw %d: width %d does not cover it", rw, w);
        if (CLEAN_THREADS == 256) CHECK(w == (rw <= 1024 ? 4 : rw <= 2048 ? 8 : 16), "rw %d: width %d", rw, w);
    }
    std::printf("width: %d value ranges\n", n);

    n = 0;
    for (int per_cu = 1; per_cu <= 8; ++per_cu)
        for (int n_cus : {1, 8, 256}) {
            const int64_t edge = 4LL * per_cu * n_cus;
            for (int64_t n_pairs : {(int64_t)1, edge - 1, edge, edge + 1, 100 * edge}) {
                for (int param = 0; param <= 2; ++param, ++n) {
                    CHECK(!cp::remap_in_clean(param, 0, n_pairs, per_cu, n_cus), "no served plot, parameter %d", param);
                    const bool want = param == 2 || (param == 1 && n_pairs <= edge);
                    CHECK(cp::remap_in_clean(param, 3, n_pairs, per_cu, n_cus) == want, "parameter %d, %lld pairs, %d x %d", param, (long long)n_pairs, per_cu, n_cus);
                }
            }
        }
    std::printf("rounds: %d cases\n", n);

    std::mt19937 rng(11);
    n = 0;
    for (int t = 0; t < 2000; ++t, ++n) {
        const size_t n_pairs = rng() % 40, n_plots = rng() % 6;
        std::vector<DPair> hp(n_pairs + n_plots);
        for (DPair& d : hp) d.cap = (rng() % 4 == 0) ? 0u : (uint32_t)(rng() % 5000);
        std::vector<DServe> serve(n_plots ? n_pairs : 0);
        for (DServe& sv : serve) {
            sv.dpair = (rng() % 2) ? (int32_t)(n_pairs + rng() % n_plots) : -1;
            sv.hit_off = -7; sv.cap = 77777u;
        }
        const int64_t tot = cp::lay_slots(hp, serve);
        int64_t at = 0;
        for (const DPair& d : hp) {
            CHECK(d.hit_off == at && d.hit_off % 4 == 0, "slot at %lld, expected %lld", (long long)d.hit_off, (long long)at);
            at += (d.cap + 3) / 4 * 4;
        }
        CHECK(tot == at + 4, "total %lld behind %lld", (long long)tot, (long long)at);
        for (const DServe& sv : serve) {
            if (sv.dpair >= 0) CHECK(sv.hit_off == hp[(size_t)sv.dpair].hit_off && sv.cap == hp[(size_t)sv.dpair].cap, "a served pair's view");
            else CHECK(sv.hit_off == -7 && sv.cap == 77777u, "an unserved pair's record was touched");
        }
    }
    std::printf("slots: %d cases\n", n);
}

static void check_post_run()
{
    std::mt19937 rng(23);
    int n = 0;
    long long grown = 0, refused = 0;
    for (int t = 0; t < 2000; ++t, ++n) {
        const int64_t n_pairs = 1 + rng() % 30, max_pair_cap = 1000 + rng() % 3000;
        const size_t n_plots = rng() % 5;
        std::vector<DPair> hp((size_t)n_pairs + n_plots);
        for (DPair& d : hp) d.cap = (uint32_t)(rng() % 3000);
        std::vector<long long> stats((size_t)n_pairs * 16);
        for (auto& s : stats) s = (long long)(rng() % 100);
        for (int64_t i = 0; i < n_pairs; ++i) {
            stats[(size_t)i * 16 + 14] = (long long)(rng() % 5000);
            stats[(size_t)i * 16 + 15] = (rng() % 3 == 0) ? 0 : (rng() % 5 == 0) ? VAPOR_E_ARG : VAPOR_E_OVERFLOW;
        }
        std::vector<unsigned long long> plots(n_plots);
        for (auto& c : plots) c = (unsigned long long)(rng() % 5000) | ((unsigned long long)rng() << 32);
        const std::vector<DPair> before = hp;
        const std::vector<long long> stats0 = stats;
        const int64_t grow = cp::grow_slots(stats.data(), n_pairs, plots, max_pair_cap, hp);
        int64_t expect = 0;
        for (size_t i = 0; i < hp.size(); ++i) {
            const bool pair = i < (size_t)n_pairs;
            const long long need = pair ? stats0[i * 16 + 14] : (long long)(plots[i - (size_t)n_pairs] & 0xFFFFFFFFull);
            const bool grows = (!pair || stats0[i * 16 + 15] == -2) && need <= max_pair_cap && need > (long long)before[i].cap;
            CHECK(hp[i].cap == (grows ? (uint32_t)need : before[i].cap), "slot %zu: cap %u", i, hp[i].cap);
            expect += grows;
        }
        CHECK(grow == expect && stats == stats0, "%lld slots grown, expected %lld", (long long)grow, (long long)expect);
        grown += grow;

        // the measured want
        std::vector<int32_t> status((size_t)n_pairs);
        for (auto& s : status) s = (rng() % 4 == 0) ? (int32_t)VAPOR_E_ARG : 0;
        std::vector<unsigned long long> counts((size_t)n_pairs);
        const uint32_t top = (t % 3 == 0) ? 12u : (t % 3 == 1) ? 3000u : 12000u;
        for (auto& c : counts) c = (unsigned long long)(rng() % top) | ((unsigned long long)(rng() % 4 == 0 ? 65536u + rng() % 1000 : rng() % 65536u) << 32);
        uint32_t most = 0;
        for (int64_t i = 0; i < n_pairs; ++i) {
            const uint32_t recs = (uint32_t)(counts[(size_t)i] & 0xFFFFFFFFull), dots = (uint32_t)(counts[(size_t)i] >> 32);
            if (status[(size_t)i] == 0 && dots <= 65535u && recs > most) most = recs;
        }
        const int want = cp::measured_want(counts, status);
        CHECK(want == (most == 0 || most > 8192 ? 0 : (int)((most + 3) / 4 * 4)), "measured want %d of at most %u records", want, most);

        // the targets of a truncated plot, then the statistics of the refused
        std::vector<DShare> shares(n_plots);
        for (DShare& sh : shares)
            for (int32_t& tg : sh.target) tg = (rng() % 3 == 0) ? -1 : (int32_t)(rng() % n_pairs);
        const std::vector<int32_t> status0 = status;
        cp::refuse_truncated_plots(plots, hp, n_pairs, shares, status);
        for (int64_t i = 0; i < n_pairs; ++i) {
            bool hit = false;
            for (size_t p = 0; p < n_plots; ++p)
                for (int32_t tg : shares[p].target)
                    if (tg == i && (plots[p] & 0xFFFFFFFFull) > hp[(size_t)n_pairs + p].cap) hit = true;
            CHECK(status[(size_t)i] == (status0[(size_t)i] != 0 ? status0[(size_t)i] : hit ? -2 : 0), "pair %lld: status %d", (long long)i, status[(size_t)i]);
        }
        cp::mask_refused(stats.data(), status, n_pairs);
        for (int64_t i = 0; i < n_pairs; ++i)
            for (int w = 0; w < 16; ++w) {
                const long long s = stats[(size_t)i * 16 + w];
                if (status[(size_t)i] == 0) CHECK(s == stats0[(size_t)i * 16 + w], "a scored pair's statistics changed");
                else CHECK(s == (w == 1 || w == 2 ? -1 : w == 15 ? status[(size_t)i] : 0), "refused pair %lld word %d: %lld", (long long)i, w, s);
            }
        for (int32_t s : status) refused += s != 0;
    }
    CHECK(VAPOR_E_OVERFLOW == -2, "the overflow code");
    CHECK(grown > 1000 && refused > 1000, "%lld slots grown, %lld pairs refused: the cases say too little", grown, refused);
    std::printf("post-run: %d cases\n", n);
}

static void check_lists()
{
    // the refusals of each entry, in their order (the narrow entry: list_cap < 0, no statement about the offsets)
    auto says = [](const cp::Refusal& r, const char* msg) { return msg ? r.code == VAPOR_E_ARG && r.msg && !std::strcmp(r.msg, msg) : (r.code == 0 && !r); };
    const int64_t off[] = {0, 2, 3}, stats[48] = {0};
    const int32_t ji[] = {1, 2, 3, 4, 65535, 0};
    int n = 0;
    for (const int64_t cap : {(int64_t)-1, (int64_t)2}) {
        const int top = cap < 0 ? 65535 : 2097151;
        CHECK(says(cp::lists_check(false, 2, ji, off, stats, top, cap), "null argument"), "no context");
        CHECK(says(cp::lists_check(true, -1, ji, off, stats, top, cap), "null argument"), "a negative count");
        CHECK(says(cp::lists_check(true, 2, ji, nullptr, stats, top, cap), "null argument"), "no offsets");
        CHECK(says(cp::lists_check(true, 2, ji, off, nullptr, top, cap), "null argument"), "no statistics");
        CHECK(says(cp::lists_check(true, 0, nullptr, nullptr, nullptr, top, cap), nullptr), "no lists");
        CHECK(says(cp::lists_check(true, 2, nullptr, off, stats, top, cap), "null hit list"), "no dots");       // (before any coordinate is read)
        CHECK(says(cp::lists_check(true, 2, ji, off, stats, top, cap), nullptr), "two good lists");
        CHECK(says(cp::lists_check(true, 2, ji, off, stats, 65534, cap), "coordinate out of range"), "a coordinate above the route's");
        const int32_t neg[] = {1, 2, 3, -4, 5, 6};
        CHECK(says(cp::lists_check(true, 2, neg, off, stats, top, cap), "coordinate out of range"), "a negative coordinate");
        const int64_t longer[] = {0, 3, 3}, back[] = {0, 2, 1};
        CHECK(says(cp::lists_check(true, 2, ji, longer, stats, top, cap), cap < 0 ? nullptr : "bad list offsets"), "a list above the cap");
        // (offsets that decrease: the narrow entry reads no dot of such a list and refuses nothing; the wide one refuses before it reads)
        CHECK(says(cp::lists_check(true, 2, ji, back, stats, top, cap), cap < 0 ? nullptr : "bad list offsets"), "offsets that decrease");
        const int32_t bad_first[] = {-1, 0, 1, 1, 2, 2};
        CHECK(says(cp::lists_check(true, 2, bad_first, longer, stats, top, cap), cap < 0 ? "coordinate out of range" : "bad list offsets"), "the offsets come first");
        n += 12;
    }
    std::printf("refusals: %d calls\n", n);

    std::mt19937 rng(31);
    int n_cases = 0;
    for (int t = 0; t < 600; ++t, ++n_cases) {
        const int64_t n_lists = 1 + rng() % 6;
        const int top = t % 5 == 0 ? 65536 : 1 + (int)(rng() % 3000);
        std::vector<int64_t> o((size_t)n_lists + 1, 0);
        for (int64_t l = 0; l < n_lists; ++l) o[(size_t)l + 1] = o[(size_t)l] + (rng() % 4 == 0 ? 0 : rng() % 23);
        std::vector<int32_t> h((size_t)o[(size_t)n_lists] * 2 + 2);
        for (auto& x : h) x = (int32_t)(rng() % top);
        std::vector<uint32_t> fl((size_t)n_lists);
        for (auto& x : fl) x = rng() % 8;
        const bool with_flags = t % 2 == 0;
        const cp::ListPack L(n_lists, h.data(), o.data(), with_flags ? fl.data() : nullptr);
        CHECK(L.poff.size() == (size_t)n_lists + 1 && L.dp.size() == (size_t)n_lists && L.counts.size() == (size_t)n_lists, "sizes");
        CHECK(L.packed.size() == (size_t)std::max<int64_t>(L.poff[(size_t)n_lists], 4), "%zu records", L.packed.size());
        int most = 0;
        int64_t at = 0;
        std::vector<bool> written(L.packed.size(), false);
        for (int64_t l = 0; l < n_lists; ++l) {
            const int64_t len = o[(size_t)l + 1] - o[(size_t)l];
            CHECK(L.poff[(size_t)l] == at && at % 4 == 0, "list %lld at %lld", (long long)l, (long long)L.poff[(size_t)l]);
            int mi = 0, mj = 0;
            for (int64_t q = 0; q < len; ++q) {
                const int j = h[(size_t)(2 * (o[(size_t)l] + q))], i = h[(size_t)(2 * (o[(size_t)l] + q) + 1)];
                const unsigned long long r = L.packed[(size_t)(at + q)];
                written[(size_t)(at + q)] = true;
                CHECK((r & 0xFFFFu) == (unsigned)i && ((r >> 16) & 0xFFFFu) == (unsigned)j && (r >> 32) == 1ull, "record %llx of dot (%d, %d)", r, j, i);
                mi = std::max(mi, i); mj = std::max(mj, j);
            }
            const DPair& d = L.dp[(size_t)l];
            CHECK(d.seq1 == 2 * l && d.seq2 == 2 * l + 1 && d.off2 == 0 && d.k == 10 && d.len1 == mi + 1 && d.len2 == mj + 1, "list %lld: pair record", (long long)l);
            CHECK(d.flags == (with_flags ? fl[(size_t)l] : 3u) && d.cap == (uint32_t)len && d.hit_off == at, "list %lld: flags, cap, slot", (long long)l);
            CHECK(L.counts[(size_t)l] == ((unsigned long long)len << 32 | (unsigned long long)len), "list %lld: count %llx", (long long)l, L.counts[(size_t)l]);
            // the kernel's own value range of the pair, (len1 + len2 + 2 + 31) / 32, never exceeds the launch's
            CHECK(std::min((d.len1 + d.len2 + 2 + 31) / 32, 4096) <= L.rw, "list %lld: value range", (long long)l);
            most = std::max(most, mi + mj);
            at += (len + 3) / 4 * 4;
        }
        for (size_t q = 0; q < L.packed.size(); ++q)
            if (!written[q]) CHECK(L.packed[q] == 0ull, "padding record %zu", q);
        CHECK(L.rw == std::max(1, std::min((most + 4 + 31) / 32, 4096)), "rw %d of the largest i + j %d", L.rw, most);
    }
    {
        const int64_t o[] = {0, 1};
        const int32_t far[] = {65535, 65535};
        CHECK(cp::ListPack(1, far, o, nullptr).rw == 4096, "the clamp");
    }
    std::printf("lists: %d cases\n", n_cases);
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::printf("usage: clean_plan_check clean_geom.json\n"); return 2; }
    check_layout();
    check_geometry_literals();
    check_fixture(argv[1]);
    check_width_rounds_slots();
    check_post_run();
    check_lists();
    if (g_bad) { std::printf("clean_plan_check: %d statements FAILED\n", g_bad); return 1; }
    std::printf("clean_plan_check: all equal\n");
    return 0;
}
