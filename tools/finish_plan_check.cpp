// finish_plan_check.cpp - the host side of the finishing and grid calls (vapor_amd/csrc/vapor_finish_plan.h) held to direct
// statements of its rules, as a program of its own under the address and undefined-behaviour sanitizers
// (tests/test_finish_plan_cpu.py builds and runs it; no HIP, no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc
//       tools/finish_plan_check.cpp -o finish_plan_check && ./finish_plan_check finish_plan.json
// The argument is tests/golden/finish_plan.json.gz, unpacked: what the checks and sizes answered before they moved into the header
// (tools/finish_plan_fixture.cpp).
#include "vapor_finish_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

namespace fp = vapor::finish_plan;

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

static bool says(const fp::Refusal& no, const char* msg)
{
    if (!msg) return !no && no.code == 0;
    return no.code == VAPOR_E_ARG && no.msg && !strcmp(no.msg, msg);
}

// ------------------------------------------------------------------------------------------
// the read table's refusals, in the order include/vapor_hip.h's callers have had them
// ------------------------------------------------------------------------------------------
static const char* const READ_MSG[3] = {"reads must be sorted by locus", "read refers to a pair outside the plan", "unknown scorer kind"};
constexpr int64_t N_PAIRS = 10, N_LOCI = 5;

// read `r` of a table of six over five loci, breaking the rules of `mask` (bit 0 locus, 1 pair index, 2 kind)
static std::vector<vapor_read> table(int r, unsigned mask, int variant)
{
    std::vector<vapor_read> t;
    for (int i = 0; i < 6; ++i) t.push_back(vapor_read{i, 9 - i, (i + 3) % 10, (i + 5) % 10, i % 4, i < 2 ? 0 : i - 1, 100 + i, 200 + i});
    vapor_read& x = t[(size_t)r];
    if (mask & 4u) x.kind = variant % 2 ? 4 : -1;
    if (mask & 2u) {
        int32_t* field[4] = {&x.ref_a, &x.alt_a, &x.ref_b, &x.alt_b};
        if (variant % 4 >= 2 && !(mask & 4u)) x.kind = 0;                  // (the second scorer's pairs are a deletion read's)
        *field[x.kind == 0 ? variant % 4 : variant % 2] = variant / 4 % 2 ? -1 : (int32_t)N_PAIRS;
    }
    if (mask & 1u) x.locus = variant % 2 ? (int32_t)N_LOCI : (r ? t[(size_t)r - 1].locus - 1 : -2);
    return t;
}
static fp::Refusal refuse(const std::vector<vapor_read>& t, int64_t n_loci = N_LOCI)
{
    std::vector<int32_t> first;
    std::vector<uint8_t> image;
    fp::ReadImage im;
    return fp::read_table((int64_t)t.size(), t.data(), n_loci, N_PAIRS, first, im, image);
}
static void check_read_refusals()
{
    int n = 0;
    CHECK(says(refuse(table(0, 0, 0)), nullptr), "a good table");
    for (int r = 0; r < 6; ++r)
        for (unsigned mask = 1; mask < 8; ++mask)
            for (int variant = 0; variant < 8; ++variant, ++n) {
                int want = 0;
                while (!(mask >> want & 1u)) ++want;
                const std::vector<vapor_read> t = table(r, mask, variant);
                const vapor_read& x = t[(size_t)r];
                // each rule of the mask is broken in words ...
                if (mask & 1u) CHECK(x.locus >= N_LOCI || x.locus < (r ? t[(size_t)r - 1].locus : -1), "read %d: locus %d", r, x.locus);
                if (mask & 2u) CHECK(x.ref_a < 0 || x.ref_a >= N_PAIRS || x.alt_a < 0 || x.alt_a >= N_PAIRS ||
                                         (x.kind == 0 && (x.ref_b < 0 || x.ref_b >= N_PAIRS || x.alt_b < 0 || x.alt_b >= N_PAIRS)), "read %d: pairs", r);
                if (mask & 4u) CHECK(x.kind < 0 || x.kind > 3, "read %d: kind %d", r, x.kind);
                // ... and the first in the written order is the one reported, by the read's check and by the table's
                CHECK(says(fp::read_refusal(x, r ? t[(size_t)r - 1].locus : -1, N_LOCI, N_PAIRS), READ_MSG[want]), "read %d, mask %u, variant %d", r, mask, variant);
                CHECK(says(refuse(t), READ_MSG[want]), "table with read %d, mask %u, variant %d", r, mask, variant);
            }
    // the first read refused decides, whatever a later one breaks
    for (unsigned early = 1; early < 8; early <<= 1)
        for (unsigned late = 1; late < 8; late <<= 1, ++n) {
            std::vector<vapor_read> t = table(1, early, 1);
            const std::vector<vapor_read> u = table(4, late, 1);
            t[4] = u[4];
            int want = 0;
            while (!(early >> want & 1u)) ++want;
            CHECK(says(refuse(t), READ_MSG[want]), "reads 1 (%u) and 4 (%u)", early, late);
        }
    // pair indices a read does not use are not read: ref_b / alt_b of kinds 1 .. 3
    std::vector<vapor_read> t = table(0, 0, 0);
    for (vapor_read& x : t)
        if (x.kind != 0) { x.ref_b = -7; x.alt_b = 1 << 30; }
    CHECK(says(refuse(t), nullptr), "unused pair indices");
    // the last pair and the last locus are inside, one more is not
    t = table(0, 0, 0);
    t[5].ref_a = (int32_t)N_PAIRS - 1; t[5].locus = (int32_t)N_LOCI - 1;
    CHECK(says(refuse(t), nullptr) && says(refuse(t, N_LOCI - 1), READ_MSG[0]), "the last pair and locus");
    std::printf("read refusals: %d tables, the first rule in order and the first read win\n", n);
}

// ------------------------------------------------------------------------------------------
// the grid's refusals
// ------------------------------------------------------------------------------------------
static const char* const GRID_MSG[5] = {"grid: the groups must cover the loci", "grid: a group holds 1 .. VAPOR_MAX_CANDIDATES consecutive loci",
                                        "grid: read ranges must not decrease", "grid: the candidates of a group score the same reads", "grid: too many reads"};
enum : unsigned { COVER = 1, SIZE = 2, DECREASE = 4, UNEQUAL = 8, TOO_MANY = 16 };
struct Grid {
    std::vector<int32_t> fl, lf;
    int64_t n_groups() const { return (int64_t)fl.size() - 1; }
    int64_t n_loci() const { return (int64_t)lf.size() - 1; }
    fp::Refusal check(std::vector<int32_t>& off) const { return fp::grid_check(n_groups(), fl.data(), n_loci(), lf.data(), off); }
};
// Three groups of 1, 3 and 2 candidates with 4, 10 and 1 reads; the rules of `mask` broken in the middle one.  SIZE: 129
// candidates; DECREASE: -2 reads a candidate; UNEQUAL: its last candidate has one read more; TOO_MANY: the group in front leaves
// `slack` slots below 2^31 (its range starts below zero: the check reads differences); COVER: a locus behind the last group.
static Grid grid(unsigned mask, int n_mid = 3, int32_t slack = 5)
{
    Grid g;
    const int sizes[3] = {1, mask & SIZE ? 129 : n_mid, 2};
    const int32_t counts[3] = {mask & TOO_MANY ? INT32_MAX - slack : 4, mask & DECREASE ? -2 : 10, 1};
    g.fl.push_back(0);
    g.lf.push_back(mask & TOO_MANY ? -(1 << 30) : 0);
    for (int q = 0; q < 3; ++q) {
        for (int c = 0; c < sizes[q]; ++c) g.lf.push_back(g.lf.back() + counts[q] + (q == 1 && c == sizes[q] - 1 && (mask & UNEQUAL) ? 1 : 0));
        g.fl.push_back(g.fl.back() + sizes[q]);
    }
    if (mask & COVER) g.lf.push_back(g.lf.back() + 1);
    return g;
}
static void check_grid_refusals()
{
    int n = 0;
    std::vector<int32_t> off;
    CHECK(says(grid(0).check(off), nullptr) && off == std::vector<int32_t>({0, 4, 14, 15}), "a good grid");
    for (unsigned mask = 1; mask < 32; ++mask) {
        if ((mask & DECREASE) && (mask & TOO_MANY)) continue;          // (a range that decreases holds no reads to be too many)
        int want = 0;
        while (!(mask >> want & 1u)) ++want;
        CHECK(says(grid(mask).check(off), GRID_MSG[want]), "mask %u", mask);
        ++n;
    }
    // an earlier group's refusal comes before a later group's, whatever their places in the order: too many reads in the middle
    // group, then a last group of 129
    Grid g = grid(TOO_MANY);
    for (int c = 0; c < 127; ++c) g.lf.push_back(g.lf.back() + 1);
    g.fl.back() += 127;
    CHECK(says(g.check(off), GRID_MSG[4]), "too many reads, then a group of 129");
    g = grid(0);
    for (int c = 0; c < 127; ++c) g.lf.push_back(g.lf.back() + 1);
    g.fl.back() += 127;
    CHECK(says(g.check(off), GRID_MSG[1]), "a last group of 129");
    // the cover: where the groups start and where they end
    g = grid(0); g.fl[0] = 1;
    CHECK(says(g.check(off), GRID_MSG[0]), "groups from locus 1");
    g = grid(0); g.lf.pop_back();
    CHECK(says(g.check(off), GRID_MSG[0]), "groups beyond the loci");
    // a group's bounds: backwards, empty, below zero, beyond the loci
    g = grid(0); g.fl[2] = 0;
    CHECK(says(g.check(off), GRID_MSG[1]), "a group running backwards");
    g = grid(0); g.fl[2] = g.fl[1];
    CHECK(says(g.check(off), GRID_MSG[1]), "an empty group");
    g = grid(0); g.fl[1] = -1;
    CHECK(says(g.check(off), GRID_MSG[1]), "a group below zero");
    g = grid(0); g.fl[1] = 50;
    CHECK(says(g.check(off), GRID_MSG[1]), "a group beyond the loci");
    n += 8;

    // vapor_grid_pick: its range checks come first, then the grid's
    g = grid(0);
    CHECK(says(fp::pick_check(g.n_groups(), g.fl.data(), g.lf.data(), off), nullptr) && off == std::vector<int32_t>({0, 4, 14, 15}), "pick: a good grid");
    g = grid(SIZE); g.lf[0] = 1;
    CHECK(says(fp::pick_check(g.n_groups(), g.fl.data(), g.lf.data(), off), "vapor_grid_pick: bad ranges"), "pick: ranges from 1");
    g = grid(SIZE); g.fl.back() = -1;
    CHECK(says(fp::pick_check(g.n_groups(), g.fl.data(), g.lf.data(), off), "vapor_grid_pick: bad ranges"), "pick: loci below zero");
    g = grid(SIZE | UNEQUAL); g.lf[g.lf.size() - 2] += 5;              // (the last group's first candidate: its second has -4 reads)
    CHECK(says(fp::pick_check(g.n_groups(), g.fl.data(), g.lf.data(), off), "vapor_grid_pick: read ranges must not decrease"), "pick: a decreasing range");
    g = grid(DECREASE);
    CHECK(says(fp::pick_check(g.n_groups(), g.fl.data(), g.lf.data(), off), "vapor_grid_pick: read ranges must not decrease"), "pick: its message for a decreasing range");
    g = grid(SIZE | UNEQUAL);
    CHECK(says(fp::pick_check(g.n_groups(), g.fl.data(), g.lf.data(), off), GRID_MSG[1]), "pick: then the grid's order");
    const double x = 0;
    CHECK(says(fp::pick_scores_check(0, nullptr), nullptr) && says(fp::pick_scores_check(3, &x), nullptr) &&
              says(fp::pick_scores_check(3, nullptr), "vapor_grid_pick: null argument"), "pick: reads without scores");
    n += 7;
    std::printf("grid refusals: %d grids, the first rule in order and the first group win\n", n);
}

// ------------------------------------------------------------------------------------------
// edges
// ------------------------------------------------------------------------------------------
static void check_edges()
{
    std::vector<int32_t> off;
    CHECK(VAPOR_MAX_CANDIDATES == 128, "the candidate bound");
    CHECK(says(grid(0, 1).check(off), nullptr) && off == std::vector<int32_t>({0, 4, 14, 15}), "a group of one candidate");
    CHECK(says(grid(0, 128).check(off), nullptr) && off == std::vector<int32_t>({0, 4, 14, 15}), "a group of 128");
    CHECK(says(grid(0, 129).check(off), GRID_MSG[1]), "a group of 129");
    Grid g = grid(0); g.fl[2] = g.fl[1];
    CHECK(says(g.check(off), GRID_MSG[1]), "a group of none");
    // read counts that differ by one, at the group's second and at its last candidate, up and down
    for (int at = 2; at <= 3; ++at)
        for (int by = -1; by <= 1; by += 2) {
            g = grid(0);
            for (size_t l = (size_t)at + 1; l < g.lf.size(); ++l) g.lf[l] += by;          // candidate `at` of the loci: 10 + by reads
            CHECK(says(g.check(off), GRID_MSG[3]), "candidate %d has %d reads", at, 10 + by);
        }
    // the winners' slots: INT32_MAX is a slot count, one more is not
    CHECK(says(grid(TOO_MANY, 3, 11).check(off), nullptr) && off == std::vector<int32_t>({0, INT32_MAX - 11, INT32_MAX - 1, INT32_MAX}), "slots up to INT32_MAX");
    CHECK(says(grid(TOO_MANY, 3, 10).check(off), GRID_MSG[4]), "one slot past INT32_MAX");         // (in the last group)
    CHECK(fp::GridImage(3, INT32_MAX, 0).winner_bytes == 8 * (size_t)INT32_MAX, "their bytes");
    // nothing at all
    const int32_t zero = 0, one = 1;
    CHECK(says(fp::grid_check(0, &zero, 0, &zero, off), nullptr) && off == std::vector<int32_t>({0}), "no groups over no loci");
    CHECK(says(fp::grid_check(0, &zero, 1, &zero, off), GRID_MSG[0]), "no groups over a locus");
    CHECK(says(fp::pick_check(0, &zero, &zero, off), nullptr) && says(fp::pick_check(0, &zero, &one, off), "vapor_grid_pick: bad ranges"), "pick: no groups");
    g = grid(0);
    for (int32_t& l : g.lf) l = 0;
    CHECK(says(g.check(off), nullptr) && off == std::vector<int32_t>({0, 0, 0, 0}) && fp::GridImage(3, off.back(), 0).winner_bytes == 8, "groups without reads");
    std::vector<int32_t> first;
    std::vector<uint8_t> image;
    fp::ReadImage im;
    CHECK(says(fp::read_table(0, nullptr, 0, N_PAIRS, first, im, image), nullptr) && first == std::vector<int32_t>({0}) && im.bytes == 40 && image == std::vector<uint8_t>(40, 0) &&
              im.score_bytes == 8 && im.loci_bytes == 64, "no reads, no loci");
    CHECK(says(fp::read_table(0, nullptr, 3, N_PAIRS, first, im, image), nullptr) && first == std::vector<int32_t>({0, 0, 0, 0}) && im.bytes == 48 && im.loci_bytes == 192, "no reads, three loci");
    const vapor_read r{0, 0, 0, 0, 1, 0, 1, 1};
    CHECK(says(fp::read_table(1, &r, 0, N_PAIRS, first, im, image), READ_MSG[0]), "a read, no loci");
    CHECK(says(fp::read_table(1, &r, 1, 0, first, im, image), READ_MSG[1]), "a read, no pairs");
    CHECK(says(fp::read_table(1, &r, 1, 1, first, im, image), nullptr) && first == std::vector<int32_t>({0, 1}) && im.bytes == 40 && im.score_bytes == 8 && im.loci_bytes == 64, "one read");
    std::printf("edges: 1 and 128 candidates, 0 and 129, counts off by one, INT32_MAX slots and one more, nothing at all\n");
}

// ------------------------------------------------------------------------------------------
// the images
// ------------------------------------------------------------------------------------------
struct Span { size_t off, bytes; };
static bool tiles(const std::vector<Span>& s, size_t total)
{
    size_t at = 0;
    for (const Span& x : s) {
        if (x.off % 8 || x.off < at || x.off - at >= 8 || x.off + x.bytes > total) return false;      // on 8 bytes, behind the one before, no gap of 8
        at = x.off + x.bytes;
    }
    return total >= at && total - at < 8;
}
static void check_images()
{
    static_assert(sizeof(vapor_read) == 32 && fp::LOCUS_DOUBLES == 8 && fp::GROUP_DOUBLES == 16 && fp::GT_ENTRIES == 8450 && fp::STATS_WORDS == 16, "the widths");
    int n = 0;
    for (size_t ng = 0; ng <= 65; ++ng)
        for (size_t nl = 0; nl <= 200; ++nl, ++n) {
            const fp::GridImage a(ng, (int32_t)(nl % 7), 0), b(ng, (int32_t)(nl % 7), nl + 1);
            bool ok = tiles({{a.first_locus.off, a.first_locus.bytes()}, {a.score_off.off, a.score_off.bytes()}, {a.winner_idx.off, a.winner_idx.bytes()}}, a.bytes);
            ok = ok && tiles({{b.first_locus.off, b.first_locus.bytes()}, {b.score_off.off, b.score_off.bytes()}, {b.winner_idx.off, b.winner_idx.bytes()}, {b.read_first.off, b.read_first.bytes()}}, b.bytes);
            ok = ok && a.first_locus.n == ng + 1 && a.score_off.n == ng + 1 && a.winner_idx.n == ng && a.read_first.n == 0 && b.read_first.n == nl + 1 && b.read_first.off == a.bytes;
            ok = ok && a.group_bytes == 128 * ng && a.winner_bytes == 8 * std::max<size_t>(nl % 7, 1) && b.group_bytes == a.group_bytes;
            // the stated difference to the packed block: four bytes behind every table of odd length
            ok = ok && a.bytes == 4 * (3 * ng + 2) + (ng % 2 ? 4 : 8) && b.bytes == a.bytes + 4 * (nl + 1) + (nl % 2 ? 0 : 4);
            const fp::ReadImage r((int64_t)(ng % 9), (int64_t)nl);
            const size_t nr = std::max<size_t>(ng % 9, 1);
            ok = ok && tiles({{r.reads.off, r.reads.bytes()}, {r.locus_first.off, r.locus_first.bytes()}}, r.bytes) && r.reads.n == nr && r.locus_first.n == nl + 1;
            ok = ok && r.locus_first.off == 32 * nr && r.bytes == 32 * nr + 4 * (nl + 1) + (nl % 2 ? 0 : 4) && r.score_bytes == 8 * nr && r.loci_bytes == 64 * std::max<size_t>(nl, 1);
            if (!ok) CHECK(false, "%zu groups, %zu loci", ng, nl);
        }
    // the filled images: the caller's tables at their places, zeros elsewhere; locus_first counts the reads in front of a locus
    std::mt19937_64 rng(7);
    int n_filled = 0;
    for (int t = 0; t < 300; ++t, ++n_filled) {
        const int64_t n_loci = 1 + (int64_t)(rng() % 40), n_reads = (int64_t)(rng() % 60);
        std::vector<vapor_read> rd;
        for (int64_t r = 0; r < n_reads; ++r)
            rd.push_back(vapor_read{(int32_t)(rng() % N_PAIRS), (int32_t)(rng() % N_PAIRS), (int32_t)(rng() % N_PAIRS), (int32_t)(rng() % N_PAIRS), (int32_t)(rng() % 4), 0, 1, 1});
        for (vapor_read& x : rd) x.locus = (int32_t)(rng() % (uint64_t)n_loci);
        std::sort(rd.begin(), rd.end(), [](const vapor_read& p, const vapor_read& q) { return p.locus < q.locus; });
        std::vector<int32_t> first;
        std::vector<uint8_t> image;
        fp::ReadImage im;
        CHECK(says(fp::read_table(n_reads, rd.data(), n_loci, N_PAIRS, first, im, image), nullptr) && image.size() == im.bytes && (int64_t)first.size() == n_loci + 1, "table %d", t);
        bool ok = true;
        for (int64_t l = 0; l <= n_loci; ++l) {
            int32_t before = 0;
            for (const vapor_read& x : rd) before += x.locus < l;
            ok = ok && first[(size_t)l] == before;
        }
        ok = ok && !memcmp(im.locus_first.in(image.data()), first.data(), 4 * first.size()) && (!n_reads || !memcmp(im.reads.in(image.data()), rd.data(), 32 * rd.size()));
        for (size_t at = n_reads ? im.reads.bytes() : 0; at < im.locus_first.off; ++at) ok = ok && image[at] == 0;
        for (size_t at = im.locus_first.off + im.locus_first.bytes(); at < im.bytes; ++at) ok = ok && image[at] == 0;
        CHECK(ok, "table %d: %lld reads over %lld loci", t, (long long)n_reads, (long long)n_loci);
        // a grid over it: every locus a group of its own
        std::vector<int32_t> fl, off;
        for (int64_t l = 0; l <= n_loci; ++l) fl.push_back((int32_t)l);
        CHECK(says(fp::grid_check(n_loci, fl.data(), n_loci, first.data(), off), nullptr) && off == first, "grid %d", t);
        for (int with = 0; with < 2; ++with) {
            const fp::GridImage gi((size_t)n_loci, off.back(), with ? first.size() : 0);
            const std::vector<uint8_t> g = gi.filled(fl.data(), off, with ? first.data() : nullptr);
            std::vector<uint8_t> want(gi.bytes, 0);
            memcpy(want.data() + gi.first_locus.off, fl.data(), 4 * fl.size());
            memcpy(want.data() + gi.score_off.off, off.data(), 4 * off.size());
            if (with) memcpy(want.data() + gi.read_first.off, first.data(), 4 * first.size());
            CHECK(g == want, "grid image %d", t);
        }
    }
    std::printf("images: %d shapes tile on 8 bytes, %d filled, locus_first counts the reads in front\n", n, n_filled);
}

// ------------------------------------------------------------------------------------------
// the run's decisions
// ------------------------------------------------------------------------------------------
static void check_run()
{
    // ran, a pair with a host-side status, the run saw a slot overflow, overflow_final -> light path, statuses uploaded again, repeated
    static const bool T[16][7] = {
        {0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 1, 0, 0, 0}, {0, 0, 1, 0, 0, 0, 0}, {0, 0, 1, 1, 0, 0, 0},     // the first run: the full path; it resizes itself
        {0, 1, 0, 0, 0, 1, 0}, {0, 1, 0, 1, 0, 1, 0}, {0, 1, 1, 0, 0, 1, 0}, {0, 1, 1, 1, 0, 1, 0},
        {1, 0, 0, 0, 1, 0, 0}, {1, 0, 0, 1, 1, 0, 0}, {1, 0, 1, 0, 1, 0, 1}, {1, 0, 1, 1, 1, 0, 0},     // a later run: light, repeated once on overflow
        {1, 1, 0, 0, 0, 1, 0}, {1, 1, 0, 1, 0, 1, 0}, {1, 1, 1, 0, 0, 1, 0}, {1, 1, 1, 1, 0, 1, 0},     // a host-side status: always the full path
    };
    for (const auto& r : T) {
        const bool light = fp::light_run(r[0], r[1]);
        CHECK(light == r[4] && fp::reupload_statuses(light, r[1]) == r[5] && fp::repeat_full(light, r[2], r[3]) == r[6], "run %d%d%d%d", r[0], r[1], r[2], r[3]);
    }
    // a status the full run itself gave is uploaded as well; the light path never uploads
    CHECK(fp::reupload_statuses(false, true) && !fp::reupload_statuses(false, false) && !fp::reupload_statuses(true, true), "statuses given by the run");
    const int32_t none[4] = {0, 0, 0, 0}, last[4] = {0, 0, 0, VAPOR_E_ARG};
    CHECK(!fp::any_status(none, 4) && fp::any_status(last, 4) && !fp::any_status(last, 3) && !fp::any_status(nullptr, 0), "any_status");
    std::vector<int64_t> st(3 * 16, 0);
    CHECK(!fp::still_overflows(st.data(), 3), "no status");
    st[16 + 15] = VAPOR_E_ARG; st[14] = VAPOR_E_OVERFLOW;
    CHECK(!fp::still_overflows(st.data(), 3), "another status, another word");
    st[32 + 15] = VAPOR_E_OVERFLOW;
    CHECK(fp::still_overflows(st.data(), 3) && !fp::still_overflows(st.data(), 2), "the last pair's status");
    // the asynchronous step: no read table, no blocking run yet, a pair the host rejected - in this order
    static const char* const ASYNC_MSG[3] = {"vapor_plan_run_loci_async: call vapor_plan_set_reads first",
                                             "vapor_plan_run_loci_async: run the plan once with vapor_plan_run_loci first (it sizes the slots)",
                                             "vapor_plan_run_loci_async: the plan holds pairs the host rejected; use vapor_plan_run_loci"};
    CHECK(says(fp::async_refusal(true, true, none, 4), nullptr), "a step");
    for (unsigned mask = 1; mask < 8; ++mask) {
        int want = 0;
        while (!(mask >> want & 1u)) ++want;
        CHECK(says(fp::async_refusal(!(mask & 1u), !(mask & 2u), mask & 4u ? last : none, 4), ASYNC_MSG[want]), "async %u", mask);
    }
    std::printf("run decisions: 16 states equal their table, 7 refused asynchronous steps in order\n");
}

// ------------------------------------------------------------------------------------------
// every integer of the file behind "rows" (tools/finish_plan_fixture.cpp), the messages by index
// ------------------------------------------------------------------------------------------
struct Rows {
    std::vector<long long> v;
    size_t at = 0;
    bool more() const { return at < v.size(); }
    long long next() { return at < v.size() ? v[at++] : (++g_bad, 0); }
    std::vector<int32_t> list(long long n)
    {
        std::vector<int32_t> x;
        for (long long i = 0; i < n; ++i) x.push_back((int32_t)next());
        return x;
    }
};
static void check_fixture(const char* path)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { CHECK(false, "cannot open %s", path); return; }
    std::string text;
    char buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
    std::fclose(f);
    const size_t m0 = text.find("\"messages\""), r0 = text.find("\"rows\"");
    if (m0 == std::string::npos || r0 == std::string::npos || r0 < m0) { CHECK(false, "no messages and rows in %s", path); return; }
    std::vector<std::string> messages;
    for (size_t at = text.find('[', m0) + 1; at < r0 && text[at] != ']';) {
        if (text[at] != '"') { ++at; continue; }
        const size_t end = text.find('"', at + 1);
        messages.push_back(text.substr(at + 1, end - at - 1));
        at = end + 1;
    }
    CHECK(messages.size() == 11 && messages[0].empty(), "%zu messages", messages.size());
    Rows R;
    for (size_t at = r0; at < text.size();) {
        if ((text[at] >= '0' && text[at] <= '9') || text[at] == '-') {
            char* end = nullptr;
            R.v.push_back(std::strtoll(text.c_str() + at, &end, 10));
            at = (size_t)(end - text.c_str());
        } else ++at;
    }
    size_t per_family[3] = {0, 0, 0}, refused[3] = {0, 0, 0};
    auto same = [&](const fp::Refusal& no, long long code, long long msg) {
        return no.code == code && msg >= 0 && (size_t)msg < messages.size() && messages[(size_t)msg] == (no.msg ? no.msg : "");
    };
    const int before = g_bad;
    while (R.more() && g_bad == before) {
        const long long fam = R.next();
        std::vector<int32_t> off;
        if (fam == 0) {
            const long long n_pairs = R.next(), n_loci = R.next(), n_reads = R.next();
            std::vector<vapor_read> rd((size_t)n_reads);
            for (vapor_read& x : rd) { x.ref_a = (int32_t)R.next(); x.alt_a = (int32_t)R.next(); x.ref_b = (int32_t)R.next(); x.alt_b = (int32_t)R.next();
                                       x.kind = (int32_t)R.next(); x.locus = (int32_t)R.next(); x.len_ref = (int32_t)R.next(); x.len_alt = (int32_t)R.next(); }
            const long long code = R.next(), msg = R.next();
            const std::vector<int32_t> want = R.list(R.next());
            std::vector<int32_t> first;
            std::vector<uint8_t> image;
            fp::ReadImage im;
            const fp::Refusal no = fp::read_table(n_reads, rd.data(), n_loci, n_pairs, first, im, image);
            CHECK(same(no, code, msg), "reads point %zu: %d %s", per_family[0], no.code, no.msg ? no.msg : "");
            if (!no) {
                const long long front = R.next(), block = R.next(), scores = R.next(), records = R.next();
                // (the block: four bytes more where locus_first has an odd length)
                CHECK(first == want && (long long)im.locus_first.off == front && (long long)im.bytes == block + (first.size() % 2 ? 4 : 0) &&
                          (long long)im.score_bytes == scores && (long long)im.loci_bytes == records, "reads point %zu: sizes", per_family[0]);
            }
            refused[0] += (bool)no;
        } else if (fam == 1 || fam == 2) {
            std::vector<int32_t> fl, lf;
            long long n_loci, n_groups;
            if (fam == 1) {
                n_loci = R.next(); lf = R.list(n_loci + 1);
                n_groups = R.next(); fl = R.list(n_groups + 1);
            } else {
                n_groups = R.next(); fl = R.list(n_groups + 1);
                lf = R.list(R.next());
                n_loci = fl.back();
            }
            const long long code = R.next(), msg = R.next();
            const std::vector<int32_t> want = R.list(R.next());
            const fp::Refusal no = fam == 1 ? fp::grid_check(n_groups, fl.data(), n_loci, lf.data(), off) : fp::pick_check(n_groups, fl.data(), lf.data(), off);
            CHECK(same(no, code, msg), "family %lld point %zu: %d %s", fam, per_family[fam], no.code, no.msg ? no.msg : "");
            if (!no) CHECK(off == want, "family %lld point %zu: off", fam, per_family[fam]);
            if (!no && n_groups > 0) {
                // the packed block's places, four bytes later for every table of odd length in front
                const size_t ng = (size_t)n_groups, pad1 = ng % 2 ? 0 : 4, pad3 = ng % 2 ? 4 : 8;
                const fp::GridImage im(ng, off.back(), fam == 2 ? lf.size() : 0);
                const long long block = R.next(), at_off = R.next(), at_idx = R.next(), at_rf = fam == 2 ? R.next() : 0;
                const long long rec = fam == 2 ? R.next() : 0, sc = fam == 2 ? R.next() : 0, group = R.next(), win = R.next();
                CHECK((long long)im.score_off.off == at_off + (long long)pad1 && (long long)im.winner_idx.off == at_idx + 2 * (long long)pad1 && (long long)im.group_bytes == group &&
                          (long long)im.winner_bytes == win, "family %lld point %zu: places", fam, per_family[fam]);
                if (fam == 1) CHECK((long long)im.bytes == block + (long long)pad3, "grid point %zu: %zu bytes", per_family[1], im.bytes);
                else CHECK((long long)im.read_first.off == at_rf + (long long)pad3 && (long long)im.bytes == block + (long long)pad3 + (lf.size() % 2 ? 4 : 0) &&
                               rec == 8 * fp::LOCUS_DOUBLES * n_loci && sc == 8 * std::max<long long>(lf.back(), 1), "pick point %zu: %zu bytes", per_family[2], im.bytes);
            }
            refused[fam] += (bool)no;
        } else {
            CHECK(false, "family %lld", fam);
            break;
        }
        ++per_family[fam];
    }
    for (size_t fam = 0; fam < 3; ++fam)
        CHECK(per_family[fam] >= 800 && refused[fam] * 5 >= per_family[fam] && refused[fam] * 5 <= 4 * per_family[fam], "family %zu: %zu points, %zu refused", fam, per_family[fam], refused[fam]);
    std::printf("fixture: %zu points equal what the calls answered before, %zu of them refusals\n", per_family[0] + per_family[1] + per_family[2], refused[0] + refused[1] + refused[2]);
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::printf("usage: finish_plan_check finish_plan.json\n"); return 2; }
    check_read_refusals();
    check_grid_refusals();
    check_edges();
    check_images();
    check_run();
    check_fixture(argv[1]);
    if (g_bad) { std::printf("finish_plan_check: %d statements FAILED\n", g_bad); return 1; }
    std::printf("finish_plan_check: all equal\n");
    return 0;
}
