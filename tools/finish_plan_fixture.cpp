// finish_plan_fixture.cpp - writes tests/golden/finish_plan.json.gz (unpacked, to stdout): what the host checks and sizes of the
// finishing and grid calls answered at a seeded sample of points when vapor_hip.hip still computed them between its launches.  The
// expressions below are those lines as they stood in vapor_plan_set_reads, grid_check, vapor_plan_set_grid and vapor_grid_pick,
// kept apart from vapor_finish_plan.h on purpose: tools/finish_plan_check.cpp compares the header against the file, which shows
// that moving them changed nothing but the stated alignment of the tables.  Run once; the file is committed.
//   g++ -O1 -std=c++17 -Iinclude tools/finish_plan_fixture.cpp -o finish_plan_fixture && ./finish_plan_fixture | gzip -9n > tests/golden/finish_plan.json.gz
// Every row is integers; a message is its index in "messages".
//   0, n_pairs, n_loci, n_reads, the reads (8 words each: ref_a alt_a ref_b alt_b kind locus len_ref len_alt)
//        -> code, message, n, first[n], then (code 0) bytes in front of locus_first, bytes of the block, of the scores, of the records
//   1, n_loci, lf[n_loci + 1], n_groups, first_locus[n_groups + 1]                                  (vapor_plan_set_grid)
//        -> code, message, n, off[n], then (code 0, groups) bytes of the block, in front of score_off, in front of winner_idx,
//           of the group records, of the winners' scores
//   2, n_groups, first_locus[n_groups + 1], n, read_first[n]                                        (vapor_grid_pick)
//        -> code, message, n, off[n], then (code 0, groups) bytes of the block, in front of score_off, of winner_idx, of read_first,
//           of the candidates' records, of their scores, of the group records, of the winners' scores
#include "vapor_hip.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

static const char* const MESSAGES[] = {"",
                                       "reads must be sorted by locus",
                                       "read refers to a pair outside the plan",
                                       "unknown scorer kind",
                                       "grid: the groups must cover the loci",
                                       "grid: a group holds 1 .. VAPOR_MAX_CANDIDATES consecutive loci",
                                       "grid: read ranges must not decrease",
                                       "grid: the candidates of a group score the same reads",
                                       "grid: too many reads",
                                       "vapor_grid_pick: bad ranges",
                                       "vapor_grid_pick: read ranges must not decrease"};
static const int N_MESSAGES = (int)(sizeof(MESSAGES) / sizeof(MESSAGES[0]));

static std::string g_err;
static int fail(int code, const std::string& m) { g_err = m; return code; }
static int message()
{
    for (int m = 0; m < N_MESSAGES; ++m)
        if (g_err == MESSAGES[m]) return m;
    return -1;
}

// ---- vapor_plan_set_reads as it stood ----
static int set_reads(int64_t n_pairs, int64_t n_reads, const vapor_read* reads, int64_t n_loci, std::vector<int32_t>& first, size_t* sizes)
{
    first.assign((size_t)n_loci + 1, 0);
    int32_t prev = -1;
    for (int64_t r = 0; r < n_reads; ++r) {
        const vapor_read& x = reads[r];
        if (x.locus < prev || x.locus >= n_loci) return fail(VAPOR_E_ARG, "reads must be sorted by locus");
        const int32_t idx[4] = {x.ref_a, x.alt_a, x.kind == 0 ? x.ref_b : x.ref_a, x.kind == 0 ? x.alt_b : x.alt_a};
        for (int32_t q : idx)
            if (q < 0 || q >= n_pairs) return fail(VAPOR_E_ARG, "read refers to a pair outside the plan");
        if (x.kind < 0 || x.kind > 3) return fail(VAPOR_E_ARG, "unknown scorer kind");
        prev = x.locus;
        first[(size_t)x.locus + 1]++;
    }
    for (int64_t l = 0; l < n_loci; ++l) first[l + 1] += first[l];
    const size_t reads_bytes = (sizeof(vapor_read) * (size_t)std::max<int64_t>(n_reads, 1) + 15) & ~(size_t)15;
    const size_t first_bytes = sizeof(int32_t) * first.size();
    sizes[0] = reads_bytes;
    sizes[1] = reads_bytes + first_bytes;
    sizes[2] = sizeof(double) * std::max<int64_t>(n_reads, 1);
    sizes[3] = sizeof(double) * 8 * std::max<int64_t>(n_loci, 1);
    return VAPOR_OK;
}

// ---- grid_check as it stood ----
static int grid_check(int64_t n_groups, const int32_t* first_locus, int64_t n_loci, const int32_t* lf, std::vector<int32_t>* off)
{
    if (first_locus[0] != 0 || first_locus[n_groups] != n_loci) return fail(VAPOR_E_ARG, "grid: the groups must cover the loci");
    off->assign((size_t)n_groups + 1, 0);
    for (int64_t g = 0; g < n_groups; ++g) {
        const int32_t a = first_locus[g], b = first_locus[g + 1];
        if (a < 0 || b <= a || b - a > VAPOR_MAX_CANDIDATES || b > n_loci)
            return fail(VAPOR_E_ARG, "grid: a group holds 1 .. VAPOR_MAX_CANDIDATES consecutive loci");
        const int32_t nr = lf[(size_t)a + 1] - lf[a];
        if (nr < 0) return fail(VAPOR_E_ARG, "grid: read ranges must not decrease");
        for (int32_t c = a; c < b; ++c)
            if (lf[(size_t)c + 1] - lf[c] != nr) return fail(VAPOR_E_ARG, "grid: the candidates of a group score the same reads");
        if ((int64_t)(*off)[g] + nr > INT32_MAX) return fail(VAPOR_E_ARG, "grid: too many reads");
        (*off)[g + 1] = (*off)[g] + nr;
    }
    return VAPOR_OK;
}

// ---- the sizes and places of vapor_plan_set_grid as they stood (n_groups > 0) ----
static void set_grid_sizes(size_t ng, const std::vector<int32_t>& off, size_t* sizes)
{
    sizes[0] = sizeof(int32_t) * (3 * ng + 2);
    sizes[1] = sizeof(int32_t) * (ng + 1);
    sizes[2] = sizeof(int32_t) * (2 * ng + 2);
    sizes[3] = sizeof(double) * 16 * ng;
    sizes[4] = sizeof(double) * (size_t)std::max<int32_t>(off[ng], 1);
}

// ---- vapor_grid_pick's checks, sizes and places as they stood ----
static int grid_pick(int64_t n_groups, const int32_t* first_locus, const int32_t* read_first, std::vector<int32_t>& off, size_t* sizes)
{
    const int64_t n_loci = first_locus[n_groups];
    if (n_loci < 0 || n_loci > INT32_MAX || read_first[0] != 0) return fail(VAPOR_E_ARG, "vapor_grid_pick: bad ranges");
    for (int64_t c = 0; c < n_loci; ++c)
        if (read_first[c + 1] < read_first[c]) return fail(VAPOR_E_ARG, "vapor_grid_pick: read ranges must not decrease");
    const int rc = grid_check(n_groups, first_locus, n_loci, read_first, &off);
    if (rc != VAPOR_OK) return rc;
    if (n_groups == 0) return VAPOR_OK;
    const size_t ng = (size_t)n_groups, nl = (size_t)n_loci, nr = (size_t)read_first[n_loci], nw = (size_t)off[ng];
    sizes[0] = sizeof(int32_t) * (3 * ng + 2 + nl + 1);
    sizes[1] = sizeof(int32_t) * (ng + 1);
    sizes[2] = sizeof(int32_t) * (2 * ng + 2);
    sizes[3] = sizeof(int32_t) * (3 * ng + 2);
    sizes[4] = sizeof(double) * 8 * nl;
    sizes[5] = sizeof(double) * std::max<size_t>(nr, 1);
    sizes[6] = sizeof(double) * 16 * ng;
    sizes[7] = sizeof(double) * std::max<size_t>(nw, 1);
    return VAPOR_OK;
}

// ---- the points ----
static std::mt19937_64 g_rng(20261021);
static long long upto(long long top) { return (long long)(g_rng() % (unsigned long long)top); }

static bool g_first = true;
static void put(const std::vector<long long>& row)
{
    std::printf("%s[", g_first ? "" : ",\n");
    for (size_t i = 0; i < row.size(); ++i) std::printf("%s%lld", i ? "," : "", row[i]);
    std::printf("]");
    g_first = false;
}
static void put_list(std::vector<long long>& row, const std::vector<int32_t>& v)
{
    row.push_back((long long)v.size());
    for (int32_t x : v) row.push_back(x);
}

static void reads_point(int t)
{
    const int64_t n_pairs = t % 7 == 0 ? 1 : 1 + upto(40), n_loci = t % 11 == 0 ? 0 : t % 5 == 0 ? 1 + upto(3) : 1 + upto(24);
    const int64_t n_reads = (n_loci == 0 && t % 2) || t % 13 == 0 ? 0 : 1 + upto(t % 3 ? 12 : 40);
    std::vector<vapor_read> rd((size_t)n_reads);
    std::vector<int32_t> loci;
    for (int64_t r = 0; r < n_reads; ++r) loci.push_back((int32_t)upto(std::max<int64_t>(n_loci, 1)));
    std::sort(loci.begin(), loci.end());
    for (int64_t r = 0; r < n_reads; ++r) {
        vapor_read& x = rd[(size_t)r];
        x.ref_a = (int32_t)upto(n_pairs); x.alt_a = (int32_t)upto(n_pairs);
        // (the second scorer's pairs are read for kind 0 only: elsewhere anything may stand there)
        x.kind = (int32_t)upto(4);
        x.ref_b = x.kind == 0 || upto(2) ? (int32_t)upto(n_pairs) : (int32_t)(n_pairs + upto(5));
        x.alt_b = x.kind == 0 || upto(2) ? (int32_t)upto(n_pairs) : -1 - (int32_t)upto(3);
        x.locus = loci[(size_t)r];
        x.len_ref = 1 + (int32_t)upto(5000); x.len_alt = 1 + (int32_t)upto(5000);
    }
    // break it: up to two faults, anywhere
    for (int b = 0, nb = n_reads ? (int)upto(4) % 3 : 0; b < nb; ++b) {
        vapor_read& x = rd[(size_t)upto(n_reads)];
        switch (upto(8)) {
        case 0: x.locus = (int32_t)n_loci + (int32_t)upto(2); break;
        case 1: x.locus = (int32_t)upto(std::max<int64_t>(n_loci, 1)) - (int32_t)upto(3); break;
        case 2: x.ref_a = (int32_t)n_pairs; break;
        case 3: x.alt_a = -1; break;
        case 4: x.kind = 0; x.ref_b = (int32_t)n_pairs + 7; break;
        case 5: x.kind = 0; x.alt_b = INT32_MIN; break;
        case 6: x.kind = 4 + (int32_t)upto(3); break;
        default: x.kind = -1 - (int32_t)upto(2); break;
        }
    }
    std::vector<long long> row{0, n_pairs, n_loci, n_reads};
    for (const vapor_read& x : rd)
        for (long long w : {x.ref_a, x.alt_a, x.ref_b, x.alt_b, x.kind, x.locus, x.len_ref, x.len_alt}) row.push_back(w);
    std::vector<int32_t> first;
    size_t sizes[4] = {0, 0, 0, 0};
    g_err.clear();
    const int rc = set_reads(n_pairs, n_reads, rd.data(), n_loci, first, sizes);
    row.push_back(rc); row.push_back(message());
    if (rc != VAPOR_OK) first.clear();
    put_list(row, first);
    if (rc == VAPOR_OK)
        for (size_t s : sizes) row.push_back((long long)s);
    put(row);
}

// groups over loci with equal read counts inside a group, then up to two faults.  edge: groups of one candidate whose read counts
// bring the winners' slots to INT32_MAX exactly (t even) or one past it (lf starts below zero: grid_check reads differences only,
// and no read table of a plan has such ranges)
static void grid_tables(int t, bool edge, std::vector<int32_t>& fl, std::vector<int32_t>& lf)
{
    fl.assign(1, 0);
    lf.assign(1, 0);
    if (edge) {
        const int32_t counts[4] = {1 << 30, (1 << 30) - (t % 2 ? 0 : 1), 0, t % 4 < 2 ? 0 : 1};
        lf[0] = -(1 << 30);
        for (int g = 0; g < 2 + t % 3; ++g) { fl.push_back(g + 1); lf.push_back(lf.back() + counts[g]); }
        return;
    }
    const int n_groups = t % 17 == 0 ? 0 : t % 4 == 0 ? 1 + (int)upto(3) : 1 + (int)upto(12);
    for (int g = 0; g < n_groups; ++g) {
        const int nc = g == 0 && t % 9 == 0 ? 128 : g == 0 && t % 31 == 0 ? 129 : 1 + (int)upto(t % 3 ? 4 : 20);
        const int32_t nr = (int32_t)upto(6);
        for (int c = 0; c < nc; ++c) lf.push_back(lf.back() + nr);
        fl.push_back(fl.back() + nc);
    }
    for (int b = 0, nb = (int)upto(5) % 3; b < nb; ++b) {
        const size_t g = (size_t)upto((long long)fl.size()), l = (size_t)upto((long long)lf.size());
        switch (upto(8)) {
        case 0: fl[0] = 1; break;
        case 1: fl.back() += 1 - 2 * (int32_t)upto(2); break;
        case 2: if (g + 1 < fl.size()) fl[g + 1] = fl[g]; break;                     // an empty group
        case 3: if (g + 1 < fl.size()) fl[g] = fl[g + 1] + 1; break;                 // a group running backwards
        case 4: if (g) fl[g] = -3; break;
        case 5: if (l) lf[l] -= 1 + (int32_t)upto(7); break;                         // unequal counts, or a decreasing range
        case 6: if (l) lf[l] += 1; break;
        default: if (g + 1 < fl.size() && g) fl[g] = (int32_t)lf.size() + 5; break;  // a group beyond the loci
        }
    }
}
static void put_values(std::vector<long long>& row, const std::vector<int32_t>& v)
{
    for (int32_t x : v) row.push_back(x);
}

static void grid_point(int t)
{
    std::vector<int32_t> fl, lf;
    grid_tables(t, t % 23 == 0, fl, lf);
    const int64_t n_groups = (int64_t)fl.size() - 1, n_loci = (int64_t)lf.size() - 1;
    std::vector<long long> row{1, n_loci};
    put_values(row, lf);
    row.push_back(n_groups);
    put_values(row, fl);
    std::vector<int32_t> off;
    g_err.clear();
    const int rc = grid_check(n_groups, fl.data(), n_loci, lf.data(), &off);
    row.push_back(rc); row.push_back(message());
    if (rc != VAPOR_OK) off.clear();
    put_list(row, off);
    if (rc == VAPOR_OK && n_groups > 0) {
        size_t sizes[5];
        set_grid_sizes((size_t)n_groups, off, sizes);
        for (size_t s : sizes) row.push_back((long long)s);
    }
    put(row);
}

static void pick_point(int t)
{
    std::vector<int32_t> fl, lf;
    grid_tables(t, false, fl, lf);
    if (t % 19 == 0) lf[0] = 1;
    if (t % 29 == 0) fl.back() = -2;
    // read_first as long as first_locus[n_groups] says (what the entry reads), where that is a length at all
    const int64_t n_groups = (int64_t)fl.size() - 1;
    if (fl.back() >= 0) lf.resize((size_t)fl.back() + 1, lf.back());
    std::vector<long long> row{2, n_groups};
    put_values(row, fl);
    put_list(row, lf);
    std::vector<int32_t> off;
    size_t sizes[8];
    g_err.clear();
    const int rc = grid_pick(n_groups, fl.data(), lf.data(), off, sizes);
    row.push_back(rc); row.push_back(message());
    if (rc != VAPOR_OK) off.clear();
    put_list(row, off);
    if (rc == VAPOR_OK && n_groups > 0)
        for (size_t s : sizes) row.push_back((long long)s);
    put(row);
}

int main()
{
    std::printf("{\"what\": \"family, arguments, answers (tools/finish_plan_fixture.cpp)\", \"messages\": [");
    for (int m = 0; m < N_MESSAGES; ++m) std::printf("%s\"%s\"", m ? ", " : "", MESSAGES[m]);
    std::printf("], \"rows\": [\n");
    for (int t = 0; t < 1500; ++t) reads_point(t);
    for (int t = 0; t < 1500; ++t) grid_point(t);
    for (int t = 0; t < 800; ++t) pick_point(t);
    std::printf("\n]}\n");
    return 0;
}
