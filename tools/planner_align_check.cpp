// planner_align_check.cpp - the window-aligned task table of the host planner (vapor_amd/csrc/vapor_planner.h: plan_launch_aligned,
// PlanParams::align_tasks) on a CPU, against direct statements of its rule: every joined pair in exactly one aligned task, one
// allele a task, at most reads_per_task reads, the same launches as the cost-balanced table over the same pair list; on
// launches small enough to enumerate: every group cut as cheaply as its number of ranges allows, no smaller bound within
// join_tasks, no group with a range the bound does not need; and `tasks` / `launches` byte for byte those of a layout made with
// default PlanParams.  The worlds come from fixed seeds like tools/planner_check.cpp's, as descriptors only (the planner reads
// lengths and symbol counts, no text): windows of 50 to 400 symbols, now and then with symbols outside upper-case ACGT, zero to two
// deletion alleles derived from each, one to nine reads a window; and by design: more windows than join_tasks, a group larger
// than reads_per_task, a group of one read, join_tasks = 1.  Nothing is compared with recorded output of the planner.
// Built and run by tests/test_planner_align_cpu.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc tools/planner_align_check.cpp
#include "vapor_planner.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace vapor;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (case %ld)\n", g_case); exit(1); } } while (0)

static std::mt19937_64 rng(20261020);
static long g_case = 0;
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }      // lo .. hi
static bool one_in(int n) { return rng() % (uint64_t)n == 0; }

enum Kind { RANDOM, MANY_WINDOWS, BIG_GROUP, SINGLE_READS, ONE_TASK };

struct World {
    std::vector<SeqDesc> h;
    int32_t n = 0, n_lit = 0;
    std::vector<std::vector<HSeg>> derived;
    std::vector<uint8_t> dflags;
    std::vector<ShareGroup> groups;
    std::vector<int32_t> group_of, slot_of;
    std::vector<std::vector<int32_t>> loci;    // per window: the window and its alleles
    std::vector<std::vector<int32_t>> reads;   // per window: its reads
    SetView view() const { return SetView{h, n, n_lit, derived, groups, group_of, slot_of}; }
};

static SeqDesc desc(int len, int n_exc)
{
    SeqDesc d;
    memset(&d, 0, sizeof d);
    d.len = len;
    d.n_exc = n_exc;
    return d;
}

static World make_world(Kind kind, bool shared_join, int reads_per_task)
{
    World w;
    const int n_win = kind == MANY_WINDOWS ? rnd(6, 14) : kind == BIG_GROUP ? rnd(1, 2) : rnd(1, 5);
    std::vector<int> n_alleles;
    for (int i = 0; i < n_win; ++i) {
        w.h.push_back(desc(rnd(50, 400), one_in(4) ? rnd(1, 9) : 0));
        w.loci.push_back({(int32_t)w.h.size() - 1});
        n_alleles.push_back(one_in(3) ? 0 : rnd(1, 2));
    }
    w.reads.resize((size_t)n_win);
    for (int i = 0; i < n_win; ++i) {
        int r = kind == SINGLE_READS ? 1 : kind == BIG_GROUP ? reads_per_task + rnd(1, 2 * reads_per_task) : rnd(1, 9);
        for (; r > 0; --r) {
            w.h.push_back(desc(one_in(12) ? rnd(5, 39) : rnd(50, 400), one_in(6) ? rnd(1, 5) : 0));
            w.reads[(size_t)i].push_back((int32_t)w.h.size() - 1);
        }
    }
    w.n_lit = (int32_t)w.h.size();
    for (int i = 0; i < n_win; ++i)
        for (int a = 0; a < n_alleles[(size_t)i]; ++a) {
            const int32_t win = w.loci[(size_t)i][0];
            const int nw = w.h[(size_t)win].len;
            int x = rnd(1, nw - 2), y = rnd(1, nw - 2);
            if (x > y) std::swap(x, y);
            ++y;                                                                     // a deletion of [x, y), 1 <= x < y <= nw - 1
            w.derived.push_back({HSeg{win, 0, x, 0, false}, HSeg{win, y, nw - y, x, false}});
            w.dflags.push_back(0);
            w.loci[(size_t)i].push_back(w.n_lit + (int32_t)w.derived.size() - 1);
        }
    w.n = w.n_lit + (int32_t)w.derived.size();
    for (const auto& sg : w.derived) w.h.push_back(desc(sg[0].len + sg[1].len, w.h[(size_t)sg[0].parent].n_exc));
    if (shared_join) {
        const auto hidden = share_layout(w.h, w.n, w.n_lit, w.derived, w.dflags, &w.groups, &w.group_of, &w.slot_of);
        for (const auto& sg : hidden) {
            int len = 0;
            for (const HSeg& x : sg) len += x.len;
            w.h.push_back(desc(len, w.h[(size_t)sg[0].parent].n_exc));
        }
    }
    return w;
}

static const int KS[4] = {10, 20, 30, 40};

// every read of a window against the window and its alleles (now and then not all of them), one or two window sizes a world
static std::vector<vapor_pair> make_pairs(const World& w)
{
    std::vector<vapor_pair> pairs;
    const int k0 = KS[rnd(0, 3)], k1 = one_in(3) ? KS[rnd(0, 3)] : k0;
    for (size_t i = 0; i < w.loci.size(); ++i)
        for (int32_t read : w.reads[i])
            for (int32_t target : w.loci[i]) {
                if (one_in(8) && !pairs.empty()) continue;
                vapor_pair p;
                p.seq1 = read; p.seq2 = target; p.k = one_in(2) ? k0 : k1; p.flags = (uint32_t)rnd(0, 7); p.off2 = 0;
                pairs.push_back(p);
            }
    for (size_t i = pairs.size(); i > 1; --i) if (one_in(3)) std::swap(pairs[i - 1], pairs[(size_t)rnd(0, (int)i - 1)]);
    return pairs;
}

struct Tally {
    long cases = 0, launches = 0, tasks = 0, groups = 0, pairs = 0;
    long small_launches = 0, cuts = 0, bounds = 0;
    long over_tasks = 0, big_groups = 0, single = 0, one_task = 0, fewer = 0, split = 0;
};
static Tally T;

// cost of pairs [a, b) of a launch as one task: the planner's units, restated
static int64_t range_cost(const World& w, const PlanParams& P, const PlanLayout& L, const Launch& la, size_t a, size_t b)
{
    int64_t cost = 0;
    for (size_t t = a; t < b; ++t) {
        const DPair& d = L.hp[(size_t)L.task_pairs[t]];
        const int64_t len1 = w.h[(size_t)d.seq1].len, len2 = w.h[(size_t)d.seq2].len;
        const int64_t tile = la.bps == 4 ? P.tile4 : P.tile2;
        const int64_t tiles = std::max<int64_t>(1, (len2 - la.k + 1 + tile - 1) / tile);
        cost += len1 * tiles + 256;
        if (t == a || d.seq2 != L.hp[(size_t)L.task_pairs[t - 1]].seq2) cost += VAPOR_BUILD_COST_X8 * len2 / 8;
    }
    return cost;
}

// best[m] = the dearest range of the cheapest cut of pairs [a, b) into exactly m ranges of at most `rpt` pairs, -1: no such cut
static std::vector<int64_t> best_cuts(const World& w, const PlanParams& P, const PlanLayout& L, const Launch& la, size_t a, size_t b)
{
    const size_t n = b - a;
    std::vector<int64_t> best(n + 1, -1);
    for (unsigned cuts = 0; cuts < (1u << (n - 1)); ++cuts) {
        int64_t worst = 0;
        size_t ranges = 0;
        bool fits = true;
        for (size_t x = 0; x < n;) {
            size_t y = x + 1;
            while (y < n && !((cuts >> (y - 1)) & 1u)) ++y;
            fits = fits && (int64_t)(y - x) <= P.reads_per_task;
            worst = std::max(worst, range_cost(w, P, L, la, a + x, a + y));
            ++ranges;
            x = y;
        }
        ++T.cuts;
        if (fits && (best[ranges] < 0 || worst < best[ranges])) best[ranges] = worst;
    }
    return best;
}

static void check_aligned(const World& w, const PlanParams& P, const PlanLayout& L)
{
    CHECK(L.alaunches.size() == L.launches.size(), "%zu aligned launches, %zu balanced", L.alaunches.size(), L.launches.size());
    size_t next_pair = 0, next_task = 0;
    for (size_t li = 0; li < L.alaunches.size(); ++li) {
        const Launch &la = L.alaunches[li], &lb = L.launches[li];
        CHECK(la.bps == lb.bps && la.k == lb.k && la.exc == lb.exc, "launch %zu: bps %d k %d exc %d, the balanced one %d %d %d", li, la.bps, la.k, la.exc, lb.bps, lb.k, lb.exc);
        CHECK(la.n_tasks >= 1 && (size_t)la.task_begin == next_task && next_task + (size_t)la.n_tasks <= L.atasks.size(), "launch of tasks %d + %d", la.task_begin, la.n_tasks);
        // the pairs of the balanced launch: the aligned one covers the same ones
        size_t n_b = 0;
        for (int t = 0; t < lb.n_tasks; ++t) n_b += (size_t)L.tasks[(size_t)(lb.task_begin + t)].n_reads;
        const size_t first = next_pair;
        struct Group { size_t a, b; int m; int64_t dearest; };
        std::vector<Group> groups;
        for (int t = 0; t < la.n_tasks; ++t) {
            const DTask& tk = L.atasks[next_task++];
            // (tasks one behind the other from the launch's first pair to its last: every pair in exactly one of them)
            CHECK((size_t)tk.first == next_pair, "task at pair %d, the one before ends at %zu", tk.first, next_pair);
            CHECK(tk.n_reads >= 1 && tk.n_reads <= P.reads_per_task && next_pair + (size_t)tk.n_reads <= first + n_b, "task of %d pairs", tk.n_reads);
            CHECK(tk.k == la.k, "task of k %d in a launch of k %d", tk.k, la.k);
            for (int r = 0; r < tk.n_reads; ++r)
                CHECK(L.hp[(size_t)L.task_pairs[next_pair + (size_t)r]].seq2 == tk.seq2, "task of allele %d holds a pair of allele %d", tk.seq2,
                      L.hp[(size_t)L.task_pairs[next_pair + (size_t)r]].seq2);
            const int64_t cost = range_cost(w, P, L, la, next_pair, next_pair + (size_t)tk.n_reads);
            if (groups.empty() || L.hp[(size_t)L.task_pairs[groups.back().a]].seq2 != tk.seq2) groups.push_back(Group{next_pair, next_pair, 0, 0});
            groups.back().b = next_pair + (size_t)tk.n_reads;
            groups.back().m++;
            groups.back().dearest = std::max(groups.back().dearest, cost);
            next_pair += (size_t)tk.n_reads;
        }
        CHECK(next_pair == first + n_b, "the aligned launch ends at pair %zu, the balanced one at %zu", next_pair, first + n_b);
        // (a group is ALL the pairs of its allele: the next group begins another one)
        for (size_t g = 1; g < groups.size(); ++g)
            CHECK(L.hp[(size_t)L.task_pairs[groups[g].a]].seq2 != L.hp[(size_t)L.task_pairs[groups[g - 1].a]].seq2, "group %zu repeats an allele", g);
        int64_t floor_sum = 0, m_sum = 0, bound = 0;
        bool small = n_b <= 12;
        for (const Group& g : groups) {
            const int64_t n_g = (int64_t)(g.b - g.a);
            floor_sum += (n_g + P.reads_per_task - 1) / P.reads_per_task;
            m_sum += g.m;
            bound = std::max(bound, g.dearest);
            small = small && n_g <= 10;
            T.big_groups += n_g > P.reads_per_task;
            T.single += n_g == 1;
            T.split += g.m > 1;
        }
        CHECK(m_sum == la.n_tasks, "%ld ranges, %d tasks", (long)m_sum, la.n_tasks);
        if (floor_sum > P.join_tasks) {
            // more groups (or reads) than join_tasks has room for: the fewest ranges reads_per_task allows
            for (const Group& g : groups)
                CHECK(g.m == (int)((g.b - g.a + (size_t)P.reads_per_task - 1) / (size_t)P.reads_per_task), "a group of %zu pairs in %d ranges, reads_per_task %d, join_tasks %d",
                      g.b - g.a, g.m, P.reads_per_task, P.join_tasks);
            ++T.over_tasks;
        } else {
            CHECK(m_sum <= P.join_tasks, "%ld tasks, join_tasks %d", (long)m_sum, P.join_tasks);
        }
        T.fewer += la.n_tasks < lb.n_tasks;
        T.one_task += P.join_tasks == 1;
        T.groups += (long)groups.size();
        T.tasks += la.n_tasks;
        T.pairs += (long)n_b;
        ++T.launches;
        if (!small) continue;
        // by enumeration: per group the cheapest cut into every number of ranges
        std::vector<std::vector<int64_t>> best;
        for (const Group& g : groups) {
            best.push_back(best_cuts(w, P, L, la, g.a, g.b));
            CHECK(best.back()[(size_t)g.m] == g.dearest, "a group of %zu pairs in %d ranges: its dearest costs %ld, the cheapest cut's %ld", g.b - g.a, g.m, (long)g.dearest,
                  (long)best.back()[(size_t)g.m]);
        }
        // ranges a group needs under a bound: the fewest whose cheapest cut stays under it (-1: none does)
        auto need = [&](size_t g, int64_t b) {
            for (size_t m = 1; m < best[g].size(); ++m)
                if (best[g][m] >= 0 && best[g][m] <= b) return (int64_t)m;
            return (int64_t)-1;
        };
        // no group has a range the launch's bound (its dearest task) does not need
        for (size_t g = 0; g < groups.size(); ++g)
            CHECK(need(g, bound) == groups[g].m, "a group of %zu pairs in %d ranges, the bound %ld needs %ld", groups[g].b - groups[g].a, groups[g].m, (long)bound,
                  (long)need(g, bound));
        // no smaller bound fits join_tasks (a bound matters only where it equals some cut's dearest range)
        if (floor_sum <= P.join_tasks)
            for (size_t g = 0; g < groups.size(); ++g)
                for (int64_t cand : best[g]) {
                    if (cand < 0 || cand >= bound) continue;
                    int64_t sum = 0;
                    bool ok = true;
                    for (size_t x = 0; x < groups.size() && ok; ++x) { const int64_t m = need(x, cand); ok = m > 0; sum += m; }
                    CHECK(!ok || sum > P.join_tasks, "bound %ld needs %ld tasks, join_tasks %d, and the launch's dearest task costs %ld", (long)cand, (long)sum, P.join_tasks,
                          (long)bound);
                    ++T.bounds;
                }
        ++T.small_launches;
    }
    CHECK(next_pair == L.task_pairs.size() && next_task == L.atasks.size(), "%zu pairs and %zu tasks in aligned launches", next_pair, next_task);
    CHECK(L.model[1].n_tasks == (int64_t)L.atasks.size() && L.model[0].n_tasks == (int64_t)L.tasks.size(), "the model counts %ld and %ld tasks", (long)L.model[0].n_tasks,
          (long)L.model[1].n_tasks);
    int64_t builds = 0;                               // one allele a task: tables built = tiles of every task's allele
    for (const Launch& la : L.alaunches)
        for (int t = 0; t < la.n_tasks; ++t) {
            const int64_t tile = la.bps == 4 ? P.tile4 : P.tile2;
            builds += std::max<int64_t>(1, (w.h[(size_t)L.atasks[(size_t)(la.task_begin + t)].seq2].len - la.k + 1 + tile - 1) / tile);
        }
    CHECK(L.model[1].builds == builds, "the model counts %ld builds, the tasks say %ld", (long)L.model[1].builds, (long)builds);
}

static void one_case(Kind kind)
{
    ++g_case;
    PlanParams P;
    const bool small = kind != RANDOM || one_in(2);
    P.join_tasks = kind == ONE_TASK ? 1 : small ? rnd(1, 6) : rnd(1, 64);
    P.reads_per_task = small ? rnd(1, 5) : rnd(1, MAX_READS_PER_TASK);
    P.max_pair_cap = (int64_t)1 << 28;
    P.shared_join = !one_in(4);
    static const int tiles[4] = {64, 300, 2048, 24576};
    P.tile2 = tiles[rnd(0, 3)];
    P.tile4 = std::max(32, P.tile2 * 7 / 8);
    const World w = make_world(kind, P.shared_join, P.reads_per_task);
    const std::vector<vapor_pair> pairs = make_pairs(w);
    const PlanLayout L0 = plan_layout(P, w.view(), (int64_t)pairs.size(), pairs.data());      // (align_tasks at its default)
    CHECK(L0.atasks.empty() && L0.alaunches.empty(), "an aligned table (%zu tasks) without the parameter", L0.atasks.size());
    P.align_tasks = true;
    const PlanLayout L = plan_layout(P, w.view(), (int64_t)pairs.size(), pairs.data());
    CHECK(L.tasks.size() == L0.tasks.size() && (L.tasks.empty() || !memcmp(L.tasks.data(), L0.tasks.data(), sizeof(DTask) * L.tasks.size())), "`tasks` differ");
    CHECK(L.launches.size() == L0.launches.size() && (L.launches.empty() || !memcmp(L.launches.data(), L0.launches.data(), sizeof(Launch) * L.launches.size())),
          "`launches` differ");
    CHECK(L.task_pairs == L0.task_pairs && L.hp.size() == L0.hp.size() && L.status == L0.status, "the pair lists differ");
    check_aligned(w, P, L);
    ++T.cases;
}

int main()
{
    for (int c = 0; c < 1600; ++c) one_case(RANDOM);
    for (int c = 0; c < 150; ++c) one_case(MANY_WINDOWS);
    for (int c = 0; c < 150; ++c) one_case(BIG_GROUP);
    for (int c = 0; c < 150; ++c) one_case(SINGLE_READS);
    for (int c = 0; c < 150; ++c) one_case(ONE_TASK);
    CHECK(T.small_launches > 500 && T.bounds > 500, "%ld launches enumerated, %ld smaller bounds tried", T.small_launches, T.bounds);
    CHECK(T.over_tasks > 100 && T.big_groups > 100 && T.single > 100 && T.one_task > 100, "%ld launches of more groups than join_tasks, %ld groups above reads_per_task, %ld of one read, %ld launches with join_tasks 1",
          T.over_tasks, T.big_groups, T.single, T.one_task);
    CHECK(T.fewer > 100 && T.split > 100, "%ld launches of fewer tasks than the balanced table, %ld groups in several ranges", T.fewer, T.split);
    printf("balanced table: %ld cases byte for byte those of default PlanParams\n", T.cases);
    printf("aligned tasks: %ld launches, %ld tasks of one allele over %ld groups, %ld pairs each in one task\n", T.launches, T.tasks, T.groups, T.pairs);
    printf("enumerated: %ld launches, every group cut as cheaply as its ranges allow (%ld cuts), no smaller bound of %ld fits, no range beyond the bound's\n", T.small_launches,
           T.cuts, T.bounds);
    printf("by design: %ld launches of more groups than join_tasks, %ld groups above reads_per_task, %ld groups of one read, %ld launches with join_tasks 1\n", T.over_tasks,
           T.big_groups, T.single, T.one_task);
    printf("planner_align_check: all hold\n");
    return 0;
}
