// vapor_planner.h - the host arithmetic that decides what the kernels are told to do, without HIP: the share groups of a
// sequence set (share_layout), the plan of a list of pairs - validation, shared joins and their remap tables, launches and
// cost-balanced join tasks (plan_layout), the window-aligned task table beside them (plan_aligned) - and the order of the clean
// workgroups (clean_order).  vapor_hip.hip calls these and does the allocations and uploads; tools/planner_check.cpp and
// tools/planner_align_check.cpp run them on a CPU under the sanitizers, against direct statements of their rules.
#pragma once
#include "vapor_records.h"
#include "vapor_hip.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

// Cost of building an allele's table relative to probing one read base against it, in eighths.  Round 2 measured 0.4 per allele
// base (a table of 20 000 positions ~10 us, a 10 000-base read ~12 us) when a task held sixteen reads; with shared joins a cfg2
// task holds eight and the same measurement (tools/task_balance.py on a -DVAPOR_BLOCK_TIMING build: tasks with one table 71 us,
// with two 82-85 us: a table 11 us = 1.5 reads of 7.5 us) gives 0.75: priced at 3 the tasks that straddle two windows were the
// launch's longest by 15 %.  At 6: cfg2 join 0.0849 -> 0.0797 ms (5 .. 10 the same; profiles/r05_join_rounds.txt).
#ifndef VAPOR_BUILD_COST_X8
#define VAPOR_BUILD_COST_X8 6
#endif

namespace vapor {

// A derived sequence as the caller described it (destination offsets added), and the groups the plan shares joins in.
struct HSeg { int32_t parent, off, len, dst; bool rc; };
struct SharePiece {                // a stretch of a member that holds k-mers its parent window does not (for the largest window size)
    int32_t slot;                  // member slot (1 ..)
    int32_t a_from, a_to;          // symbols [a_from, a_to) of the member
    int32_t tile_off;              // where they lie in the shared sequence
};
struct ShareGroup {                // a window uploaded as bytes (or its upper-cased twin) and the sequences derived from it
    int32_t parent = -1;           // the literal sequence
    bool upper = false;
    int32_t identity = -1;         // user index of the sequence that IS the window (slot 0), -1: not in the set
    int32_t t_seq = -1;            // hidden shared sequence: the window followed by the pieces
    std::vector<int32_t> members;  // user indices of the derived sequences (slot 1 + position), at most 3
    std::vector<SharePiece> pieces;
};
constexpr int SHARE_KMAX = 40;     // the largest window size (pieces carry SHARE_KMAX - 1 symbols of context)

struct Launch {
    int bps, k, task_begin, n_tasks;
    int exc;       // 2-bit planes: 1 = alleles with symbols outside upper-case ACGT, 2 = reads with such symbols (join_kernel<.., EXC>)
};

inline bool k_supported(int k) { return k == 10 || k == 20 || k == 30 || k == 40; }

// The groups a plan shares joins in: every derived sequence goes to the group of the literal that gives it most of its symbols
// (same upper-casing), a derived sequence that is that literal from end to end (an upper-cased twin) is the group's identity,
// and the hidden sequence of a group is the window followed by the stretches of its members that hold k-mers the window does
// not: around every junction of two segments and over every segment that is not a long enough forward or reversed slice of
// the window itself, with SHARE_KMAX - 1 symbols of context on either side (cut for the largest window size, so that one
// hidden sequence serves every k; the plan cuts the interval maps for its k).  `h` holds the n sequences the caller sees (n_lit
// given as bytes, then the derived ones, whose segments and flags are `derived` and `dflags`).  Returns the hidden sequences'
// segment lists; hidden sequence t is sequence n + t.
inline std::vector<std::vector<HSeg>> share_layout(const std::vector<SeqDesc>& h, int32_t n, int32_t n_lit,
                                                   const std::vector<std::vector<HSeg>>& derived, const std::vector<uint8_t>& dflags,
                                                   std::vector<ShareGroup>* groups, std::vector<int32_t>* group_of,
                                                   std::vector<int32_t>* slot_of)
{
    std::vector<std::vector<HSeg>> hidden;
    const int32_t n_der = (int32_t)derived.size();
    group_of->assign((size_t)n, -1);
    slot_of->assign((size_t)n, -1);
    std::map<std::pair<int32_t, bool>, int32_t> gid;
    for (int32_t d = 0; d < n_der; ++d) {
        const auto& sg = derived[(size_t)d];
        const bool up = dflags[(size_t)d] & VAPOR_SEQ_UPPER;
        // the literal with the largest share of this sequence's symbols (forward or reversed)
        std::map<int32_t, int64_t> share;
        for (const HSeg& g : sg) share[g.parent] += g.len;
        int32_t par = -1; int64_t best = 0;
        for (auto& kv : share) if (kv.second > best) { best = kv.second; par = kv.first; }
        if (par < 0) continue;
        if ((h[(size_t)par].flags & VAPOR_SEQ_UPPER) && !up) continue;     // (the literal was upper-cased at upload: not this one's text)
        auto it = gid.find({par, up});
        if (it == gid.end()) {
            it = gid.emplace(std::make_pair(par, up), (int32_t)groups->size()).first;
            ShareGroup g; g.parent = par; g.upper = up;
            if (!up) { g.identity = par; }
            groups->push_back(g);
        }
        ShareGroup& g = (*groups)[(size_t)it->second];
        const bool whole = sg.size() == 1 && sg[0].parent == par && sg[0].off == 0 && sg[0].len == h[(size_t)par].len && !sg[0].rc;
        if (whole && g.identity < 0) { g.identity = n_lit + d; continue; }
        if (whole && g.identity >= 0) continue;                     // (another copy of the window - plain, or a second upper-cased twin: it
                                                                    // would only take one of the group's three member slots; its pairs are joined on their own)
        if (g.members.size() < 3) g.members.push_back(n_lit + d);
    }
    for (size_t q = 0; q < groups->size(); ++q) {
        ShareGroup& g = (*groups)[q];
        if (g.members.empty()) continue;
        const int32_t n_r = h[(size_t)g.parent].len;
        std::vector<HSeg> t;                                         // the hidden sequence's segments
        t.push_back(HSeg{g.parent, 0, n_r, 0, false});
        int64_t t_len = n_r;
        for (size_t m = 0; m < g.members.size(); ++m) {
            const auto& sg = derived[(size_t)(g.members[m] - n_lit)];
            const int32_t n_a = h[(size_t)g.members[m]].len;
            // k-mer starts of the member that are k-mers of the window at the largest window size
            std::vector<std::pair<int32_t, int32_t>> mapped;
            for (const HSeg& x : sg)
                if (x.parent == g.parent && x.len >= SHARE_KMAX) mapped.push_back({x.dst, x.dst + x.len - SHARE_KMAX});
            int32_t u = 0;
            auto add_piece = [&](int32_t from, int32_t to_start) {       // novel k-mer starts [from, to_start]
                const int32_t a0 = from, a1 = std::min(n_a, to_start + SHARE_KMAX);
                if (a1 <= a0) return;
                g.pieces.push_back(SharePiece{(int32_t)m + 1, a0, a1, (int32_t)t_len});
                // its symbols as slices of the member's own segments
                for (const HSeg& x : sg) {
                    const int32_t lo = std::max(a0, x.dst), hi = std::min(a1, x.dst + x.len);
                    if (hi <= lo) continue;
                    HSeg y;
                    y.parent = x.parent; y.len = hi - lo; y.rc = x.rc; y.dst = (int32_t)t_len + (lo - a0);
                    y.off = x.rc ? x.off + (x.dst + x.len - hi) : x.off + (lo - x.dst);
                    t.push_back(y);
                }
                t_len += a1 - a0;
            };
            for (auto& r : mapped) {                                     // (segments come in order of dst)
                if (r.first > u) add_piece(u, r.first - 1);
                u = std::max(u, r.second + 1);
            }
            if (u <= n_a - 1) add_piece(u, n_a - 1);
        }
        if (t_len > VAPOR_MAX_SEQ_LEN || t_len > (int64_t)2 * n_r + 4096) { g.members.clear(); g.pieces.clear(); continue; }   // not worth sharing
        g.t_seq = n + (int32_t)hidden.size();
        hidden.push_back(std::move(t));
        if (g.identity >= 0) { (*group_of)[(size_t)g.identity] = (int32_t)q; (*slot_of)[(size_t)g.identity] = 0; }
        for (size_t m = 0; m < g.members.size(); ++m) { (*group_of)[(size_t)g.members[m]] = (int32_t)q; (*slot_of)[(size_t)g.members[m]] = (int32_t)m + 1; }
    }
    return hidden;
}

// What the planner reads of the context ...
struct PlanParams {
    int reads_per_task;            // upper bound on pairs per join task
    int join_tasks;                // join tasks aimed for per launch
    int64_t max_pair_cap;
    bool shared_join;
    int tile2, tile4;              // allele positions per join tile on the 2-bit and on the 4-bit planes (tile_pos<JoinCfg, BPS>())
    bool align_tasks = false;      // also make the window-aligned task table (PlanLayout::atasks); `tasks` is the same either way
};
// ... and of the sequence set: its host view.
struct SetView {
    const std::vector<SeqDesc>& h;             // the n sequences the caller sees, the hidden shared ones behind them
    int32_t n, n_lit;
    const std::vector<std::vector<HSeg>>& derived;
    const std::vector<ShareGroup>& groups;
    const std::vector<int32_t>& group_of;
    const std::vector<int32_t>& slot_of;
};

// A task table in the planner's own cost units (plan_launch_tasks): every task's probes and table builds summed, the dearest
// task of every launch summed over the launches (they run one behind the other), and the tables built (per task: alleles x tiles).
struct TableModel { int64_t sum = 0, path = 0, builds = 0, n_tasks = 0; };

// What a plan is before anything of it is on the device.
struct PlanLayout {
    std::vector<DPair> hp;                     // the caller's pairs, then the (read, shared sequence) pairs the shared joins run
    std::vector<int32_t> status;
    std::vector<DTask> tasks;
    std::vector<int32_t> task_pairs;
    std::vector<Launch> launches;
    // the window-aligned table (PlanParams::align_tasks): the same launches over the same task_pairs, every task the pairs of ONE
    // allele (plan_launch_aligned)
    std::vector<DTask> atasks;
    std::vector<Launch> alaunches;
    TableModel model[2];                       // what the planner's cost units say of `tasks` [0] and of `atasks` [1]
    // shared joins (remap_kernel): pairs n_pairs .. n_pairs + shares.size() - 1 of hp are the (read, shared sequence) pairs the
    // join runs instead of the pairs they serve
    std::vector<DShare> shares;
    std::vector<int32_t> tables;               // per (group, k): boundaries and op words (remap_kernel)
    std::vector<DServe> serve;                 // per pair: where its records come from when a shared join serves it
    int64_t n_served = 0;
    int range_words_cap = 1;
    int64_t hwant = 1024;                      // records expected of the plan's largest pair (an estimate, not clamped)
};

// The pair mode.  2: 2-bit planes; 3: 2-bit planes, the allele has symbols outside upper-case ACGT (a launch of its own: the table
// leaves their k-mers out and runs end before them); 5: 2-bit planes, the read has such symbols (a launch of its own:
// their positions are masked out of the lookup, runs end before them); 4: both sides have them - the 4-bit planes
inline int pair_mode(const SeqDesc& s1, const SeqDesc& s2)
{
    return (s1.n_exc > 0 && s2.n_exc > 0) ? 4 : (s2.n_exc > 0 ? 3 : (s1.n_exc > 0 ? 5 : 2));
}
inline Launch launch_of_mode(int m, int k, int task_begin) { return Launch{m == 4 ? 4 : 2, k, task_begin, 0, m == 3 ? 1 : m == 5 ? 2 : 0}; }

// record slots of a pair of n1 x n2 symbols
inline uint32_t pair_slot_cap(int64_t n1, int64_t n2, int64_t max_pair_cap)
{
    return (uint32_t)std::min<int64_t>(std::min(n1, n2) + ((n1 * n2) >> 17) + 1024, max_pair_cap);
}

// join tiles of an allele of len_a symbols in mode m
inline int allele_tiles(const PlanParams& P, int32_t len_a, int k, int m)
{
    const int ta = m != 4 ? P.tile2 : P.tile4;
    return std::max(1, (len_a - k + 1 + ta - 1) / ta);
}

// Validates the caller's pairs and sizes their record slots; `order` gets the pairs that have a k-mer on both sides.
inline void plan_pairs(const PlanParams& P, const SetView& S, int64_t n_pairs, const vapor_pair* pairs, PlanLayout* L,
                       std::vector<uint8_t>* mode, std::vector<int32_t>* order)
{
    L->hp.resize((size_t)std::max<int64_t>(n_pairs, 1));
    memset(L->hp.data(), 0, sizeof(DPair) * L->hp.size());
    L->status.assign((size_t)n_pairs, 0);
    order->reserve((size_t)n_pairs);
    mode->assign((size_t)n_pairs, 2);
    int rw = 1;
    int64_t hwant = 1024;
    for (int64_t i = 0; i < n_pairs; ++i) {
        const vapor_pair& a = pairs[i];
        DPair& d = L->hp[i];
        d.seq1 = a.seq1; d.seq2 = a.seq2; d.off2 = a.off2; d.k = a.k; d.flags = a.flags; d.cap = 0;
        if (a.seq1 < 0 || a.seq1 >= S.n || a.seq2 < 0 || a.seq2 >= S.n || a.off2 < 0 || !k_supported(a.k)) {
            L->status[i] = VAPOR_E_ARG;
            d.seq1 = d.seq2 = 0;
            continue;
        }
        const SeqDesc& s1 = S.h[a.seq1];
        const SeqDesc& s2 = S.h[a.seq2];
        d.len1 = s1.len; d.len2 = s2.len;
        if (s1.len > VAPOR_MAX_SEQ_LEN || s2.len > VAPOR_MAX_SEQ_LEN) { L->status[i] = VAPOR_E_ARG; continue; }
        if (s1.len - a.k + 1 > 0 && s1.n_invalid > 0) { L->status[i] = VAPOR_E_KEYERROR; continue; }
        int64_t n1 = s1.len, n2 = std::max(0, s2.len - a.off2);
        d.cap = pair_slot_cap(n1, n2, P.max_pair_cap);
        (*mode)[i] = (uint8_t)pair_mode(s1, s2);
        rw = std::max(rw, (s1.len + s2.len + 2 + 31) / 32);
        // records expected: the shared diagonal in runs of a few dots plus the chance dots
        hwant = std::max<int64_t>(hwant, std::min(n1, n2) / 10 + ((n1 * n2) >> 19) + 192);
        if (s1.len - a.k + 1 > 0 && s2.len - a.k + 1 > 0) order->push_back((int32_t)i);
    }
    L->range_words_cap = rw;
    L->hwant = hwant;
}

// Shared joins: a read that is scored against a window AND against alleles derived from it (the usual case: the
// reference's dotdata(read, ref) and dotdata(read, alt), SF:185-186) is joined once against the group's hidden sequence -
// the window followed by the alleles' own stretches - and remap_kernel cuts that dot plot into the targets'.  Appends the
// (read, hidden sequence) pairs to hp and mode, and replaces the pairs they serve by them in `order`.
inline void plan_shared_joins(const PlanParams& P, const SetView& S, int64_t n_pairs, PlanLayout* L, std::vector<uint8_t>* mode,
                              std::vector<int32_t>* order)
{
    struct Cand { int32_t seq1, group, k, slot, pair; };
    std::vector<Cand> cand;
    for (int32_t x : *order) {
        const DPair& d = L->hp[(size_t)x];
        const int32_t g = S.group_of[(size_t)d.seq2];
        if (g >= 0 && S.groups[(size_t)g].t_seq >= 0) cand.push_back(Cand{d.seq1, g, d.k, S.slot_of[(size_t)d.seq2], x});
    }
    std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) {
        if (a.seq1 != b.seq1) return a.seq1 < b.seq1;
        if (a.group != b.group) return a.group < b.group;
        if (a.k != b.k) return a.k < b.k;
        if (a.slot != b.slot) return a.slot < b.slot;
        return a.pair < b.pair;
    });
    std::vector<DMap> maps;                                                          // the interval maps the tables are cut from
    std::map<std::pair<int32_t, int32_t>, std::pair<int32_t, int32_t>> maps_of;      // (group, k) -> (first map, maps); n < 0: cannot
    auto build_maps = [&](int32_t gi, int k) -> std::pair<int32_t, int32_t> {
        auto it = maps_of.find({gi, k});
        if (it != maps_of.end()) return it->second;
        const ShareGroup& g = S.groups[(size_t)gi];
        const int32_t first = (int32_t)maps.size();
        const int32_t n_r = S.h[(size_t)g.parent].len;
        bool ok = true;
        if (n_r >= k) maps.push_back(DMap{0, n_r - k, 0, 0, 0});
        for (size_t m = 0; m < g.members.size() && ok; ++m) {
            const auto& sg = S.derived[(size_t)(g.members[m] - S.n_lit)];
            const int32_t n_a = S.h[(size_t)g.members[m]].len;
            int32_t u = 0;                                   // next k-mer start of the member not yet accounted for
            auto novel = [&](int32_t from, int32_t to) {     // k-mer starts [from, to] lie in one of the member's own stretches
                for (const SharePiece& pc : g.pieces)
                    if (pc.slot == (int32_t)m + 1 && pc.a_from <= from && to + k <= pc.a_to) {
                        maps.push_back(DMap{pc.tile_off + (from - pc.a_from), pc.tile_off + (to - pc.a_from), from, 0, (uint16_t)(m + 1)});
                        return;
                    }
                ok = false;
            };
            for (const HSeg& x : sg) {
                if (x.parent != g.parent || x.len < k) continue;
                if (x.dst > u) novel(u, x.dst - 1);
                if (!ok) break;
                maps.push_back(DMap{x.off, x.off + x.len - k, x.rc ? x.dst + x.len - k : x.dst, (uint16_t)(x.rc ? 1 : 0), (uint16_t)(m + 1)});
                u = x.dst + x.len - k + 1;
            }
            if (ok && u <= n_a - k) novel(u, n_a - k);
        }
        std::pair<int32_t, int32_t> res{-1, -1};
        if (ok && (int32_t)maps.size() > first) {
            // the maps cut at each other's ends: boundaries over the k-mer starts of the shared sequence and, per elementary
            // interval, the op words of the maps that cover it (remap_kernel)
            std::vector<int32_t> bd{0};
            for (size_t m = (size_t)first; m < maps.size(); ++m) { bd.push_back(maps[m].lo); bd.push_back(maps[m].hi + 1); }
            std::sort(bd.begin(), bd.end());
            bd.erase(std::unique(bd.begin(), bd.end()), bd.end());
            const int n_iv = (int)bd.size() - 1;
            if (n_iv >= 1 && n_iv <= REMAP_MAX_IV) {
                std::vector<int32_t> ops((size_t)n_iv * REMAP_OPS, 0);
                for (int t = 0; t < n_iv && ok; ++t)
                    for (size_t m = (size_t)first; m < maps.size(); ++m) {
                        const DMap& mp = maps[m];
                        if (!(mp.lo <= bd[(size_t)t] && bd[(size_t)t + 1] - 1 <= mp.hi)) continue;
                        const int32_t delta = mp.flip ? mp.base + mp.lo : mp.base - mp.lo;
                        int32_t* o = &ops[(size_t)t * REMAP_OPS + (size_t)mp.slot * 2];
                        const int c = (o[0] & 1) ? 1 : 0;
                        if (c == 1 && (o[1] & 1)) { ok = false; break; }            // a third copy of one stretch in one allele
                        o[c] = (int32_t)(((uint32_t)delta << 2) | (mp.flip ? 2u : 0u) | 1u);
                    }
                if (ok) {
                    res = {(int32_t)L->tables.size(), n_iv};
                    L->tables.insert(L->tables.end(), bd.begin(), bd.end());
                    L->tables.insert(L->tables.end(), ops.begin(), ops.end());
                }
            }
        }
        maps.resize((size_t)first);
        maps_of[{gi, k}] = res;
        return res;
    };
    std::vector<uint8_t> served((size_t)n_pairs, 0);
    { DServe none; memset(&none, 0, sizeof(none)); none.dpair = -1; L->serve.assign((size_t)n_pairs, none); }
    for (size_t a = 0; a < cand.size();) {
        size_t b = a;
        while (b < cand.size() && cand[b].seq1 == cand[a].seq1 && cand[b].group == cand[a].group && cand[b].k == cand[a].k) ++b;
        int32_t tgt[4] = {-1, -1, -1, -1};
        int n_t = 0;
        for (size_t c = a; c < b; ++c)
            if (cand[c].slot >= 0 && cand[c].slot < 4 && tgt[cand[c].slot] < 0) { tgt[cand[c].slot] = cand[c].pair; ++n_t; }
        const Cand c0 = cand[a];
        a = b;
        if (n_t < 2) continue;
        const ShareGroup& g = S.groups[(size_t)c0.group];
        const SeqDesc& s1 = S.h[(size_t)c0.seq1];
        const SeqDesc& st = S.h[(size_t)g.t_seq];
        if (st.len - c0.k + 1 <= 0) continue;
        const int md = pair_mode(s1, st);
        int sep = 0;
        for (int t = 0; t < 4; ++t)
            if (tgt[t] >= 0) sep += allele_tiles(P, L->hp[(size_t)tgt[t]].len2, c0.k, (*mode)[(size_t)tgt[t]]);
        if (allele_tiles(P, st.len, c0.k, md) >= sep) continue;           // (a shared sequence of more tiles than its targets together: no gain)
        const auto mp = build_maps(c0.group, c0.k);
        if (mp.second <= 0) continue;
        DPair d;
        memset(&d, 0, sizeof d);
        d.seq1 = c0.seq1; d.seq2 = g.t_seq; d.off2 = 0; d.k = c0.k; d.flags = 0;
        d.len1 = s1.len; d.len2 = st.len;
        d.cap = pair_slot_cap(s1.len, st.len, P.max_pair_cap);
        DShare sh;
        memset(&sh, 0, sizeof sh);
        sh.dpair = (int32_t)L->hp.size();
        sh.iv_first = mp.first; sh.n_iv = mp.second;
        bool counted = false;
        for (int t = 0; t < 4; ++t) {
            sh.target[t] = tgt[t];
            if (tgt[t] >= 0) {
                served[(size_t)tgt[t]] = 1; ++L->n_served;
                DServe& sv = L->serve[(size_t)tgt[t]];
                sv.dpair = sh.dpair; sv.iv_first = sh.iv_first; sv.n_iv = sh.n_iv; sv.slot = t;      // (slot and cap of the join: plan_alloc_hits)
                sv.pad = counted ? 0 : 1;          // (the target whose clean workgroup counts an overflow of the SHARED plot: once per plot)
                counted = true;
            }
        }
        L->hp.push_back(d);
        mode->push_back((uint8_t)md);
        L->shares.push_back(sh);
    }
    if (!L->shares.empty()) {
        std::vector<int32_t> kept;
        kept.reserve(order->size());
        for (int32_t x : *order) if (!served[(size_t)x]) kept.push_back(x);
        for (size_t t = 0; t < L->shares.size(); ++t) kept.push_back((int32_t)(n_pairs + (int64_t)t));
        order->swap(kept);
    }
}

// The planner's cost units: probing a read against the tiles of an allele, and building an allele's table
inline int64_t probe_cost(const PlanParams& P, const SetView& S, const DPair& d, int k, int m)
{
    return (int64_t)S.h[d.seq1].len * allele_tiles(P, S.h[d.seq2].len, k, m) + 256;
}
inline int64_t build_cost(const SetView& S, const DPair& d) { return (VAPOR_BUILD_COST_X8 * (int64_t)S.h[d.seq2].len) / 8; }

// The tasks of one launch: pairs task_pairs[q, e), all of mode m and one k, sorted by allele.
// Cost of a range of consecutive pairs = its probe passes + one table build for its first allele + one for
// every further allele it reaches into.  The ranges are the contiguous partition into at most `want`
// pieces whose most expensive piece is cheapest (binary search on that bound, greedy packing under it).
inline void plan_launch_tasks(const PlanParams& P, const SetView& S, size_t q, size_t e, int m, PlanLayout* L)
{
    const std::vector<int32_t>& order = L->task_pairs;
    const int k = L->hp[order[q]].k;
    const size_t n = e - q;
    std::vector<int64_t> probe(n), build(n);
    int64_t total = 0, biggest = 0;
    for (size_t t = q; t < e; ++t) {
        const DPair& d = L->hp[order[t]];
        probe[t - q] = probe_cost(P, S, d, k, m);
        build[t - q] = build_cost(S, d);
        total += probe[t - q] + build[t - q];
        biggest = std::max(biggest, probe[t - q] + build[t - q]);
    }
    // `join_tasks` ranges (one per CU) - or, when the limit of reads per task asks for more than that, WHOLE ROUNDS of them: a
    // launch of 625 tasks on 256 CUs takes three rounds' time for 2.44 rounds' work (BASELINE configs[2]: 40 000 reads in
    // tasks of at most 64), 768 equal tasks take three rounds of 52 reads each - join 2.42 -> 2.10 ms with one plan in flight
    // (profiles/r05_join_rounds.txt; with two plans in flight the other plan's clean kernel filled that tail already)
    int64_t want = std::max<int64_t>(1, std::min<int64_t>((int64_t)n, P.join_tasks));
    {
        const int64_t need = ((int64_t)n + P.reads_per_task - 1) / P.reads_per_task;
        if (need > want) want = std::min<int64_t>((int64_t)n, (need + want - 1) / want * want);
    }
    // (what a pair adds to a range it does not start: its probe, and a table build when it brings a new allele)
    std::vector<int64_t> inside(n);
    for (size_t t = 0; t < n; ++t)
        inside[t] = probe[t] + ((t > 0 && L->hp[order[q + t]].seq2 != L->hp[order[q + t - 1]].seq2) ? build[t] : 0);
    // number of ranges a bound needs (cuts[] = first pair of every range when asked for)
    auto pack = [&](int64_t bound, std::vector<size_t>* cuts) {
        int64_t ranges = 0, acc = 0;
        size_t t0 = 0;
        for (size_t t = 0; t < n; ++t) {
            const int64_t add = t == t0 ? probe[t] + build[t] : inside[t];
            const bool full = (int)(t - t0) >= P.reads_per_task;
            if (t > t0 && (acc + add > bound || full)) {
                ++ranges;
                if (cuts) cuts->push_back(t0);
                t0 = t;
                acc = probe[t] + build[t];
            } else {
                acc += add;
            }
        }
        ++ranges;
        if (cuts) cuts->push_back(t0);
        return ranges;
    };
    // the smallest bound that needs at most `want` ranges: no partition can do with less than the costs inside
    // ranges shared out evenly, a doubling search finds a bound that is enough, bisection the smallest between
    int64_t in_sum = 0;
    for (size_t t = 0; t < n; ++t) in_sum += inside[t];
    int64_t lo = std::max(biggest, in_sum / want), hi = lo;
    while (hi < total && pack(hi, nullptr) > want) { lo = hi + 1; hi = std::min(total, hi * 2); }
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (pack(mid, nullptr) <= want) hi = mid; else lo = mid + 1;
    }
    std::vector<size_t> cuts;
    pack(lo, &cuts);
    L->launches.push_back(launch_of_mode(m, k, (int)L->tasks.size()));
    for (size_t c = 0; c < cuts.size(); ++c) {
        const size_t t0 = q + cuts[c], t1 = q + (c + 1 < cuts.size() ? cuts[c + 1] : n);
        DTask tk;
        tk.seq2 = L->hp[order[t0]].seq2; tk.k = k; tk.n_reads = (int32_t)(t1 - t0); tk.first = (int32_t)t0;
        L->tasks.push_back(tk);
        L->launches.back().n_tasks++;
    }
}

// The same launch cut at allele boundaries: every task holds pairs of ONE allele, so that a workgroup builds one table (per tile)
// and no table is built again by the neighbour that a cost-balanced range reaches into.  A group is the pairs of one allele; a
// range of it costs its probes plus one build.  Under a bound a group needs the fewest ranges greedy packing gives (reads are
// indivisible, at most reads_per_task a range); the launch takes the smallest bound whose groups need at most `join_tasks`
// ranges together (bisection, as above) - or, when the groups' fewest ranges are more than that already (more windows than CUs),
// those fewest - and every group is then cut into exactly the ranges that bound needs, as evenly as that many ranges allow:
// ranges beyond them would be builds for nothing.
// "No table built twice" therefore holds between windows, not inside one: the smallest bound uses the tasks `join_tasks` offers,
// so a launch of fewer groups than that cuts its groups further - down to one read a task when the tasks suffice (a launch of
// four reads of one window and join_tasks 7: four tasks, four builds of the one table, where one task would build it once; cfg2's
// 250 tasks for 100 windows are the same rule).  Those builds run side by side on CUs that would stand idle, so they shorten the
// launch and cost CU-time; the table's model carries them (TableModel::sum), and the library takes the aligned table only where
// that sum still comes out below the balanced table's (join_align_pays).
inline void plan_launch_aligned(const PlanParams& P, const SetView& S, size_t q, size_t e, int m, PlanLayout* L)
{
    const std::vector<int32_t>& order = L->task_pairs;
    const int k = L->hp[order[q]].k;
    const size_t n = e - q;
    std::vector<int64_t> probe(n);
    std::vector<size_t> group{0};                     // first pair of every group, then n
    int64_t total = 0, biggest = 0;
    for (size_t t = 0; t < n; ++t) {
        const DPair& d = L->hp[order[q + t]];
        probe[t] = probe_cost(P, S, d, k, m);
        if (t > 0 && d.seq2 != L->hp[order[q + t - 1]].seq2) group.push_back(t);
        total += probe[t] + build_cost(S, d);
        biggest = std::max(biggest, probe[t] + build_cost(S, d));
    }
    group.push_back(n);
    const size_t n_g = group.size() - 1;
    // ranges group g needs under a bound (cuts[] = first pair of every range when asked for)
    auto pack = [&](size_t g, int64_t bound, std::vector<size_t>* cuts) {
        const int64_t build = build_cost(S, L->hp[order[q + group[g]]]);
        int64_t ranges = 0, acc = 0;
        size_t t0 = group[g];
        for (size_t t = group[g]; t < group[g + 1]; ++t) {
            if (t > t0 && (acc + probe[t] > bound || (int)(t - t0) >= P.reads_per_task)) {
                ++ranges;
                if (cuts) cuts->push_back(t0);
                t0 = t;
                acc = 0;
            }
            if (t == t0) acc = build;
            acc += probe[t];
        }
        if (cuts) cuts->push_back(t0);
        return ranges + 1;
    };
    auto pack_all = [&](int64_t bound) {
        int64_t ranges = 0;
        for (size_t g = 0; g < n_g; ++g) ranges += pack(g, bound, nullptr);
        return ranges;
    };
    const int64_t want = std::max(1, P.join_tasks);
    int64_t lo = biggest, hi = total;                 // (under `total` only reads_per_task cuts a group)
    if (pack_all(hi) <= want)
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (pack_all(mid) <= want) hi = mid; else lo = mid + 1;
        }
    const int64_t bound = hi;
    L->alaunches.push_back(launch_of_mode(m, k, (int)L->atasks.size()));
    std::vector<size_t> cuts;
    for (size_t g = 0; g < n_g; ++g) {
        // the group's own smallest bound for the ranges the launch's bound gives it
        const int64_t m_g = pack(g, bound, nullptr);
        int64_t glo = 0, ghi = bound;
        for (size_t t = group[g]; t < group[g + 1]; ++t) glo = std::max(glo, probe[t]);
        glo += build_cost(S, L->hp[order[q + group[g]]]);
        while (glo < ghi) {
            const int64_t mid = glo + (ghi - glo) / 2;
            if (pack(g, mid, nullptr) <= m_g) ghi = mid; else glo = mid + 1;
        }
        cuts.clear();
        pack(g, ghi, &cuts);
        for (size_t c = 0; c < cuts.size(); ++c) {
            const size_t t0 = q + cuts[c], t1 = q + (c + 1 < cuts.size() ? cuts[c + 1] : group[g + 1]);
            DTask tk;
            tk.seq2 = L->hp[order[t0]].seq2; tk.k = k; tk.n_reads = (int32_t)(t1 - t0); tk.first = (int32_t)t0;
            L->atasks.push_back(tk);
            L->alaunches.back().n_tasks++;
        }
    }
}

inline int mode_of_launch(const Launch& la) { return la.bps == 4 ? 4 : (la.exc == 1 ? 3 : la.exc == 2 ? 5 : 2); }

// A task table of the layout in the planner's cost units
inline TableModel table_model(const PlanParams& P, const SetView& S, const PlanLayout& L, const std::vector<DTask>& tasks,
                              const std::vector<Launch>& launches)
{
    TableModel M;
    for (const Launch& la : launches) {
        const int m = mode_of_launch(la);
        int64_t dearest = 0;
        for (int x = 0; x < la.n_tasks; ++x) {
            const DTask& tk = tasks[(size_t)(la.task_begin + x)];
            int64_t cost = 0;
            for (int32_t t = tk.first; t < tk.first + tk.n_reads; ++t) {
                const DPair& d = L.hp[(size_t)L.task_pairs[(size_t)t]];
                cost += probe_cost(P, S, d, la.k, m);
                if (t == tk.first || d.seq2 != L.hp[(size_t)L.task_pairs[(size_t)t - 1]].seq2) {
                    cost += build_cost(S, d);
                    M.builds += allele_tiles(P, S.h[d.seq2].len, la.k, m);
                }
            }
            M.sum += cost;
            dearest = std::max(dearest, cost);
        }
        M.path += dearest;
        M.n_tasks += la.n_tasks;
    }
    return M;
}

// The window-aligned table of a layout beside its cost-balanced one: launch by launch over the same pairs.  plan_layout makes it
// when PlanParams::align_tasks asks for it; a caller that may never need it makes it later, with the parameters of the layout.
inline void plan_aligned(const PlanParams& P, const SetView& S, PlanLayout* L)
{
    L->atasks.clear();
    L->alaunches.clear();
    for (const Launch& la : L->launches) {
        const DTask &t0 = L->tasks[(size_t)la.task_begin], &t1 = L->tasks[(size_t)(la.task_begin + la.n_tasks - 1)];
        plan_launch_aligned(P, S, (size_t)t0.first, (size_t)(t1.first + t1.n_reads), mode_of_launch(la), L);
    }
    L->model[1] = table_model(P, S, *L, L->atasks, L->alaunches);
}

// The plan of `pairs` over a sequence set, everything but its device blocks.
inline PlanLayout plan_layout(const PlanParams& P, const SetView& S, int64_t n_pairs, const vapor_pair* pairs)
{
    PlanLayout L;
    std::vector<int32_t> order;
    std::vector<uint8_t> mode;
    plan_pairs(P, S, n_pairs, pairs, &L, &mode, &order);
    if (P.shared_join && !S.groups.empty() && n_pairs > 0) plan_shared_joins(P, S, n_pairs, &L, &mode, &order);
    // Sort by (mode, k, allele): one launch per (mode, k); inside a launch the sorted pair list is
    // cut into contiguous, cost-balanced ranges (tasks).  A workgroup rebuilds its allele hash table
    // only where the allele changes inside its range.
    // (the three fields packed into one word per pair, the index behind it: the comparisons touch nothing else)
    {
        std::vector<std::pair<uint64_t, int32_t>> keyed(order.size());
        for (size_t t = 0; t < order.size(); ++t) {
            const int32_t x = order[t];
            keyed[t] = {((uint64_t)mode[(size_t)x] << 48) | ((uint64_t)(uint32_t)L.hp[(size_t)x].k << 32) | (uint32_t)L.hp[(size_t)x].seq2, x};
        }
        std::sort(keyed.begin(), keyed.end());
        for (size_t t = 0; t < order.size(); ++t) order[t] = keyed[t].second;
    }
    L.task_pairs = std::move(order);
    const std::vector<int32_t>& tp = L.task_pairs;
    for (size_t q = 0; q < tp.size();) {
        size_t e = q;
        const int m = mode[tp[q]], k = L.hp[tp[q]].k;
        while (e < tp.size() && mode[tp[e]] == m && L.hp[tp[e]].k == k) ++e;
        plan_launch_tasks(P, S, q, e, m, &L);
        q = e;
    }
    L.model[0] = table_model(P, S, L, L.tasks, L.launches);
    if (P.align_tasks) plan_aligned(P, S, &L);
    return L;
}

// The clean kernel is one workgroup per pair, dealt out in grid order, a few per CU at a time: a plan of a couple of rounds of
// them (4 000 pairs at seven or eight per CU: two rounds and a bit) ends when the LAST round's slowest workgroup does, so the
// pairs that take longest go first and the tail is made of the shortest (longest-processing-time order; measured on cfg2: clean
// 0.091 -> 0.079 ms, profiles/r05_clean_order.txt).  What a pair takes: its records - about the shorter sequence's length -
// times the passes its flags ask for: C1 two clusterings, C2 one or two more, the directed statistics five passes over the kept
// records, plus the cutting of a served pair.  Pairs of equal cost keep their order (a read's two pairs lie side by side and
// read the same shared plot); sorting by the record counts a blocking run measured instead was tried and is no better - it
// scatters those neighbours (0.0738 -> 0.0749 ms) - so the library does not use it.
inline int64_t clean_cost(const PlanLayout& L, int64_t i)
{
    const DPair& d = L.hp[(size_t)i];
    const bool c1 = d.flags & VAPOR_PF_C1, c2 = d.flags & VAPOR_PF_C2, dir = (d.flags & VAPOR_PF_DIR) && c1;
    int64_t w = 4 + (c1 ? 8 : 0) + (c2 ? (c1 ? 5 : 8) : 0) + (dir ? 7 : 0);
    if (!L.serve.empty() && L.serve[(size_t)i].dpair >= 0) w += L.serve[(size_t)i].slot == 0 ? 2 : 4;
    const int64_t size = std::min<int64_t>(d.len1, std::max(0, d.len2 - d.off2));
    return L.status[(size_t)i] == 0 ? w * size : 0;
}
// the caller's pairs (0 .. n_pairs - 1), most expensive first
inline std::vector<int32_t> clean_order(const PlanLayout& L, int64_t n_pairs)
{
    std::vector<std::pair<int64_t, int32_t>> cost((size_t)n_pairs);
    for (int64_t i = 0; i < n_pairs; ++i) cost[(size_t)i] = {-clean_cost(L, i), (int32_t)i};
    std::stable_sort(cost.begin(), cost.end());
    std::vector<int32_t> ord((size_t)n_pairs);
    for (int64_t i = 0; i < n_pairs; ++i) ord[(size_t)i] = cost[(size_t)i].second;
    return ord;
}

}  // namespace vapor
