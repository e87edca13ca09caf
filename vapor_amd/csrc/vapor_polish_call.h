// vapor_polish_call.h - the host plan of one vapor_realign_polish / vapor_realign_revote call, without HIP:
// everything the entry computes before its first allocation and after its one synchronisation.  The call's checks in their order
// (check_args), the pair, locus and vote records with the statuses a refused locus hands down, the re-vote's allele of every locus,
// the groups with every offset relative to its group, where a group's stagings land in the host copy the spelt output is dealt from,
// the one upload image with each table's place stated once (Table), and the dealing itself (deal_spelt).  The rules it puts together
// are vapor_polish_plan.h's and vapor_revote_plan.h's; tools/polish_check.cpp and tools/revote_check.cpp hold the assembled plan to
// direct statements on the host under the sanitizers.  The entry in vapor_hip.hip is allocations, one upload, the launches, the
// copies back and one synchronisation.
#pragma once

#include "vapor_image.h"
#include "vapor_revote_plan.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace vapor_polish_call {

namespace ra = vapor_realign;
namespace tr = vapor_trace;
namespace pp = vapor_polish;
namespace vr = vapor_revote;

// why a call is refused (here: the message without the entry's name, the entry prepends "<name>: "), and the upload image's tables,
// every one starting on 8 bytes (vapor_image.h; vapor_realign_trace carves its two tables the same way)
using vapor_image::Carve;
using vapor_image::Refusal;
using vapor_image::Table;

// the set as the plan headers' helpers take it: sequences, the length and the first 32-symbol chunk of sequence s
template <typename LenOf, typename ChunkOf>
struct Seqs {
    int32_t n;
    LenOf len_of;
    ChunkOf chunk_of;
};
template <typename LenOf, typename ChunkOf>
inline Seqs<LenOf, ChunkOf> seqs(int32_t n, LenOf len_of, ChunkOf chunk_of) { return {n, len_of, chunk_of}; }

// the refusals every realign entry makes first, in their order; handles: context and set are there, args_ok: so are the pointers
// a call with pairs needs
inline Refusal realign_args(bool handles, int64_t n_pairs, bool args_ok, int32_t band)
{
    if (!handles || n_pairs < 0 || n_pairs > ra::MAX_PAIRS || (n_pairs && !args_ok))
        return {VAPOR_E_ARG, "null argument or a pair count outside 0 .. 2^26"};
    if (!ra::band_ok(band)) return {VAPOR_E_ARG, "band outside 1 .. VAPOR_MAX_BAND"};
    return {};
}

// what vapor_realign_revote adds to vapor_realign_polish's arguments
struct RevoteArgs {
    int64_t n_votes;
    const vapor_pair* votes;
    const int64_t* vfirst;
    int32_t *vout, *lout;
    const int64_t* spelt_off;
    uint8_t* spelt;
};

// A call as either entry states it.  handles: context and set are there; rv: null for the polish alone.
struct Call {
    bool handles;
    int64_t n_pairs;
    const vapor_pair* pairs;
    int32_t band;
    int64_t n_loci;
    const int64_t *first, *col_off;
    int32_t* stats;
    uint8_t* calls;
    int32_t* sites;
    uint8_t* ins;
    uint32_t* counts;
    const RevoteArgs* rv;
};

// The call's checks, in their order.  nothing: the call is not refused and has nothing to run - no pairs, loci or vote pairs at
// all, or, once the tables have passed, no locus.
inline Refusal check_args(const Call& c, bool& nothing)
{
    const RevoteArgs* rv = c.rv;
    nothing = false;
    if (const Refusal no = realign_args(c.handles, c.n_pairs, c.pairs != nullptr, c.band)) return no;
    if (c.n_loci < 0 || c.n_loci > ra::MAX_PAIRS) return {VAPOR_E_ARG, "a locus count outside 0 .. 2^26"};
    if (rv && (rv->n_votes < 0 || rv->n_votes > ra::MAX_PAIRS)) return {VAPOR_E_ARG, "a vote pair count outside 0 .. 2^26"};
    if (c.n_loci == 0 && c.n_pairs == 0 && (!rv || rv->n_votes == 0)) {
        nothing = true;
        return {};
    }
    if (!pp::tables_ok(c.n_pairs, c.n_loci, c.first, c.col_off))
        return {VAPOR_E_ARG, "first / col_off must ascend from 0, first must end at n_pairs, a locus has at most VAPOR_MAX_SEQ_LEN columns"};
    if (rv && !vr::vfirst_ok(rv->n_votes, c.n_loci, rv->vfirst)) return {VAPOR_E_ARG, "vfirst must ascend from 0 to n_votes"};
    if (rv && rv->spelt && !vr::spelt_off_ok(c.n_loci, rv->spelt_off)) return {VAPOR_E_ARG, "spelt_off must ascend from 0"};
    if (c.n_loci == 0) {
        nothing = true;
        return {};
    }
    if (!c.stats || !c.sites || !c.ins || (c.col_off[c.n_loci] && !c.calls)) return {VAPOR_E_ARG, "null output"};
    if (rv && (!rv->lout || (rv->n_votes && (!rv->votes || !rv->vout)))) return {VAPOR_E_ARG, "null output"};
    return {};
}

// The plan of a call that passed check_args with something to run.  The vectors are what the image is filled from; the re-vote's
// (vloci, vrecs, the stagings) are empty for the polish alone.
struct Plan {
    std::vector<ra::RPair> recs;           // a pair of a refused locus carries the locus's status, unless it has one of its own
    std::vector<uint64_t> off;             // a pair's first trace dword inside its group's workspace
    std::vector<pp::PLocus> loci;          // col0 relative to the group
    std::vector<int32_t> pair_locus;       // a pair's locus among its group's loci
    std::vector<vr::VLocus> vloci;
    std::vector<vr::VPair> vrecs;          // `locus` among the group's loci; the vote pairs of a refused locus say why
    std::vector<pp::Group> groups;
    int64_t most = 0;                      // dwords of the largest group's buffer
    // per group: where its stagings start in its buffer, their dwords, and where they land in the host copy (`staged_words` in
    // all; the host copy exists only when the spelt output is asked for)
    std::vector<int64_t> stage_base, stage_words, stage_host;
    int64_t staged_words = 0;
    // the upload image, in this order
    Table<ra::RPair> t_recs;
    Table<uint64_t> t_off;
    Table<pp::PLocus> t_loci;
    Table<int32_t> t_pair_locus;
    Table<vr::VLocus> t_vloci;
    Table<vr::VPair> t_vrecs;
    std::vector<uint8_t> image;

    template <typename S>
    Plan(const Call& c, const S& set, int64_t trace_budget)
    {
        const RevoteArgs* rv = c.rv;
        const int W = ra::lane_width(c.band);
        const int64_t n_pairs = c.n_pairs, n_loci = c.n_loci;
        const size_t np = (size_t)n_pairs, nl = (size_t)n_loci, nv = rv ? (size_t)rv->n_votes : 0;
        recs.resize(np);
        for (size_t t = 0; t < np; ++t) recs[t] = ra::pair_record(c.pairs[t], set.n, set.len_of, set.chunk_of);
        // the loci: status, trace words, run cap
        loci.resize(nl);
        pair_locus.resize(np);
        std::vector<int64_t> twords(nl), cap(nl);
        for (int64_t g = 0; g < n_loci; ++g) {
            const int64_t a = c.first[g], b = c.first[g + 1], span = c.col_off[g + 1] - c.col_off[g];
            const int status = pp::locus_status(recs.data(), a, b, span, c.band, W, trace_budget, [&](int64_t t) { return c.pairs[t].seq2; },
                                                [&](int64_t t) { return (int64_t)set.len_of(c.pairs[t].seq2); }, twords[(size_t)g]);
            pp::PLocus& lc = loci[(size_t)g];
            lc = pp::PLocus{};
            lc.len = (int32_t)span;
            lc.n_pairs = (int32_t)(status ? 0 : b - a);
            lc.status = status;
            lc.word2 = (!status && b > a) ? recs[(size_t)a].word2 : 0;
            cap[(size_t)g] = 1;
            for (int64_t t = a; t < b; ++t) {
                if (status) recs[(size_t)t].status = recs[(size_t)t].status ? recs[(size_t)t].status : status;     // (no pair of a refused locus runs)
                cap[(size_t)g] = std::max(cap[(size_t)g], pp::run_cap(recs[(size_t)t]));
            }
        }
        // the re-vote's loci and vote pairs: a locus's allele is its pairs' seq2, else that of its first vote pair that fits its columns
        std::vector<int64_t> extra(rv ? nl : 0), spans(rv ? nl : 0);
        vloci.resize(rv ? nl : 0);
        vrecs.resize(nv);
        for (int64_t g = 0; rv && g < n_loci; ++g) {
            const int64_t a = c.first[g], b = c.first[g + 1], va = rv->vfirst[g], vb = rv->vfirst[g + 1], span = c.col_off[g + 1] - c.col_off[g];
            vr::VLocus& vl = vloci[(size_t)g];
            vl = vr::VLocus{};
            vl.status = loci[(size_t)g].status;
            int64_t allele = -1;
            if (!vl.status && b > a) allele = c.pairs[a].seq2;
            for (int64_t t = va; t < vb && !vl.status && allele < 0; ++t)
                if (!ra::pair_status(rv->votes[t], set.n, set.len_of) && (int64_t)set.len_of(rv->votes[t].seq2) == span) allele = rv->votes[t].seq2;
            if (!vl.status && allele < 0) vl.status = VAPOR_E_ARG;
            if (!vl.status) {
                vl.word2 = (uint64_t)set.chunk_of((int32_t)allele) * 4u;
                vl.cap = (int32_t)vr::spelt_cap(span);
                vl.short_slot = rv->spelt && !vr::slot_ok(rv->spelt_off[g + 1] - rv->spelt_off[g], span);
                extra[(size_t)g] = vr::locus_extra(span);
            }
            spans[(size_t)g] = span;
            for (int64_t t = va; t < vb; ++t) {
                vrecs[(size_t)t] = vr::vote_record(rv->votes[t], set.n, allele, 0, set.len_of, set.chunk_of);
                if (vl.status) vrecs[(size_t)t].status = vl.status;       // (the pairs of a refused locus say why)
            }
        }
        most = pp::plan_groups(n_loci, c.first, c.col_off, twords.data(), cap.data(), trace_budget, groups, rv ? extra.data() : nullptr);
        // the pairs' workspace offsets, their loci and the loci's columns, relative to their group (the two trace kernels are launched
        // with the group's pointers and t0 = 0)
        off.assign(np, 0);
        for (const pp::Group& gr : groups) {
            uint64_t used = 0;
            for (int64_t t = gr.pair0; t < gr.pair1; ++t) {
                const ra::RPair& r = recs[(size_t)t];
                off[(size_t)t] = used;
                if (!r.status) used += (uint64_t)tr::pair_words(ra::rows_walked(r.n, r.m, c.band), W);
            }
            for (int64_t g = gr.locus0; g < gr.locus1; ++g) {
                loci[(size_t)g].col0 = c.col_off[g] - c.col_off[gr.locus0];
                for (int64_t t = c.first[g]; t < c.first[g + 1]; ++t) pair_locus[(size_t)t] = (int32_t)(g - gr.locus0);
                if (rv)
                    for (int64_t t = rv->vfirst[g]; t < rv->vfirst[g + 1]; ++t) vrecs[(size_t)t].locus = (int32_t)(g - gr.locus0);
            }
        }
        // the re-vote's pieces inside every group's buffer, and where a group's stagings land in the host copy
        const size_t ng = rv ? groups.size() : 0;
        stage_base.resize(ng);
        stage_words.resize(ng);
        stage_host.resize(ng);
        for (size_t k = 0; k < ng; ++k) {
            const pp::Group& gr = groups[k];
            const size_t l0 = (size_t)gr.locus0;
            const int64_t gl = gr.locus1 - gr.locus0;
            vr::place(gr.extra_off, gl, spans.data() + l0, extra.data() + l0, vloci.data() + l0, stage_base[k]);
            stage_words[k] = gl ? vloci[l0].plane_off - stage_base[k] : 0;
            stage_host[k] = staged_words;
            if (rv->spelt) staged_words += stage_words[k];
        }
        Carve carve;
        carve.take(t_recs, np);
        carve.take(t_off, np);
        carve.take(t_loci, nl);
        carve.take(t_pair_locus, np);
        carve.take(t_vloci, vloci.size());
        carve.take(t_vrecs, nv);
        image.resize(carve.off);
        t_recs.fill(image, recs);
        t_off.fill(image, off);
        t_loci.fill(image, loci);
        t_pair_locus.fill(image, pair_locus);
        t_vloci.fill(image, vloci);
        t_vrecs.fill(image, vrecs);
    }

    // The spelt codes, dealt to the caller's slots after the call's synchronisation: plen bytes (lout's, never more than the
    // locus's cap) of every locus that was spelt and whose slot holds them, from the host copy of its group's stagings.
    void deal_spelt(const uint32_t* staged, const int32_t* lout, const int64_t* spelt_off, uint8_t* spelt) const
    {
        for (size_t k = 0; spelt && k < stage_base.size(); ++k) {
            const pp::Group& gr = groups[k];
            for (int64_t g = gr.locus0; g < gr.locus1; ++g) {
                const vr::VLocus& vl = vloci[(size_t)g];
                if (vl.status || vl.short_slot) continue;
                const int64_t plen = std::min<int64_t>(lout[vr::LOUT * g + vr::L_PLEN], vl.cap);
                if (plen > 0)
                    memcpy(spelt + spelt_off[g], reinterpret_cast<const uint8_t*>(staged + stage_host[k] + (vl.stage_off - stage_base[k])), (size_t)plen);
            }
        }
    }
};

}  // namespace vapor_polish_call
