// seqset_check.cpp - the host plan of a vapor_seqset_create* call (vapor_amd/csrc/vapor_seqset_plan.h) on a CPU, against direct
// statements: every refusal of every entry with its code and text, and among several faults the one a plain transcription of the
// entries' checks meets first; the size limits on both sides, with made-up lengths and no bytes; on drawn sets where every sequence
// lies in the planes, the staging image table by table (the ASCII, the maps, the mixed block, the derived tables spelt through the
// parents' first chunks), its size by the formula written out, the threaded staging for every thread count against the image one
// thread makes, and what follows the counts.  The sets come from fixed seeds; nothing is compared with recorded output.  A literal
// the device holds points into a page that cannot be read, so that a byte of it read on the host ends the program.
// Built and run by tests/test_seqset_cpu.py:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ivapor_amd/csrc tools/seqset_check.cpp
// and the slices a second time (argument "slices") with -fsanitize=thread.
#include "seq_spell.h"
#include "vapor_seqset_plan.h"

#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>

using namespace vapor;
namespace sp = vapor_seqset_plan;
using sp::Call;
using sp::Refusal;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (case %ld)\n", g_case); exit(1); } } while (0)

static std::mt19937_64 rng(20251021);
static long g_case = 0;
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); }      // lo .. hi
static bool one_in(int n) { return rng() % (uint64_t)n == 0; }

static const uint8_t* g_unreadable = nullptr;      // a page no read survives: where device-held literals "lie"
static const size_t UNREADABLE_BYTES = (size_t)1 << 20;

static std::string dna(int n)
{
    std::string s((size_t)n, 'A');
    for (char& c : s) c = "ACGTacgtNnRX"[rng() % 12];
    return s;
}

// ---- a set as a caller states it ----
struct Set {
    std::vector<std::string> text;                 // of the literals (of a device-held one: what the device would expand; no pointer leads to it)
    std::vector<int32_t> len;
    std::vector<uint8_t> flags, kind, dflags;
    std::vector<int64_t> first;
    std::vector<const uint8_t*> ptr;
    std::string blob;
    std::vector<int64_t> off;
    std::vector<int32_t> seg_first{0};
    std::vector<vapor_segment> segs;
    bool any_dev = false;

    void literal(const std::string& t, uint8_t fl = 0, int src_kind = 0)
    {
        text.push_back(t);
        len.push_back((int32_t)t.size());
        flags.push_back(fl);
        kind.push_back((uint8_t)src_kind);
        any_dev = any_dev || src_kind;
        // (kind 2 reads downwards from its first base)
        first.push_back(src_kind == 0 ? 0 : src_kind == 1 ? rnd(0, 1000) : (int64_t)t.size() - 1 + rnd(0, 1000));
    }
    void derived_seq(const std::vector<vapor_segment>& sg, uint8_t fl)
    {
        segs.insert(segs.end(), sg.begin(), sg.end());
        seg_first.push_back((int32_t)segs.size());
        dflags.push_back(fl);
    }
    // pointers and the blob, once the texts stand (a device-held literal: somewhere in the unreadable page)
    void seal()
    {
        blob.clear();
        off.clear();
        for (const std::string& t : text) { blob += "**"; off.push_back((int64_t)blob.size()); blob += t; }
        blob += "*";
        segs.reserve(1);                           // (derived sequences without a segment still need a segment pointer)
        ptr.clear();
        for (size_t i = 0; i < text.size(); ++i)
            ptr.push_back(kind[i] ? g_unreadable + rnd(0, 4000) : reinterpret_cast<const uint8_t*>(text[i].data()));
    }
    int32_t n_derived() const { return (int32_t)dflags.size(); }
    Call call(sp::Entry e) const
    {
        const bool der = e == sp::DERIVED || e == sp::MIXED;
        return Call{e, true, (int32_t)text.size(), e == sp::BLOB ? reinterpret_cast<const uint8_t*>(blob.data()) : nullptr, e == sp::BLOB ? off.data() : nullptr,
                    e == sp::BLOB ? nullptr : ptr.data(), len.data(), flags.data(), e == sp::MIXED ? kind.data() : nullptr, e == sp::MIXED ? first.data() : nullptr,
                    der ? n_derived() : 0, der ? seg_first.data() : nullptr, der ? segs.data() : nullptr, der ? dflags.data() : nullptr};
    }
};

static bool in_unreadable(const uint8_t* a, const uint8_t* b) { return a >= g_unreadable && b >= a && b < g_unreadable + UNREADABLE_BYTES; }

// what a call is refused with before a byte moves: the entry's checks, then the layout's
static Refusal refusal_of(const Call& c, bool shared_join = true)
{
    if (const Refusal no = sp::check_args(c, in_unreadable)) return no;
    sp::Layout L;
    return L.build(c, shared_join);
}

// ---- section 1: refusals ----
// The entries' checks as they were written before there was a plan: one function per entry, then the loops all of them shared.
static const char* naive_layout(const Call& c)
{
    uint64_t pl = 0;
    for (int32_t i = 0; i < c.n_seqs; ++i) {
        if (c.len[i] < 0) return "negative sequence length";
        pl += ((uint64_t)c.len[i] + 31) / 32 + 3;
        if (pl > 0xFFFFFFF0ull) return "sequence set too large";
    }
    for (int32_t d = 0; d < c.n_derived; ++d) {
        const int32_t g0 = c.seg_first[d], g1 = c.seg_first[d + 1];
        if (g1 < g0 || g1 - g0 > 16) return "vapor_seqset_create_derived: bad segment count";
        int64_t tot = 0;
        for (int32_t g = g0; g < g1; ++g) {
            const vapor_segment& x = c.segs[g];
            if (x.parent < 0 || x.parent >= c.n_seqs || x.off < 0 || x.len < 0 || (int64_t)x.off + x.len > c.len[x.parent])
                return "vapor_seqset_create_derived: segment outside its parent";
            if (x.len == 0) continue;
            if (c.flags && (c.flags[x.parent] & 1u) && !(c.derived_flags && (c.derived_flags[d] & 1u)))
                return "vapor_seqset_create_derived: a derived sequence without VAPOR_SEQ_UPPER over a parent uploaded with it";
            tot += x.len;
            if (tot > 0x7FFFFFF0LL) return "vapor_seqset_create_derived: sequence too long";
        }
    }
    return nullptr;
}
static const char* naive_refusal(const Call& c)
{
    const bool derived_ptrs = c.n_derived && (!c.seg_first || !c.segs);
    switch (c.entry) {
    case sp::BLOB:
        if (!c.handles || c.n_seqs < 0 || (c.n_seqs && (!c.blob || !c.off || !c.len))) return "vapor_seqset_create: null argument";
        break;
    case sp::PTRS:
        if (!c.handles || c.n_seqs < 0 || (c.n_seqs && (!c.seq || !c.len))) return "vapor_seqset_create_ptrs: null argument";
        for (int32_t i = 0; i < c.n_seqs; ++i)
            if (c.len[i] > 0 && !c.seq[i]) return "vapor_seqset_create_ptrs: null sequence";
        break;
    case sp::DERIVED:
        if (!c.handles || c.n_seqs < 0 || c.n_derived < 0 || (c.n_seqs && (!c.seq || !c.len)) || derived_ptrs) return "vapor_seqset_create_derived: null argument";
        if ((int64_t)c.n_seqs + c.n_derived > 0x7FFFFFF0LL) return "vapor_seqset_create_derived: too many sequences";
        for (int32_t i = 0; i < c.n_seqs; ++i)
            if (c.len[i] > 0 && !c.seq[i]) return "vapor_seqset_create_derived: null sequence";
        break;
    case sp::MIXED:
        if (!c.handles || c.n_seqs < 0 || c.n_derived < 0 || (c.n_seqs && (!c.seq || !c.len)) || derived_ptrs) return "vapor_seqset_create_mixed: null argument";
        if ((int64_t)c.n_seqs + c.n_derived > 0x7FFFFFF0LL) return "vapor_seqset_create_mixed: too many sequences";
        for (int32_t i = 0; i < c.n_seqs; ++i) {
            if (c.len[i] < 0) return "negative sequence length";
            if (c.len[i] > 0 && !c.seq[i]) return "vapor_seqset_create_mixed: null sequence";
            if (!c.src_kind || !c.src_kind[i]) continue;
            if ((c.src_kind[i] != 1 && c.src_kind[i] != 2) || !c.src_first || c.src_first[i] < 0 || c.src_first[i] > 0x7FFFFFF0LL ||
                (c.src_kind[i] == 2 && (int64_t)c.len[i] > c.src_first[i] + 1))
                return "vapor_seqset_create_mixed: bad source description";
            if (c.len[i] == 0) continue;
            const int64_t lo = c.src_kind[i] == 2 ? c.src_first[i] - c.len[i] + 1 : c.src_first[i];
            if (!in_unreadable(c.seq[i] + (lo >> 1), c.seq[i] + ((lo + c.len[i] - 1) >> 1))) return "vapor_seqset_create_mixed: a device source outside every live batch";
        }
        break;
    }
    return naive_layout(c);
}

// a good set of ten literals (two of them the device's for the mixed entry, one upper-cased) and four derived sequences
static Set good_set(bool mixed)
{
    Set s;
    for (int i = 0; i < 10; ++i) s.literal(dna(rnd(40, 200)), i == 7 ? VAPOR_SEQ_UPPER : 0, mixed && (i == 3 || i == 8) ? 1 + (i == 8) : 0);
    s.derived_seq({{0, 3, 20, 0}, {1, 0, 30, VAPOR_SEG_REVCOMP}}, 0);
    s.derived_seq({{7, 1, 10, 0}}, VAPOR_SEQ_UPPER);
    s.derived_seq({}, 0);
    s.derived_seq({{2, 0, 0, 0}, {4, 5, 25, 0}}, 0);
    s.seal();
    return s;
}

// A fault: what it spoils in a set or its call, what the entry must say, and which entries can be made to say it.
struct Fault {
    const char* name;
    unsigned entries;                              // bit e: entry e makes this refusal
    const char* msg[4];                            // per entry
    void (*spoil)(Set&, Call&, int at);            // `at`: the literal or derived sequence it is planted in
};
#define ALL4(tail) {"vapor_seqset_create: " tail, "vapor_seqset_create_ptrs: " tail, "vapor_seqset_create_derived: " tail, "vapor_seqset_create_mixed: " tail}
#define SAME4(text) {text, text, text, text}
static const unsigned B = 1u << sp::BLOB, P = 1u << sp::PTRS, D = 1u << sp::DERIVED, M = 1u << sp::MIXED;
static int32_t g_bad_first[2] = {5, 3};
// the first segment of derived sequence d (0, 1 and 3 have one), or of the only one another fault has left
static vapor_segment* seg_of(Set& s, int d) { return &s.segs[(size_t)d + 1 < s.seg_first.size() ? (size_t)s.seg_first[(size_t)d] : 0]; }
static const Fault FAULTS[] = {
    {"no handles", B | P | D | M, ALL4("null argument"), [](Set&, Call& c, int) { c.handles = false; }},
    {"n_seqs < 0", B | P | D | M, ALL4("null argument"), [](Set&, Call& c, int) { c.n_seqs = -1; }},
    {"no sources", B | P | D | M, ALL4("null argument"), [](Set&, Call& c, int) { c.blob = nullptr; c.seq = nullptr; }},
    {"no offsets", B, ALL4("null argument"), [](Set&, Call& c, int) { c.off = nullptr; }},
    {"no lengths", B | P | D | M, ALL4("null argument"), [](Set&, Call& c, int) { c.len = nullptr; }},
    {"n_derived < 0", D | M, ALL4("null argument"), [](Set&, Call& c, int) { c.n_derived = -1; }},
    {"no seg_first", D | M, ALL4("null argument"), [](Set&, Call& c, int) { c.seg_first = nullptr; }},
    {"no segments", D | M, ALL4("null argument"), [](Set&, Call& c, int) { c.segs = nullptr; }},
    {"too many", D | M, ALL4("too many sequences"), [](Set&, Call& c, int) { c.n_derived = 0x7FFFFFF0 - c.n_seqs + 1; }},
    {"null sequence", P | D | M, ALL4("null sequence"), [](Set& s, Call&, int at) { s.ptr[(size_t)at] = nullptr; }},
    {"negative length", B | P | D | M, SAME4("negative sequence length"), [](Set& s, Call&, int at) { s.len[(size_t)at] = -1 - rnd(0, 5); }},
    {"source kind 3", M, ALL4("bad source description"), [](Set& s, Call&, int at) { s.kind[(size_t)at] = 3; }},
    {"no first bases", M, ALL4("bad source description"), [](Set&, Call& c, int) { c.src_first = nullptr; }},
    {"first base < 0", M, ALL4("bad source description"), [](Set& s, Call&, int) { s.first[3] = -1; }},
    {"first base too far", M, ALL4("bad source description"), [](Set& s, Call&, int) { s.first[3] = 0x7FFFFFF1LL; }},
    {"kind 2 runs below base 0", M, ALL4("bad source description"), [](Set& s, Call&, int) { s.first[8] = s.len[8] - 2; }},
    {"before every batch", M, ALL4("a device source outside every live batch"), [](Set& s, Call&, int) { s.ptr[3] = g_unreadable - 600; }},
    {"ends behind its batch", M, ALL4("a device source outside every live batch"),
     [](Set& s, Call&, int) { s.ptr[8] = g_unreadable + UNREADABLE_BYTES - (s.first[8] >> 1); }},             // (its last byte is the first one outside)
    {"segments descend", D | M, SAME4("vapor_seqset_create_derived: bad segment count"), [](Set&, Call& c, int) { c.seg_first = g_bad_first; c.n_derived = 1; }},
    {"17 segments", D | M, SAME4("vapor_seqset_create_derived: bad segment count"),
     [](Set& s, Call& c, int) {
         s.segs.assign(17, vapor_segment{0, 0, 1, 0});
         s.seg_first = {0, 17};
         c.segs = s.segs.data(); c.seg_first = s.seg_first.data(); c.n_derived = 1;
     }},
    {"parent < 0", D | M, SAME4("vapor_seqset_create_derived: segment outside its parent"), [](Set& s, Call&, int at) { seg_of(s, at)->parent = -1; }},
    {"parent is no literal", D | M, SAME4("vapor_seqset_create_derived: segment outside its parent"), [](Set& s, Call&, int at) { seg_of(s, at)->parent = 10; }},
    {"segment offset < 0", D | M, SAME4("vapor_seqset_create_derived: segment outside its parent"), [](Set& s, Call&, int at) { seg_of(s, at)->off = -1; }},
    {"segment length < 0", D | M, SAME4("vapor_seqset_create_derived: segment outside its parent"), [](Set& s, Call&, int at) { seg_of(s, at)->len = -1; }},
    {"segment ends behind its parent", D | M, SAME4("vapor_seqset_create_derived: segment outside its parent"),
     [](Set& s, Call&, int at) {
         vapor_segment* x = seg_of(s, at);
         if (x->parent >= 0 && x->parent < (int32_t)s.len.size()) x->len = s.len[(size_t)x->parent] - x->off + 1;      // (else another fault has it outside already)
     }},
    {"not upper over upper", D | M, SAME4("vapor_seqset_create_derived: a derived sequence without VAPOR_SEQ_UPPER over a parent uploaded with it"),
     [](Set& s, Call&, int) { s.dflags[1] = 0; }},
};
static const int N_FAULTS = (int)(sizeof FAULTS / sizeof FAULTS[0]);

// where fault f may be planted: a host-held literal for the per-literal ones, a derived sequence with a segment for the segments'
static int place_of(int f)
{
    const std::string name = FAULTS[f].name;
    static const int host[8] = {0, 1, 2, 4, 5, 6, 7, 9}, with_seg[3] = {0, 1, 3};
    if (name == "null sequence" || name == "negative length" || name == "source kind 3") return host[rnd(0, 7)];
    return with_seg[rnd(0, 2)];
}

static long check_refusals(long& n_pairs)
{
    long singles = 0;
    for (int e = 0; e < 4; ++e) {
        {   // the good call is not refused
            const Set s = good_set(e == sp::MIXED);
            const Refusal no = refusal_of(s.call((sp::Entry)e));
            CHECK(!no && !naive_refusal(s.call((sp::Entry)e)), "entry %d refuses a good call: %s", e, no.msg);
        }
        for (int f = 0; f < N_FAULTS; ++f) {
            if (!(FAULTS[f].entries >> e & 1u)) continue;
            for (int rep = 0; rep < 4; ++rep) {
                ++g_case;
                Set s = good_set(e == sp::MIXED);
                Call c = s.call((sp::Entry)e);
                FAULTS[f].spoil(s, c, place_of(f));
                const Refusal no = refusal_of(c);
                CHECK(no.code == VAPOR_E_ARG && no.msg && std::string(no.msg) == FAULTS[f].msg[e], "entry %d, %s: code %d, \"%s\", not \"%s\"", e, FAULTS[f].name, no.code,
                      no.msg ? no.msg : "(none)", FAULTS[f].msg[e]);
                ++singles;
            }
            // two faults: the one the transcription meets first
            for (int g = 0; g < N_FAULTS; ++g) {
                if (g == f || !(FAULTS[g].entries >> e & 1u)) continue;
                for (int rep = 0; rep < 3; ++rep) {
                    ++g_case;
                    Set s = good_set(e == sp::MIXED);
                    Call c = s.call((sp::Entry)e);
                    FAULTS[f].spoil(s, c, place_of(f));
                    FAULTS[g].spoil(s, c, place_of(g));
                    const char* want = naive_refusal(c);
                    const Refusal no = refusal_of(c);
                    CHECK(want && no.code == VAPOR_E_ARG && no.msg && std::string(no.msg) == want, "entry %d, %s and %s: \"%s\", the transcription says \"%s\"", e,
                          FAULTS[f].name, FAULTS[g].name, no.msg ? no.msg : "(none)", want ? want : "(none)");
                    CHECK(std::string(want) == FAULTS[f].msg[e] || std::string(want) == FAULTS[g].msg[e], "neither fault's message: \"%s\"", want);
                    ++n_pairs;
                }
            }
        }
    }
    return singles;
}

// ---- section 2: the limits, with made-up lengths ----
struct Lengths {                                   // a call that is lengths and segments alone: every pointer to bytes is the unreadable page
    std::vector<int32_t> len;
    std::vector<const uint8_t*> ptr;
    std::vector<int32_t> seg_first{0};
    std::vector<vapor_segment> segs;
    Call call()
    {
        ptr.assign(len.size(), g_unreadable);
        const int32_t nd = (int32_t)seg_first.size() - 1;
        return Call{nd ? sp::DERIVED : sp::PTRS, true, (int32_t)len.size(), nullptr, nullptr, ptr.data(), len.data(), nullptr, nullptr, nullptr, nd,
                    nd ? seg_first.data() : nullptr, nd ? segs.data() : nullptr, nullptr};
    }
};
static void expect(Lengths& w, const char* want, const char* what)
{
    ++g_case;
    const Refusal no = refusal_of(w.call(), false);
    if (!want) { CHECK(!no, "%s is refused: %s", what, no.msg); return; }
    CHECK(no.code == VAPOR_E_ARG && no.msg && std::string(no.msg) == want, "%s: \"%s\", not \"%s\"", what, no.msg ? no.msg : "(none)", want);
}
static long check_limits()
{
    long n = 0;
    const int64_t full = (int64_t)1 << 26;                                           // chunks of a literal of 2^31 - 1 symbols
    // 63 literals of 2^26 chunks and one that fills the planes to 0xFFFFFFF0 chunks exactly, pads included
    const int64_t last = (int64_t)0xFFFFFFF0LL - 63 * (full + VP_PAD_CHUNKS) - VP_PAD_CHUNKS;
    CHECK(last > 0 && last <= full, "%ld chunks left", (long)last);
    {
        Lengths w;
        w.len.assign(63, 0x7FFFFFFF);
        w.len.push_back((int32_t)(last * 32));
        expect(w, nullptr, "literals of 0xFFFFFFF0 chunks");
        sp::Layout L;
        Call c = w.call();
        CHECK(!L.build(c, false) && L.plane_chunks == 0xFFFFFFF0ull + VP_PAD_CHUNKS + 1 && L.h[63].chunk0 == (uint32_t)(0xFFFFFFF0ull - VP_PAD_CHUNKS - (uint64_t)last),
              "%zu plane chunks", L.plane_chunks);
        w.len.back() += 1;
        expect(w, "sequence set too large", "literals of one chunk more");
        n += 2;
    }
    {   // the same chunks, all but the first literal's as derived sequences (each the first symbols of literal 0)
        Lengths w;
        w.len.push_back(0x7FFFFFFF);
        for (int d = 0; d < 62; ++d) { w.segs.push_back(vapor_segment{0, 0, 0x7FFFFFF0, 0}); w.seg_first.push_back((int32_t)w.segs.size()); }
        w.segs.push_back(vapor_segment{0, 0, (int32_t)(last * 32), 0});
        w.seg_first.push_back((int32_t)w.segs.size());
        CHECK(sp::chunks_of(0x7FFFFFF0) == (size_t)full, "a derived sequence of %zu chunks", sp::chunks_of(0x7FFFFFF0));
        expect(w, nullptr, "derived sequences to 0xFFFFFFF0 chunks");
        w.segs.back().len += 1;
        expect(w, "sequence set too large", "derived sequences of one chunk more");
        n += 2;
    }
    {   // a derived sequence of 0x7FFFFFF0 symbols, and of one more
        Lengths w;
        w.len.push_back(0x7FFFFFFF);
        w.segs = {vapor_segment{0, 0, 0x7FFFFFF0 - 10, 0}, vapor_segment{0, 7, 10, VAPOR_SEG_REVCOMP}};
        w.seg_first.push_back(2);
        expect(w, nullptr, "a derived sequence of 0x7FFFFFF0 symbols");
        w.segs[1].len = 11;
        expect(w, "vapor_seqset_create_derived: sequence too long", "a derived sequence of 0x7FFFFFF1 symbols");
        n += 2;
    }
    {   // VAPOR_MAX_SEGMENTS segments, and one more
        Lengths w;
        w.len.push_back(100);
        w.segs.assign(VAPOR_MAX_SEGMENTS, vapor_segment{0, 1, 2, 0});
        w.seg_first.push_back(VAPOR_MAX_SEGMENTS);
        expect(w, nullptr, "VAPOR_MAX_SEGMENTS segments");
        w.segs.push_back(vapor_segment{0, 1, 2, 0});
        w.seg_first.back() += 1;
        expect(w, "vapor_seqset_create_derived: bad segment count", "VAPOR_MAX_SEGMENTS + 1 segments");
        n += 2;
    }
    {   // n_seqs + n_derived at 0x7FFFFFF0 (the checks alone: nobody holds that many segment lists)
        const int32_t one_len = 5, sf[2] = {0, 0};
        const uint8_t* one_seq = g_unreadable;
        const vapor_segment sg{0, 0, 0, 0};
        for (int entry : {sp::DERIVED, sp::MIXED}) {
            const char* too_many = entry == sp::DERIVED ? "vapor_seqset_create_derived: too many sequences" : "vapor_seqset_create_mixed: too many sequences";
            Call c{(sp::Entry)entry, true, 0, nullptr, nullptr, &one_seq, &one_len, nullptr, nullptr, nullptr, 0x7FFFFFF0, sf, &sg, nullptr};
            CHECK(!sp::check_args(c, in_unreadable), "0x7FFFFFF0 derived sequences are refused");
            c.n_derived = 0x7FFFFFF1;
            Refusal no = sp::check_args(c, in_unreadable);
            CHECK(no.code == VAPOR_E_ARG && std::string(no.msg) == too_many, "0x7FFFFFF1 derived sequences: %s", no.msg ? no.msg : "(none)");
            c.n_seqs = 1; c.n_derived = 0x7FFFFFF0 - 1;
            CHECK(!sp::check_args(c, in_unreadable), "0x7FFFFFF0 sequences are refused");
            c.n_derived = 0x7FFFFFF0;
            no = sp::check_args(c, in_unreadable);
            CHECK(no.code == VAPOR_E_ARG && std::string(no.msg) == too_many, "0x7FFFFFF1 sequences: %s", no.msg ? no.msg : "(none)");
            n += 4;
        }
    }
    return n;
}

// ---- sections 3 and 4: drawn sets ----
static const int EDGE_LENGTHS[5] = {0, 1, 31, 32, 33};

// a window with alleles derived from it (so that share_layout finds groups), reads, literals of the edge lengths, derived
// sequences with empty segments and of no symbols at all; `mixed`: some reads are the device's
static Set draw_set(bool mixed)
{
    Set s;
    const int n_win = rnd(0, 2);
    std::vector<int> wins;
    for (int w = 0; w < n_win; ++w) {
        wins.push_back((int)s.text.size());
        s.literal(dna(rnd(80, 400)), one_in(5) ? VAPOR_SEQ_UPPER : 0);
    }
    for (int r = rnd(1, 12); r > 0; --r) {
        const int n = one_in(3) ? EDGE_LENGTHS[rnd(0, 4)] : one_in(2) ? 32 * rnd(1, 6) + rnd(-1, 1) : rnd(2, 300);
        s.literal(dna(n), one_in(8) ? VAPOR_SEQ_UPPER : 0, mixed && one_in(2) ? rnd(1, 2) : 0);
    }
    if (mixed && !s.any_dev) s.literal(dna(rnd(0, 70)), 0, rnd(1, 2));
    const int n_lit = (int)s.text.size();
    for (int d = rnd(0, 6); d > 0; --d) {
        std::vector<vapor_segment> sg;
        const bool up = one_in(3);
        bool upper_parent = false;
        if (!wins.empty() && !one_in(4)) {                                           // a deletion, an inversion or an insertion in a window
            const int w = wins[(size_t)rnd(0, (int)wins.size() - 1)], n = s.len[(size_t)w];
            int x = rnd(1, n - 2), y = rnd(1, n - 2);
            if (x > y) std::swap(x, y);
            ++y;
            const int what = rnd(0, 2), ins = rnd(0, n_lit - 1);
            sg.push_back(vapor_segment{w, 0, x, 0});
            if (what == 1) sg.push_back(vapor_segment{w, x, y - x, VAPOR_SEG_REVCOMP});
            if (what == 2) sg.push_back(vapor_segment{ins, 0, s.len[(size_t)ins], one_in(3) ? VAPOR_SEG_REVCOMP : 0u});
            if (one_in(3)) sg.push_back(vapor_segment{w, x, 0, 0});                  // (an empty segment between others)
            sg.push_back(vapor_segment{w, what == 2 ? x : y, n - (what == 2 ? x : y), 0});
        } else {
            for (int g = rnd(0, 5); g > 0; --g) {
                const int p = rnd(0, n_lit - 1), n = s.len[(size_t)p], off = rnd(0, n);
                sg.push_back(vapor_segment{p, off, one_in(4) ? 0 : rnd(0, n - off), one_in(3) ? VAPOR_SEG_REVCOMP : 0u});
            }
        }
        for (const vapor_segment& x : sg) upper_parent = upper_parent || (x.len > 0 && (s.flags[(size_t)x.parent] & VAPOR_SEQ_UPPER));
        s.derived_seq(sg, up || upper_parent ? VAPOR_SEQ_UPPER : 0);                  // (the library refuses the other case)
    }
    s.seal();
    return s;
}

// what the caller's derived sequence d spells, from the caller's own segments
static std::string derived_text(const Set& s, int d)
{
    std::string t;
    for (int32_t g = s.seg_first[(size_t)d]; g < s.seg_first[(size_t)d + 1]; ++g) {
        const vapor_segment& x = s.segs[(size_t)g];
        const std::string& par = s.flags[(size_t)x.parent] & VAPOR_SEQ_UPPER ? seq_spell::upper(s.text[(size_t)x.parent]) : s.text[(size_t)x.parent];
        const std::string cut = par.substr((size_t)x.off, (size_t)x.len);
        t += x.flags & VAPOR_SEG_REVCOMP ? seq_spell::revcomp(cut) : cut;
    }
    return s.dflags[(size_t)d] & VAPOR_SEQ_UPPER ? seq_spell::upper(t) : t;
}

struct Tally {
    long sets = 0, seqs = 0, hidden = 0, empty = 0, shared_off = 0;                  // layout
    long images = 0, chunks = 0, spelt = 0, device_held = 0, mixed = 0;             // image
    long sliced = 0, sends = 0;                                                      // slices
    long raw = 0, rc_refused = 0, rc_taken = 0;                                      // after the counts
};
static Tally T;

static void check_layout(const Set& s, const sp::Layout& L, bool shared_join)
{
    const size_t n_lit = s.text.size(), n = n_lit + (size_t)s.n_derived();
    CHECK(L.n_lit == (int32_t)n_lit && L.n == (int32_t)n && L.h.size() == std::max<size_t>(n, 1) + L.hidden.size(), "%d literals, %d sequences, %zu descriptors", L.n_lit,
          L.n, L.h.size());
    CHECK(shared_join || (L.hidden.empty() && L.groups.empty()), "shared joins are off and there are %zu hidden sequences", L.hidden.size());
    // lengths and flags
    size_t hidden_seen = 0;
    for (size_t i = 0; i < n_lit; ++i) CHECK(L.h[i].len == s.len[i] && L.h[i].flags == s.flags[i], "literal %zu: %d symbols, flags %u", i, L.h[i].len, L.h[i].flags);
    for (size_t d = 0; d < (size_t)s.n_derived(); ++d)
        CHECK((size_t)L.h[n_lit + d].len == derived_text(s, (int)d).size() && L.h[n_lit + d].flags == s.dflags[d], "derived sequence %zu: %d symbols", d, L.h[n_lit + d].len);
    for (const ShareGroup& g : L.groups) {
        if (g.t_seq < 0) continue;
        CHECK((size_t)g.t_seq == n + hidden_seen && L.h[(size_t)g.t_seq].flags == (g.upper ? VAPOR_SEQ_UPPER : 0u), "hidden sequence %d, flags %u", g.t_seq,
              L.h[(size_t)g.t_seq].flags);
        ++hidden_seen;
    }
    CHECK(hidden_seen == L.hidden.size(), "%zu groups have a hidden sequence, there are %zu", hidden_seen, L.hidden.size());
    // the planes: chunk ranges ascend, disjoint, VP_PAD_CHUNKS free chunks behind each, VP_PAD_CHUNKS + 1 more at the end
    std::vector<int32_t> owner(L.plane_chunks, -1);
    size_t next = 0, asc = 0, der = 0, n_seg = 0;
    for (size_t i = 0; i < (n ? L.h.size() : 0); ++i) {
        const size_t ch = ((size_t)L.h[i].len + 31) / 32;
        CHECK(L.h[i].chunk0 == next, "sequence %zu begins at chunk %u, the one before it and its pad end at %zu", i, L.h[i].chunk0, next);
        CHECK(next + ch + VP_PAD_CHUNKS <= L.plane_chunks, "sequence %zu ends behind the planes", i);
        for (size_t c = 0; c < ch; ++c) { CHECK(owner[next + c] < 0, "chunk %zu has two owners", next + c); owner[next + c] = (int32_t)i; }
        next += ch + VP_PAD_CHUNKS;
        // asc0: literals count among the staged chunks, derived and hidden sequences among the derived chunks alone
        CHECK(L.h[i].asc0 == (i < n_lit ? asc : der), "sequence %zu: asc0 %u, %zu chunks of its kind before it", i, L.h[i].asc0, i < n_lit ? asc : der);
        (i < n_lit ? asc : der) += ch;
        T.empty += ch == 0;
    }
    CHECK(L.plane_chunks == next + VP_PAD_CHUNKS + 1, "%zu plane chunks, the sequences and their pads take %zu", L.plane_chunks, next);
    for (const auto& v : L.derived) n_seg += v.size();
    for (const auto& v : L.hidden) n_seg += v.size();
    CHECK(L.n_asc == asc && L.der_chunks == der && L.n_seg == n_seg, "n_asc %zu, der_chunks %zu, n_seg %zu", L.n_asc, L.der_chunks, L.n_seg);
    CHECK(L.mixed == s.any_dev, "mixed %d", (int)L.mixed);
    ++T.sets;
    T.seqs += (long)L.h.size();
    T.hidden += (long)L.hidden.size();
    T.shared_off += !shared_join;
}

// the staging image of a call, every byte nobody writes left at 0xAA
static std::vector<uint8_t> image_of(const Call& c, const sp::Layout& L, const sp::Staging& st)
{
    std::vector<uint8_t> image(st.need, 0xAA);
    sp::stage_range(c, L, st, image.data(), 0, L.n_lit);
    if (L.mixed) sp::fill_sources(c, st, image.data());
    sp::fill_derived(L, st, image.data());
    return image;
}

static void check_image(const Set& s, const Call& c, const sp::Layout& L)
{
    const sp::Staging st(c, L);
    const size_t n_lit = s.text.size(), n = n_lit + (size_t)s.n_derived();
    // the size and the places, by the formulas written out
    const size_t n_asc = L.n_asc, n_dseq = L.h.size() - n_lit;
    const size_t mix_off = (n_asc * 36 + 7) & ~(size_t)7, mix_bytes = s.any_dev ? n_lit * 12 : 0, der_off = (mix_off + mix_bytes + 63) & ~(size_t)63;
    const size_t der_bytes = L.der_chunks ? 20 * std::max<size_t>(L.n_seg, 1) + 4 * (n_dseq + 1) + 4 * L.der_chunks : 0;
    CHECK(st.need == std::max<size_t>(der_off + der_bytes, 64), "need %zu, the formula says %zu", st.need, std::max<size_t>(der_off + der_bytes, 64));
    CHECK(st.asc.off == 0 && st.asc.bytes() == n_asc * 32 && st.map.off == n_asc * 32 && st.map.n == n_asc, "ASCII at %zu, map at %zu", st.asc.off, st.map.off);
    CHECK(st.mix_bytes == mix_bytes && (!s.any_dev || (st.src.off == mix_off && st.first.off == mix_off + 8 * n_lit && st.src.off % 8 == 0)), "mixed block at %zu", st.src.off);
    CHECK(st.der_bytes == der_bytes && (!L.der_chunks || (st.segs.off == der_off && der_off % 64 == 0 && st.seg_first.off == der_off + 20 * std::max<size_t>(L.n_seg, 1) &&
                                                          st.der_map.off == st.seg_first.off + 4 * (n_dseq + 1))), "derived block at %zu", st.segs.off);
    CHECK(s.any_dev || (st.src.n == 0 && st.first.n == 0), "a set without device-held literals has a mixed block");
    CHECK(L.der_chunks || (st.segs.n == 0 && st.seg_first.n == 0 && st.der_map.n == 0), "a set without derived chunks has a derived block");
    size_t host_end = s.any_dev ? 0 : n_asc;
    for (size_t i = 0; s.any_dev && i < n_lit; ++i)
        if (!s.kind[i] && s.len[i] > 0) host_end = std::max(host_end, (size_t)L.h[i].asc0 + ((size_t)s.len[i] + 31) / 32);
    CHECK(st.host_end == host_end, "host_end %zu, not %zu", st.host_end, host_end);
    CHECK(st.sliced == (!s.any_dev && n_asc * 32 >= ((size_t)4 << 20) && n_lit >= 8), "sliced %d", (int)st.sliced);

    const std::vector<uint8_t> image = image_of(c, L, st);
    const uint8_t* asc = st.asc.in(image.data());
    const uint32_t* map = st.map.in(image.data());
    for (size_t i = 0; i < n_lit; ++i) {
        const size_t ch = ((size_t)s.len[i] + 31) / 32, at = (size_t)L.h[i].asc0 * 32;
        for (size_t k = 0; k < ch; ++k) CHECK(map[L.h[i].asc0 + k] == i, "chunk %zu belongs to %u, not %zu", L.h[i].asc0 + k, map[L.h[i].asc0 + k], i);
        for (size_t b = 0; b < ch * 32; ++b) {
            // a literal the device holds: bam_expand_kernel's to write, the host leaves it alone
            const uint8_t want = s.kind[i] ? 0xAA : b < (size_t)s.len[i] ? (uint8_t)s.text[i][b] : 0;
            CHECK(asc[at + b] == want, "literal %zu, byte %zu: %u, not %u", i, b, asc[at + b], want);
        }
        T.device_held += s.kind[i] != 0;
        T.chunks += (long)ch;
    }
    if (s.any_dev) {
        const unsigned long long* src = st.src.in(image.data());
        const int32_t* first = st.first.in(image.data());
        for (size_t i = 0; i < n_lit; ++i) {
            const unsigned long long want = s.kind[i] ? (unsigned long long)reinterpret_cast<uintptr_t>(s.ptr[i]) | (s.kind[i] == 2 ? 0x8000000000000000ull : 0ull) : 0ull;
            CHECK(src[i] == want && first[i] == (s.kind[i] ? (int32_t)s.first[i] : 0), "source %zu: %llx from base %d", i, src[i], first[i]);
        }
        ++T.mixed;
    }
    if (L.der_chunks) {
        // the derived tables, spelt through the parents' first chunks: the caller's sequences give the texts their own segments
        // spell, the hidden ones the texts share_layout's lists spell
        const DSeg* segs = st.segs.in(image.data());
        const int32_t* seg_first = st.seg_first.in(image.data());
        const uint32_t* der_map = st.der_map.in(image.data());
        std::map<uint32_t, int32_t> literal_at;
        std::vector<std::string> as_packed;                                          // (a parent's planes hold its upper-cased text when it was uploaded so)
        for (size_t i = 0; i < n_lit; ++i) {
            literal_at[L.h[i].chunk0] = (int32_t)i;
            as_packed.push_back(s.flags[i] & VAPOR_SEQ_UPPER ? seq_spell::upper(s.text[i]) : s.text[i]);
        }
        CHECK(seg_first[0] == 0 && (size_t)seg_first[n_dseq] == L.n_seg, "the segment lists run from %d to %d", seg_first[0], seg_first[n_dseq]);
        for (size_t t = 0; t < n_dseq; ++t) {
            std::vector<HSeg> through;
            for (int32_t g = seg_first[t]; g < seg_first[t + 1]; ++g) {
                CHECK(literal_at.count(segs[g].chunk0), "segment %d reads chunk %u, where no literal begins", g, segs[g].chunk0);
                CHECK(segs[g].rc <= 1, "segment %d: rc %u", g, segs[g].rc);
                through.push_back(HSeg{literal_at[segs[g].chunk0], segs[g].off, segs[g].len, segs[g].dst, segs[g].rc == 1});
            }
            std::string got, want, why;
            const bool up = L.h[n_lit + t].flags & VAPOR_SEQ_UPPER;
            CHECK(seq_spell::spell(as_packed, (int32_t)n_lit, through, up, got, why), "sequence %zu: %s", n_lit + t, why.c_str());
            if (n_lit + t < n) want = derived_text(s, (int)t);
            else CHECK(seq_spell::spell(as_packed, (int32_t)n_lit, L.hidden[n_lit + t - n], up, want, why), "hidden sequence %zu: %s", n_lit + t, why.c_str());
            CHECK(got == want && got.size() == (size_t)L.h[n_lit + t].len, "sequence %zu spells %zu symbols, not the %zu of its text", n_lit + t, got.size(), want.size());
            for (size_t k = 0; k < (got.size() + 31) / 32; ++k)
                CHECK(der_map[L.h[n_lit + t].asc0 + k] == n_lit + t, "derived chunk %zu belongs to %u", L.h[n_lit + t].asc0 + k, der_map[L.h[n_lit + t].asc0 + k]);
            ++T.spelt;
        }
    }
    ++T.images;
}

// ---- section 5: the threaded staging ----
static const int THREADS[7] = {1, 2, 3, 5, 12, 13, 64};

static Set slice_set(int which)
{
    Set s;
    switch (which) {
    case 0: for (int i = rnd(1, 11); i > 0; --i) s.literal(dna(rnd(0, 400))); break;                  // fewer sequences than slices
    case 1:                                                                                          // one sequence holds nearly all bytes
        for (int i = rnd(0, 9); i > 0; --i) s.literal(dna(rnd(0, 40)));
        s.literal(dna(rnd(20000, 40000)));
        for (int i = rnd(0, 9); i > 0; --i) s.literal(dna(rnd(0, 40)));
        break;
    case 2:                                                                                          // empty sequences at the cut points
        for (int k = 0; k < sp::STAGE_SLICES; ++k) {
            for (int e = rnd(1, 3); e > 0; --e) s.literal("");
            s.literal(dna(32 * 20));
        }
        s.literal("");
        break;
    default: for (int i = rnd(12, 200); i > 0; --i) s.literal(dna(one_in(6) ? 0 : rnd(1, 700)), one_in(7) ? VAPOR_SEQ_UPPER : 0); break;
    }
    s.seal();
    return s;
}

static void check_slices(const Set& s)
{
    const Call c = s.call(one_in(2) ? sp::BLOB : sp::PTRS);
    sp::Layout L;
    CHECK(!L.build(c, true), "a set of literals is refused");
    sp::Staging st(c, L);
    const std::vector<uint8_t> one = image_of(c, L, st);
    st.cut = sp::slice_cuts(L);                                                       // (Staging cuts a set only when it is large enough to slice)
    // every sequence in exactly one slice, and a slice's chunks are its sequences'
    CHECK(st.cut[0] == 0 && st.cut[sp::STAGE_SLICES] == L.n_lit, "the cuts run from %d to %d", st.cut[0], st.cut[sp::STAGE_SLICES]);
    for (int k = 0; k < sp::STAGE_SLICES; ++k) {
        CHECK(st.cut[(size_t)k] <= st.cut[(size_t)k + 1], "cut %d: %d, then %d", k, st.cut[(size_t)k], st.cut[(size_t)k + 1]);
        // equal shares of the bytes: slice k begins with the first sequence at or behind chunk n_asc * k / STAGE_SLICES
        int32_t begins = 0;
        while (begins < L.n_lit && (uint64_t)L.h[(size_t)begins].asc0 < (uint64_t)L.n_asc * (uint64_t)k / sp::STAGE_SLICES) ++begins;
        CHECK(st.cut[(size_t)k] == begins, "slice %d begins with sequence %d, not %d", k, st.cut[(size_t)k], begins);
        size_t chunks = 0;
        for (int32_t i = st.cut[(size_t)k]; i < st.cut[(size_t)k + 1]; ++i) chunks += ((size_t)s.len[(size_t)i] + 31) / 32;
        CHECK(st.slice_chunk(L, k + 1) - st.slice_chunk(L, k) == chunks, "slice %d: chunks %zu .. %zu, its sequences have %zu", k, st.slice_chunk(L, k),
              st.slice_chunk(L, k + 1), chunks);
    }
    for (int n_thr : THREADS) {
        std::vector<uint8_t> image(st.need, 0xAA), device(st.need, 0xAA);
        size_t sent_to = 0;
        long sends = 0;
        sp::stage_sliced(c, L, st, image.data(), n_thr, [&](size_t c0, size_t c1) {
            CHECK(c0 == sent_to && c1 > c0 && c1 <= L.n_asc, "%d threads: chunks %zu .. %zu are sent, %zu were sent before", n_thr, c0, c1, sent_to);
            memcpy(device.data() + c0 * 32, image.data() + c0 * 32, (c1 - c0) * 32);         // (the slice is staged: reading it races with nothing)
            sent_to = c1;
            ++sends;
        });
        CHECK(sent_to == L.n_asc && sends <= sp::STAGE_SLICES, "%d threads: %zu of %zu chunks sent in %ld pieces", n_thr, sent_to, L.n_asc, sends);
        CHECK(image == one, "%d threads: the image is not the one a single thread makes", n_thr);
        CHECK(!memcmp(device.data(), one.data(), L.n_asc * 32), "%d threads: the pieces sent are not the single thread's ASCII", n_thr);
        T.sends += sends;
    }
    ++T.sliced;
}

// ---- section 6: after the counts ----
static void check_after_counts(const Set& s, sp::Layout L)
{
    const size_t n_lit = s.text.size();
    for (size_t i = 0; i < L.h.size(); ++i) {
        L.h[i].n_exc = rnd(0, 50);
        L.h[i].n_invalid = one_in(3) ? rnd(1, 9) : 0;
        L.h[i].n_nocomp = i < n_lit && one_in(6) ? rnd(1, 3) : 0;
    }
    std::vector<int64_t> raw_off(3, 77);
    const size_t raw_bytes = sp::raw_layout(L, raw_off);
    CHECK(raw_off.size() == L.h.size(), "%zu offsets", raw_off.size());
    size_t all = 0;
    for (size_t i = 0; i < L.h.size(); ++i) {
        int64_t want = -1;
        if (i < n_lit && L.h[i].n_invalid > 0) {
            want = 0;
            for (size_t j = 0; j < i; ++j) if (L.h[j].n_invalid > 0) want += ((int64_t)s.len[j] + 15) / 16 * 16;
            all = (size_t)want + ((size_t)s.len[i] + 15) / 16 * 16;
        }
        CHECK(raw_off[i] == want && (want < 0 || want % 16 == 0), "sequence %zu keeps its bytes at %ld, not %ld", i, (long)raw_off[i], (long)want);
    }
    CHECK(raw_bytes == all, "%zu raw bytes, not %zu", raw_bytes, all);
    T.raw += raw_bytes != 0;
    bool refused = false;
    for (const vapor_segment& x : s.segs) refused = refused || (x.len > 0 && (x.flags & VAPOR_SEG_REVCOMP) && L.h[(size_t)x.parent].n_nocomp > 0);
    const Refusal no = sp::revcomp_refusal(L);
    CHECK((bool)no == refused, "a reversed segment over a parent with dropped characters: %d, refused: %d", (int)refused, (int)(bool)no);
    CHECK(!no || (no.code == VAPOR_E_ARG && std::string(no.msg) == "vapor_seqset_create_derived: a reverse-complemented segment's parent holds characters complementary() "
                                                                    "drops (outside ATGCN/atgcn, SF:471-478); upload that allele as bytes"), "%s", no.msg);
    (refused ? T.rc_refused : T.rc_taken) += 1;
    std::vector<int32_t> info(2 * (size_t)L.n + 2, -7);
    sp::fill_seq_info(L, info.data());
    sp::fill_seq_info(L, nullptr);
    for (size_t i = 0; i < (size_t)L.n; ++i) CHECK(info[2 * i] == L.h[i].n_exc && info[2 * i + 1] == L.h[i].n_invalid, "seq_info of sequence %zu", i);
    CHECK(info[2 * (size_t)L.n] == -7, "seq_info written behind the caller's sequences");
}

int main(int argc, char** argv)
{
    void* page = mmap(nullptr, UNREADABLE_BYTES, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (page == MAP_FAILED) { perror("mmap"); return 1; }
    g_unreadable = static_cast<const uint8_t*>(page);
    const bool slices_only = argc > 1 && std::string(argv[1]) == "slices";
    if (!slices_only) {
        long n_pairs = 0;
        const long singles = check_refusals(n_pairs);
        printf("refusals: %ld calls with one fault say what the fault is, %ld with two what the entries' own order meets first\n", singles, n_pairs);
        printf("limits: %ld calls of made-up lengths on both sides of every limit\n", check_limits());
        for (int k = 0; k < 3000; ++k) {
            ++g_case;
            const bool mixed = k % 3 == 2, shared_join = k % 5 != 0;
            const Set s = k < 6 ? Set() : draw_set(mixed);                            // (the empty set first)
            Set empty;
            empty.seal();
            const Set& use = k < 6 ? empty : s;
            const Call c = use.call(mixed ? sp::MIXED : k % 3 == 1 || use.n_derived() ? sp::DERIVED : one_in(2) ? sp::BLOB : sp::PTRS);
            CHECK(!naive_refusal(c), "a drawn set the transcription refuses: %s", naive_refusal(c));
            CHECK(!sp::check_args(c, in_unreadable), "a drawn set is refused");
            sp::Layout L;
            const Refusal no = L.build(c, shared_join);
            CHECK(!no, "a drawn set is refused: %s", no.msg);
            check_layout(use, L, shared_join);
            check_image(use, c, L);
            check_after_counts(use, L);
        }
        CHECK(T.hidden > 300 && T.shared_off > 300 && T.empty > 1000, "%ld hidden sequences, %ld sets without shared joins, %ld empty sequences", T.hidden, T.shared_off, T.empty);
        CHECK(T.mixed > 500 && T.device_held > 1000 && T.spelt > 2000, "%ld mixed sets, %ld device-held literals, %ld sequences spelt", T.mixed, T.device_held, T.spelt);
        CHECK(T.raw > 1000 && T.rc_refused > 100 && T.rc_taken > 1000, "%ld sets keep raw bytes, %ld are refused, %ld taken", T.raw, T.rc_refused, T.rc_taken);
        printf("layout: %ld sets (%ld sequences, %ld of them hidden, %ld of no symbols; %ld sets without shared joins)\n", T.sets, T.seqs, T.hidden, T.empty, T.shared_off);
        printf("image: %ld sets (%ld chunks of ASCII, %ld derived and hidden sequences spelt through their tables, %ld mixed sets with %ld device-held literals never read)\n",
               T.images, T.chunks, T.spelt, T.mixed, T.device_held);
        printf("after the counts: %ld sets (%ld keep raw bytes, %ld refused for a reversed segment, %ld not)\n", T.sets, T.raw, T.rc_refused, T.rc_taken);
    }
    for (int k = 0; k < (slices_only ? 60 : 200); ++k) {
        ++g_case;
        check_slices(slice_set(k % 4));
    }
    printf("slices: %ld sets staged by 1, 2, 3, 5, 12, 13 and 64 threads equal the single thread's image (%ld pieces sent)\n", T.sliced, T.sends);
    printf("seqset_check: all equal\n");
    return 0;
}
