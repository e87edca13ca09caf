// vapor_sa.h - the SA:Z tag of a BAM record as `--links` reads it: where the first aux field named SA lies, how
// its value is cut into pieces, and which piece is an entry.  HIP-free: the host reader (vapor_bam.cpp bam_links_impl) works
// through it, tools/sa_check.cpp holds it to direct statements of the grammar, and bam_link_kernel (vapor_bamdev.h) is the same
// rule across a wavefront - this file is the C++ statement it follows; vapor_amd/links.py parse_sa is the Python one.
//
// A piece is well-formed iff it matches, as bytes and in full,
//     ([^,;]+),([0-9]{1,10}),([+-]),((?:[0-9]{1,9}[MIDNSHP=X])+),([0-9]{1,3}),([0-9]+)
// with pos in 1 .. 2^31 - 1, mapq at most 255 and every operation length at most 2^28 - 1.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vapor_sa {

constexpr int64_t POS_MAX = ((int64_t)1 << 31) - 1;      // the largest 1-based position of an entry
constexpr int64_t OP_MAX = ((int64_t)1 << 28) - 1;       // the longest operation a BAM record holds
constexpr int FIND_NONE = 0, FIND_VALUE = 1, FIND_MALFORMED = 2;

struct Entry {
    const uint8_t* name = nullptr;     // rname, name_len bytes (not terminated)
    size_t name_len = 0;
    int64_t a = 0, b = 0;              // the reference interval, 0-based half-open: a = pos - 1, b = a + sum of M D N = X
    bool minus = false;                // strand '-'
    uint32_t mapq = 0;
};

inline bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// the code of an operation letter (M I D N S H P = X: 0..8), -1 for another byte
inline int op_code(uint8_t c)
{
    switch (c) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
    case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
    default: return -1;
    }
}

// The first aux field named SA among [p, end) (vapor_bam.cpp find_cg's walk): FIND_VALUE with the bytes before its NUL when its
// type is Z; FIND_NONE when there is none or its type is another (nothing behind that field is looked at); FIND_MALFORMED when
// the area is damaged before one is found (an unknown type, a field, string or array that runs past the record - an SA:Z
// without its NUL included).  What a reader does with a malformed area is its own rule.
inline int find_sa(const uint8_t* p, const uint8_t* end, const uint8_t** value, size_t* len)
{
    *value = nullptr;
    *len = 0;
    while (p + 3 <= end) {
        const uint8_t t0 = p[0], t1 = p[1], ty = p[2];
        p += 3;
        const bool sa = t0 == 'S' && t1 == 'A';
        if (sa && ty != 'Z') return FIND_NONE;
        size_t sz = 0;
        switch (ty) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': {
            const uint8_t* q = p;
            while (q < end && *q) ++q;
            if (q >= end) return FIND_MALFORMED;
            if (sa) { *value = p; *len = (size_t)(q - p); return FIND_VALUE; }
            p = q + 1;
            continue;
        }
        case 'B': {
            if (p + 5 > end) return FIND_MALFORMED;
            const uint8_t sub = p[0];
            const int32_t cnt = (int32_t)((uint32_t)p[1] | ((uint32_t)p[2] << 8) | ((uint32_t)p[3] << 16) | ((uint32_t)p[4] << 24));
            p += 5;
            const int es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (cnt < 0 || (int64_t)cnt * es > (int64_t)(end - p)) return FIND_MALFORMED;
            p += (size_t)cnt * (size_t)es;
            continue;
        }
        default: return FIND_MALFORMED;
        }
        if (sz > (size_t)(end - p)) return FIND_MALFORMED;
        p += sz;
    }
    return FIND_NONE;
}

// a decimal field [s, e) of 1 .. max_digits digits; false for anything else
inline bool parse_number(const uint8_t* s, const uint8_t* e, int max_digits, int64_t* v)
{
    if (e <= s || e - s > max_digits) return false;
    int64_t x = 0;
    for (const uint8_t* q = s; q < e; ++q) {
        if (!is_digit(*q)) return false;
        x = 10 * x + (*q - '0');
    }
    *v = x;
    return true;
}

// One piece [s, e) of a value (no ';' inside): true and the entry iff it is well-formed.
inline bool parse_piece(const uint8_t* s, const uint8_t* e, Entry* out)
{
    const uint8_t* c[5];
    int n = 0;
    for (const uint8_t* q = s; q < e; ++q) {
        if (*q == ';') return false;
        if (*q == ',') {
            if (n == 5) return false;                    // an extra field
            c[n++] = q;
        }
    }
    if (n != 5 || c[0] == s) return false;               // a missing field, an empty name
    int64_t pos = 0, mapq = 0;
    if (!parse_number(c[0] + 1, c[1], 10, &pos) || pos < 1 || pos > POS_MAX) return false;
    if (c[2] - c[1] != 2 || (c[1][1] != '+' && c[1][1] != '-')) return false;
    if (!parse_number(c[3] + 1, c[4], 3, &mapq) || mapq > 255) return false;
    if (c[4] + 1 >= e) return false;                     // an empty NM
    for (const uint8_t* q = c[4] + 1; q < e; ++q)
        if (!is_digit(*q)) return false;
    // the CIGAR: one or more of 1..9 digits and a letter
    const uint8_t *q = c[2] + 1, *ce = c[3];
    if (q >= ce) return false;
    int64_t span = 0;
    while (q < ce) {
        int64_t len = 0;
        int d = 0;
        while (q < ce && is_digit(*q)) {
            if (++d > 9) return false;
            len = 10 * len + (*q - '0');
            ++q;
        }
        if (d == 0 || q >= ce) return false;
        const int code = op_code(*q++);
        if (code < 0 || len > OP_MAX) return false;
        if (code == 0 || code == 2 || code == 3 || code == 7 || code == 8) span += len;
    }
    out->name = s;
    out->name_len = (size_t)(c[0] - s);
    out->a = pos - 1;
    out->b = pos - 1 + span;
    out->minus = c[1][1] == '-';
    out->mapq = (uint32_t)mapq;
    return true;
}

// The pieces of a value in text order: cut at every ';', empty pieces dropped, a last piece without ';' a piece.  f(ok, entry) is
// called once per piece - ok: whether it is well-formed - and ends the walk by returning true.
template <typename PerPiece>
inline void for_each_piece(const uint8_t* value, size_t len, PerPiece f)
{
    const uint8_t *s = value, *end = value + len;
    while (s < end) {
        const uint8_t* e = s;
        while (e < end && *e != ';') ++e;
        if (e > s) {
            Entry en;
            const bool ok = parse_piece(s, e, &en);
            if (f(ok, en)) return;
        }
        s = e + 1;
    }
}

}  // namespace vapor_sa
