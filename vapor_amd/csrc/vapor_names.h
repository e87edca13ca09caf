// vapor_names.h - the identity of a molecule by its QNAME and the rule that keeps one record of it (`--dedup-qname`, DESIGN.md
// 4.18), without HIP: the arithmetic bam_dedup_kernel (vapor_bamdev.h) and the native host reader (vapor_bam.cpp) share, so that
// the two cannot drift apart.  tools/names_check.cpp runs it on a CPU under the sanitizers, against direct statements of its
// rules; vapor_amd/seqio.py name_key is the Python statement.
//
//   name_key   b_0 .. b_{n-1} the QNAME bytes without the NUL, 0 <= n <= 254:
//                  h   = n + sum_i (b_i + 1) * M^(i+1)  mod 2^64,   M = 0x9E3779B97F4A7C15
//                  key = fin(h), the splitmix64 finaliser
//              M is odd, so a change of one byte changes h, and fin is a bijection: two names that differ in one byte never
//              collide.  Names that differ in more may, and then they are ONE molecule on every route - all of them use this
//              one function.
//   drops      rule W over the kept records of one (file, region, anchor kind), in record order, sec = (FLAG & 0x900) != 0:
//              entry i is dropped iff some j has the same key and (sec_j, j) < (sec_i, i).  Exactly one entry per key survives:
//              the first that is neither secondary nor supplementary, else the first.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define VN_FN __attribute__((host)) __attribute__((device)) inline
#else
#define VN_FN inline
#endif

namespace vapor_names {

constexpr uint64_t NAME_M = 0x9E3779B97F4A7C15ull;
constexpr int QNAME_MAX = 254;                // l_read_name is one byte and counts the NUL
constexpr uint32_t SEC_FLAGS = 0x900u;        // secondary | supplementary

// p[k] = M^k mod 2^64, k = 0 .. 256: lane l of a wavefront takes bytes 4l .. 4l + 3 and reads p[4l + 1 .. 4l + 4].  The struct is
// constant-initialised, so a `__device__ const PowTable` of a kernel's translation unit is data of its code object.
struct PowTable {
    uint64_t p[257];
    constexpr PowTable() : p{}
    {
        uint64_t x = 1;
        for (int k = 0; k <= 256; ++k) { p[k] = x; x *= NAME_M; }
    }
};

VN_FN uint64_t fin(uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the four terms lane `lane` adds to h: bytes 4 * lane .. 4 * lane + 3 of the name, none at or behind n (nothing behind the name
// is read)
VN_FN uint64_t lane_terms(const uint8_t* name, int n, int lane, const uint64_t* pw)
{
    uint64_t s = 0;
    for (int t = 0; t < 4; ++t) {
        const int i = 4 * lane + t;
        if (i < n) s += ((uint64_t)name[i] + 1ull) * pw[i + 1];
    }
    return s;
}

// key of the name from the sum of its terms
VN_FN uint64_t key_of_sum(int n, uint64_t sum) { return fin((uint64_t)n + sum); }

// the definition, byte by byte (no table)
VN_FN uint64_t name_key(const uint8_t* name, int n)
{
    uint64_t h = (uint64_t)n, x = NAME_M;
    for (int i = 0; i < n; ++i) { h += ((uint64_t)name[i] + 1ull) * x; x *= NAME_M; }
    return fin(h);
}

// rule W: whether entry i of the n kept records is dropped
VN_FN bool drops(const uint64_t* key, const uint8_t* sec, int n, int i)
{
    const uint64_t k = key[i];
    const bool si = sec[i] != 0;
    bool d = false;
    for (int j = 0; j < n; ++j) {
        const bool sj = sec[j] != 0;
        d = d || (key[j] == k && (sj != si ? si : j < i));     // (sec_j, j) < (sec_i, i)
    }
    return d;
}

}  // namespace vapor_names
