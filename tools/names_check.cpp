// names_check.cpp - the name key and the drop rule of `--dedup-qname` (vapor_amd/csrc/vapor_names.h) on a CPU,
// against direct statements of their rules.  Nothing here is compared with recorded output.
//   name_key        byte by byte against the sum of the 64 lanes' terms from the power table (what bam_dedup_kernel adds up), for
//                   names of 0 .. 254 bytes from a fixed seed; the table against repeated multiplication; fin against its inverse
//                   (it is a bijection); a change of one byte changes the key.
//   drops           against the O(n^2) statement "some j has the key and (sec_j, j) < (sec_i, i)" on random (key, sec) arrays
//                   of 0, 1, 2, 64, 65 and 256 entries with few distinct keys; one survivor per key, the one the rule names.
//   names on argv   `names_check <file>`: a QNAME per line as hex digits (an empty line is the empty name); prints its key as 16 hex
//                   digits per line behind the self-checks, for tests/test_dedup_cpu.py to hold against seqio.name_key.
// Built and run by tests/test_dedup_cpu.py:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ivapor_amd/csrc tools/names_check.cpp
#include "vapor_names.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

using namespace vapor_names;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static std::mt19937_64 rng(20261019);

static const PowTable POW;

// the inverse of x ^= x >> s
static uint64_t unxorshift(uint64_t x, int s)
{
    uint64_t r = x;
    for (int i = s; i < 64; i += s) r = x ^ (r >> s);
    return r;
}
static uint64_t unfin(uint64_t z)
{
    z = unxorshift(z, 31); z *= 0x319642B2D24D8EC3ull;      // (the inverses of the two odd multipliers mod 2^64)
    z = unxorshift(z, 27); z *= 0x96DE1B173F119089ull;
    z = unxorshift(z, 30);
    return z;
}

static uint64_t key_by_lanes(const std::vector<uint8_t>& name)
{
    // (an exact-size copy: a read behind the name is the sanitizer's to report)
    std::vector<uint8_t> exact(name);
    uint64_t sum = 0;
    for (int lane = 0; lane < 64; ++lane) sum += lane_terms(exact.data(), (int)exact.size(), lane, POW.p);
    return key_of_sum((int)exact.size(), sum);
}

int main(int argc, char** argv)
{
    // ---- the table
    {
        uint64_t x = 1;
        for (int k = 0; k <= 256; ++k) { CHECK(POW.p[k] == x, "p[%d]", k); x *= NAME_M; }
        CHECK(0xBF58476D1CE4E5B9ull * 0x96DE1B173F119089ull == 1ull && 0x94D049BB133111EBull * 0x319642B2D24D8EC3ull == 1ull, "inverses");
        printf("table: 257 powers\n");
    }
    // ---- name_key
    long n_names = 0;
    for (int n = 0; n <= QNAME_MAX; ++n) {
        for (int rep = 0; rep < 8; ++rep) {
            std::vector<uint8_t> name((size_t)n);
            for (auto& b : name) b = (uint8_t)(rep < 4 ? 33 + rng() % 94 : rng() % 256);
            const uint64_t k = name_key(name.data(), n);
            CHECK(k == key_by_lanes(name), "lanes, n = %d", n);
            // the definition once more, with the powers from the table
            uint64_t h = (uint64_t)n;
            for (int i = 0; i < n; ++i) h += ((uint64_t)name[(size_t)i] + 1) * POW.p[i + 1];
            CHECK(unfin(k) == h, "fin is not inverted, n = %d", n);
            if (n) {
                std::vector<uint8_t> other(name);
                const size_t at = (size_t)(rng() % (uint64_t)n);
                other[at] = (uint8_t)(other[at] + 1 + rng() % 255);
                CHECK(name_key(other.data(), n) != k, "one byte changed, n = %d", n);
                other = name;
                other.pop_back();
                CHECK(name_key(other.data(), n - 1) != k, "a prefix, n = %d", n);
            }
            ++n_names;
        }
    }
    printf("name_key: %ld names equal the lanes' sum\n", n_names);
    // ---- drops
    long n_arrays = 0;
    for (int n : {0, 1, 2, 64, 65, 256}) {
        for (int rep = 0; rep < 200; ++rep) {
            std::vector<uint64_t> key((size_t)n);
            std::vector<uint8_t> sec((size_t)n);
            const int distinct = 1 + (int)(rng() % (uint64_t)(rep % 3 == 0 ? 3 : (n ? n : 1)));
            for (int i = 0; i < n; ++i) { key[(size_t)i] = fin(rng() % (uint64_t)distinct); sec[(size_t)i] = (uint8_t)(rng() % 3 == 0); }
            std::map<uint64_t, int> survivor;
            for (int i = 0; i < n; ++i) {
                bool want = false;
                for (int j = 0; j < n; ++j)
                    if (key[(size_t)j] == key[(size_t)i] && (sec[(size_t)j] < sec[(size_t)i] || (sec[(size_t)j] == sec[(size_t)i] && j < i))) want = true;
                const bool got = drops(key.data(), sec.data(), n, i);
                CHECK(got == want, "drops, n = %d, i = %d", n, i);
                if (!got) { CHECK(!survivor.count(key[(size_t)i]), "two survivors, n = %d", n); survivor[key[(size_t)i]] = i; }
            }
            for (int i = 0; i < n; ++i) {
                CHECK(survivor.count(key[(size_t)i]), "no survivor, n = %d", n);
                const int s = survivor[key[(size_t)i]];
                // the first that is neither secondary nor supplementary, else the first
                int first = -1, first_prim = -1;
                for (int j = 0; j < n; ++j)
                    if (key[(size_t)j] == key[(size_t)i]) { if (first < 0) first = j; if (first_prim < 0 && !sec[(size_t)j]) first_prim = j; }
                CHECK(s == (first_prim >= 0 ? first_prim : first), "the survivor, n = %d", n);
            }
            ++n_arrays;
        }
    }
    printf("drops: %ld arrays equal the direct statement\n", n_arrays);
    // ---- the caller's names
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        CHECK(f != nullptr, "cannot open %s", argv[1]);
        std::string line;
        int c;
        auto emit = [&] {
            std::vector<uint8_t> name;
            for (size_t i = 0; i + 1 < line.size(); i += 2) name.push_back((uint8_t)strtoul(line.substr(i, 2).c_str(), nullptr, 16));
            printf("key %016llx\n", (unsigned long long)name_key(name.data(), (int)name.size()));
            line.clear();
        };
        while ((c = fgetc(f)) != EOF) {
            if (c == '\n') emit();
            else if (c != '\r') line.push_back((char)c);
        }
        if (!line.empty()) emit();
        fclose(f);
    }
    printf("names_check: all equal\n");
    return 0;
}
