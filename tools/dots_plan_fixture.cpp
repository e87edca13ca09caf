// dots_plan_fixture.cpp - writes tests/golden/dots_plan.json.gz (unpacked, to stdout): what the sizes of the explicit-dot routes were
// at a seeded sample of points when vapor_hip.hip still computed them between its launches.  The expressions below are those
// lines as they stood (WideRoute::count, anyk_count, anyk_edit_launch, AnykRoute::count, wide_clean), kept apart from
// vapor_dots_plan.h on purpose: tools/dots_plan_check.cpp compares the header against the file, which shows that moving them
// changed nothing.  Run once; the file is committed.
//   g++ -O1 -std=c++17 tools/dots_plan_fixture.cpp -o dots_plan_fixture && ./dots_plan_fixture | gzip -9n > tests/golden/dots_plan.json.gz
// A row is eight numbers: family, three arguments, four answers.
//   0  nk1, k, 0          -> H, key bytes, entries, 0              (the wide join's table)
//   1  n, 0, 0            -> np, launches of the sort, 0, 0
//   2  n, nk2, edit_pairs -> per, launches of the edit pass, 0, 0
//   3  len1, n2, inv      -> o_r1, o_s2, bytes, 0                  (the symbol buffer)
//   4  maxi, maxj, 0      -> R, shift, scratch bytes, 0
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>

static const int ANYK_TILE = 512, ANYK_EDIT_WAVES = 4;

static size_t anyk_pad(int n) { return ((size_t)n + 16 + 15) & ~(size_t)15; }

static bool g_first = true;
static void row(int fam, long long a, long long b, long long c, long long r0, long long r1, long long r2, long long r3)
{
    std::printf("%s[%d,%lld,%lld,%lld,%lld,%lld,%lld,%lld]", g_first ? "" : ",\n", fam, a, b, c, r0, r1, r2, r3);
    g_first = false;
}

int main()
{
    std::mt19937_64 rng(20261021);
    auto upto = [&](long long top) { return (long long)(rng() % (unsigned long long)top); };
    std::printf("{\"what\": \"family, three arguments, four answers (tools/dots_plan_fixture.cpp)\", \"rows\": [\n");
    // the wide join: WideRoute::count
    for (int t = 0; t < 1000; ++t) {
        const int nk1 = t < 300 ? 1 + t : t < 600 ? (int)(1 + upto(70000)) : (int)(1 + upto(1 << 20));
        const int k = 10 * (1 + t % 4);
        const int64_t ne = 2 * (int64_t)nk1;
        uint32_t H;
        for (H = 1; (int64_t)H < 2 * ne;) H <<= 1;
        row(0, nk1, k, 0, H, (long long)((size_t)ne * sizeof(uint32_t) * ((4 * k + 31) / 32)), ne, 0);
    }
    // the sort: anyk_count
    for (int t = 0; t < 800; ++t) {
        const int n = t < 40 ? (t % 2 ? (1 << (t / 2 + 2)) + 1 : 1 << (t / 2 + 2)) : t < 400 ? (int)(1 + upto(5000)) : (int)(1 + upto(1 << 21));
        int np = ANYK_TILE;
        while (np < n) np <<= 1;
        int launches = 1;
        for (int kk = 2 * ANYK_TILE; kk <= np; kk <<= 1) {
            for (int jj = kk >> 1; jj >= ANYK_TILE; jj >>= 1) ++launches;
            ++launches;
        }
        row(1, n, 0, 0, np, launches, 0, 0);
    }
    // the edit cut: anyk_edit_launch
    const long long caps[] = {1, 4, 1008, 2016, 16128, 1ll << 20, 1ll << 31, 1ll << 40, INT64_MAX};
    for (int t = 0; t < 900; ++t) {
        const int n = t % 3 == 0 ? (int)(1 + upto(600)) : (int)(1 + upto(1 << 21));
        const int nk2 = t % 5 == 0 ? (int)(1 + upto(500)) : (int)(1 + upto(1 << 20));
        const long long edit_pairs = t % 2 ? caps[t % 9] : 1 + upto(1ll << 34);
        const long long per = std::max<long long>(ANYK_EDIT_WAVES, edit_pairs / std::max(n, 1) / ANYK_EDIT_WAVES * ANYK_EDIT_WAVES);
        long long launches = 0;
        for (long long j0 = 0; j0 < nk2; j0 += per) ++launches;
        row(2, n, nk2, edit_pairs, per, launches, 0, 0);
    }
    // the symbol buffer: AnykRoute::count
    for (int t = 0; t < 600; ++t) {
        const int len1 = t < 200 ? t : (int)upto(1 << 20), n2 = t < 200 ? (int)upto(300) : (int)upto(1 << 20);
        const bool inv = t % 2;
        const size_t o_r1 = anyk_pad(len1), o_s2 = o_r1 + (inv ? anyk_pad(len1) : 0);
        row(3, len1, n2, inv, (long long)o_r1, (long long)o_s2, (long long)(o_s2 + anyk_pad(n2)), 0);
    }
    // the cleaning's scratch: wide_clean
    for (int t = 0; t < 500; ++t) {
        const int maxi = t < 100 ? (int)upto(50) : (int)upto(1 << 20), maxj = t < 100 ? (int)upto(50) : (int)upto(1 << 20);
        const int R = maxi + maxj + 1, shift = maxj;
        row(4, maxi, maxj, 0, R, shift, (long long)(sizeof(uint32_t) * 3 * (size_t)R), 0);
    }
    std::printf("\n]}\n");
    return 0;
}
