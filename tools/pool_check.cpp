// pool_check.cpp - the block pool's policy (vapor_amd/csrc/vapor_pool.h) held to direct statements of its rules over fake
// allocators, as a program of its own under the address and undefined-behaviour sanitizers (tests/test_pool_cpu.py builds and runs
// it; no HIP, no device):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ivapor_amd/csrc
//       tools/pool_check.cpp -o pool_check && ./pool_check
// The fake allocator hands out addresses it never dereferences (so 16 GiB of "device memory" cost nothing) and logs every call;
// the fake fill logs what it is given and looks at what the caller can see at that moment.
#include "vapor_pool.h"

#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

namespace vp = vapor_pool;

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

constexpr size_t KiB = 1024, MiB = 1024 * KiB, GiB = 1024 * MiB;

// What the library would do with the device, recorded instead of done.
struct Fake {
    struct Alloc { void* p; size_t cap; bool host; };
    struct Fill { void* p; size_t cap; bool host; int byte; };
    std::vector<Alloc> allocs;
    std::vector<Fill> fills;
    std::vector<std::pair<void*, bool>> releases;
    std::set<void*> live;
    uintptr_t next = 0x100000;
    int fail_alloc = 0, fail_fill = 0;          // the status the next call answers (0: it works)

    vp::BlockPool pool;

    int take(void** out, size_t bytes, bool host)
    {
        return vp::take(
            pool, out, bytes, host,
            [this](void** o, size_t cap, bool h) {
                if (fail_alloc) return fail_alloc;
                *o = reinterpret_cast<void*>(next);
                next += (cap + 0xFFF) & ~(uintptr_t)0xFFF;
                allocs.push_back({*o, cap, h});
                live.insert(*o);
                return 0;
            },
            [this](void* p, size_t cap, bool h, int byte) {
                fills.push_back({p, cap, h, byte});
                return fail_fill;
            });
    }
    void* must_take(size_t bytes, bool host)
    {
        void* p = nullptr;
        const int e = take(&p, bytes, host);
        CHECK(e == 0 && p != nullptr, "a request of %zu bytes", bytes);
        return p;
    }
    void give(void* p, bool host, bool alive = true)
    {
        vp::give(alive ? &pool : nullptr, p, host, [this](void* q, bool h) {
            releases.push_back({q, h});
            live.erase(q);
        });
    }
    // the pool's books: the cached byte counts are the sums of the free lists, and every free block is known by its capacity
    void check_books(const char* where)
    {
        size_t d = 0, h = 0;
        for (auto& b : pool.free_dev) {
            d += b.first;
            auto it = pool.cap_of.find(b.second);
            CHECK(it != pool.cap_of.end() && it->second == b.first, "%s: a free device block of %zu bytes", where, b.first);
        }
        for (auto& b : pool.free_host) {
            h += b.first;
            auto it = pool.cap_of.find(b.second);
            CHECK(it != pool.cap_of.end() && it->second == b.first, "%s: a free pinned block of %zu bytes", where, b.first);
        }
        CHECK(d == pool.cached_dev && h == pool.cached_host, "%s: cached %zu / %zu, lists %zu / %zu", where, pool.cached_dev, pool.cached_host, d, h);
    }
};

// the rounding written out longhand: 256, the next power of two below 64 KiB, the next multiple of 64 KiB from there
static size_t round_longhand(size_t bytes)
{
    if (bytes <= 256) return 256;
    for (size_t p = 512; p <= 32 * KiB; p *= 2)
        if (bytes <= p) return p;
    if (bytes <= 64 * KiB) return 64 * KiB;
    return (bytes + 64 * KiB - 1) / (64 * KiB) * (64 * KiB);
}

static void check_round()
{
    long long n = 0;
    CHECK(vp::pool_round(0) == 256 && vp::pool_round(1) == 256 && vp::pool_round(255) == 256 && vp::pool_round(256) == 256 && vp::pool_round(257) == 512,
          "both sides of 256");
    ++n;
    for (size_t p = 256; p <= 64 * KiB; p *= 2) {       // every power of two up to 64 KiB: itself, one below stays, one above goes up
        CHECK(vp::pool_round(p) == p, "%zu", p);
        CHECK(vp::pool_round(p - 1) == p, "%zu - 1", p);
        CHECK(vp::pool_round(p + 1) == (p < 64 * KiB ? 2 * p : p + 64 * KiB), "%zu + 1", p);
        ++n;
    }
    for (size_t k = 1; k <= 4096; k = k < 40 ? k + 1 : k * 2 + 1) {     // the 64 KiB steps above
        const size_t s = k * 64 * KiB;
        CHECK(vp::pool_round(s) == s && vp::pool_round(s - 1) == s && vp::pool_round(s + 1) == s + 64 * KiB, "step %zu", k);
        ++n;
    }
    CHECK(vp::pool_round(16 * GiB + 1) == 16 * GiB + 64 * KiB, "above 16 GiB");
    for (size_t b = 0; b <= 300 * KiB; ++b) CHECK(vp::pool_round(b) == round_longhand(b) && vp::pool_round(b) >= b, "%zu bytes", b);
    std::printf("round: %lld edges and every size to 300 KiB\n", n);
}

// A request is served from the free list exactly when a block lies in [cap, 2 cap + 1 MiB], and by the smallest such block.
static void check_window()
{
    long long n = 0;
    const size_t requests[] = {1, 256, 300, 4000, 65535, 65536, 65537, 200000, 1 * MiB, 5 * MiB + 3, 300 * MiB};
    for (int host = 0; host < 2; ++host)
        for (size_t req : requests) {
            const size_t cap = vp::pool_round(req), end = 2 * cap + 1 * MiB;
            CHECK(vp::window_end(cap) == end, "window of %zu", cap);
            // the capacities a block can have around both ends (a capacity is a rounded size: the nearest ones, and one byte
            // either side by way of a block the pool is told about directly)
            struct Case { size_t have; bool served; };
            const Case cases[] = {{cap - 1, false}, {cap, true}, {cap + 1, true}, {end - 1, true}, {end, true}, {end + 1, false}};
            for (const Case& c : cases) {
                Fake f;
                void* blk = reinterpret_cast<void*>((uintptr_t)0x7000000);
                f.pool.cap_of[blk] = c.have;                 // a block of exactly this capacity lies free
                (host ? f.pool.free_host : f.pool.free_dev).emplace(c.have, blk);
                (host ? f.pool.cached_host : f.pool.cached_dev) = c.have;
                // ... and one of the other kind, which never serves
                void* other = reinterpret_cast<void*>((uintptr_t)0x9000000);
                f.pool.cap_of[other] = cap;
                (host ? f.pool.free_dev : f.pool.free_host).emplace(cap, other);
                (host ? f.pool.cached_dev : f.pool.cached_host) = cap;
                void* got = f.must_take(req, host != 0);
                CHECK((got == blk) == c.served, "request %zu (cap %zu), a free block of %zu", req, cap, c.have);
                CHECK(f.allocs.size() == (c.served ? 0u : 1u), "request %zu, block %zu: %zu allocations", req, c.have, f.allocs.size());
                if (!c.served) CHECK(f.allocs[0].cap == cap && f.allocs[0].host == (host != 0) && f.pool.cap_of[got] == cap, "a fresh block of %zu", cap);
                CHECK((host ? f.pool.cached_host : f.pool.cached_dev) == (c.served ? 0 : c.have), "request %zu, block %zu: cached bytes", req, c.have);
                CHECK(got != other && (host ? f.pool.free_dev : f.pool.free_host).size() == 1, "the other kind's block stays");
                f.check_books("window");
                ++n;
            }
        }
    // the smallest block in the window, whatever the order they came back in; blocks below and above stay
    {
        Fake f;
        const size_t sizes[] = {3 * MiB, 64 * KiB, 1 * MiB + 64 * KiB, 2 * MiB, 40 * MiB, 1 * MiB, 2 * MiB};
        std::vector<void*> blk;
        for (size_t s : sizes) blk.push_back(f.must_take(s, false));
        CHECK(f.allocs.size() == 7, "seven fresh blocks");
        for (void* p : blk) f.give(p, false);
        f.check_books("all back");
        CHECK(f.pool.free_dev.size() == 7 && f.releases.empty(), "all seven cached");
        void* a = f.must_take(1 * MiB + 1, false);           // cap 1 MiB + 64 KiB, window to 3 MiB + 128 KiB
        CHECK(a == blk[2], "the 1 MiB + 64 KiB block serves, not the 2 MiB or 3 MiB ones");
        void* b = f.must_take(1 * MiB + 1, false);
        CHECK(b == blk[3] || b == blk[6], "then a 2 MiB one");
        void* c = f.must_take(1 * MiB + 1, false);
        CHECK((c == blk[3] || c == blk[6]) && c != b, "then the other 2 MiB one");
        void* d = f.must_take(1 * MiB + 1, false);
        CHECK(d == blk[0], "then the 3 MiB one");
        void* e = f.must_take(1 * MiB + 1, false);           // 40 MiB lies outside: fresh
        CHECK(f.allocs.size() == 8 && e == f.allocs[7].p && f.allocs[7].cap == 1 * MiB + 64 * KiB, "then a fresh one");
        void* g = f.must_take(100, false);                   // cap 256, window to 1 MiB + 512: the 64 KiB and 1 MiB blocks lie in it
        CHECK(g == blk[1], "256 bytes are served by the 64 KiB block");
        void* h = f.must_take(100, false);
        CHECK(h == blk[5], "then by the 1 MiB block");
        void* i = f.must_take(100, false);
        CHECK(f.allocs.size() == 9 && i == f.allocs[8].p && f.allocs[8].cap == 256, "then by a fresh one of 256");
        CHECK(f.pool.free_dev.size() == 1 && f.pool.cached_dev == 40 * MiB, "the 40 MiB block is still free");
        f.check_books("smallest first");
        n += 9;
    }
    std::printf("window: %lld requests, served exactly inside [cap, 2 cap + 1 MiB], smallest block first\n", n);
}

// A block comes back: cached up to the limit and including it, released beyond; unknown pointers and dead contexts release.
static void check_limits()
{
    long long n = 0;
    for (int host = 0; host < 2; ++host) {
        const size_t limit = host ? 2 * GiB : 16 * GiB;
        CHECK(limit == (host ? vp::HOST_CACHE_MAX : vp::DEV_CACHE_MAX), "the limits");
        for (int over = 0; over < 2; ++over) {
            Fake f;
            // blocks that fill the cache to 64 KiB below the limit, then one that reaches the limit exactly or passes it by 64 KiB
            std::vector<void*> blk;
            const size_t big = limit / 4;
            for (int i = 0; i < 3; ++i) blk.push_back(f.must_take(big, host != 0));
            blk.push_back(f.must_take(big - 64 * KiB, host != 0));
            void* last = f.must_take(64 * KiB + (over ? 1 : 0), host != 0);
            void* small = f.must_take(10, host != 0);
            for (void* p : blk) f.give(p, host != 0);
            CHECK((host ? f.pool.cached_host : f.pool.cached_dev) == limit - 64 * KiB && f.releases.empty(), "64 KiB below the limit");
            f.give(last, host != 0);
            if (!over) {
                CHECK(f.releases.empty() && (host ? f.pool.cached_host : f.pool.cached_dev) == limit, "a block that reaches the limit exactly is kept");
                f.give(small, host != 0);
                CHECK(f.releases.size() == 1 && f.releases[0].first == small && f.releases[0].second == (host != 0), "the next one, 256 bytes, is released");
                CHECK(!f.pool.cap_of.count(small), "... and forgotten");
            } else {
                CHECK(f.releases.size() == 1 && f.releases[0].first == last && f.releases[0].second == (host != 0) && !f.pool.cap_of.count(last),
                      "a block that passes the limit by 64 KiB is released and forgotten");
                CHECK((host ? f.pool.cached_host : f.pool.cached_dev) == limit - 64 * KiB, "the cache is as it was");
                f.give(small, host != 0);
                CHECK(f.releases.size() == 1 && (host ? f.pool.cached_host : f.pool.cached_dev) == limit - 64 * KiB + 256, "a smaller one still fits");
            }
            // the other kind's cache is not charged
            CHECK((host ? f.pool.cached_dev : f.pool.cached_host) == 0, "the other kind's cache");
            f.check_books("limits");
            n += 2;
        }
    }
    {
        Fake f;
        void* mine = f.must_take(1000, false);
        int local = 0;
        void* foreign = &local;
        f.give(foreign, false);                                  // a pointer the pool never handed out
        CHECK(f.releases.size() == 1 && f.releases[0].first == foreign && !f.releases[0].second && f.pool.free_dev.empty(), "a foreign pointer is released directly");
        f.give(foreign, true);
        CHECK(f.releases.size() == 2 && f.releases[1].second && f.pool.free_host.empty(), "... as the kind the caller names");
        f.give(nullptr, false);
        CHECK(f.releases.size() == 2, "a null pointer is nobody's");
        f.give(mine, false, /*alive=*/false);                    // the context is gone: released, the lists untouched
        CHECK(f.releases.size() == 3 && f.releases[2].first == mine && f.pool.free_dev.empty() && f.pool.cached_dev == 0, "a block of a dead context is released");
        // a failing allocation is handed on and nothing is remembered
        f.fail_alloc = 2;
        void* p = nullptr;
        const size_t known = f.pool.cap_of.size();
        CHECK(f.take(&p, 5000, false) == 2 && p == nullptr && f.pool.cap_of.size() == known, "a failing allocation");
        n += 5;
    }
    std::printf("limits: %lld give-backs, kept up to 16 GiB / 2 GiB and no further, foreign pointers released\n", n);
}

// Under fill: once per hand-out, fresh or recycled, over the block's capacity, before the pointer is returned; never when off.
static void check_fill()
{
    long long n = 0;
    for (int host = 0; host < 2; ++host) {
        Fake f;
        // off: no fill, whatever is handed out
        void* a = f.must_take(100000, host != 0);                // cap 128 KiB
        f.give(a, host != 0);
        void* b = f.must_take(70000, host != 0);
        CHECK(b == a && f.fills.empty(), "fill off: no call");
        f.give(b, host != 0);
        n += 2;
        for (int byte : {0xFF, 0x5A, 0}) {
            f.pool.fill = byte;
            const size_t before = f.fills.size();
            // recycled: a request of 1000 bytes (cap 1024) gets the 128 KiB block - and the fill its 128 KiB
            void* c = f.must_take(1000, host != 0);
            CHECK(c == a && f.fills.size() == before + 1, "one fill for a recycled block");
            CHECK(f.fills.back().p == a && f.fills.back().cap == 128 * KiB && f.fills.back().host == (host != 0) && f.fills.back().byte == byte,
                  "the fill of a recycled block: %zu bytes of 0x%02X", f.fills.back().cap, f.fills.back().byte);
            // fresh: 70001 bytes round to 128 KiB - the fill gets the capacity, not the request
            void* d = f.must_take(70001, host != 0);
            CHECK(d != a && f.fills.size() == before + 2 && f.fills.back().p == d && f.fills.back().cap == 128 * KiB && f.fills.back().byte == byte,
                  "the fill of a fresh block: %zu bytes", f.fills.back().cap);
            f.give(c, host != 0);
            f.give(d, host != 0);
            n += 2;
        }
        // before the pointer is returned: take() has not answered yet when the fill runs, and a fill that fails keeps the block
        {
            f.pool.fill = 0x5A;
            f.fail_fill = 7;
            void* p = reinterpret_cast<void*>((uintptr_t)1);
            const size_t cached = host ? f.pool.cached_host : f.pool.cached_dev, fills = f.fills.size();
            const int e = f.take(&p, 1000, host != 0);
            CHECK(e == 7 && p == nullptr && f.fills.size() == fills + 1, "a failing fill is handed on, the caller gets no block");
            CHECK((host ? f.pool.cached_host : f.pool.cached_dev) == cached, "... and the block is back in the list");
            f.fail_fill = 0;
            f.check_books("failed fill");
            ++n;
        }
        f.pool.fill = vp::FILL_OFF;
        const size_t fills = f.fills.size();
        void* e = f.must_take(1000, host != 0);
        void* g = f.must_take(1 << 20, host != 0);
        CHECK(f.fills.size() == fills && e && g, "fill off again: no call");
        ++n;
    }
    // the order of events inside one hand-out: allocation, then fill, then the answer
    {
        struct Ev { char what; size_t cap; };
        std::vector<Ev> ev;
        vp::BlockPool pool;
        pool.fill = 0xFF;
        static char arena[512];
        void* out = nullptr;
        void** outp = &out;
        const int e = vp::take(
            pool, &out, 300, false,
            [&](void** o, size_t cap, bool) { ev.push_back({'a', cap}); *o = arena; return 0; },
            [&](void* p, size_t cap, bool, int byte) {
                ev.push_back({'f', cap});
                for (size_t i = 0; i < cap; ++i) static_cast<char*>(p)[i] = (char)byte;      // (a real fill: the capacity is there to write)
                CHECK(p == arena && *outp == arena, "the fill sees the block");
                return 0;
            });
        ev.push_back({'r', 0});
        CHECK(e == 0 && out == arena && ev.size() == 3 && ev[0].what == 'a' && ev[0].cap == 512 && ev[1].what == 'f' && ev[1].cap == 512 && ev[2].what == 'r',
              "allocate, fill, return");
        CHECK((unsigned char)arena[0] == 0xFF && (unsigned char)arena[511] == 0xFF, "filled to the last byte of the capacity");
        ++n;
    }
    CHECK(vp::valid_fill(-1) && vp::valid_fill(0) && vp::valid_fill(255) && !vp::valid_fill(-2) && !vp::valid_fill(256) && !vp::valid_fill(1LL << 40),
          "the parameter's range");
    std::printf("fill: %lld hand-outs, one fill each over the block's capacity before the answer, none when off\n", n);
}

// A sequence of calls as the library makes them - a mix of sizes taken and given back in rounds - against a model of the rules
// written out longhand over plain vectors: the same blocks served, the same fresh allocations in the same order and sizes.
static void check_sequence()
{
    struct Free { size_t cap; int id; uint64_t seq; };
    Fake f;
    std::vector<Free> model_free;                                // the model's free device list
    std::vector<size_t> model_cap;                               // by block id
    std::vector<void*> addr;
    uint64_t seq = 0, state = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
    long long n = 0, recycled = 0;
    for (int round = 0; round < 200; ++round) {
        std::vector<int> held;
        const int k = 1 + (int)(rnd() % 12);
        for (int i = 0; i < k; ++i) {
            const int sh = (int)(rnd() % 24);
            const size_t bytes = ((size_t)1 << sh) + rnd() % ((size_t)1 << sh);
            const size_t cap = round_longhand(bytes);
            int best = -1;                                       // the smallest free block in the window, the one that came back first among equals
            for (int j = 0; j < (int)model_free.size(); ++j) {
                const Free& c = model_free[j];
                if (c.cap < cap || c.cap > 2 * cap + 1 * MiB) continue;
                if (best < 0 || c.cap < model_free[best].cap || (c.cap == model_free[best].cap && c.seq < model_free[best].seq)) best = j;
            }
            const size_t allocs = f.allocs.size();
            void* p = f.must_take(bytes, false);
            if (best >= 0) {
                CHECK(p == addr[model_free[best].id] && f.allocs.size() == allocs, "round %d: %zu bytes from the free list", round, bytes);
                held.push_back(model_free[best].id);
                model_free.erase(model_free.begin() + best);
                ++recycled;
            } else {
                CHECK(f.allocs.size() == allocs + 1 && f.allocs.back().cap == cap && f.allocs.back().p == p, "round %d: a fresh block of %zu", round, cap);
                held.push_back((int)addr.size());
                addr.push_back(p);
                model_cap.push_back(cap);
            }
            ++n;
        }
        for (int id : held) {
            f.give(addr[id], false);
            model_free.push_back({model_cap[id], id, seq++});
        }
        f.check_books("sequence");
        CHECK(f.pool.free_dev.size() == model_free.size(), "round %d: %zu free blocks, the model %zu", round, f.pool.free_dev.size(), model_free.size());
    }
    CHECK(recycled > n / 2 && f.releases.empty(), "%lld of %lld recycled", recycled, n);
    std::printf("sequence: 200 rounds of requests, the blocks and fresh allocations of the rules written out longhand\n");
}

int main()
{
    check_round();
    check_window();
    check_limits();
    check_fill();
    check_sequence();
    if (g_bad) {
        std::printf("pool_check: %d statements FAILED\n", g_bad);
        return 1;
    }
    std::printf("pool_check: all equal\n");
    return 0;
}
