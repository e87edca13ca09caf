// vapor_pool.h - the policy of a context's block pool, without HIP: which capacity a request is rounded to
// (pool_round), which free block serves it (the smallest whose capacity lies in [cap, 2 * cap + WINDOW_SLACK]), what the pool
// remembers of a block (cap_of), which blocks it keeps when they come back (the caching limits) and which it releases at once.
// Allocating, releasing and filling come in as callables: the functions in vapor_hip.hip hand hipMalloc / hipHostMalloc,
// hipFree / hipHostFree and the test fill to them, tools/pool_check.cpp hands fakes and holds the rules to direct statements on
// the host under the sanitizers.  One host thread per context (include/vapor_hip.h), so the lists need no lock.
#pragma once

#include <cstddef>
#include <map>

namespace vapor_pool {

constexpr size_t WINDOW_SLACK = (size_t)1 << 20;         // a free block of up to 2 * cap + this many bytes serves a request of cap
constexpr size_t DEV_CACHE_MAX = (size_t)16 << 30;       // bytes of free device blocks a pool keeps: a block that would pass it is released
constexpr size_t HOST_CACHE_MAX = (size_t)2 << 30;       // ... and of free pinned blocks
constexpr int FILL_OFF = -1;                             // BlockPool::fill: hand blocks out as they are

struct BlockPool {
    std::multimap<size_t, void*> free_dev, free_host;
    std::map<const void*, size_t> cap_of;               // capacity of every block this pool has handed out or holds
    size_t cached_dev = 0, cached_host = 0;
    int fill = FILL_OFF;                                // test parameter pool_fill: 0 .. 255, the byte every block is filled with at hand-out
};

inline size_t pool_round(size_t bytes)
{
    if (bytes <= 256) return 256;
    if (bytes < ((size_t)1 << 16)) { size_t c = 256; while (c < bytes) c <<= 1; return c; }
    return (bytes + 0xFFFF) & ~(size_t)0xFFFF;          // 64 KB steps above that
}

inline size_t window_end(size_t cap) { return 2 * cap + WINDOW_SLACK; }     // the largest capacity that serves a request rounded to cap
inline bool valid_fill(long long v) { return v >= FILL_OFF && v <= 255; }

// A block of at least `bytes`: the smallest free one in the window, else a fresh one of pool_round(bytes) from
// allocate(out, cap, host) -> status (0: done; any other value is handed on and nothing is remembered).  With pool.fill set,
// fill(block, capacity, host, byte) -> status runs once before the block is handed out, over the capacity the pool knows the
// block by - a recycled block's own, not the request's; a block whose fill fails stays with the pool and *out is null.
template <typename Allocate, typename Fill>
inline int take(BlockPool& pool, void** out, size_t bytes, bool host, Allocate&& allocate, Fill&& fill)
{
    size_t cap = pool_round(bytes);
    auto& fl = host ? pool.free_host : pool.free_dev;
    size_t& cached = host ? pool.cached_host : pool.cached_dev;
    auto it = fl.lower_bound(cap);
    if (it != fl.end() && it->first <= window_end(cap)) {
        *out = it->second;
        cap = it->first;
        cached -= cap;
        fl.erase(it);
    } else {
        const int e = allocate(out, cap, host);
        if (e != 0) return e;
        pool.cap_of[*out] = cap;
    }
    if (pool.fill == FILL_OFF) return 0;
    const int e = fill(*out, cap, host, pool.fill);
    if (e != 0) {
        fl.emplace(cap, *out);
        cached += cap;
        *out = nullptr;
    }
    return e;
}

// A block comes back.  `pool` is null when its context is gone.  A block the pool handed out joins the free list unless the
// cached bytes would pass the limit; that one, and a pointer the pool does not know, goes to release(p, host).
template <typename Release>
inline void give(BlockPool* pool, void* p, bool host, Release&& release)
{
    if (!p) return;
    if (pool) {
        auto it = pool->cap_of.find(p);
        if (it != pool->cap_of.end()) {
            size_t& cached = host ? pool->cached_host : pool->cached_dev;
            if (cached + it->second <= (host ? HOST_CACHE_MAX : DEV_CACHE_MAX)) {
                (host ? pool->free_host : pool->free_dev).emplace(it->second, p);
                cached += it->second;
                return;
            }
            pool->cap_of.erase(it);
        }
    }
    release(p, host);
}

}  // namespace vapor_pool
