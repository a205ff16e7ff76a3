// pcl_pool.hip -- the process-wide caching pool every device allocation of the library comes from (pcl_pool_alloc / pcl_pool_free, pcl_own.h).
#include <map>
#include <mutex>
#include <unordered_map>

#include "pcl_internal.h"

// ================================================================ device memory pool
// Size classes: powers of two up to 1 MiB, eighths of a power of two above (a block wastes < 12.5 %), so that batches of
// similar shape -- the chunks of a ragged stream, the one-utterance batches of the drop-in classes -- reuse each other's
// blocks.  The cache is trimmed (largest blocks first) when it exceeds PCL_POOL_MAX_MB (default 65536), and released
// altogether before an allocation is reported as failed.
thread_local int pcl_tls_free_synced = 0;
namespace {
struct PoolBlock { size_t bytes; int device; };
std::mutex g_pool_mu;
std::unordered_map<void *, PoolBlock> g_pool_live;                 // every block handed out or cached
std::multimap<std::pair<int, size_t>, void *> g_pool_free;           // (device, class bytes) -> cached block
size_t g_pool_cached = 0;
uint64_t g_pool_device_allocs = 0, g_pool_device_waits = 0;         // successful hipMalloc calls / device-wide waits of pcl_pool_free (pcl_pool_stats)
size_t pool_class(size_t n) {
    if (n <= 256) return 256;
    size_t p2 = 256;
    while (p2 < n) p2 <<= 1;
    if (p2 <= (1u << 20)) return p2;
    const size_t step = p2 >> 4;                                    // eighths of the lower power of two
    return (n + step - 1) / step * step;
}
size_t pool_limit() {
    static const size_t lim = (size_t)(getenv("PCL_POOL_MAX_MB") ? atol(getenv("PCL_POOL_MAX_MB")) : 65536) << 20;
    return lim;
}
void pool_release_locked(size_t keep) {                              // hipFree cached blocks, largest first, down to `keep` bytes
    while (g_pool_cached > keep && !g_pool_free.empty()) {
        auto best = g_pool_free.begin();
        for (auto it = g_pool_free.begin(); it != g_pool_free.end(); ++it)
            if (it->first.second > best->first.second) best = it;
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != best->first.first) (void)hipSetDevice(best->first.first);
        (void)hipFree(best->second);
        if (cur != best->first.first) (void)hipSetDevice(cur);
        g_pool_cached -= best->first.second;
        g_pool_live.erase(best->second);
        g_pool_free.erase(best);
    }
}
}  // namespace

void *pcl_pool_alloc(int device, size_t bytes) {
    const size_t cls = pool_class(bytes);
    std::lock_guard<std::mutex> lock(g_pool_mu);
    auto it = g_pool_free.find(std::make_pair(device, cls));
    if (it != g_pool_free.end()) {
        void *p = it->second;
        g_pool_free.erase(it);
        g_pool_cached -= cls;
        return p;
    }
    void *p = nullptr;
    if (hipMalloc(&p, cls) != hipSuccess) {
        (void)hipGetLastError();
        pool_release_locked(0);                                      // give the cache back and try once more
        if (hipMalloc(&p, cls) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
    }
    ++g_pool_device_allocs;
    g_pool_live[p] = PoolBlock{cls, device};                        // (overwrites a stale entry, should a block ever have left the pool by a raw hipFree)
    return p;
}

void pcl_pool_free(void *p) {
    if (!p) return;
    const bool wait = pcl_tls_free_synced <= 0;
    if (wait) (void)hipDeviceSynchronize();                         // what hipFree did: nobody on the device still uses the block
    std::lock_guard<std::mutex> lock(g_pool_mu);
    if (wait) ++g_pool_device_waits;
    auto it = g_pool_live.find(p);
    if (it == g_pool_live.end()) {                                   // not ours (never happens): the runtime's problem
        (void)hipFree(p);
        return;
    }
    g_pool_free.emplace(std::make_pair(it->second.device, it->second.bytes), p);
    g_pool_cached += it->second.bytes;
    if (g_pool_cached > pool_limit()) pool_release_locked(pool_limit() / 2);
}

extern "C" int pcl_pool_stats(size_t *handed_out_blocks, size_t *handed_out_bytes, size_t *cached_bytes, uint64_t *device_allocs, uint64_t *device_waits) {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    size_t live_bytes = 0;
    for (const auto &kv : g_pool_live) live_bytes += kv.second.bytes;
    if (handed_out_blocks) *handed_out_blocks = g_pool_live.size() - g_pool_free.size();
    if (handed_out_bytes) *handed_out_bytes = live_bytes - g_pool_cached;
    if (cached_bytes) *cached_bytes = g_pool_cached;
    if (device_allocs) *device_allocs = g_pool_device_allocs;
    if (device_waits) *device_waits = g_pool_device_waits;
    return PCL_OK;
}
