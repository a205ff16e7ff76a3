// Stand-alone check of the owning types of the host runtime (poccala_amd/csrc/pcl_own.h: device buffer, handle, handle pair, page-locked
// buffer) and of the descriptor stager's bookkeeping (pcl_desc.h) against malloc-backed, counting stubs: no call reaches the HIP runtime.
// Built with the host sanitizers and run as its own process by tests/test_devbuf_host.py: exit status 0 and no sanitizer report = pass.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <vector>

#include "../poccala_amd/csrc/pcl_own.h"
#include "../poccala_amd/csrc/pcl_desc.h"

struct pcl_ctx {
    int device = 0;
    std::string err;
};
int pcl_ctx_device(const pcl_ctx *ctx) { return ctx->device; }
void pcl_set_error(pcl_ctx *ctx, const char *msg) { ctx->err = msg; }
thread_local int pcl_tls_free_synced = 0;

static std::set<void *> g_live;
static long g_allocs = 0, g_frees = 0, g_waits = 0;
static bool g_fail_next = false;
void *pcl_pool_alloc(int, size_t bytes) {
    if (g_fail_next) {
        g_fail_next = false;
        return nullptr;
    }
    void *p = malloc(bytes);
    g_live.insert(p);
    ++g_allocs;
    return p;
}
void pcl_pool_free(void *p) {
    if (!p) return;
    if (pcl_tls_free_synced <= 0) ++g_waits;
    if (!g_live.erase(p)) {
        fprintf(stderr, "FAIL: free of a block that is not live\n");
        exit(2);
    }
    ++g_frees;
    free(p);
}

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

// a handle that counts: create hands out 1, 2, 3 ... and fails when told to; destroy insists on a live handle
static std::set<long> g_handles;
static long g_made = 0, g_destroyed = 0;
static int g_fail_create_in = 0;             // n > 0: the n-th create from now fails
struct CountOps {
    static hipError_t create(long *h) {
        if (g_fail_create_in > 0 && --g_fail_create_in == 0) return hipErrorOutOfMemory;
        *h = ++g_made;
        g_handles.insert(*h);
        return hipSuccess;
    }
    static void destroy(long h) {
        if (!g_handles.erase(h)) {
            fprintf(stderr, "FAIL: destroy of a handle that is not live\n");
            exit(2);
        }
        ++g_destroyed;
    }
};
using Handle = Owned<long, CountOps>;

// page-locked memory from malloc, counted
static std::set<void *> g_pins;
static long g_pin_allocs = 0, g_pin_frees = 0;
static bool g_pin_fail_next = false;
struct StubPinOps {
    static hipError_t alloc(void **p, size_t bytes) {
        if (g_pin_fail_next) {
            g_pin_fail_next = false;
            return hipErrorOutOfMemory;
        }
        *p = malloc(bytes);
        g_pins.insert(*p);
        ++g_pin_allocs;
        return hipSuccess;
    }
    static void destroy(PinBlock b) {
        if (!g_pins.erase(b.p)) {
            fprintf(stderr, "FAIL: free of page-locked memory that is not live\n");
            exit(2);
        }
        ++g_pin_frees;
        free(b.p);
    }
};

// the stager with a small floor for its buffer, and a flush that records what it was handed (and checks it against the buffer's bytes)
constexpr size_t SMALL_MIN = 8192;          // (PCL_DESC_MAX one-byte entries fit: the table fills before the buffer does)
using Stager = DescStager<StubPinOps, SMALL_MIN>;
struct Flushed {
    DescCopyArgs a;
    std::vector<std::string> data;           // the bytes of every entry as they stood in the staging buffer
};
static std::vector<Flushed> g_flushes;
static hipError_t record_flush(const DescCopyArgs &a, const char *pin) {
    Flushed f;
    f.a = a;
    for (int k = 0; k < a.n; ++k) f.data.emplace_back(pin + a.off[k], (size_t)a.bytes[k]);
    g_flushes.push_back(f);
    return hipSuccess;
}
struct StubGroup {                           // pcl_desc_group's shape over a bare stager
    Stager &st;
    bool open = true;
    explicit StubGroup(Stager &s) : st(s) { st.enter(); }
    hipError_t finish() {
        if (!open) return hipSuccess;
        open = false;
        return st.leave(record_flush);
    }
    ~StubGroup() { (void)finish(); }
};
static int early_return(Stager &st, void *dst, const std::string &src) {
    StubGroup g(st);
    CHECK(st.stage(dst, src.data(), src.size(), record_flush) == hipSuccess);
    return PCL_ERR_INVALID;                  // no finish(): the destructor flushes
}

struct Group {
    DevBuf<double> a, b;
    DevBuf<int> c;
    int n = 0;
};

static int two_allocs(pcl_ctx *ctx, int fail_between) {
    DevBuf<float> first, second;
    TRY(first.alloc(ctx, 8));
    CHECK(g_live.size() == 1);
    TRY(fail_between);                       // the early return: `first` must go back
    TRY(second.alloc(ctx, 8));
    return PCL_OK;
}

int main() {
    pcl_ctx ctx;
    {   // alloc over a held block frees the old one; element count 0 still takes a block
        DevBuf<double> b;
        CHECK(!b && b.cap == 0);
        CHECK(b.alloc(&ctx, 10) == PCL_OK && b && b.cap == 10 && g_live.size() == 1);
        b[9] = 1.0;                          // (exactly n elements: the sanitizer watches the tenth and the eleventh)
        double *old = b;
        CHECK(b.alloc(&ctx, 20) == PCL_OK && b.cap == 20 && g_live.size() == 1 && !g_live.count(old));
        CHECK(b.alloc(&ctx, 0) == PCL_OK && b && b.cap == 0 && g_live.size() == 1);
        b.release();
        CHECK(!b && b.cap == 0 && g_live.empty());
        b.release();                         // twice is once
        CHECK(g_frees == 3);
    }
    {   // reserve grows only and keeps the pointer below the capacity
        DevBuf<int> b;
        CHECK(b.reserve(&ctx, 16) == PCL_OK && b.cap == 16);
        int *p = b;
        CHECK(b.reserve(&ctx, 4) == PCL_OK && (int *)b == p && b.cap == 16);
        CHECK(b.reserve(&ctx, 16) == PCL_OK && (int *)b == p);
        CHECK(b.reserve(&ctx, 17) == PCL_OK && b.cap == 17 && g_live.size() == 1);
    }
    CHECK(g_live.empty());
    {   // a move leaves the source empty and the block is freed once
        const long frees = g_frees;
        DevBuf<int> a;
        CHECK(a.alloc(&ctx, 4) == PCL_OK);
        int *p = a;
        DevBuf<int> b(std::move(a));
        CHECK(!a && a.cap == 0 && (int *)b == p && b.cap == 4);
        DevBuf<int> c;
        CHECK(c.alloc(&ctx, 2) == PCL_OK);
        c = std::move(b);                    // c's own block goes, b's arrives
        CHECK(!b && (int *)c == p && c.cap == 4 && g_live.size() == 1 && g_frees == frees + 1);
        c = std::move(c);                    // self-assignment keeps it
        CHECK((int *)c == p && g_live.size() == 1);
    }
    CHECK(g_live.empty());
    {   // a struct of several buffers frees all of them on `= {}` and on destruction
        Group g;
        CHECK(g.a.alloc(&ctx, 3) == PCL_OK && g.b.alloc(&ctx, 3) == PCL_OK && g.c.alloc(&ctx, 3) == PCL_OK);
        g.n = 7;
        CHECK(g_live.size() == 3);
        g = {};
        CHECK(g_live.empty() && !g.a && !g.b && !g.c && g.n == 0);
        CHECK(g.a.alloc(&ctx, 3) == PCL_OK && g.c.alloc(&ctx, 3) == PCL_OK);
        Group *h = new Group();
        CHECK(h->b.alloc(&ctx, 5) == PCL_OK && g_live.size() == 3);
        delete h;
        CHECK(g_live.size() == 2);
    }
    CHECK(g_live.empty());
    // an early return through TRY between two allocations frees the first
    CHECK(two_allocs(&ctx, PCL_ERR_INVALID) == PCL_ERR_INVALID && g_live.empty());
    CHECK(two_allocs(&ctx, PCL_OK) == PCL_OK && g_live.empty());
    {   // a failing allocation leaves the buffer empty, also over a held block, and reports it
        DevBuf<double> b;
        CHECK(b.alloc(&ctx, 4) == PCL_OK);
        g_fail_next = true;
        ctx.err.clear();
        CHECK(b.alloc(&ctx, 8) == PCL_ERR_NOMEM && !b && b.cap == 0 && g_live.empty() && !ctx.err.empty());
        g_fail_next = true;
        CHECK(b.reserve(&ctx, 8) == PCL_ERR_NOMEM && !b && b.cap == 0);
    }
    {   // a release waits for the device unless a synced scope is open; a scope declared before a local covers its destructor
        const long waits = g_waits;
        {
            pcl_free_synced_scope done;
            DevBuf<int> covered;
            CHECK(covered.alloc(&ctx, 1) == PCL_OK);
        }
        CHECK(g_waits == waits);
        {
            DevBuf<int> bare;
            CHECK(bare.alloc(&ctx, 1) == PCL_OK);
        }
        CHECK(g_waits == waits + 1 && pcl_tls_free_synced == 0);
    }
    {   // the handle: destroyed exactly once however it travels
        {
            Handle never;                        // never made: nothing to destroy
            CHECK(!never);
        }
        CHECK(g_made == 0 && g_destroyed == 0);
        Handle a;
        CHECK(a.make() == hipSuccess && a == 1 && a.make() == hipSuccess && a == 1 && g_made == 1);   // a second make keeps it
        Handle b(std::move(a));                  // move-construct
        CHECK(!a && b == 1 && g_destroyed == 0);
        Handle c;
        CHECK(c.make() == hipSuccess && c == 2);
        c = std::move(b);                        // move-assign over a live handle: c's own goes, once
        CHECK(!b && c == 1 && g_destroyed == 1 && !g_handles.count(2));
        Handle &same = c;
        c = std::move(same);                     // self-move-assign keeps it
        CHECK(c == 1 && g_destroyed == 1 && g_handles.size() == 1);
        c.destroy();                             // explicit destroy, then the destructor: once
        CHECK(!c && g_destroyed == 2);
        c.destroy();
        CHECK(g_destroyed == 2);
    }
    CHECK(g_handles.empty() && g_made == 2 && g_destroyed == 2);
    {   // a pair is made whole or not at all
        OwnedPair<long, CountOps> p;
        g_fail_create_in = 2;
        CHECK(p.make() == hipErrorOutOfMemory && !p.first && !p.second && g_handles.empty() && g_made == 3 && g_destroyed == 3);
        g_fail_create_in = 1;
        CHECK(p.make() == hipErrorOutOfMemory && !p.first && !p.second && g_made == 3);
        CHECK(p.make() == hipSuccess && p.first && p.second && g_handles.size() == 2);
        std::vector<OwnedPair<long, CountOps>> v;
        v.push_back(std::move(p));               // (how a timer group keeps them)
        CHECK(!p.first && !p.second && g_handles.size() == 2);
        v.clear();
        CHECK(g_handles.empty());
    }
    CHECK(g_handles.empty() && g_made == g_destroyed);
    {   // the page-locked buffer
        PinBuf<short, StubPinOps> b;
        CHECK(!b && b.cap() == 0);
        CHECK(b.reserve(100) == hipSuccess && b && b.cap() == 100 && g_pin_allocs == 1);
        b[99] = 7;                               // (exactly n elements, as above)
        short *p = b;
        CHECK(b.reserve(100) == hipSuccess && b.reserve(3) == hipSuccess && (short *)b == p && g_pin_allocs == 1);   // below the capacity: nothing
        CHECK(b.reserve(101) == hipSuccess && b.cap() == 101 && g_pin_allocs == 2 && g_pin_frees == 1 && !g_pins.count(p) && g_pins.size() == 1);
        g_pin_fail_next = true;
        CHECK(b.reserve(500) == hipErrorOutOfMemory && !b && b.cap() == 0 && g_pins.empty() && g_pin_frees == 2);
        CHECK(b.reserve(8) == hipSuccess && b.cap() == 8);
        PinBuf<short, StubPinOps> c(std::move(b));
        CHECK(!b && b.cap() == 0 && c.cap() == 8 && g_pins.size() == 1);
    }
    CHECK(g_pins.empty() && g_pin_allocs == g_pin_frees);
    {   // the stager's bookkeeping
        Stager st;
        char dst[40][8];                         // destinations are only compared: any distinct addresses
        const std::string s100(100, 'a'), s300(300, 'b'), s256(256, 'c'), s1(1, 'd');
        {   // (a) offsets are multiples of 256 and do not overlap   (b) a later entry with the same destination supersedes the earlier one
            // (h) a zero-byte upload stages nothing
            StubGroup g(st);
            CHECK(st.stage(dst[0], s100.data(), 100, record_flush) == hipSuccess);
            CHECK(st.pin.cap() == SMALL_MIN && g_pin_allocs - g_pin_frees == 1);              // the first array outgrew the empty buffer: the floor
            CHECK(st.stage(dst[1], s300.data(), 300, record_flush) == hipSuccess);
            CHECK(st.stage(dst[2], s256.data(), 256, record_flush) == hipSuccess);
            CHECK(st.stage(dst[3], s1.data(), 0, record_flush) == hipSuccess && st.pending.n == 3);
            CHECK(st.stage(dst[0], s1.data(), 1, record_flush) == hipSuccess && st.pending.n == 4);
            CHECK(g_flushes.empty() && st.used == 256 + 512 + 256 + 256);
            CHECK(g.finish() == hipSuccess && g_flushes.size() == 1 && st.used == 0 && st.pending.n == 0 && st.group == 0);
            const Flushed &f = g_flushes[0];
            CHECK(f.a.n == 4);
            for (int k = 0; k < 4; ++k) {
                CHECK(f.a.off[k] % 256 == 0);
                if (k) CHECK(f.a.off[k] >= f.a.off[k - 1] + ((k == 1 ? 100 : k == 2 ? 300 : 256) + 255) / 256 * 256);
            }
#ifndef PCL_DESC_RACE_REPRO
            CHECK(f.a.dst[0] == dst[0] && f.a.bytes[0] == 0);                                // superseded
#else
            CHECK(f.a.dst[0] == dst[0] && f.a.bytes[0] == 100);                              // (the mutation build disables exactly this)
#endif
            CHECK(f.a.dst[3] == dst[0] && f.a.bytes[3] == 1 && f.data[3] == s1);
            CHECK(f.a.dst[1] == dst[1] && f.a.bytes[1] == 300 && f.data[1] == s300 && f.a.bytes[2] == 256 && f.data[2] == s256);
        }
        g_flushes.clear();
        {   // (c) entry 25 of a group forces a flush of the first 24 before it is staged
            StubGroup g(st);
            for (int k = 0; k < PCL_DESC_MAX; ++k) CHECK(st.stage(dst[k], s1.data(), 1, record_flush) == hipSuccess);
            CHECK(g_flushes.empty() && st.pending.n == PCL_DESC_MAX);
            CHECK(st.stage(dst[24], s100.data(), 100, record_flush) == hipSuccess);
            CHECK(g_flushes.size() == 1 && g_flushes[0].a.n == PCL_DESC_MAX && st.pending.n == 1 && st.pending.off[0] == 0 && st.used == 256);
            CHECK(g.finish() == hipSuccess && g_flushes.size() == 2 && g_flushes[1].a.n == 1 && g_flushes[1].data[0] == s100);
        }
        g_flushes.clear();
        {   // (d) an entry that does not fit what is left forces a flush first, in the same buffer
            StubGroup g(st);
            const std::string big(SMALL_MIN - 256, 'e');
            const long allocs = g_pin_allocs;
            CHECK(st.stage(dst[0], big.data(), big.size(), record_flush) == hipSuccess && g_flushes.empty());
            CHECK(st.stage(dst[1], s300.data(), 300, record_flush) == hipSuccess);
            CHECK(g_flushes.size() == 1 && g_flushes[0].a.n == 1 && g_flushes[0].data[0] == big && g_pin_allocs == allocs);
            CHECK(st.pending.n == 1 && st.pending.off[0] == 0 && st.used == 512);
            // (e) a single array larger than the buffer: what is pending lands, then the buffer grows to max(floor, 2 x need), the old one freed once
            const std::string huge(3 * SMALL_MIN + 5, 'f');
            const long frees = g_pin_frees;
            CHECK(st.stage(dst[2], huge.data(), huge.size(), record_flush) == hipSuccess);
            CHECK(g_flushes.size() == 2 && g_flushes[1].data[0] == s300);
            CHECK(st.pin.cap() == 2 * (3 * SMALL_MIN + 256) && g_pin_allocs == allocs + 1 && g_pin_frees == frees + 1 && g_pins.size() == 1);
            CHECK(g.finish() == hipSuccess && g_flushes.size() == 3 && g_flushes[2].data[0] == huge);
            // ... and a failed growth is reported, with nothing left behind
            StubGroup g2(st);
            const std::string huger(st.pin.cap() + 1, 'g');
            g_pin_fail_next = true;
            CHECK(st.stage(dst[0], huger.data(), huger.size(), record_flush) == hipErrorOutOfMemory && !st.pin && st.pin.cap() == 0 && st.pending.n == 0);
        }
        CHECK(st.group == 0 && g_pins.empty());
        g_flushes.clear();
        {   // (f) nested groups flush once, at the outermost finish()
            StubGroup outer(st);
            CHECK(st.stage(dst[0], s100.data(), 100, record_flush) == hipSuccess);
            {
                StubGroup inner(st);
                CHECK(st.stage(dst[1], s300.data(), 300, record_flush) == hipSuccess);
                CHECK(inner.finish() == hipSuccess && g_flushes.empty() && st.group == 1);
            }
            CHECK(g_flushes.empty() && st.pending.n == 2);
            CHECK(outer.finish() == hipSuccess && g_flushes.size() == 1 && g_flushes[0].a.n == 2);
            CHECK(outer.finish() == hipSuccess && g_flushes.size() == 1 && st.group == 0);       // finish() twice is once
        }
        CHECK(g_flushes.size() == 1);
        g_flushes.clear();
        // (g) a group left by an early return flushes in its destructor
        CHECK(early_return(st, dst[5], s256) == PCL_ERR_INVALID);
        CHECK(g_flushes.size() == 1 && g_flushes[0].a.n == 1 && g_flushes[0].a.dst[0] == dst[5] && g_flushes[0].data[0] == s256 && st.group == 0);
        {   // an empty group launches nothing
            StubGroup g(st);
        }
        CHECK(g_flushes.size() == 1);
    }
    CHECK(g_pins.empty() && g_pin_allocs == g_pin_frees);
    CHECK(g_live.empty() && g_allocs == g_frees);
    printf("devbuf_host_check: OK (%ld blocks)\n", g_allocs);
    return 0;
}
