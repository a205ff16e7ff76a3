// Stand-alone check of the owning device buffer (poccala_amd/csrc/pcl_own.h) against a malloc-backed stub pool that counts live blocks.
// Built with the host sanitizers and run as its own process by tests/test_devbuf_host.py: exit status 0 and no sanitizer report = pass.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>

#include "../poccala_amd/csrc/pcl_own.h"

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
    CHECK(g_live.empty() && g_allocs == g_frees);
    printf("devbuf_host_check: OK (%ld blocks)\n", g_allocs);
    return 0;
}
