// Stand-alone check of the host helpers of poccala_amd/csrc/frame_spans.h (spans_check, speakers_check, DevSpans, plan_chunks, ChunkLists,
// upload_row_labels, env_positive_ll) against a stub context and a malloc-backed stub pool.  Built with the host sanitizers and run as its own process by
// tests/test_frame_spans_host.py: exit status 0 and no sanitizer report = pass.  Every expected value is written out by hand.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "../poccala_amd/csrc/pcl_own.h"

struct pcl_ctx {
    int device = 0;
    int64_t F = 0;
    float *frames32 = nullptr;
    std::string err;
};
int pcl_ctx_device(const pcl_ctx *ctx) { return ctx->device; }
void pcl_set_error(pcl_ctx *ctx, const char *msg) { ctx->err = msg; }
thread_local int pcl_tls_free_synced = 0;

static std::set<void *> g_live;
void *pcl_pool_alloc(int, size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    g_live.insert(p);
    return p;
}
void pcl_pool_free(void *p) {
    if (!p) return;
    if (!g_live.erase(p)) {
        fprintf(stderr, "FAIL: free of a block that is not live\n");
        exit(2);
    }
    free(p);
}
static hipError_t pcl_h2d(pcl_ctx *, void *dst, const void *src, size_t bytes) {   // the "device" is the stub pool's host memory
    memcpy(dst, src, bytes);
    return hipSuccess;
}

#define hipSetDevice(device) ((void)(device), hipSuccess)            // (the stub pool has no device to set)

namespace {
#include "../poccala_amd/csrc/frame_spans.h"
}

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static const char *WHO = "who", *ONCE = "a frame is counted ONCE";
static bool says(const pcl_ctx &ctx, const char *text) { return ctx.err == text; }

int main() {
    float row = 0.0f;
    pcl_ctx ctx;
    int Tmax = -1;
    {   // no frames: a state error of its own, asked for by the caller where the caller wants it
        CHECK(frames_loaded_check(&ctx, WHO) == PCL_ERR_STATE && says(ctx, "who: no frames loaded"));
        ctx.F = 100;
        CHECK(frames_loaded_check(&ctx, WHO) == PCL_ERR_STATE);   // rows without a matrix
        ctx.frames32 = &row;
        CHECK(frames_loaded_check(&ctx, WHO) == PCL_OK);
    }
    {   // U = 0, 1, 65535 and 65536; NULL arguments
        const int32_t T1[1] = {7};
        const int64_t b1[1] = {93};
        CHECK(spans_check(&ctx, WHO, ONCE, 0, T1, b1, &Tmax) == PCL_ERR_INVALID && says(ctx, "who: U = 0 utterances (1 .. 65535), or a NULL argument"));
        CHECK(spans_check(&ctx, WHO, ONCE, 1, T1, b1, &Tmax) == PCL_OK && Tmax == 7);   // ends exactly at F = 100
        CHECK(spans_check(&ctx, WHO, ONCE, 1, nullptr, b1, &Tmax) == PCL_ERR_INVALID && says(ctx, "who: U = 1 utterances (1 .. 65535), or a NULL argument"));
        CHECK(spans_check(&ctx, WHO, ONCE, 1, T1, nullptr, &Tmax) == PCL_ERR_INVALID);
        CHECK(spans_args_check(&ctx, WHO, 1, T1, b1) == PCL_OK && spans_args_check(&ctx, WHO, -1, T1, b1) == PCL_ERR_INVALID);
        std::vector<int32_t> Tz(65536, 0);
        std::vector<int64_t> bz(65536, 0);
        Tmax = -1;
        CHECK(spans_check(&ctx, WHO, ONCE, 65535, Tz.data(), bz.data(), &Tmax) == PCL_OK && Tmax == 0);   // utterances of no frames lie nowhere
        CHECK(spans_check(&ctx, WHO, ONCE, 65536, Tz.data(), bz.data(), &Tmax) == PCL_ERR_INVALID &&
              says(ctx, "who: U = 65536 utterances (1 .. 65535), or a NULL argument"));
    }
    {   // the end of the matrix, negative lengths and starts
        const int32_t T[2] = {10, 8};
        const int64_t at_end[2] = {0, 92}, past[2] = {0, 93}, neg_b[2] = {-1, 50};
        const int32_t neg_T[2] = {10, -1};
        CHECK(spans_check(&ctx, WHO, ONCE, 2, T, at_end, &Tmax) == PCL_OK && Tmax == 10);
        CHECK(spans_check(&ctx, WHO, ONCE, 2, T, past, &Tmax) == PCL_ERR_INVALID &&
              says(ctx, "who: utterance 1 covers rows [93, 101) of a frame matrix of 100 rows"));
        CHECK(spans_check(&ctx, WHO, ONCE, 2, neg_T, at_end, &Tmax) == PCL_ERR_INVALID &&
              says(ctx, "who: utterance 1 covers rows [92, 91) of a frame matrix of 100 rows"));
        CHECK(spans_check(&ctx, WHO, ONCE, 2, T, neg_b, &Tmax) == PCL_ERR_INVALID &&
              says(ctx, "who: utterance 0 covers rows [-1, 9) of a frame matrix of 100 rows"));
    }
    {   // two that touch with a zero-length utterance between them (given out of order), then one row of overlap
        const int32_t T[3] = {10, 0, 10};
        const int64_t touch[3] = {30, 30, 20}, over[3] = {30, 30, 21};
        Tmax = -1;
        CHECK(spans_check(&ctx, WHO, ONCE, 3, T, touch, &Tmax) == PCL_OK && Tmax == 10);
        Tmax = -1;
        CHECK(spans_check(&ctx, WHO, ONCE, 3, T, over, &Tmax) == PCL_ERR_INVALID && Tmax == -1 &&
              says(ctx, "who: the utterances overlap in the frame matrix at row 30 (a frame is counted ONCE)"));
    }
    {   // speakers -2, -1, S - 1 and S; NULL
        const int S = 4;
        const int32_t ok[3] = {-1, S - 1, 0}, low[3] = {0, -2, 0}, high[3] = {0, 0, S};
        CHECK(speakers_check(&ctx, WHO, 3, ok, S) == PCL_OK);
        CHECK(speakers_check(&ctx, WHO, 3, low, S) == PCL_ERR_INVALID && says(ctx, "who: utterance 1 has speaker -2, outside [-1, 4)"));
        CHECK(speakers_check(&ctx, WHO, 3, high, S) == PCL_ERR_INVALID && says(ctx, "who: utterance 2 has speaker 4, outside [-1, 4)"));
        CHECK(speakers_check(&ctx, WHO, 3, nullptr, S) == PCL_ERR_INVALID && says(ctx, "who: utt_speaker is NULL"));
    }
    {   // the upload: three blocks with speakers, two without, exactly U entries each (the sanitizer watches entry U), all given back
        const int32_t T[3] = {10, 0, 10}, spk[3] = {1, -1, 0};
        const int64_t begin[3] = {30, 30, 20};
        {
            DevSpans d;
            CHECK(d.upload(&ctx, 3, T, begin, spk) == PCL_OK && g_live.size() == 3);
            CHECK(d.T[2] == 10 && d.spk[1] == -1 && d.begin[2] == 20 && d.T.cap == 3 && d.spk.cap == 3 && d.begin.cap == 3);
        }
        CHECK(g_live.empty());
        {
            DevSpans d;
            CHECK(d.upload(&ctx, 3, T, begin, nullptr) == PCL_OK && g_live.size() == 2 && !d.spk);
            CHECK(d.T[0] == 10 && d.begin[0] == 30);
        }
        CHECK(g_live.empty());
    }
    {   // chunks: an empty group, a group of exactly `chunk` rows, one of chunk + 1, one shorter than a chunk
        std::vector<int> g0, v0, n;
        plan_chunks({0, 50, 51, 7}, 50, &g0, &v0, &n);
        CHECK((g0 == std::vector<int>{0, 0, 1, 3, 4}));
        CHECK((v0 == std::vector<int>{0, 50, 100, 101}));
        CHECK((n == std::vector<int>{50, 50, 1, 7}));
        plan_chunks({5}, 1ll << 30, &g0, &v0, &n);                 // the lists of a call before are dropped
        CHECK((g0 == std::vector<int>{0, 1}) && (v0 == std::vector<int>{0}) && (n == std::vector<int>{5}));
        plan_chunks({}, 50, &g0, &v0, &n);
        CHECK((g0 == std::vector<int>{0}) && v0.empty() && n.empty());
    }
    {   // the plan as one list: R + 1 group offsets, then C and C entries, behind nothing and behind two prefix lists; uploaded as it is
        ChunkLists p;
        p.plan({}, {0, 50, 51, 7}, 50);
        CHECK(p.C == 4 && p.o_chunk0 == 0 && p.o_cv0 == 5 && p.o_cn == 9);
        CHECK((p.lists == std::vector<int>{0, 0, 1, 3, 4, 0, 50, 100, 101, 50, 50, 1, 7}) && (p.group_chunk0 == std::vector<int>{0, 0, 1, 3, 4}));
        CHECK(p.upload(&ctx) == PCL_OK && g_live.size() == 1 && p.d_lists.cap == 13);
        CHECK(p.chunk0()[4] == 4 && p.chunk_v0()[3] == 101 && p.chunk_n()[0] == 50 && p.chunk_n()[3] == 7);
        const std::vector<int> a{9, 8, 7}, b{6};
        ChunkLists q;
        q.plan({&a, &b}, {0, 50, 51, 7}, 50);
        CHECK(q.C == 4 && q.o_chunk0 == 4 && q.o_cv0 == 9 && q.o_cn == 13);
        CHECK((q.lists == std::vector<int>{9, 8, 7, 6, 0, 0, 1, 3, 4, 0, 50, 100, 101, 50, 50, 1, 7}));
        ChunkLists one;                                           // one group of one chunk
        one.plan({}, {5}, 1ll << 30);
        CHECK(one.C == 1 && one.o_cv0 == 2 && one.o_cn == 3 && (one.lists == std::vector<int>{0, 1, 0, 5}));
        ChunkLists none;                                          // an empty plan: groups without rows, and no group at all
        none.plan({&b}, {0, 0}, 50);
        CHECK(none.C == 0 && none.o_chunk0 == 1 && none.o_cv0 == 4 && none.o_cn == 4 && (none.lists == std::vector<int>{6, 0, 0, 0}));
        none.plan({}, {}, 50);
        CHECK(none.C == 0 && none.o_cv0 == 1 && none.o_cn == 1 && (none.lists == std::vector<int>{0}));
    }
    CHECK(g_live.empty());
    {   // a label per frame row (F = 100): NULL, -2 and R refused with the FIRST offender named, -1 and R - 1 accepted and uploaded
        const int R = 3;
        std::vector<int32_t> lab(100, 0);
        DevBuf<int32_t> d;
        CHECK(upload_row_labels(&ctx, WHO, "frame_class", "class", nullptr, R, &d) == PCL_ERR_INVALID && says(ctx, "who: frame_class is NULL") && !d);
        lab[7] = -2;
        lab[9] = R;
        CHECK(upload_row_labels(&ctx, WHO, "frame_class", "class", lab.data(), R, &d) == PCL_ERR_INVALID &&
              says(ctx, "who: frame_class[7] = -2 is neither -1 nor a class in [0, 3)") && !d);
        lab[7] = 0;
        CHECK(upload_row_labels(&ctx, WHO, "frame_row", "row", lab.data(), R, &d) == PCL_ERR_INVALID &&
              says(ctx, "who: frame_row[9] = 3 is neither -1 nor a row in [0, 3)") && !d && g_live.empty());
        lab[9] = R - 1;
        lab[99] = -1;
        CHECK(upload_row_labels(&ctx, WHO, "frame_row", "row", lab.data(), R, &d) == PCL_OK && d.cap == 100 && d[9] == R - 1 && d[99] == -1);
        pcl_ctx empty;                                            // no frames: after the NULL check, before the scan
        CHECK(upload_row_labels(&empty, WHO, "frame_row", "row", nullptr, R, &d) == PCL_ERR_INVALID);
        CHECK(upload_row_labels(&empty, WHO, "frame_row", "row", lab.data(), R, &d) == PCL_ERR_STATE && says(empty, "who: no frames loaded"));
    }
    CHECK(g_live.empty());
    {   // a positive integer, else the fallback; read on every call
        unsetenv("PCL_TEST_CHUNK");
        CHECK(env_positive_ll("PCL_TEST_CHUNK", 4096) == 4096);
        setenv("PCL_TEST_CHUNK", "50", 1);
        CHECK(env_positive_ll("PCL_TEST_CHUNK", 4096) == 50);
        setenv("PCL_TEST_CHUNK", "0", 1);
        CHECK(env_positive_ll("PCL_TEST_CHUNK", 4096) == 4096);
        setenv("PCL_TEST_CHUNK", "-3", 1);
        CHECK(env_positive_ll("PCL_TEST_CHUNK", 0) == 0);
        setenv("PCL_TEST_CHUNK", "many", 1);
        CHECK(env_positive_ll("PCL_TEST_CHUNK", 7) == 7);
        setenv("PCL_TEST_CHUNK", "4294967296", 1);
        CHECK(env_positive_ll("PCL_TEST_CHUNK", 7) == 4294967296ll);
    }
    printf("frame_spans_host_check: OK\n");
    return 0;
}
