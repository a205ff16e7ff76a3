// Stand-alone check of the host helpers of poccala_amd/csrc/pitch_check.h (pitch_geometry_check, pitch_frame_count, pitch_rows_check: the
// argument and geometry checks the four pitch entry points share) against a stub context.  Built with the host sanitizers and run as its own
// process by tests/test_pitch_host.py: exit status 0 and no sanitizer report = pass.  Every expected value is written out by hand.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../poccala_amd/csrc/pcl_own.h"

struct pcl_ctx {
    int device = 0;
    std::string err;
};
int pcl_ctx_device(const pcl_ctx *ctx) { return ctx->device; }
void pcl_set_error(pcl_ctx *ctx, const char *msg) { ctx->err = msg; }
thread_local int pcl_tls_free_synced = 0;
void *pcl_pool_alloc(int, size_t bytes) { return malloc(bytes ? bytes : 1); }
void pcl_pool_free(void *p) { free(p); }

#include "../poccala_amd/csrc/pitch_check.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "FAIL %s:%d: %s\n  last error: %s\n", __FILE__, __LINE__, #c, ctx.err.c_str()); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static pcl_ctx ctx;
static bool has(const char *text) { return ctx.err.find(text) != std::string::npos; }

// the defaults but for what a case changes
static int geom(int rate, double f_min, double f_max, const double *g, int n_lags, PitchGeom *out, double sampletime = 0.025, double overlap = 0.5,
                double ballast = 7000.0, double soft = 10.0, double pf = 0.1) {
    ctx.err.clear();
    return pitch_geometry_check(&ctx, "who", rate, sampletime, overlap, f_min, f_max, ballast, soft, pf, g, n_lags, out);
}

int main() {
    std::vector<double> g(2048, 0.0);
    PitchGeom gm{};
    {   // the two rates of the tests: 8 kHz -> 200 / 100, lags 20 .. 160; 16 kHz -> 400 / 200, lags 40 .. 320
        CHECK(geom(8000, 50.0, 400.0, g.data(), 141, &gm) == PCL_OK);
        CHECK(gm.size == 200 && gm.step == 100 && gm.Lmin == 20 && gm.Lmax == 160 && gm.L == 141);
        CHECK(pitch_lds_bytes(gm) == (200 + 160 + 64) * 8);
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm) == PCL_OK);
        CHECK(gm.size == 400 && gm.step == 200 && gm.Lmin == 40 && gm.Lmax == 320 && gm.L == 281);
        // a rate the bounds do not divide: ceil and floor
        CHECK(geom(11025, 60.0, 330.0, g.data(), 183 - 34 + 1, &gm) == PCL_OK && gm.Lmin == 34 && gm.Lmax == 183 && gm.size == 275 && gm.step == 137);
    }
    {   // the refusals, each with its text, none of which writes *out
        PitchGeom keep{1, 2, 3, 4, 5};
        gm = keep;
        CHECK(geom(16000, 50.0, 8000.5, g.data(), 1, &gm) == PCL_ERR_INVALID && has("above half the sample rate"));
        CHECK(geom(16000, 50.0, 8000.0, g.data(), 320 - 2 + 1, &gm) == PCL_OK && gm.Lmin == 2);            // exactly rate / 2 passes
        gm = keep;
        CHECK(geom(16000, 10.0, 400.0, g.data(), 1561, &gm) == PCL_ERR_INVALID && has("1561 lags, at most 1024"));
        CHECK(geom(16000, 15.1, 400.0, g.data(), 1059 - 40 + 1, &gm) == PCL_OK && gm.L == 1020);
        CHECK(geom(44100, 45.0, 400.0, g.data(), 980 - 111 + 1, &gm) == PCL_OK && gm.L == 870);
        // L = 1024 exactly and 1025: lags 40 .. 1063 need f_min in (16000 / 1064, 16000 / 1063]
        CHECK(geom(16000, 15.05, 400.0, g.data(), 1024, &gm) == PCL_OK && gm.Lmax == 1063 && gm.L == 1024);
        CHECK(geom(16000, 15.03, 400.0, g.data(), 1025, &gm) == PCL_ERR_INVALID && has("1025 lags"));
        gm = keep;
        CHECK(geom(16000, 399.0, 400.0, g.data(), 1, &gm) == PCL_ERR_INVALID && has("are 1 lags, at least 2"));
        CHECK(geom(16000, 390.0, 400.0, g.data(), 2, &gm) == PCL_OK && gm.Lmin == 40 && gm.Lmax == 41);
        gm = keep;
        CHECK(geom(16000, 400.0, 50.0, g.data(), 1, &gm) == PCL_ERR_INVALID && has("0 < f_min < f_max"));
        CHECK(geom(16000, 0.0, 400.0, g.data(), 1, &gm) == PCL_ERR_INVALID && has("0 < f_min < f_max"));
        CHECK(geom(16000, -5.0, 400.0, g.data(), 1, &gm) == PCL_ERR_INVALID);
        CHECK(geom(16000, NAN, 400.0, g.data(), 1, &gm) == PCL_ERR_INVALID);
        CHECK(geom(16000, 50.0, NAN, g.data(), 1, &gm) == PCL_ERR_INVALID);
        CHECK(geom(16000, 50.0, INFINITY, g.data(), 1, &gm) == PCL_ERR_INVALID);
        CHECK(geom(0, 50.0, 400.0, g.data(), 281, &gm) == PCL_ERR_INVALID && has("sample rate 0"));
        CHECK(geom(16000, 50.0, 400.0, nullptr, 281, &gm) == PCL_ERR_INVALID && has("NULL table"));
        CHECK(geom(16000, 50.0, 400.0, g.data(), 280, &gm) == PCL_ERR_INVALID && has("has 280 entries, the lag grid 40 .. 320 has 281"));
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.025, 0.5, -1.0) == PCL_ERR_INVALID && has("ballast"));
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.025, 0.5, NAN) == PCL_ERR_INVALID);
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.025, 0.5, 0.0) == PCL_OK);                   // no ballast is a choice
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.025, 0.5, 7000.0, -1.0) == PCL_ERR_INVALID && has("soft_min_f0"));
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.025, 0.5, 7000.0, 10.0, INFINITY) == PCL_ERR_INVALID);
        // the frame: no samples, no step, an overlap that would step past the frame, a window beyond 64 KiB of LDS
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.0) == PCL_ERR_INVALID && has("bad geometry"));
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, NAN) == PCL_ERR_INVALID);
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 1.0e9) == PCL_ERR_INVALID);
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.025, 0.0) == PCL_ERR_INVALID && has("step 0"));
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.025, 1.5) == PCL_ERR_INVALID);
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.025, NAN) == PCL_ERR_INVALID);
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.49) == PCL_ERR_INVALID && has("bytes of LDS"));   // 7840 + 320 + 64 doubles
        CHECK(geom(16000, 50.0, 400.0, g.data(), 281, &gm, 0.48) == PCL_OK && pitch_lds_bytes(gm) == (7680 + 320 + 64) * 8);
    }
    {   // the MFCC's frame count, at least 1
        CHECK(pitch_frame_count(0, 200, 100) == 1 && pitch_frame_count(37, 200, 100) == 1 && pitch_frame_count(200, 200, 100) == 1);
        CHECK(pitch_frame_count(201, 200, 100) == 2 && pitch_frame_count(300, 200, 100) == 2 && pitch_frame_count(301, 200, 100) == 3);
        CHECK(pitch_frame_count(6400, 400, 200) == 31);
    }
    {   // the rows of a ragged batch; a short signal is one frame, or the MFCC's refusal
        CHECK(geom(8000, 50.0, 400.0, g.data(), 141, &gm) == PCL_OK);
        const int64_t off[6] = {0, 37, 237, 438, 438, 2838};          // 37, 200, 201, 0 and 2400 samples
        std::vector<long long> ro;
        CHECK(pitch_rows_check(&ctx, "who", 5, off, gm, false, &ro) == PCL_OK);
        CHECK((ro == std::vector<long long>{0, 1, 2, 4, 5, 28}));
        CHECK(pitch_rows_check(&ctx, "who", 5, off, gm, true, &ro) == PCL_ERR_INVALID && has("signal 0 has 37 samples, fewer than one frame (200)"));
        CHECK(pitch_rows_check(&ctx, "who", 2, off + 1, gm, true, &ro) == PCL_ERR_INVALID && has("sig_off[0] must be 0"));
        const int64_t whole[3] = {0, 200, 401};
        CHECK(pitch_rows_check(&ctx, "who", 2, whole, gm, true, &ro) == PCL_OK && (ro == std::vector<long long>{0, 1, 3}));
        const int64_t back[3] = {0, 300, 200};
        CHECK(pitch_rows_check(&ctx, "who", 2, back, gm, false, &ro) == PCL_ERR_INVALID && has("signal 1 has -100 samples"));
        CHECK(pitch_rows_check(&ctx, "who", 0, off, gm, false, &ro) == PCL_ERR_INVALID && has("0 utterances"));
        CHECK(pitch_rows_check(&ctx, "who", 65536, off, gm, false, &ro) == PCL_ERR_INVALID);
        CHECK(pitch_rows_check(&ctx, "who", 1, nullptr, gm, false, &ro) == PCL_ERR_INVALID && has("NULL sig_off"));
        const int64_t huge[3] = {0, 150000000000ll, 300000000000ll};   // 1.5e9 frames each: one fits an int, the two together do not
        CHECK(pitch_rows_check(&ctx, "who", 1, huge, gm, false, &ro) == PCL_OK && ro[1] == 1 + (150000000000ll - 200 + 99) / 100);
        CHECK(pitch_rows_check(&ctx, "who", 2, huge, gm, false, &ro) == PCL_ERR_INVALID && has("more than 2^31 - 1 frames at signal 1"));
    }
    printf("pitch_host_check: OK\n");
    return 0;
}
