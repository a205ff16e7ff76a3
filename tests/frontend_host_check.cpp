// Stand-alone check of the host helpers of poccala_amd/csrc/frontend_host.h (the argument structs, the one frame geometry, frame_rows in both
// of its modes, frame_utt_of, pitch_geometry_check, pitch_frame_count: what the eight front-end entry points share) against a stub context.
// Built with the host sanitizers and run as its own process by tests/test_frontend_host.py: exit status 0 and no sanitizer report = pass.
// Every expected value is written out by hand.
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

#include "../poccala_amd/csrc/frontend_host.h"

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
    return pitch_geometry_check(&ctx, "who", FrameSpec{rate, sampletime, overlap}, PitchArgs{f_min, f_max, ballast, soft, pf, g, n_lags}, out);
}

// frame_rows over U signals at offsets `off` (the samples themselves are never looked at)
static int pitch_rows_check(pcl_ctx *c, const char *who, int U, const int64_t *off, const FrameGeom &g, bool whole_frame, std::vector<long long> *ro) {
    return frame_rows(c, who, SignalView{nullptr, true, U, off}, g, whole_frame, ro);
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
    {   // whole frames (pcl_mfcc*, pcl_frontend*) at the one-frame edge: 8 kHz, 25 ms, half overlap -> 200 / 100
        const FrameGeom fg = FrameSpec{8000, 0.025, 0.5}.frame();
        CHECK(fg.size == 200 && fg.step == 100);
        const FrameGeom odd = FrameSpec{11025, 0.025, 0.5}.frame();   // 275.625 -> 275, 137.5 -> 137: both truncated
        CHECK(odd.size == 275 && odd.step == 137);
        std::vector<long long> ro;
        const int64_t edge[4] = {0, 200, 401, 702};                   // n = size, size + 1, size + step + 1
        CHECK(pitch_rows_check(&ctx, "who", 3, edge, fg, true, &ro) == PCL_OK && (ro == std::vector<long long>{0, 1, 3, 6}));
        CHECK(pitch_rows_check(&ctx, "who", 3, edge, fg, false, &ro) == PCL_OK && (ro == std::vector<long long>{0, 1, 3, 6}));   // the same rows in both modes
        const int64_t shy[3] = {0, 200, 399};                         // n = size - 1, behind a good one
        CHECK(pitch_rows_check(&ctx, "pcl_mfcc", 2, shy, fg, true, &ro) == PCL_ERR_INVALID);
        CHECK(ctx.err == "pcl_mfcc: signal 1 has 199 samples, fewer than one frame (200)");
        CHECK(pitch_rows_check(&ctx, "pcl_frontend_pcm16", 1, shy + 1, fg, true, &ro) == PCL_ERR_INVALID && ctx.err == "pcl_frontend_pcm16: sig_off[0] must be 0");
        const int64_t lone[2] = {0, 199};
        CHECK(pitch_rows_check(&ctx, "pcl_frontend_pcm16", 1, lone, fg, true, &ro) == PCL_ERR_INVALID);
        CHECK(ctx.err == "pcl_frontend_pcm16: signal 0 has 199 samples, fewer than one frame (200)");
        CHECK(pitch_rows_check(&ctx, "who", 1, lone, fg, false, &ro) == PCL_OK && (ro == std::vector<long long>{0, 1}));          // ... which the pitch rows pad
        const int64_t back[3] = {0, 300, 200};                        // a negative length is "fewer than one frame" to the MFCC
        CHECK(pitch_rows_check(&ctx, "who", 2, back, fg, true, &ro) == PCL_ERR_INVALID && ctx.err == "who: signal 1 has -100 samples, fewer than one frame (200)");
        // a ragged batch of five: 200, 201, 300, 301 and 2400 samples -> 1, 2, 2, 3 and 1 + 2200 / 100 = 23 frames
        const int64_t five[6] = {0, 200, 401, 701, 1002, 3402};
        CHECK(pitch_rows_check(&ctx, "who", 5, five, fg, true, &ro) == PCL_OK && (ro == std::vector<long long>{0, 1, 3, 5, 8, 31}));
        std::vector<int> want{0, 1, 1, 2, 2, 3, 3, 3};
        want.insert(want.end(), 23, 4);
        CHECK(frame_utt_of(ro) == want && want.size() == 31);
        FrameRows fr;
        fr.row_off = ro;
        CHECK(fr.rows() == 31 && fr.longest() == 23);
        CHECK(frame_utt_of(std::vector<long long>{0, 0, 2, 2}) == (std::vector<int>{1, 1}));     // utterances without rows (pcl_vad's callers) own none
        // the limits of the pitch entry points do not reach the MFCC's rows: 65536 one-frame signals are 65536 rows
        std::vector<int64_t> many(65537);
        for (size_t u = 0; u < many.size(); ++u) many[u] = 200 * (int64_t)u;
        CHECK(pitch_rows_check(&ctx, "who", 65536, many.data(), fg, true, &ro) == PCL_OK && ro.size() == 65537 && ro.back() == 65536);
        CHECK(pitch_rows_check(&ctx, "who", 65536, many.data(), fg, false, &ro) == PCL_ERR_INVALID && has("65536 utterances, 1 .. 65535 per call"));
    }
    {   // the MFCC's width from its flags (1 = energy, 2 = deltas, 4 = their deltas), the signal's size on the wire
        MfccSpec m{{16000, 0.025, 0.5}, 512, 26, 13, 1, nullptr, nullptr, nullptr, nullptr};
        CHECK(m.dim() == 13 && m.frame().size == 400 && m.frame().step == 200 && !m.tables());
        m.flags = 3;
        CHECK(m.dim() == 26);
        m.flags = 7;
        CHECK(m.dim() == 39);
        m.flags = 0;
        CHECK(m.dim() == 13);
        const double t[1] = {0.0};
        m.twc = m.tws = m.resp = t;
        CHECK(!m.tables());
        m.dct = t;
        CHECK(m.tables());
        const int64_t off[3] = {0, 400, 1001};
        const SignalView s16{nullptr, true, 2, off}, s64{nullptr, false, 2, off};
        CHECK(s16.total() == 1001 && s16.total() * s16.sample_bytes() == 2002 && s64.total() * s64.sample_bytes() == 8008);
    }
    printf("frontend_host_check: OK\n");
    return 0;
}
