// The argument and geometry checks the four pitch entry points share (pcl_pitch, pcl_pitch_pcm16, pcl_frontend_pitch,
// pcl_frontend_pitch_pcm16): host code only, every check before the first launch.  Needs pcl_own.h's error macros and nothing of the
// device, so that tests/pitch_host_check.cpp can compile it against a stub context under the host sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

constexpr int PITCH_MAX_LAGS = 1024;              // one lane per lag in the track kernel: a workgroup of at most 1024
constexpr int PITCH_MEAN_PARTS = 64;              // partial sums of P1's mean
constexpr size_t PITCH_LDS_LIMIT = 64u * 1024u;   // the correlation kernel's window in LDS, without asking for more than the default grant

struct PitchGeom {
    int size, step;      // the MFCC's frame: int(rate * sampletime), int(size * overlap)
    int Lmin, Lmax, L;   // lags ceil(rate / f_max) .. floor(rate / f_min)
};

// the correlation kernel's dynamic LDS: the window of size + Lmax samples and the partial sums of its mean
static inline size_t pitch_lds_bytes(const PitchGeom &g) { return ((size_t)g.size + (size_t)g.Lmax + PITCH_MEAN_PARTS) * sizeof(double); }

// rate, frame and lag grid, the parameters, the caller's table of n_lags = L entries
static inline int pitch_geometry_check(pcl_ctx *ctx, const char *who, int rate, double sampletime, double overlap, double f_min, double f_max,
                                       double ballast, double soft_min_f0, double pf, const double *g, int n_lags, PitchGeom *out) {
    if (rate < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: sample rate %d", who, rate);
    const double fsize = (double)rate * sampletime;
    if (!(fsize >= 1.0) || !(fsize < 1.0e6)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: bad geometry (a frame of %g samples)", who, fsize);
    const int size = (int)fsize, step = (overlap > 0.0 && overlap <= 1.0) ? (int)(size * overlap) : 0;   // (a step beyond the frame would skip samples)
    if (step < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: bad geometry (frame size %d, step %d)", who, size, step);
    if (!(f_min > 0.0) || !(f_max > f_min) || !(f_max < INFINITY))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: pitch range f_min = %g, f_max = %g (0 < f_min < f_max)", who, f_min, f_max);
    if (f_max > (double)rate / 2.0)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: f_max = %g is above half the sample rate (%d / 2)", who, f_max, rate);
    const double flo = ceil((double)rate / f_max), fhi = floor((double)rate / f_min);
    if (flo < 1.0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the shortest lag ceil(%d / %g) is below 1", who, rate, f_max);
    if (fhi - flo + 1.0 > (double)PITCH_MAX_LAGS)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: f_min = %g .. f_max = %g at %d Hz are %.0f lags, at most %d", who, f_min, f_max, rate, fhi - flo + 1.0,
                 PITCH_MAX_LAGS);
    const int Lmin = (int)flo, Lmax = (int)fhi, L = Lmax - Lmin + 1;
    if (L < 2) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: f_min = %g .. f_max = %g at %d Hz are %d lags, at least 2", who, f_min, f_max, rate, L);
    if (!(ballast >= 0.0) || !(ballast < INFINITY)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: ballast %g (finite, not negative)", who, ballast);
    if (!(soft_min_f0 >= 0.0) || !(soft_min_f0 < INFINITY) || !(pf >= 0.0) || !(pf < INFINITY))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: soft_min_f0 %g, pf %g (finite, not negative)", who, soft_min_f0, pf);
    if (!g) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: NULL table of ln(lag)", who);
    if (n_lags != L) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the table of ln(lag) has %d entries, the lag grid %d .. %d has %d", who, n_lags, Lmin, Lmax, L);
    const PitchGeom gm{size, step, Lmin, Lmax, L};
    if (pitch_lds_bytes(gm) > PITCH_LDS_LIMIT)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: a window of %d + %d samples needs %zu bytes of LDS, at most %zu", who, size, Lmax, pitch_lds_bytes(gm),
                 PITCH_LDS_LIMIT);
    *out = gm;
    return PCL_OK;
}

// the MFCC's frame count (AudioProcessing.frame_count), at least 1: a signal shorter than a frame is one zero-padded frame
static inline long long pitch_frame_count(long long n, int size, int step) { return n <= size ? 1 : 1 + (n - size + step - 1) / step; }

// row_off[u] = first row of utterance u (U + 1 entries).  whole_frame: a signal shorter than one frame is refused, as the MFCC refuses it
// (the front-end's rows are the MFCC's); otherwise it is one frame.
static inline int pitch_rows_check(pcl_ctx *ctx, const char *who, int U, const int64_t *sig_off, const PitchGeom &g, bool whole_frame,
                                   std::vector<long long> *row_off) {
    if (U <= 0 || U > 65535) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %d utterances, 1 .. 65535 per call", who, U);
    if (!sig_off) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: NULL sig_off", who);
    if (sig_off[0] != 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: sig_off[0] must be 0", who);
    row_off->assign(1, 0);
    for (int u = 0; u < U; ++u) {
        const long long n = sig_off[u + 1] - sig_off[u];
        if (n < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: signal %d has %lld samples", who, u, n);
        if (whole_frame && n < g.size) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: signal %d has %lld samples, fewer than one frame (%d)", who, u, n, g.size);
        const long long T = pitch_frame_count(n, g.size, g.step);
        if (T > 0x7fffffffll || row_off->back() + T > 0x7fffffffll) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: more than 2^31 - 1 frames at signal %d", who, u);
        row_off->push_back(row_off->back() + T);
    }
    return PCL_OK;
}
