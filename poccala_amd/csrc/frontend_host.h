// The front-end's host side in one place: what the eight entry points of mfcc.hip, vad.hip and pitch.hip are handed (the signals, the MFCC,
// detector and pitch parameters), the ONE frame geometry they share, the rows it gives, and the checks of the pitch parameters.  Every check
// runs before the first launch.  Host code only: needs pcl_own.h's error macros and nothing of the device, so that
// tests/frontend_host_check.cpp can compile it against a stub context under the host sanitizers.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

// U signals back to back: signal u is samples [sig_off[u], sig_off[u + 1]) of `samples` (int16_t when pcm16, else double)
struct SignalView {
    const void *samples;
    bool pcm16;
    int U;
    const int64_t *sig_off;
    size_t total() const { return (size_t)sig_off[U]; }
    size_t sample_bytes() const { return pcm16 ? sizeof(int16_t) : sizeof(double); }
};

// the frame every part of the front-end cuts the signals into, as the caller names it and in samples: derived HERE and nowhere else
struct FrameGeom {
    int size, step;      // int(rate * sampletime), int(size * overlap)
};
struct FrameSpec {
    int rate;
    double sampletime, overlap;
    FrameGeom frame() const {
        const int size = (int)(rate * sampletime);
        return FrameGeom{size, (int)(size * overlap)};
    }
};

struct MfccSpec : FrameSpec {
    int nfft, nfilt, rank, flags;                       // flags: 1 = c0 <- ln(energy), 2 = deltas, 4 = and their deltas
    const double *twc, *tws, *resp, *dct;               // host tables: twiddle cos | sin (nfft), mel response (nfilt, nfft / 2 + 1), DCT basis (rank, nfilt)
    int dim() const { return rank * ((flags & 4) ? 3 : (flags & 2) ? 2 : 1); }
    bool tables() const { return twc && tws && resp && dct; }
};

struct VadSpec {
    int simple_size;
    double alpha, beta;
    int h;               // the order statistic int(beta * (2 s + 1)) of V3: vad_check's, 0 where no frame is filtered
};

// the parameters of rule P1-P5 beside the geometry
struct PitchArgs {
    double f_min, f_max, ballast, soft_min_f0, pf;
    const double *g;             // host: ln(lag) for the n_lags lags
    int n_lags;
};

constexpr int PITCH_MAX_LAGS = 1024;              // one lane per lag in the track kernel: a workgroup of at most 1024
constexpr int PITCH_MEAN_PARTS = 64;              // partial sums of P1's mean
constexpr size_t PITCH_LDS_LIMIT = 64u * 1024u;   // the correlation kernel's window in LDS, without asking for more than the default grant

struct PitchGeom : FrameGeom {
    int Lmin, Lmax, L;   // lags ceil(rate / f_max) .. floor(rate / f_min)
    int rate;
};

// the correlation kernel's dynamic LDS: the window of size + Lmax samples and the partial sums of its mean
static inline size_t pitch_lds_bytes(const PitchGeom &g) { return ((size_t)g.size + (size_t)g.Lmax + PITCH_MEAN_PARTS) * sizeof(double); }

// rate, frame and lag grid, the parameters, the caller's table of n_lags = L entries
static inline int pitch_geometry_check(pcl_ctx *ctx, const char *who, const FrameSpec &f, const PitchArgs &a, PitchGeom *out) {
    const int rate = f.rate;
    if (rate < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: sample rate %d", who, rate);
    const double fsize = (double)rate * f.sampletime;
    if (!(fsize >= 1.0) || !(fsize < 1.0e6)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: bad geometry (a frame of %g samples)", who, fsize);
    // (a step beyond the frame would skip samples; frame() is asked only once both conversions are known to be in range)
    const FrameGeom fg = (f.overlap > 0.0 && f.overlap <= 1.0) ? f.frame() : FrameGeom{(int)fsize, 0};
    const int size = fg.size, step = fg.step;
    if (step < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: bad geometry (frame size %d, step %d)", who, size, step);
    if (!(a.f_min > 0.0) || !(a.f_max > a.f_min) || !(a.f_max < INFINITY))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: pitch range f_min = %g, f_max = %g (0 < f_min < f_max)", who, a.f_min, a.f_max);
    if (a.f_max > (double)rate / 2.0)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: f_max = %g is above half the sample rate (%d / 2)", who, a.f_max, rate);
    const double flo = ceil((double)rate / a.f_max), fhi = floor((double)rate / a.f_min);
    if (flo < 1.0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the shortest lag ceil(%d / %g) is below 1", who, rate, a.f_max);
    if (fhi - flo + 1.0 > (double)PITCH_MAX_LAGS)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: f_min = %g .. f_max = %g at %d Hz are %.0f lags, at most %d", who, a.f_min, a.f_max, rate, fhi - flo + 1.0,
                 PITCH_MAX_LAGS);
    const int Lmin = (int)flo, Lmax = (int)fhi, L = Lmax - Lmin + 1;
    if (L < 2) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: f_min = %g .. f_max = %g at %d Hz are %d lags, at least 2", who, a.f_min, a.f_max, rate, L);
    if (!(a.ballast >= 0.0) || !(a.ballast < INFINITY)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: ballast %g (finite, not negative)", who, a.ballast);
    if (!(a.soft_min_f0 >= 0.0) || !(a.soft_min_f0 < INFINITY) || !(a.pf >= 0.0) || !(a.pf < INFINITY))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: soft_min_f0 %g, pf %g (finite, not negative)", who, a.soft_min_f0, a.pf);
    if (!a.g) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: NULL table of ln(lag)", who);
    if (a.n_lags != L)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the table of ln(lag) has %d entries, the lag grid %d .. %d has %d", who, a.n_lags, Lmin, Lmax, L);
    const PitchGeom gm{{size, step}, Lmin, Lmax, L, rate};
    if (pitch_lds_bytes(gm) > PITCH_LDS_LIMIT)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: a window of %d + %d samples needs %zu bytes of LDS, at most %zu", who, size, Lmax, pitch_lds_bytes(gm),
                 PITCH_LDS_LIMIT);
    *out = gm;
    return PCL_OK;
}

// the MFCC's frame count (AudioProcessing.frame_count), at least 1: a signal shorter than a frame is one zero-padded frame
static inline long long pitch_frame_count(long long n, int size, int step) { return n <= size ? 1 : 1 + (n - size + step - 1) / step; }

// THE rows of a call: row_off[u] = first row (frame) of signal u, U + 1 entries.
// whole_frame (pcl_mfcc*, pcl_frontend*: the front-end's rows are the MFCC's): a signal shorter than one frame is refused; otherwise
// (pcl_pitch*) it is one zero-padded frame.  sig_off[0] = 0 is every entry point's contract and held for all of them.  The two limits are
// the pitch entry points' ALONE: the MFCC serves more than 65535 signals in a call, and a front-end call beyond the row limit is the
// detector's check's or the launch's to refuse, in its own words.  The entry points check U, the pointers and the geometry before they come
// here, each with its own text.
static inline int frame_rows(pcl_ctx *ctx, const char *who, const SignalView &sig, const FrameGeom &g, bool whole_frame,
                             std::vector<long long> *row_off) {
    if (!whole_frame && (sig.U <= 0 || sig.U > 65535)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %d utterances, 1 .. 65535 per call", who, sig.U);
    if (!sig.sig_off) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: NULL sig_off", who);
    if (sig.sig_off[0] != 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: sig_off[0] must be 0", who);
    row_off->assign(1, 0);
    for (int u = 0; u < sig.U; ++u) {
        const long long n = sig.sig_off[u + 1] - sig.sig_off[u];
        if (whole_frame && n < g.size) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: signal %d has %lld samples, fewer than one frame (%d)", who, u, n, g.size);
        if (n < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: signal %d has %lld samples", who, u, n);
        const long long T = pitch_frame_count(n, g.size, g.step);      // 1 + ceil((n - size) / step)  (AudioProcessing.py:218)
        if (!whole_frame && (T > 0x7fffffffll || row_off->back() + T > 0x7fffffffll))
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: more than 2^31 - 1 frames at signal %d", who, u);
        row_off->push_back(row_off->back() + T);
    }
    return PCL_OK;
}

// frame_utt[r] = the signal that row r belongs to
static inline std::vector<int> frame_utt_of(const std::vector<long long> &row_off) {
    std::vector<int> fu((size_t)row_off.back());
    for (size_t u = 0; u + 1 < row_off.size(); ++u)
        for (long long r = row_off[u]; r < row_off[u + 1]; ++r) fu[(size_t)r] = (int)u;
    return fu;
}

// the rows of one call as the kernels want them; frame_utt is filled (frame_utt_of) once the call is known to run
struct FrameRows {
    std::vector<long long> row_off;
    std::vector<int> frame_utt;
    long long rows() const { return row_off.back(); }
    long long longest() const {
        long long m = 0;
        for (size_t u = 0; u + 1 < row_off.size(); ++u) m = row_off[u + 1] - row_off[u] > m ? row_off[u + 1] - row_off[u] : m;
        return m;
    }
};
