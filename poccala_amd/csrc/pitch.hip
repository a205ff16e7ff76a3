// pitch.hip -- pitch and voicing features for gfx950: a normalised cross-correlation over the lag grid, a dynamic programme over the lags,
// and three float64 columns per frame (voicing, ln f0, delta ln f0) on the MFCC's frame grid.  The reference has no pitch code: the rule
// (P1-P5, include/poccala_hip.h at pcl_pitch) is this project's own, and tests/_pitch_twin.py is its definition in NumPy.
//
// Three kernel groups:
//   pitch_nccf_kernel   one workgroup per frame.  The window of size + Lmax samples is staged ONCE in LDS as doubles (an int16 sample is
//                       converted at the load, as mfcc.hip does it), its mean taken off in place; then one lane per lag runs the three dot
//                       products a.b_l, a.a, b_l.b_l over the sample index in ascending order.  Lane l reads w[i] (the same address in every
//                       lane: a broadcast) and w[l + i] (consecutive doubles across the lanes: 32 lanes cover one 256-byte bank row, so a
//                       ds_read_b64 of a half-wave has no conflict whatever l + i is).
//   pitch_track_kernel  one workgroup per utterance, one lane per lag (L <= 1024: up to 16 waves).  The previous column of `best` lives in
//                       LDS twice over: frame t reads copy (t - 1) & 1 and writes copy t & 1, ONE barrier per frame (a lane that has passed
//                       the barrier of frame t has finished its reads of copy (t - 1) & 1, which frame t + 1 overwrites).  int16
//                       back-pointers (T, L) in a pooled global buffer; lane 0 takes the last frame's minimum and walks them back.
//   pitch_out_kernel / pitch_delta_kernel   P5: one lane per row.
// Summation order (P2): one lane per (frame, lag), p = p + a[i] * b[i] for i = 0 .. size - 1, one rounded multiplication and one rounded
// addition at a time; e0 and el the same way (el directly for every lag, not from e_{l-1}; e0 again in every lane, which costs a third of
// the kernel's arithmetic and saves a barrier and a special lane).  No atomics anywhere: two runs give the same bits.
//
// This file is built with -ffp-contract=off (FLAGS_pitch in the Makefile): hipcc would otherwise contract a * b + c into an fma and the
// sums, costs and candidates would not be the twin's bits.  The only operation that is not the twin's bit for bit is the final log.
#include <optional>

#include "pcl_internal.h"

namespace {

// P1 + P2.  Dynamic LDS: w[size + Lmax] | part[64]  (pitch_lds_bytes).
template <typename S>
__global__ __launch_bounds__(1024) void pitch_nccf_kernel(const S *__restrict__ signal, const long long *__restrict__ sig_off,
                                                           const long long *__restrict__ row_off, const int *__restrict__ frame_utt, int size,
                                                           int step, int Lmin, int L, double ballast, double *__restrict__ bal,
                                                           double *__restrict__ raw) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    const int W = size + Lmin + L - 1;                           // size + Lmax
    double *w = sh;                                              // [W]
    double *part = sh + W;                                       // [PITCH_MEAN_PARTS]
    const int tid = threadIdx.x;
    const int u = frame_utt[blockIdx.x];
    const long long t = (long long)blockIdx.x - row_off[u];
    const long long n = sig_off[u + 1] - sig_off[u];
    const S *s = signal + sig_off[u];
    const long long i0 = t * step;
    for (int i = tid; i < W; i += blockDim.x) {
        const long long k = i0 + i;
        w[i] = k < n ? (double)s[k] : 0.0;                       // zero padding past the signal
    }
    __syncthreads();
    if (tid < PITCH_MEAN_PARTS) {
        double acc = 0.0;
        for (int i = tid; i < size; i += PITCH_MEAN_PARTS) acc = acc + w[i];
        part[tid] = acc;
    }
    __syncthreads();
    double tot = 0.0;
    for (int j = 0; j < PITCH_MEAN_PARTS; ++j) tot = tot + part[j];
    const double mean = tot / (double)size;
    for (int i = tid; i < W; i += blockDim.x) w[i] = w[i] - mean;   // (every lane rewrites the entries it wrote)
    __syncthreads();
    for (int li = tid; li < L; li += blockDim.x) {
        const double *b = w + Lmin + li;                         // b[size - 1] = w[Lmin + li + size - 1], at most w[W - 1]
        double p = 0.0, e0 = 0.0, el = 0.0;
        for (int i = 0; i < size; ++i) {
            const double av = w[i], bv = b[i];
            p = p + av * bv;
            e0 = e0 + av * av;
            el = el + bv * bv;
        }
        const double den = e0 * el, db = den + ballast;
        const size_t o = (size_t)blockIdx.x * L + li;
        raw[o] = den == 0.0 ? 0.0 : p / sqrt(den);
        bal[o] = db == 0.0 ? 0.0 : p / sqrt(db);
    }
}

// P3 + P4.  Dynamic LDS: g[L] | best[2][L].  blockDim.x = L rounded up to a multiple of 64.
__global__ __launch_bounds__(1024) void pitch_track_kernel(const double *__restrict__ bal, const long long *__restrict__ row_off,
                                                            const double *__restrict__ g, int Lmin, int L, double rate, double soft_min_f0,
                                                            double pf, short *__restrict__ bp, int *__restrict__ lagidx) {
    extern __shared__ __attribute__((aligned(16))) double sh[];
    double *gs = sh;                                             // [L]
    double *best = sh + L;                                       // [2][L]
    const int l = threadIdx.x;
    const bool on = l < L;
    const long long base = row_off[blockIdx.x];
    const int T = (int)(row_off[blockIdx.x + 1] - base);
    const double gl = on ? g[l] : 0.0;
    const double fac = 1.0 - soft_min_f0 * (double)(Lmin + l) / rate;
    if (on) {
        gs[l] = gl;
        best[l] = 1.0 - bal[(size_t)base * L + l] * fac;
    }
    __syncthreads();
    double nb = (on && T > 1) ? bal[(size_t)(base + 1) * L + l] : 0.0;
    for (int t = 1; t < T; ++t) {
        const double c = 1.0 - nb * fac;
        if (on && t + 1 < T) nb = bal[(size_t)(base + t + 1) * L + l];   // the next frame's value travels under this frame's minimum
        if (on) {
            const double *pv = best + (size_t)((t - 1) & 1) * L;
            double d = gl - gs[0];
            double m = pv[0] + pf * (d * d);
            int arg = 0;
            for (int k = 1; k < L; ++k) {
                d = gl - gs[k];
                const double cand = pv[k] + pf * (d * d);
                if (cand < m) {                                  // strictly: ties stay with the smallest l'
                    m = cand;
                    arg = k;
                }
            }
            best[(size_t)(t & 1) * L + l] = c + m;
            bp[(size_t)(base + t) * L + l] = (short)arg;
        }
        __syncthreads();                                         // also orders the workgroup's back-pointer stores before lane 0's reads below
    }
    if (l == 0) {
        const double *pv = best + (size_t)((T - 1) & 1) * L;
        double m = pv[0];
        int arg = 0;
        for (int k = 1; k < L; ++k)
            if (pv[k] < m) {
                m = pv[k];
                arg = k;
            }
        for (int t = T - 1; t >= 0; --t) {
            lagidx[base + t] = arg;
            if (t > 0) arg = bp[(size_t)(base + t) * L + arg];
        }
    }
}

// P5: v and ln f0 of every row (columns 0 and 1 of out (rows, 3)), the lag in samples
__global__ __launch_bounds__(256) void pitch_out_kernel(const double *__restrict__ raw, const int *__restrict__ lagidx, long long rows, int Lmin, int L,
                                                         double rate, double *__restrict__ out, int *__restrict__ lag) {
    const long long row = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int li = lagidx[row];
    const double *r = raw + (size_t)row * L;
    const double y0 = r[li];
    double shift = 0.0;
    if (li > 0 && li < L - 1) {
        const double ym = r[li - 1], yp = r[li + 1];
        const double den = (ym - 2.0 * y0) + yp;
        if (den < 0.0) {
            shift = 0.5 * (ym - yp) / den;
            shift = shift > 0.5 ? 0.5 : (shift < -0.5 ? -0.5 : shift);
        }
    }
    out[(size_t)row * 3] = y0;
    out[(size_t)row * 3 + 1] = log(rate / ((double)(Lmin + li) + shift));
    if (lag) lag[row] = Lmin + li;
}

// ... and the delta of column 1 into column 2, over the utterance's own rows
__global__ __launch_bounds__(256) void pitch_delta_kernel(const long long *__restrict__ row_off, const int *__restrict__ frame_utt, long long rows,
                                                           double *__restrict__ out) {
    const long long row = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int u = frame_utt[row];
    const long long base = row_off[u], T = row_off[u + 1] - base, t = row - base;
    auto at = [&](long long k) {
        k = k < 0 ? 0 : (k >= T ? T - 1 : k);
        return out[(size_t)(base + k) * 3 + 1];
    };
    out[(size_t)row * 3 + 2] = ((at(t + 1) - at(t - 1)) + 2.0 * (at(t + 2) - at(t - 2))) / 10.0;
}

// the signal of one stand-alone call on the device.  A failure path may leave the staging stream copying into `sig`: it is drained first.
struct PitchSig {
    pcl_ctx *ctx;
    DevBuf<unsigned char> sig;
    explicit PitchSig(pcl_ctx *c) : ctx(c) {}
    ~PitchSig() {
        if (sig && ctx->pcm.stream) (void)hipStreamSynchronize(ctx->pcm.stream);
    }
};

// where a stand-alone call leaves its results on the host (each may be NULL); with PCL_PITCH_NCCF_IN nccf_bal / nccf_raw are its input
struct PitchOut {
    double *out;
    int32_t *lag;
    double *nccf_bal, *nccf_raw;
    int64_t n_rows;
};

int pitch_to_host(pcl_ctx *ctx, const char *who, const SignalView &sig, const FrameSpec &f, const PitchArgs &a, int flags, const PitchOut &o) {
    if (!ctx) return PCL_ERR_INVALID;
    const bool nccf_in = (flags & PCL_PITCH_NCCF_IN) != 0;
    if (flags & ~PCL_PITCH_NCCF_IN) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: unknown flags %d", who, flags);
    PitchGeom gm;
    TRY(pitch_geometry_check(ctx, who, f, a, &gm));
    FrameRows fr;
    TRY(frame_rows(ctx, who, sig, gm, false, &fr.row_off));
    const long long rows = fr.rows();
    if (rows != o.n_rows) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: caller expects %lld frames, geometry gives %lld", who, (long long)o.n_rows, rows);
    if (nccf_in && (!o.nccf_bal || !o.nccf_raw)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: PCL_PITCH_NCCF_IN without nccf_bal and nccf_raw", who);
    if (!nccf_in && !sig.samples) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: NULL signal", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    fr.frame_utt = frame_utt_of(fr.row_off);
    const size_t nl = (size_t)rows * gm.L;
    std::optional<pcl_free_synced_scope> synced;                 // engaged once the main stream has been waited for: declared before the buffers
    PitchSig s(ctx);
    PitchWork w;
    w.nccf_in = nccf_in;
    w.want_lag = o.lag != nullptr;
    if (nccf_in) {
        TRY(w.bal.alloc(ctx, nl));
        TRY(w.raw.alloc(ctx, nl));
        HIPCHK(ctx, pcl_h2d(ctx, w.bal, o.nccf_bal, nl * sizeof(double)));
        HIPCHK(ctx, pcl_h2d(ctx, w.raw, o.nccf_raw, nl * sizeof(double)));
    } else {
        TRY(s.sig.alloc(ctx, sig.total() * sig.sample_bytes()));
        TRY(pcl_signal_upload(ctx, who, s.sig, sig));
    }
    TRY(pcl_pitch_device(ctx, who, gm, a, sig, fr, s.sig, &w));
    hipError_t e = hipSuccess;
    if (o.out) e = pcl_d2h_queue(ctx, o.out, w.out, (size_t)rows * 3 * sizeof(double));
    if (e == hipSuccess && o.lag) e = pcl_d2h_queue(ctx, o.lag, w.lag, (size_t)rows * sizeof(int));
    if (e == hipSuccess && !nccf_in && o.nccf_bal) e = pcl_d2h_queue(ctx, o.nccf_bal, w.bal, nl * sizeof(double));
    if (e == hipSuccess && !nccf_in && o.nccf_raw) e = pcl_d2h_queue(ctx, o.nccf_raw, w.raw, nl * sizeof(double));
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) PCL_FAIL(ctx, PCL_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    synced.emplace();                                            // the kernels and copies are done (and every staged chunk they waited for)
    return PCL_OK;
}

}  // namespace

// P1-P5 queued on the main stream (NOT waited for): every buffer of the call is in *w and stays the caller's until it has waited.
// d_sig: the concatenated samples on the device (int16_t when sig.pcm16, else double; not read with w->nccf_in, when w->bal / w->raw hold
// the caller's arrays).  The checks (frontend_host.h) are the caller's: gm and fr come from them.
int pcl_pitch_device(pcl_ctx *ctx, const char *who, const PitchGeom &gm, const PitchArgs &a, const SignalView &sig, const FrameRows &fr,
                     const void *d_sig, PitchWork *w) {
    const int U = sig.U, L = gm.L;
    const long long rows = fr.rows();
    const std::vector<long long> so(sig.sig_off, sig.sig_off + U + 1);
    TRY(w->row_off.alloc(ctx, (size_t)U + 1));
    TRY(w->sig_off.alloc(ctx, (size_t)U + 1));
    TRY(w->frame_utt.alloc(ctx, (size_t)rows));
    TRY(w->g.alloc(ctx, (size_t)L));
    TRY(w->out.alloc(ctx, (size_t)rows * 3));
    TRY(w->bp.alloc(ctx, (size_t)rows * L));
    TRY(w->lagidx.alloc(ctx, (size_t)rows));
    if (w->want_lag) TRY(w->lag.alloc(ctx, (size_t)rows));
    if (!w->nccf_in) {
        TRY(w->bal.alloc(ctx, (size_t)rows * L));
        TRY(w->raw.alloc(ctx, (size_t)rows * L));
    }
    HIPWHO(ctx, who, pcl_h2d(ctx, w->row_off, fr.row_off.data(), ((size_t)U + 1) * sizeof(long long)));
    HIPWHO(ctx, who, pcl_h2d(ctx, w->sig_off, so.data(), ((size_t)U + 1) * sizeof(long long)));
    HIPWHO(ctx, who, pcl_h2d(ctx, w->frame_utt, fr.frame_utt.data(), (size_t)rows * sizeof(int)));
    HIPWHO(ctx, who, pcl_h2d(ctx, w->g, a.g, (size_t)L * sizeof(double)));
    const unsigned lanes = (unsigned)((L + 63) / 64 * 64);       // <= 1024 (PITCH_MAX_LAGS)
    if (!w->nccf_in) {
        const size_t shm = pitch_lds_bytes(gm);                  // <= 64 KiB (pitch_geometry_check)
        pcl_timer_begin(ctx, "pitch_nccf");
        if (sig.pcm16)
            hipLaunchKernelGGL(pitch_nccf_kernel<int16_t>, dim3((unsigned)rows), dim3(lanes), shm, ctx->stream, (const int16_t *)d_sig, w->sig_off,
                               w->row_off, w->frame_utt, gm.size, gm.step, gm.Lmin, L, a.ballast, w->bal, w->raw);
        else
            hipLaunchKernelGGL(pitch_nccf_kernel<double>, dim3((unsigned)rows), dim3(lanes), shm, ctx->stream, (const double *)d_sig, w->sig_off,
                               w->row_off, w->frame_utt, gm.size, gm.step, gm.Lmin, L, a.ballast, w->bal, w->raw);
        pcl_timer_end(ctx, "pitch_nccf");
    }
    pcl_timer_begin(ctx, "pitch_track");
    hipLaunchKernelGGL(pitch_track_kernel, dim3((unsigned)U), dim3(lanes), (size_t)3 * L * sizeof(double), ctx->stream, w->bal, w->row_off, w->g,
                       gm.Lmin, L, (double)gm.rate, a.soft_min_f0, a.pf, w->bp, w->lagidx);
    pcl_timer_end(ctx, "pitch_track");
    pcl_timer_begin(ctx, "pitch_out");
    const unsigned blocks = (unsigned)((rows + 255) / 256);
    hipLaunchKernelGGL(pitch_out_kernel, dim3(blocks), dim3(256), 0, ctx->stream, w->raw, w->lagidx, rows, gm.Lmin, L, (double)gm.rate, w->out,
                       w->want_lag ? w->lag.p : nullptr);
    hipLaunchKernelGGL(pitch_delta_kernel, dim3(blocks), dim3(256), 0, ctx->stream, w->row_off, w->frame_utt, rows, w->out);
    pcl_timer_end(ctx, "pitch_out");
    HIPWHO(ctx, who, hipGetLastError());
    return PCL_OK;
}

extern "C" int pcl_pitch(pcl_ctx *ctx, int U, const double *signal, const int64_t *sig_off, int framerate, double sampletime, double overlap,
                         double f_min, double f_max, double ballast, double soft_min_f0, double pf, const double *g, int n_lags, int flags,
                         double *out, int32_t *lag, double *nccf_bal, double *nccf_raw, int64_t out_rows) {
    return pitch_to_host(ctx, "pcl_pitch", SignalView{signal, false, U, sig_off}, FrameSpec{framerate, sampletime, overlap},
                         PitchArgs{f_min, f_max, ballast, soft_min_f0, pf, g, n_lags}, flags, PitchOut{out, lag, nccf_bal, nccf_raw, out_rows});
}

extern "C" int pcl_pitch_pcm16(pcl_ctx *ctx, int U, const int16_t *signal, const int64_t *sig_off, int framerate, double sampletime, double overlap,
                               double f_min, double f_max, double ballast, double soft_min_f0, double pf, const double *g, int n_lags, int flags,
                               double *out, int32_t *lag, double *nccf_bal, double *nccf_raw, int64_t out_rows) {
    return pitch_to_host(ctx, "pcl_pitch_pcm16", SignalView{signal, true, U, sig_off}, FrameSpec{framerate, sampletime, overlap},
                         PitchArgs{f_min, f_max, ballast, soft_min_f0, pf, g, n_lags}, flags, PitchOut{out, lag, nccf_bal, nccf_raw, out_rows});
}
