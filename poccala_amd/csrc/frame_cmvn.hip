// CMVN (row f14): cepstral mean and variance normalisation of the resident frame matrix, per speaker from resident statistics and over a
// sliding window, in place.  The model is never touched.
//   pcl_cmvn_zero             the context's per-speaker statistics n (S), [s | q] (S, 2, D) made and cleared
//   pcl_cmvn_accumulate       per (utterance, chunk of 1024 rows) the partial sums of x and x^2, then one workgroup per speaker adds its
//                             utterances' sums onto the resident ones
//   pcl_frames_cmvn           one workgroup per speaker decides its status and forms m and sqrt(v); then y = (x - m) / sqrt(v) elementwise
//   pcl_frames_cmvn_sliding   a blocked prefix sum of x and x^2 per utterance into a pool block, then the same apply from window sums
// The rule and every summation order are stated in include/poccala_hip.h; tests/_cmvn_twin.py is its NumPy twin.  Everything is float64;
// no floating-point atomics: two runs give the same bits.  Built with -ffp-contract=off: every kernel runs one rounded operation at a time.
// Every index a kernel forms is bounded by what the host validated: speakers < S, features < Dh <= FD <= 64, rows inside [begin[u],
// begin[u] + T[u]) <= F; an element group of the apply kernels is read or written as a vector only when it lies inside its utterance.
#include <math.h>

#include "pcl_internal.h"

namespace {

#include "frame_spans.h"                      // the checks and the upload of a call's utterances

constexpr int CH_ROWS = 1024;                 // rows per chunk of the statistics: the fixed partition the summation order is defined on
constexpr int ROW_LANES = 4;                  // row lanes of a chunk's workgroup (x 64 feature lanes)
constexpr int SCAN_ROWS = 64;                 // rows per block of the sliding form's prefix
constexpr int WINDOW_MAX = 1 << 20;

// ---------------------------------------------------------------- statistics
// One workgroup per (chunk, utterance): thread (r, d) adds x and x^2 of the chunk's rows r, r + 4, ... in ascending order; the four row
// lanes are then added 0, 1, 2, 3.  partial[(choff[u] + chunk) * 128 + d] = the sum of x, + 64 = of x^2.
__global__ __launch_bounds__(256) void cmvn_partial_kernel(const int *__restrict__ T, const long long *__restrict__ begin, const int *__restrict__ spk,
                                                           const long long *__restrict__ choff, const double *__restrict__ x64,
                                                           const float *__restrict__ x32, int FD, int Dh, double *__restrict__ partial) {
    __shared__ double ls[ROW_LANES][64], lq[ROW_LANES][64];
    const int u = blockIdx.y, Tu = T[u];
    const long long lo = (long long)blockIdx.x * CH_ROWS;
    if (spk[u] < 0 || lo >= Tu) return;                           // (uniform in the workgroup)
    const int d = threadIdx.x & 63, r = threadIdx.x >> 6;
    const long long hi = min((long long)Tu, lo + CH_ROWS), row0 = begin[u];
    double as = 0.0, aq = 0.0;
    if (d < Dh)
        for (long long t = lo + r; t < hi; t += ROW_LANES) {
            const size_t at = (size_t)(row0 + t) * FD + d;
            const double x = x64 ? x64[at] : (double)x32[at];
            as = as + x;
            aq = aq + x * x;
        }
    ls[r][d] = as;
    lq[r][d] = aq;
    __syncthreads();
    if (r == 0) {
        double s = ls[0][d], q = lq[0][d];
#pragma unroll
        for (int k = 1; k < ROW_LANES; ++k) {
            s = s + ls[k][d];
            q = q + lq[k][d];
        }
        double *p = partial + (size_t)(choff[u] + blockIdx.x) * 128;
        p[d] = s;
        p[64 + d] = q;
    }
}

// One workgroup per speaker, thread (k, d): over the speaker's utterances of this call in ascending index (list[ptr[s] .. ptr[s + 1])), the
// utterance's chunk partials are added in chunk order from 0, and the utterance's sum is added onto the resident one.  n: thread 0.
__global__ __launch_bounds__(128) void cmvn_speaker_kernel(const int *__restrict__ T, const long long *__restrict__ choff, const int *__restrict__ ptr,
                                                           const int *__restrict__ list, const double *__restrict__ partial, int Dh,
                                                           long long *__restrict__ n_res, double *__restrict__ sq_res) {
    const int s = blockIdx.x, d = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int a = ptr[s], b = ptr[s + 1];
    if (a == b) return;
    if (threadIdx.x == 0) {
        long long n = n_res[s];
        for (int i = a; i < b; ++i) n += T[list[i]];
        n_res[s] = n;
    }
    if (d >= Dh) return;
    double res = sq_res[((size_t)s * 2 + k) * Dh + d];
    for (int i = a; i < b; ++i) {
        const int u = list[i];
        const int nc = (T[u] + CH_ROWS - 1) / CH_ROWS;
        const double *p = partial + (size_t)choff[u] * 128 + k * 64 + d;
        double us = 0.0;
        for (int c = 0; c < nc; ++c) us = us + p[(size_t)c * 128];
        res = res + us;
    }
    sq_res[((size_t)s * 2 + k) * Dh + d] = res;
}

// ---------------------------------------------------------------- the rule, one rounded operation at a time
__device__ __forceinline__ double cmvn_floor(double q_over_n, double m, double var_floor) {
    const double t = q_over_n - m * m;
    return t > var_floor ? t : var_floor;
}

// One wave per speaker: its status, and for an accepted speaker ms[s][0][d] = m, ms[s][1][d] = sqrt(v).  Nothing of the frames is touched.
__global__ __launch_bounds__(64) void cmvn_decide_kernel(const long long *__restrict__ n_res, const double *__restrict__ sq_res, int Dh, long long min_count,
                                                         double var_floor, int *__restrict__ status, double *__restrict__ ms) {
    const int s = blockIdx.x, d = threadIdx.x;
    const long long n = n_res[s];
    const double sum = d < Dh ? sq_res[((size_t)s * 2) * Dh + d] : 0.0, sqr = d < Dh ? sq_res[((size_t)s * 2 + 1) * Dh + d] : 0.0;
    const bool bad = !(fabs(sum) < INFINITY) || !(fabs(sqr) < INFINITY);
    const int st = n < min_count ? PCL_CMVN_LOW_COUNT : (__ballot(bad) != 0ull ? PCL_CMVN_NOT_FINITE : PCL_CMVN_OK);
    if (d == 0) status[s] = st;
    if (st != PCL_CMVN_OK || d >= Dh) return;
    const double nn = (double)n, m = sum / nn;
    ms[((size_t)s * 2) * Dh + d] = m;
    ms[((size_t)s * 2 + 1) * Dh + d] = sqrt(cmvn_floor(sqr / nn, m, var_floor));
}

// ---------------------------------------------------------------- element groups of the apply kernels
// The rows of an utterance are one contiguous run of T FD elements [g0, g1) of the frame matrix.  A thread owns the aligned group of G
// consecutive elements [ga, ga + G), ga a multiple of G: G = 2 with the float64 copy (16-byte loads and stores of it, 8-byte stores of the
// float32 rows), G = 4 without (16-byte loads and stores of the float32 rows).  A group that sticks out of the utterance is read element by
// element, and one that holds a padding column is written so: nothing outside the utterance's rows is read, nothing outside their D
// columns is written.
template <int G>
struct Group {
    double x[G];
    bool on[G];                               // the element is a feature column of a row of the utterance
    int t[G], d[G];                           // its row inside the utterance and its column
    bool whole;                               // every element is on: vector stores
};
template <int G>
__device__ __forceinline__ void group_load(Group<G> &g, const double *x64, const float *x32, long long ga, long long g0, long long g1,
                                           int FD, int Dh) {
    long long t;
    int d;
    if (ga >= g0) {
        const unsigned long long loc = (unsigned long long)(ga - g0);
        if (loc < (1ull << 32)) {
            t = (unsigned)loc / (unsigned)FD;
            d = (int)((unsigned)loc - (unsigned)t * (unsigned)FD);
        } else {
            t = (long long)(loc / (unsigned)FD);
            d = (int)(loc - (unsigned long long)t * (unsigned)FD);
        }
    } else {                                  // (the first group of the utterance may start before it: FD > G)
        t = -1;
        d = FD - (int)(g0 - ga);
    }
    const bool inside = ga >= g0 && ga + G <= g1;
    g.whole = true;
#pragma unroll
    for (int e = 0; e < G; ++e) {
        g.on[e] = ga + e >= g0 && ga + e < g1 && d < Dh;
        g.t[e] = (int)t;
        g.d[e] = d;
        g.whole = g.whole && g.on[e];
        if (++d == FD) {
            d = 0;
            ++t;
        }
    }
    if (inside) {
        if constexpr (G == 2) {
            const double2 v = *reinterpret_cast<const double2 *>(x64 + ga);
            g.x[0] = v.x;
            g.x[1] = v.y;
        } else {
            const float4 v = *reinterpret_cast<const float4 *>(x32 + ga);
            g.x[0] = (double)v.x;
            g.x[1] = (double)v.y;
            g.x[2] = (double)v.z;
            g.x[3] = (double)v.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < G; ++e) g.x[e] = g.on[e] ? (G == 2 ? x64[ga + e] : (double)x32[ga + e]) : 0.0;
    }
}
template <int G>
__device__ __forceinline__ void group_store(const Group<G> &g, const double (&y)[G], double *x64, float *x32, long long ga) {
    if (g.whole) {
        if constexpr (G == 2) {
            *reinterpret_cast<double2 *>(x64 + ga) = make_double2(y[0], y[1]);
            *reinterpret_cast<float2 *>(x32 + ga) = make_float2((float)y[0], (float)y[1]);
        } else {
            *reinterpret_cast<float4 *>(x32 + ga) = make_float4((float)y[0], (float)y[1], (float)y[2], (float)y[3]);
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < G; ++e)
        if (g.on[e]) {
            if constexpr (G == 2) x64[ga + e] = y[e];
            x32[ga + e] = (float)y[e];
        }
}

// y = (x - m) / sqrt(v) (norm_vars) or x - m for the rows of utterance u, one workgroup per (256 groups, utterance)
template <int G>
__global__ __launch_bounds__(256) void cmvn_apply_kernel(const int *__restrict__ T, const long long *__restrict__ begin, const int *__restrict__ spk,
                                                         const int *__restrict__ status, const double *__restrict__ ms, int norm_vars,
                                                         double *__restrict__ x64, float *__restrict__ x32, int FD, int Dh) {
    const int u = blockIdx.y, s = spk[u];
    if (s < 0 || status[s] != PCL_CMVN_OK) return;               // (uniform in the workgroup)
    const long long g0 = begin[u] * FD, g1 = g0 + (long long)T[u] * FD;
    const long long ga = (g0 / G + (long long)blockIdx.x * 256 + threadIdx.x) * G;
    if (ga >= g1) return;
    Group<G> g;
    group_load<G>(g, x64, x32, ga, g0, g1, FD, Dh);
    double y[G];
#pragma unroll
    for (int e = 0; e < G; ++e) {
        y[e] = 0.0;
        if (g.on[e]) {
            const double c = g.x[e] - ms[((size_t)s * 2) * Dh + g.d[e]];
            y[e] = norm_vars ? c / ms[((size_t)s * 2 + 1) * Dh + g.d[e]] : c;
        }
    }
    group_store<G>(g, y, x64, x32, ga);
}

// ---------------------------------------------------------------- sliding window: the blocked prefix
// One wave per (utterance, block of 64 rows), lane d: the block's local inclusive prefix of x and x^2 in ascending row order into
// loc[k][(poff[u] + t) * Dh + d], the block's totals into tot[k][(boff[u] + block) * Dh + d]
__global__ __launch_bounds__(256) void cmvn_scan_local_kernel(const int *__restrict__ T, const long long *__restrict__ begin, const long long *__restrict__ poff,
                                                              const long long *__restrict__ boff, const double *__restrict__ x64,
                                                              const float *__restrict__ x32, int FD, int Dh, double *__restrict__ loc_s,
                                                              double *__restrict__ loc_q, double *__restrict__ tot_s, double *__restrict__ tot_q) {
    const int u = blockIdx.y, Tu = T[u], d = threadIdx.x & 63;
    const long long blk = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), lo = blk * SCAN_ROWS;
    if (lo >= Tu || d >= Dh) return;
    const long long hi = min((long long)Tu, lo + SCAN_ROWS), row0 = begin[u], p0 = poff[u];
    double as = 0.0, aq = 0.0;
    for (long long t = lo; t < hi; ++t) {
        const size_t at = (size_t)(row0 + t) * FD + d;
        const double x = x64 ? x64[at] : (double)x32[at];
        as = as + x;
        aq = aq + x * x;
        loc_s[(size_t)(p0 + t) * Dh + d] = as;
        loc_q[(size_t)(p0 + t) * Dh + d] = aq;
    }
    tot_s[(size_t)(boff[u] + blk) * Dh + d] = as;
    tot_q[(size_t)(boff[u] + blk) * Dh + d] = aq;
}

// One workgroup per utterance, thread (k, d): the block totals become the blocks' offsets, scanned in ascending block order from 0, in place
__global__ __launch_bounds__(128) void cmvn_scan_offsets_kernel(const int *__restrict__ T, const long long *__restrict__ boff, int Dh,
                                                                double *__restrict__ tot_s, double *__restrict__ tot_q) {
    const int u = blockIdx.x, d = threadIdx.x & 63;
    if (d >= Dh) return;
    double *tot = (threadIdx.x >> 6) ? tot_q : tot_s;
    const long long nb = ((long long)T[u] + SCAN_ROWS - 1) / SCAN_ROWS;
    double a = 0.0;
#pragma unroll 8
    for (long long b = 0; b < nb; ++b) {
        const size_t at = (size_t)(boff[u] + b) * Dh + d;
        const double t = tot[at];
        tot[at] = a;
        a = a + t;
    }
}

// P[r], r in [0, T]: 0 at r = 0, else offset[block of row r - 1] + local[r - 1]
__device__ __forceinline__ double cmvn_prefix(const double *__restrict__ loc, const double *__restrict__ off, long long p0, long long b0, long long r, int Dh, int d) {
    if (r == 0) return 0.0;
    return off[(size_t)(b0 + (r - 1) / SCAN_ROWS) * Dh + d] + loc[(size_t)(p0 + r - 1) * Dh + d];
}

template <int G>
__global__ __launch_bounds__(256) void cmvn_sliding_kernel(const int *__restrict__ T, const long long *__restrict__ begin, const long long *__restrict__ poff,
                                                           const long long *__restrict__ boff, const double *__restrict__ loc_s,
                                                           const double *__restrict__ loc_q, const double *__restrict__ off_s,
                                                           const double *__restrict__ off_q, int window, int min_window, int center, int norm_vars,
                                                           double var_floor, double *__restrict__ x64, float *__restrict__ x32, int FD, int Dh) {
    const int u = blockIdx.y;
    const long long Tu = T[u];
    const long long g0 = begin[u] * FD, g1 = g0 + Tu * FD;
    const long long ga = (g0 / G + (long long)blockIdx.x * 256 + threadIdx.x) * G;
    if (ga >= g1) return;
    const long long p0 = poff[u], b0 = boff[u];
    Group<G> g;
    group_load<G>(g, x64, x32, ga, g0, g1, FD, Dh);
    double y[G];
#pragma unroll
    for (int e = 0; e < G; ++e) {
        y[e] = 0.0;
        if (!g.on[e]) continue;
        const long long t = g.t[e];
        long long lo, hi;
        if (center) {
            lo = t - window / 2;
            hi = lo + window;
            if (lo < 0) {
                hi -= lo;
                lo = 0;
            }
            if (hi > Tu) {
                lo = max(0ll, lo - (hi - Tu));
                hi = Tu;
            }
        } else {
            lo = max(0ll, t - window + 1);
            hi = t + 1;
            if (hi - lo < min_window) hi = min(Tu, lo + min_window);
        }
        const int d = g.d[e];
        const double n = (double)(hi - lo);
        const double sum = cmvn_prefix(loc_s, off_s, p0, b0, hi, Dh, d) - cmvn_prefix(loc_s, off_s, p0, b0, lo, Dh, d);
        const double m = sum / n, c = g.x[e] - m;
        if (norm_vars) {
            const double sqr = cmvn_prefix(loc_q, off_q, p0, b0, hi, Dh, d) - cmvn_prefix(loc_q, off_q, p0, b0, lo, Dh, d);
            y[e] = c / sqrt(cmvn_floor(sqr / n, m, var_floor));
        } else {
            y[e] = c;
        }
    }
    group_store<G>(g, y, x64, x32, ga);
}

// ---------------------------------------------------------------- host side
// T / frame_begin of a call: frames loaded, then inside the frame matrix and disjoint (a frame is counted, or normalised, ONCE)
int cmvn_check_ranges(pcl_ctx *ctx, const char *who, int U, const int32_t *T, const int64_t *frame_begin, int *Tmax_out) {
    TRY(frames_loaded_check(ctx, who));
    return spans_check(ctx, who, "a frame is normalised ONCE", U, T, frame_begin, Tmax_out);
}

// the sliding form's rows per group of utterances (env PCL_CMVN_GROUP_ROWS, read on every call): the prefix block of a group holds
// 2 x rows x D doubles.  Default: 2^28 / D rows (4 GiB).  The result does not depend on it.
long long cmvn_group_rows(int Dh) { return env_positive_ll("PCL_CMVN_GROUP_ROWS", (1ll << 28) / Dh); }

}  // namespace

extern "C" int pcl_cmvn_zero(pcl_ctx *ctx, int S) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_cmvn_zero";
    if (!ctx->frames32 || ctx->F <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no frames loaded (the statistics are taken at the frame matrix's dimension)", who);
    if (S < 1 || S > 65535) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: S = %d speakers, need 1 .. 65535", who, S);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int Dh = ctx->FDhost;
    CmvnStats fresh{{}, {}, S, Dh};                               // the statistics in place stay until the new set is there and cleared
    TRY(fresh.n.alloc(ctx, (size_t)S));
    TRY(fresh.sq.alloc(ctx, (size_t)S * 2 * Dh));
    HIPCHK(ctx, hipMemsetAsync(fresh.n, 0, (size_t)S * sizeof(long long), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(fresh.sq, 0, (size_t)S * 2 * Dh * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cmvn = std::move(fresh);
    return PCL_OK;
}

extern "C" int pcl_cmvn_accumulate(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *utt_speaker) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_cmvn_accumulate";
    int Tmax = 0;
    TRY(cmvn_check_ranges(ctx, who, U, T, frame_begin, &Tmax));
    TRY(stats_fits(ctx, who, ctx->cmvn));
    const int S = ctx->cmvn.S, Dh = ctx->cmvn.D;
    TRY(speakers_check(ctx, who, U, utt_speaker, S));
    // per utterance the offset of its chunks' partials; per speaker the list of its utterances with frames, ascending
    std::vector<long long> choff(U, 0);
    std::vector<int> lists(S + 1, 0);
    long long C = 0;
    int Tspk = 0;
    for (int u = 0; u < U; ++u) {
        choff[u] = C;
        if (utt_speaker[u] < 0 || T[u] == 0) continue;
        C += (T[u] + CH_ROWS - 1) / CH_ROWS;
        Tspk = std::max(Tspk, (int)T[u]);
        ++lists[utt_speaker[u] + 1];
    }
    if (C == 0) return PCL_OK;
    for (int s = 0; s < S; ++s) lists[s + 1] += lists[s];
    const size_t o_list = lists.size();
    lists.resize(o_list + lists[S]);
    {
        std::vector<int> fill(lists.begin(), lists.begin() + S);
        for (int u = 0; u < U; ++u)
            if (utt_speaker[u] >= 0 && T[u] > 0) lists[o_list + fill[utt_speaker[u]]++] = u;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevSpans d;
    DevBuf<int> d_lists;
    DevBuf<long long> d_choff;
    DevBuf<double> d_partial;
    TRY(d.upload(ctx, U, T, frame_begin, utt_speaker));
    TRY(d_lists.alloc(ctx, lists.size()));
    TRY(d_choff.alloc(ctx, (size_t)U));
    TRY(d_partial.alloc(ctx, (size_t)C * 128));
    HIPCHK(ctx, pcl_h2d(ctx, d_lists, lists.data(), lists.size() * sizeof(int)));
    HIPCHK(ctx, pcl_h2d(ctx, d_choff, choff.data(), (size_t)U * sizeof(long long)));
    pcl_timer_begin(ctx, "cmvn_stats");
    hipLaunchKernelGGL(cmvn_partial_kernel, dim3((unsigned)((Tspk + CH_ROWS - 1) / CH_ROWS), (unsigned)U), dim3(256), 0, st, d.T, d.begin, d.spk, d_choff,
                       ctx->frames64.p, ctx->frames32, ctx->FD, Dh, d_partial.p);
    hipLaunchKernelGGL(cmvn_speaker_kernel, dim3((unsigned)S), dim3(128), 0, st, d.T, d_choff, d_lists.p, d_lists.p + o_list, d_partial.p, Dh, ctx->cmvn.n.p,
                       ctx->cmvn.sq.p);
    pcl_timer_end(ctx, "cmvn_stats");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));                        // (the locals above are free to go)
    return PCL_OK;
}

extern "C" int pcl_cmvn_stats_download(pcl_ctx *ctx, int64_t *n, double *s, double *q) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_cmvn_stats_download";
    TRY(stats_fits(ctx, who, ctx->cmvn));
    const int S = ctx->cmvn.S, Dh = ctx->cmvn.D;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n) {
        static_assert(sizeof(long long) == sizeof(int64_t), "n travels as it is held");
        HIPCHK(ctx, hipMemcpyAsync(n, ctx->cmvn.n, (size_t)S * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (s || q) {
        std::vector<double> host((size_t)S * 2 * Dh);
        HIPCHK(ctx, hipMemcpyAsync(host.data(), ctx->cmvn.sq, host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (int sp = 0; sp < S; ++sp) {
            if (s) memcpy(s + (size_t)sp * Dh, &host[((size_t)sp * 2) * Dh], (size_t)Dh * sizeof(double));
            if (q) memcpy(q + (size_t)sp * Dh, &host[((size_t)sp * 2 + 1) * Dh], (size_t)Dh * sizeof(double));
        }
    }
    return PCL_OK;
}

extern "C" int pcl_frames_cmvn(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *utt_speaker, int S, int norm_vars,
                               double var_floor, int64_t min_count, int32_t *status_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_frames_cmvn";
    int Tmax = 0;
    TRY(cmvn_check_ranges(ctx, who, U, T, frame_begin, &Tmax));
    TRY(stats_fits(ctx, who, ctx->cmvn));
    if (S != ctx->cmvn.S) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: S = %d speakers, the resident statistics hold %d", who, S, ctx->cmvn.S);
    TRY(speakers_check(ctx, who, U, utt_speaker, S));
    if (norm_vars && !(var_floor > 0.0 && std::isfinite(var_floor))) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: var_floor = %g is not a finite number > 0", who, var_floor);
    if (min_count < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: min_count = %lld, need at least 1", who, (long long)min_count);
    const int Dh = ctx->cmvn.D, FD = ctx->FD;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevSpans d;
    DevBuf<int> d_status;
    DevBuf<double> d_ms;
    TRY(d.upload(ctx, U, T, frame_begin, utt_speaker));
    TRY(d_status.alloc(ctx, (size_t)S));
    TRY(d_ms.alloc(ctx, (size_t)S * 2 * Dh));
    pcl_timer_begin(ctx, "cmvn_apply");
    hipLaunchKernelGGL(cmvn_decide_kernel, dim3((unsigned)S), dim3(64), 0, st, ctx->cmvn.n.p, ctx->cmvn.sq.p, Dh, (long long)min_count,
                       norm_vars ? var_floor : 0.0, d_status.p, d_ms.p);
    if (Tmax > 0) {
        if (ctx->frames64) {
            const unsigned gx = (unsigned)(((long long)Tmax * FD + 2) / 2 / 256 + 1);   // (a run of n elements meets at most n / G + 1 aligned groups)
            hipLaunchKernelGGL(cmvn_apply_kernel<2>, dim3(gx, (unsigned)U), dim3(256), 0, st, d.T, d.begin, d.spk, d_status, d_ms, norm_vars, ctx->frames64.p,
                               ctx->frames32, FD, Dh);
        } else {
            const unsigned gx = (unsigned)(((long long)Tmax * FD + 4) / 4 / 256 + 1);
            hipLaunchKernelGGL(cmvn_apply_kernel<4>, dim3(gx, (unsigned)U), dim3(256), 0, st, d.T, d.begin, d.spk, d_status, d_ms, norm_vars, (double *)nullptr,
                               ctx->frames32, FD, Dh);
        }
    }
    pcl_timer_end(ctx, "cmvn_apply");
    HIPCHK(ctx, hipGetLastError());
    if (status_out) HIPCHK(ctx, hipMemcpyAsync(status_out, d_status, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return PCL_OK;
}

extern "C" int pcl_frames_cmvn_sliding(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, int window, int min_window, int center,
                                       int norm_vars, double var_floor) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_frames_cmvn_sliding";
    int Tall = 0;
    TRY(cmvn_check_ranges(ctx, who, U, T, frame_begin, &Tall));
    if (window < 1 || window > WINDOW_MAX || min_window < 1 || min_window > window)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: window = %d, min_window = %d, need 1 <= min_window <= window <= %d", who, window, min_window, WINDOW_MAX);
    if (norm_vars && !(var_floor > 0.0 && std::isfinite(var_floor))) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: var_floor = %g is not a finite number > 0", who, var_floor);
    if (Tall == 0) return PCL_OK;
    const int Dh = ctx->FDhost, FD = ctx->FD;
    // groups of consecutive utterances whose prefix block fits; per utterance its first row and first block inside its group's block
    const long long cap = cmvn_group_rows(Dh);
    std::vector<long long> begin(frame_begin, frame_begin + U), poff(U, 0), boff(U, 0);
    std::vector<int> group0(1, 0);
    long long rows = 0, blocks = 0, rows_max = 0, blocks_max = 0;
    for (int u = 0; u < U; ++u) {
        if (rows > 0 && rows + T[u] > cap) {
            group0.push_back(u);
            rows = blocks = 0;
        }
        poff[u] = rows;
        boff[u] = blocks;
        rows += T[u];
        blocks += (T[u] + SCAN_ROWS - 1) / SCAN_ROWS;
        rows_max = std::max(rows_max, rows);
        blocks_max = std::max(blocks_max, blocks);
    }
    group0.push_back(U);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<int> d_T;
    DevBuf<long long> d_off;                                       // [begin | poff | boff]
    DevBuf<double> d_loc, d_tot;
    TRY(d_T.alloc(ctx, (size_t)U));
    TRY(d_off.alloc(ctx, (size_t)U * 3));
    TRY(d_loc.alloc(ctx, (size_t)rows_max * Dh * 2));
    TRY(d_tot.alloc(ctx, (size_t)blocks_max * Dh * 2));
    HIPCHK(ctx, pcl_h2d(ctx, d_T, T, (size_t)U * sizeof(int32_t)));
    HIPCHK(ctx, pcl_h2d(ctx, d_off, begin.data(), (size_t)U * sizeof(long long)));
    HIPCHK(ctx, pcl_h2d(ctx, d_off + U, poff.data(), (size_t)U * sizeof(long long)));
    HIPCHK(ctx, pcl_h2d(ctx, d_off + 2 * (size_t)U, boff.data(), (size_t)U * sizeof(long long)));
    double *loc_s = d_loc.p, *loc_q = d_loc.p + (size_t)rows_max * Dh, *tot_s = d_tot.p, *tot_q = d_tot.p + (size_t)blocks_max * Dh;
    pcl_timer_begin(ctx, "cmvn_sliding");
    for (size_t gi = 0; gi + 1 < group0.size(); ++gi) {            // a group's prefix is complete before any of its rows is written (stream order)
        const int u0 = group0[gi], nu = group0[gi + 1] - u0;
        int Tmax = 0;
        for (int u = u0; u < u0 + nu; ++u) Tmax = std::max(Tmax, (int)T[u]);
        if (Tmax == 0) continue;
        const int *gT = d_T.p + u0;
        const long long *gb = d_off.p + u0, *gp = d_off.p + U + u0, *gbo = d_off.p + 2 * (size_t)U + u0;
        hipLaunchKernelGGL(cmvn_scan_local_kernel, dim3((unsigned)((Tmax + 4 * SCAN_ROWS - 1) / (4 * SCAN_ROWS)), (unsigned)nu), dim3(256), 0, st, gT, gb, gp, gbo,
                           ctx->frames64.p, ctx->frames32, FD, Dh, loc_s, loc_q, tot_s, tot_q);
        hipLaunchKernelGGL(cmvn_scan_offsets_kernel, dim3((unsigned)nu), dim3(128), 0, st, gT, gbo, Dh, tot_s, tot_q);
        if (ctx->frames64) {
            const unsigned gx = (unsigned)(((long long)Tmax * FD + 2) / 2 / 256 + 1);
            hipLaunchKernelGGL(cmvn_sliding_kernel<2>, dim3(gx, (unsigned)nu), dim3(256), 0, st, gT, gb, gp, gbo, loc_s, loc_q, tot_s, tot_q, window, min_window,
                               center ? 1 : 0, norm_vars, norm_vars ? var_floor : 0.0, ctx->frames64.p, ctx->frames32, FD, Dh);
        } else {
            const unsigned gx = (unsigned)(((long long)Tmax * FD + 4) / 4 / 256 + 1);
            hipLaunchKernelGGL(cmvn_sliding_kernel<4>, dim3(gx, (unsigned)nu), dim3(256), 0, st, gT, gb, gp, gbo, loc_s, loc_q, tot_s, tot_q, window, min_window,
                               center ? 1 : 0, norm_vars, norm_vars ? var_floor : 0.0, (double *)nullptr, ctx->frames32, FD, Dh);
        }
    }
    pcl_timer_end(ctx, "cmvn_sliding");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    return PCL_OK;
}
