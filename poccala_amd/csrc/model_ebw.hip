// Discriminative re-estimation (row f18): MMI by extended Baum-Welch from two resident statistics sets, on the device.
//   pcl_ebw_hold            the live statistics block -> a second block of the same layout, the NUMERATOR set; it belongs to the model it was
//                           accumulated under and goes with the next derive pass (pcl_ebw_release: model_derive.hip), as mllr_W goes with the model
//   pcl_ebw_drop            ... by hand
//   pcl_ebw_stats_download  pcl_stats_download of the held set
//   pcl_mstep_ebw           means, variances and weights from (numerator = held set, denominator = live block), then the derive pass pcl_mstep runs
// The rule (include/poccala_hip.h states it in full; tests/_ebw_twin.py is the same rule in NumPy) in coordinates centred on the current mean:
// per set g = acc, x = mean_acc - (bias + mu) acc, c = cov_acc; I-smoothing of the numerator; D = max(E gd, 2 Dmin), Dmin the largest over the
// dimensions of the larger root of v D^2 + (c + g v) D + (c g - x^2) = 0; Povey's iteration for the weights.
// Two kernels.  Means and variances: a wave per mixture, its lanes over the feature dimension, Dmin by a max over the wave; this is the pass that
// streams both statistics blocks and the master copy once.  Weights, one workgroup per state: mixture m lives in thread m % 256, slot m / 256, in
// registers; every iteration's sum is a per-thread sum in slot order, a butterfly over the wave and the four waves' partials in wave order.
// No floating-point atomics (the four counts are integer sums): two calls on the same inputs give the same bits.  Built with -ffp-contract=off: one rounded operation at a time, as the twin runs them.
// Every index a kernel forms is bounded by what the host validated: states < J, mixtures < M <= Mpad, dimensions < Dhost <= D <= 64.
#include <math.h>

#include "pcl_internal.h"

namespace {

constexpr double STAT_BIAS = 100.0;           // mean_acc holds sum gamma (o + bias): pcl_launch_mstep_range passes the same constant
constexpr int EBW_T = 256, EBW_WAVES = EBW_T / 64;

struct EbwArgs {
    const double *n_acc, *n_mean, *n_cov;     // the held (numerator) set
    const double *d_acc, *d_mean, *d_cov;     // the live (denominator) block
    double *mean, *var, *w;                   // the master copy, updated in place
    double *D_used;                           // [J][Mpad], 0 for a kept mixture
    int *counts;                              // [4]: mixtures updated, mixtures kept, variance elements floored, states whose weights were kept
    int M, Mpad, Dd, Dh, weight_iters;
    double E, tau, floor_var;
};

__device__ __forceinline__ bool finite_d(double a) { return fabs(a) < INFINITY; }   // (false for a NaN)

__device__ __forceinline__ double wave_max(double a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmax(a, __shfl_xor(a, o));
    return a;
}
__device__ __forceinline__ double wave_sum(double a) {                              // a butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = a + __shfl_xor(a, o);
    return a;
}
// the workgroup's sum / max of one value per thread: waves in ascending order; `red` is EBW_WAVES doubles of LDS
__device__ __forceinline__ double block_sum(double a, double *red) {
    a = wave_sum(a);
    __syncthreads();                                                                // (the last call's readers are done with red)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < EBW_WAVES; ++k) s = s + red[k];
    return s;
}
__device__ __forceinline__ double block_max(double a, double *red) {
    a = wave_max(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < EBW_WAVES; ++k) s = fmax(s, red[k]);
    return s;
}

// Means and variances: one workgroup per (EBW_CHUNK mixtures, state); wave `wave` takes the chunk's mixtures wave, wave + 4, ...; lane d < Dh one
// feature dimension.  counts[0..2] += mixtures updated, mixtures kept, variance elements floored (integer atomics: any order, the same sum).
constexpr int EBW_CHUNK = 64;
__global__ __launch_bounds__(EBW_T) void ebw_gauss_kernel(EbwArgs a, int nchunk) {
    const int j = blockIdx.x / nchunk, m0 = (blockIdx.x - j * nchunk) * EBW_CHUNK, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Dh = a.Dh, m_end = min(a.M, m0 + EBW_CHUNK);
    const size_t jm0 = (size_t)j * a.Mpad;
    int n_upd = 0, n_keep = 0, n_floor = 0;                       // (wave-uniform)
    const bool on = lane < Dh;
    for (int m = m0 + wave; m < m_end; m += EBW_WAVES) {
        const size_t jm = jm0 + m, e = jm * a.Dd + lane;
        const double gn = a.n_acc[jm], gd = a.d_acc[jm];
        double mu = 0.0, v = 1.0, xn = 0.0, xd = 0.0, cn = 0.0, cd = 0.0;
        if (on) {
            mu = a.mean[e];
            v = a.var[e];
            const double sh = STAT_BIAS + mu;
            xn = a.n_mean[e] - sh * gn;
            xd = a.d_mean[e] - sh * gd;
            cn = a.n_cov[e];
            cd = a.d_cov[e];
        }
        double gs = gn;
        if (finite_d(gn) && gn > 0.0) {                           // I-smoothing: tau more points at the numerator's own mean and variance
            xn = xn + a.tau * xn / gn;
            cn = cn + a.tau * cn / gn;
            gs = gn + a.tau;
        }
        const double g = gs - gd, x = xn - xd, c = cn - cd;
        // the larger root of v D^2 + (c + g v) D + (c g - x^2) = 0, where it is real and positive
        const double qb = c + g * v, qc = c * g - x * x, disc = qb * qb - 4.0 * v * qc;
        double root = 0.0;
        if (on && disc >= 0.0) {
            const double r = (sqrt(disc) - qb) / (2.0 * v);
            if (r > 0.0) root = r;
        }
        const double Dmin = wave_max(root);
        const double Dc = fmax(a.E * gd, 2.0 * Dmin), den = g + Dc;
        const bool bad_el = on && !(finite_d(x) && finite_d(c));
        const bool keep = !finite_d(gn) || !finite_d(gd) || __any(bad_el) || (gn == 0.0 && gd == 0.0) || !(finite_d(den) && den > 0.0);
        if (keep) {                                               // (uniform in the wave)
            ++n_keep;
            if (lane == 0) a.D_used[jm] = 0.0;
            continue;
        }
        ++n_upd;
        bool floored = false;
        if (on) {
            const double delta = x / den;
            double vn = (c + Dc * v) / den - delta * delta;
            if (!(vn >= a.floor_var)) {
                vn = a.floor_var;
                floored = true;
            }
            a.mean[e] = mu + delta;
            a.var[e] = vn;
        }
        n_floor += __popcll(__ballot(floored));
        if (lane == 0) a.D_used[jm] = Dc;
    }
    if (lane == 0) {
        if (n_upd) atomicAdd(a.counts + 0, n_upd);
        if (n_keep) atomicAdd(a.counts + 1, n_keep);
        if (n_floor) atomicAdd(a.counts + 2, n_floor);
    }
}

// Weights on the unsmoothed numerator, one workgroup per state: c_m <- (gn_m + (kmax - k_m) c_m) / sum, k_m = gd_m / w_m over the mixtures with
// w_m > 0.  NT = register slots per thread: M <= NT * EBW_T.  counts[3] += 1 for a state that keeps its weights.
template <int NT>
__global__ __launch_bounds__(EBW_T) void ebw_weight_kernel(EbwArgs a) {
    __shared__ double red[EBW_WAVES];
    const int j = blockIdx.x, tid = threadIdx.x, M = a.M;
    const size_t jm0 = (size_t)j * a.Mpad;
    double gnr[NT], kr[NT], cr[NT];
    bool live[NT];
    double kmax = -INFINITY;
    bool any_occ = false;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int m = tid + i * EBW_T;
        gnr[i] = kr[i] = cr[i] = 0.0;
        live[i] = false;
        if (m < M) {
            const double gn = a.n_acc[jm0 + m], gd = a.d_acc[jm0 + m], w = a.w[jm0 + m];
            any_occ = any_occ || !(gn == 0.0 && gd == 0.0);
            if (w > 0.0) {
                live[i] = true;
                gnr[i] = gn;
                kr[i] = gd / w;
                cr[i] = w;
                kmax = fmax(kmax, kr[i]);
            }
        }
    }
    kmax = block_max(kmax, red);
    bool keep_w = block_max(any_occ ? 1.0 : 0.0, red) == 0.0;     // nothing reached the state in either set
#pragma unroll
    for (int i = 0; i < NT; ++i) kr[i] = live[i] ? kmax - kr[i] : 0.0;
    for (int it = 0; it < a.weight_iters && !keep_w; ++it) {      // (keep_w is uniform in the workgroup)
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            cr[i] = live[i] ? gnr[i] + kr[i] * cr[i] : 0.0;
            s = s + cr[i];
        }
        s = block_sum(s, red);
        if (!(finite_d(s) && s > 0.0)) keep_w = true;
#pragma unroll
        for (int i = 0; i < NT; ++i) cr[i] = cr[i] / s;
    }
    if (!keep_w && a.weight_iters > 0) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int m = tid + i * EBW_T;
            if (m < M && live[i]) a.w[jm0 + m] = cr[i];
        }
    }
    if (tid == 0 && keep_w) atomicAdd(a.counts + 3, 1);
}

int derive_after(pcl_ctx *ctx) {                                  // what pcl_launch_mstep runs behind its kernel; waits for the stream
    pcl_timer_begin(ctx, "derive");
    const int rc = pcl_launch_derive(ctx);
    pcl_timer_end(ctx, "derive");
    return rc;
}

}  // namespace

extern "C" int pcl_ebw_hold(pcl_ctx *ctx) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ctx->mean64 || !ctx->stats || ctx->J <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_ebw_hold: no model uploaded, so no statistics either");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, pcl_stats_join(ctx));
    TRY(ctx->ebw_num.reserve(ctx, ctx->stats_len));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ebw_num, ctx->stats, ctx->stats_len * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

extern "C" int pcl_ebw_drop(pcl_ctx *ctx) {
    if (!ctx) return PCL_ERR_INVALID;
    pcl_ebw_release(ctx);
    return PCL_OK;
}

extern "C" int pcl_ebw_stats_download(pcl_ctx *ctx, double *acc, double *alpha_acc, double *mean_acc, double *cov_acc) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ctx->ebw_num) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_ebw_stats_download: no statistics held for this model (pcl_ebw_hold first)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return pcl_stats_block_download(ctx, ctx->ebw_num, acc, alpha_acc, mean_acc, cov_acc);
}

extern "C" int pcl_mstep_ebw(pcl_ctx *ctx, double E, double tau, double c_covariance, int weight_iters, double *D_out, int64_t *counts_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_mstep_ebw";
    if (!ctx->mean64 || !ctx->stats || ctx->J <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no model uploaded", who);
    if (!ctx->ebw_num) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no numerator statistics held for this model (pcl_ebw_hold after the numerator pass)", who);
    if (!(E > 0.0) || !std::isfinite(E)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: E = %g is not a finite number > 0", who, E);
    if (!(tau >= 0.0) || !std::isfinite(tau)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: tau = %g is not a finite number >= 0", who, tau);
    if (!(c_covariance >= 0.0) || !std::isfinite(c_covariance)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: c_covariance = %g is not a finite number >= 0", who, c_covariance);
    if (weight_iters < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: weight_iters = %d", who, weight_iters);
    const int J = ctx->J, M = ctx->M, Mpad = ctx->Mpad;
    if (M > 16 * EBW_T || ctx->D > 64 || (long long)J * ((M + EBW_CHUNK - 1) / EBW_CHUNK) > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: M = %d mixtures or D = %d, the kernel holds at most %d and 64", who, M, ctx->D, 16 * EBW_T);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, pcl_stats_join(ctx));
    DevBuf<double> d_D;
    DevBuf<int> d_cnt;
    TRY(d_D.alloc(ctx, (size_t)J * Mpad));
    TRY(d_cnt.alloc(ctx, 4));
    const size_t nm = (size_t)J * Mpad * ctx->D;
    const double *num = ctx->ebw_num;                             // the live block's layout: [acc | alpha | mean | cov]
    EbwArgs a{num, num + (size_t)J * Mpad + J, num + (size_t)J * Mpad + J + nm, ctx->st_acc, ctx->st_mean, ctx->st_cov, ctx->mean64, ctx->var64, ctx->w64,
              d_D, d_cnt, M, Mpad, ctx->D, ctx->Dhost, weight_iters, E, tau, c_covariance};
    const int nchunk = (M + EBW_CHUNK - 1) / EBW_CHUNK;
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 4 * sizeof(int), ctx->stream));
    pcl_timer_begin(ctx, "ebw");
    // (the weight kernel reads the weights it rewrites and nothing the other kernel writes: their order is free)
    hipLaunchKernelGGL(ebw_gauss_kernel, dim3((unsigned)(J * nchunk)), dim3(EBW_T), 0, ctx->stream, a, nchunk);
    if (M <= EBW_T) hipLaunchKernelGGL(ebw_weight_kernel<1>, dim3(J), dim3(EBW_T), 0, ctx->stream, a);
    else if (M <= 4 * EBW_T) hipLaunchKernelGGL(ebw_weight_kernel<4>, dim3(J), dim3(EBW_T), 0, ctx->stream, a);
    else hipLaunchKernelGGL(ebw_weight_kernel<16>, dim3(J), dim3(EBW_T), 0, ctx->stream, a);
    pcl_timer_end(ctx, "ebw");
    HIPCHK(ctx, hipGetLastError());
    std::vector<double> hD(D_out ? (size_t)J * Mpad : 0);
    int hc[4] = {0, 0, 0, 0};
    if (D_out) HIPCHK(ctx, pcl_d2h_queue(ctx, hD.data(), d_D, hD.size() * sizeof(double)));
    HIPCHK(ctx, pcl_d2h_queue(ctx, hc, d_cnt, sizeof(hc)));
    const int rc = derive_after(ctx);                             // (waits for the stream; a new model: the held set goes, pcl_ebw_release)
    TRY(rc);
    if (D_out)
        for (int j = 0; j < J; ++j) memcpy(D_out + (size_t)j * M, hD.data() + (size_t)j * Mpad, (size_t)M * sizeof(double));
    if (counts_out)
        for (int k = 0; k < 4; ++k) counts_out[k] = hc[k];
    return PCL_OK;
}
