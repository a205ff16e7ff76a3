// Speaker adaptation (row f10): MLLR mean transforms and MAP means from the resident E-step statistics, on the device.
//   pcl_mllr_estimate          statistics -> (G, k) per (class, feature dimension): a split-K float64 GEMM over the class's mixtures on
//                              v_mfma_f64_16x16x4_f64, per-chunk partials reduced in chunk order -> Cholesky + two triangular solves per
//                              (class, dimension) -> W[r] (D x (D+1), column 0 the offset), kept resident with the model
//   pcl_model_transform_means  mean <- A_r mean + b_r in place on the float64 master copy, then the derive pass pcl_mstep runs
//   pcl_mstep_map              mean <- (tau mean + s) / (tau + acc), then the same derive pass
// The rule (include/poccala_hip.h states it in full): s = mean_acc - bias acc (bias = 100, the accumulate pass's), a mixture contributes
// when its acc is finite and > 0, padding mixtures are never visited.  Everything is float64; no floating-point atomics: a chunk's partial
// is summed wave by wave, the chunks of a class chunk by chunk, so two runs give the same bits.  Built with -ffp-contract=off: the MAP and
// apply kernels run one rounded operation at a time, as the NumPy twin (tests/_adapt_twin.py) does.
// Every index a kernel forms is bounded by what the host validated: states < J, mixtures < M, dimensions < Dhost <= 48, classes < R.
#include <math.h>

#include "pcl_internal.h"

namespace {

#include "frame_spans.h"                      // env_positive_ll
#include "adapt_common.h"                     // the GEMM over an operand source, the chunk reduction, the solve: shared with frame_adapt.hip

constexpr double STAT_BIAS = 100.0;           // mean_acc holds sum gamma (o + bias): pcl_launch_mstep_range passes the same constant

// The GEMM's operand source: the model, the statistics and the walk over a class's mixtures.  A class's mixture space is its states in
// list order (cls_states[cls_off[r] ...], ascending state index), M real mixtures each; chunk c covers [chunk_e0[c], + chunk_n[c]) of it.
// The two operands of mixture `le` of a chunk for feature dimension i and row / column p of the padded (D + 2) grid:
//   a = xi[p]                        xi = (1, mu_1 .. mu_D), 0 beyond
//   b = (acc / var_i) xi[p]  (p <= D),  (mean_acc_i - bias acc) / var_i  (p = D + 1: the column that sums to k),  0 beyond
// so that sum a[p] b[q] = G[p][q] (q <= D) and k[p] (q = D + 1).  A mixture that does not contribute gives exact zeros.
struct GkArgs {
    const double *mean, *var, *acc, *macc;
    const int *cls_states, *cls_off, *chunk_cls, *chunk_e0, *chunk_n;
    int M, Mpad, Dd, Dh;
    struct Chunk {
        int s0, e0, n;
    };
    __device__ __forceinline__ Chunk chunk(int c) const { return Chunk{cls_off[chunk_cls[c]], chunk_e0[c], chunk_n[c]}; }
    __device__ __forceinline__ void operands(const Chunk &ch, int le, int i, int p, double &a, double &b) const {
        a = b = 0.0;
        if (le >= ch.n || p > Dh + 1) return;
        const int e = ch.e0 + le, js = e / M, m = e - js * M;
        const size_t jm = (size_t)cls_states[ch.s0 + js] * Mpad + m;
        const double oc = acc[jm];
        if (!(oc > 0.0 && oc < INFINITY)) return;
        const double v = var[jm * Dd + i];
        if (p == Dh + 1) {
            b = (macc[jm * Dd + i] - STAT_BIAS * oc) / v;
            return;
        }
        a = p == 0 ? 1.0 : mean[jm * Dd + p - 1];
        b = (oc / v) * a;
    }
};

// Per chunk: the occupancy and the number of its contributing mixtures (a fixed tree: the same bits every run)
__global__ __launch_bounds__(256) void mllr_occ_kernel(GkArgs g, double *__restrict__ occ_part, int *__restrict__ cnt_part) {
    __shared__ double so[256];
    __shared__ int sc[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int r = g.chunk_cls[c], e0 = g.chunk_e0[c], n = g.chunk_n[c], s0 = g.cls_off[r];
    double o = 0.0;
    int k = 0;
    for (int le = tid; le < n; le += 256) {
        const int e = e0 + le, js = e / g.M, m = e - js * g.M;
        const double oc = g.acc[(size_t)g.cls_states[s0 + js] * g.Mpad + m];
        if (oc > 0.0 && oc < INFINITY) {
            o += oc;
            ++k;
        }
    }
    so[tid] = o;
    sc[tid] = k;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            so[tid] += so[tid + w];
            sc[tid] += sc[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        occ_part[c] = so[0];
        cnt_part[c] = sc[0];
    }
}

// Per class, in chunk order: occupancy, contributing mixtures, and the refusals that need no factorisation
__global__ void mllr_class_kernel(const int *__restrict__ cls_chunk0, const double *__restrict__ occ_part, const int *__restrict__ cnt_part, int R, int Dh,
                                  double min_occ, double *__restrict__ occ, int *__restrict__ status) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    double o = 0.0;
    long long k = 0;
    for (int c = cls_chunk0[r]; c < cls_chunk0[r + 1]; ++c) {
        o += occ_part[c];
        k += cnt_part[c];
    }
    occ[r] = o;
    status[r] = o < min_occ ? PCL_MLLR_LOW_OCCUPANCY : k < Dh + 1 ? PCL_MLLR_FEW_MIXTURES : PCL_MLLR_OK;
}

// Per class: a failed pivot in any of its D factorisations refuses it; a refused class gets the identity [0 | I]
__global__ __launch_bounds__(64) void mllr_finish_kernel(const int *__restrict__ pivot_bad, int Dh, int *__restrict__ status, double *__restrict__ W) {
    __shared__ int st;
    const int r = blockIdx.x, n = Dh + 1, tid = threadIdx.x;
    if (tid == 0) {
        int s = status[r];
        if (s == PCL_MLLR_OK)
            for (int i = 0; i < Dh; ++i)
                if (pivot_bad[r * Dh + i]) s = PCL_MLLR_NOT_POSITIVE_DEFINITE;
        status[r] = s;
        st = s;
    }
    __syncthreads();
    if (st == PCL_MLLR_OK) return;
    for (int x = tid; x < Dh * n; x += 64) W[(size_t)r * Dh * n + x] = (x % n == x / n + 1) ? 1.0 : 0.0;
}

// mean[j, m, :] <- b_r + A_r mean[j, m, :], one workgroup per (32 mixtures, state): the tile's rows and W[r] are staged in LDS, so the
// update is in place.  The sum runs b, then the terms in ascending feature order, one rounded product and one rounded sum each.
constexpr int APPLY_TM = 32;
__global__ __launch_bounds__(256) void mllr_apply_kernel(double *__restrict__ mean64, const int *__restrict__ state_class, const double *__restrict__ W,
                                                         const int *__restrict__ skip, int M, int Mpad, int Dd, int Dh) {
    __shared__ double Wl[ADAPT_D_MAX * (ADAPT_D_MAX + 1)], mu[APPLY_TM * ADAPT_D_MAX];
    const int j = blockIdx.y, m0 = blockIdx.x * APPLY_TM, n = Dh + 1, tid = threadIdx.x;
    const int r = state_class[j];
    if (r < 0 || skip[r]) return;                                 // (uniform in the workgroup)
    for (int x = tid; x < Dh * n; x += 256) Wl[x] = W[(size_t)r * Dh * n + x];
    for (int x = tid; x < APPLY_TM * Dh; x += 256) {
        const int m = m0 + x / Dh;
        mu[x] = m < M ? mean64[((size_t)j * Mpad + m) * Dd + x % Dh] : 0.0;
    }
    __syncthreads();
    for (int x = tid; x < APPLY_TM * Dh; x += 256) {
        const int ml = x / Dh, d = x % Dh, m = m0 + ml;
        if (m >= M) continue;
        double s = Wl[d * n];
        for (int e = 0; e < Dh; ++e) s = s + Wl[d * n + 1 + e] * mu[ml * Dh + e];
        mean64[((size_t)j * Mpad + m) * Dd + d] = s;
    }
}

// mean <- (tau mean + s) / (tau + acc), s = mean_acc - bias acc, for mixtures with a finite acc > 0; one thread per (state, mixture, dim)
__global__ void map_mean_kernel(const double *__restrict__ st_acc, const double *__restrict__ st_mean, int J, int M, int Mpad, int Dd, int Dh, double tau,
                                double *__restrict__ mean64) {
    const long long total = (long long)J * Mpad * Dd;
    for (long long gid = blockIdx.x * (long long)blockDim.x + threadIdx.x; gid < total; gid += (long long)gridDim.x * blockDim.x) {
        const int d = (int)(gid % Dd);
        const long long jm = gid / Dd;
        if ((int)(jm % Mpad) >= M || d >= Dh) continue;
        const double a = st_acc[jm];
        if (!(a > 0.0 && a < INFINITY)) continue;
        const double s = st_mean[gid] - STAT_BIAS * a;
        mean64[gid] = (tau * mean64[gid] + s) / (tau + a);
    }
}

int derive_after(pcl_ctx *ctx) {                                  // what pcl_launch_mstep runs behind its kernel; waits for the stream
    pcl_timer_begin(ctx, "derive");
    const int rc = pcl_launch_derive(ctx);
    pcl_timer_end(ctx, "derive");
    return rc;
}

// state_class (J, or NULL = all 0) validated against [-1, R)
int check_classes(pcl_ctx *ctx, const char *who, int R, const int32_t *state_class) {
    if (R < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: R = %d regression classes, need at least 1", who, R);
    if (state_class)
        for (int j = 0; j < ctx->J; ++j)
            if (state_class[j] < -1 || state_class[j] >= R)
                PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: state %d has class %d, outside [-1, %d)", who, j, (int)state_class[j], R);
    return PCL_OK;
}

}  // namespace

extern "C" int pcl_mllr_estimate(pcl_ctx *ctx, int R, const int32_t *state_class, double min_occ, double *W_out, double *occ_out, int32_t *status_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_mllr_estimate";
    if (!ctx->mean64 || !ctx->stats || ctx->J <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no model uploaded, so no statistics either", who);
    TRY(check_classes(ctx, who, R, state_class));
    if (!(min_occ >= 0.0) || !std::isfinite(min_occ)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: min_occ = %g is not a finite number >= 0", who, min_occ);
    const int J = ctx->J, M = ctx->M, Dh = ctx->Dhost, n = Dh + 1;
    if (Dh > ADAPT_D_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d, the solve holds at most %d", who, Dh, ADAPT_D_MAX);
    if ((long long)J * M > 0x7fffffffLL || (long long)R * Dh > 0x7fffffffLL / 64) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: J * M = %lld mixtures or R = %d classes do not fit the index", who, (long long)J * M, R);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, pcl_stats_join(ctx));
    hipStream_t st = ctx->stream;

    // states grouped by class (ascending state index inside a class), and every class's mixture space cut into chunks
    const long long chunk = std::min<long long>(mllr_chunk(), 1 << 30);
    std::vector<int> cls_off(R + 1, 0), cls_states, cls_chunk0(R + 1, 0), chunk_cls, chunk_e0, chunk_n;
    for (int j = 0; j < J; ++j) {
        const int r = state_class ? state_class[j] : 0;
        if (r >= 0) ++cls_off[r + 1];
    }
    for (int r = 0; r < R; ++r) cls_off[r + 1] += cls_off[r];
    cls_states.assign(std::max(cls_off[R], 1), 0);
    {
        std::vector<int> fill(cls_off.begin(), cls_off.end() - 1);
        for (int j = 0; j < J; ++j) {
            const int r = state_class ? state_class[j] : 0;
            if (r >= 0) cls_states[fill[r]++] = j;
        }
    }
    for (int r = 0; r < R; ++r) {
        const long long nmix = (long long)(cls_off[r + 1] - cls_off[r]) * M;
        for (long long e0 = 0; e0 < nmix; e0 += chunk) {
            chunk_cls.push_back(r);
            chunk_e0.push_back((int)e0);
            chunk_n.push_back((int)std::min(chunk, nmix - e0));
        }
        cls_chunk0[r + 1] = (int)chunk_cls.size();
    }
    const int C = (int)chunk_cls.size();
    const int NT = (Dh + 2 + 15) / 16, ntiles = NT * (NT + 1) / 2;
    if ((long long)C * Dh > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %d chunks x %d dimensions do not fit a grid: raise PCL_MLLR_CHUNK", who, C, Dh);
    std::vector<int> lists;                                      // one upload: [cls_off | cls_states | cls_chunk0 | chunk_cls | chunk_e0 | chunk_n]
    const size_t o_states = R + 1, o_chunk0 = o_states + cls_states.size(), o_ccls = o_chunk0 + R + 1, o_ce0 = o_ccls + C, o_cn = o_ce0 + C;
    lists.insert(lists.end(), cls_off.begin(), cls_off.end());
    lists.insert(lists.end(), cls_states.begin(), cls_states.end());
    lists.insert(lists.end(), cls_chunk0.begin(), cls_chunk0.end());
    lists.insert(lists.end(), chunk_cls.begin(), chunk_cls.end());
    lists.insert(lists.end(), chunk_e0.begin(), chunk_e0.end());
    lists.insert(lists.end(), chunk_n.begin(), chunk_n.end());

    DevBuf<int> d_lists, d_cnt, d_pivot, d_status;
    DevBuf<double> d_partial, d_occ_part, d_occ, d_Gk, d_W;
    TRY(d_lists.alloc(ctx, lists.size()));
    TRY(d_partial.alloc(ctx, (size_t)C * Dh * ntiles * 256));
    TRY(d_occ_part.alloc(ctx, (size_t)C));
    TRY(d_cnt.alloc(ctx, (size_t)C));
    TRY(d_occ.alloc(ctx, (size_t)R));
    TRY(d_Gk.alloc(ctx, (size_t)R * Dh * n * (n + 1)));
    TRY(d_pivot.alloc(ctx, (size_t)R * Dh));
    TRY(d_W.alloc(ctx, (size_t)R * Dh * n));
    TRY(d_status.alloc(ctx, (size_t)R));
    HIPCHK(ctx, pcl_h2d(ctx, d_lists, lists.data(), lists.size() * sizeof(int)));
    GkArgs g{ctx->mean64, ctx->var64, ctx->st_acc, ctx->st_mean, d_lists + o_states, d_lists, d_lists + o_ccls, d_lists + o_ce0, d_lists + o_cn,
             M, ctx->Mpad, ctx->D, Dh};
    const int *d_chunk0 = d_lists + o_chunk0;

    pcl_timer_begin(ctx, "adapt");                               // the whole call's kernels; "adapt_gk" / "adapt_solve": its two halves
    pcl_timer_begin(ctx, "adapt_gk");
    if (C > 0) {
        const bool valu = mllr_use_valu();
        const int blocks = C * Dh;
        launch_gk(valu, NT, blocks, st, g, d_partial);
        hipLaunchKernelGGL(mllr_occ_kernel, dim3(C), dim3(256), 0, st, g, d_occ_part, d_cnt);
    }
    hipLaunchKernelGGL(gk_reduce_kernel, dim3(R * Dh), dim3(256), 0, st, d_partial, d_chunk0, Dh, NT, d_Gk, false);
    pcl_timer_end(ctx, "adapt_gk");
    pcl_timer_begin(ctx, "adapt_solve");
    hipLaunchKernelGGL(mllr_class_kernel, dim3((R + 63) / 64), dim3(64), 0, st, d_chunk0, d_occ_part, d_cnt, R, Dh, min_occ, d_occ, d_status);
    hipLaunchKernelGGL(gk_solve_kernel, dim3(R * Dh), dim3(64), 0, st, d_Gk, d_status, Dh, d_W, d_pivot, (double *)nullptr);
    hipLaunchKernelGGL(mllr_finish_kernel, dim3(R), dim3(64), 0, st, d_pivot, Dh, d_status, d_W);
    pcl_timer_end(ctx, "adapt_solve");
    pcl_timer_end(ctx, "adapt");
    HIPCHK(ctx, hipGetLastError());

    std::vector<int32_t> status(R);
    HIPCHK(ctx, hipMemcpyAsync(status.data(), d_status, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (W_out) HIPCHK(ctx, hipMemcpyAsync(W_out, d_W, (size_t)R * Dh * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (occ_out) HIPCHK(ctx, hipMemcpyAsync(occ_out, d_occ, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (status_out) memcpy(status_out, status.data(), (size_t)R * sizeof(int32_t));
    ctx->mllr_W = std::move(d_W);                                // the resident estimate: dies with the model (ModelDev)
    ctx->mllr_R = R;
    return PCL_OK;
}

extern "C" int pcl_model_transform_means(pcl_ctx *ctx, int R, const int32_t *state_class, const double *W) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_model_transform_means";
    if (!ctx->mean64 || !ctx->stats || ctx->J <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no model uploaded", who);
    TRY(check_classes(ctx, who, R, state_class));
    const int J = ctx->J, M = ctx->M, Dh = ctx->Dhost, n = Dh + 1;
    if (Dh > ADAPT_D_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d, the kernel holds at most %d", who, Dh, ADAPT_D_MAX);
    if (!W && (!ctx->mllr_W || ctx->mllr_R != R))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: W is NULL and the context holds no estimate of %d classes for this model (pcl_mllr_estimate first)", who, R);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, pcl_stats_join(ctx));
    hipStream_t st = ctx->stream;
    DevBuf<double> d_W;
    DevBuf<int> d_class, d_skip;
    std::vector<int32_t> cls(J, 0);
    if (state_class) memcpy(cls.data(), state_class, (size_t)J * sizeof(int32_t));
    TRY(d_class.alloc(ctx, (size_t)J));
    TRY(d_skip.alloc(ctx, (size_t)R));
    HIPCHK(ctx, pcl_h2d(ctx, d_class, cls.data(), (size_t)J * sizeof(int32_t)));
    if (W) {
        TRY(d_W.alloc(ctx, (size_t)R * Dh * n));
        HIPCHK(ctx, pcl_h2d(ctx, d_W, W, (size_t)R * Dh * n * sizeof(double)));
    }
    const double *dW = W ? d_W.p : ctx->mllr_W.p;
    pcl_timer_begin(ctx, "adapt");
    hipLaunchKernelGGL(gk_identity_kernel, dim3(R), dim3(64), 0, st, dW, Dh, d_skip);
    for (int j0 = 0; j0 < J; j0 += 65535)                        // (the grid's y extent)
        hipLaunchKernelGGL(mllr_apply_kernel, dim3((M + APPLY_TM - 1) / APPLY_TM, std::min(J - j0, 65535)), dim3(256), 0, st,
                           ctx->mean64 + (size_t)j0 * ctx->Mpad * ctx->D, d_class + j0, dW, d_skip, M, ctx->Mpad, ctx->D, Dh);
    pcl_timer_end(ctx, "adapt");
    HIPCHK(ctx, hipGetLastError());
    return derive_after(ctx);                                    // (waits for the stream: the locals above are free to go)
}

extern "C" int pcl_mstep_map(pcl_ctx *ctx, double tau) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_mstep_map";
    if (!ctx->mean64 || !ctx->stats || ctx->J <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no model uploaded", who);
    if (!(tau >= 0.0) || !std::isfinite(tau)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: tau = %g is not a finite number >= 0", who, tau);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, pcl_stats_join(ctx));
    const long long work = (long long)ctx->J * ctx->Mpad * ctx->D;
    pcl_timer_begin(ctx, "adapt");
    hipLaunchKernelGGL(map_mean_kernel, dim3((unsigned)std::min<long long>(4096, (work + 255) / 256)), dim3(256), 0, ctx->stream, ctx->st_acc, ctx->st_mean,
                       ctx->J, ctx->M, ctx->Mpad, ctx->D, ctx->Dhost, tau, ctx->mean64);
    pcl_timer_end(ctx, "adapt");
    HIPCHK(ctx, hipGetLastError());
    return derive_after(ctx);
}
