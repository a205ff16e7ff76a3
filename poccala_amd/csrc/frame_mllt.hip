// MLLT (row f13): ONE square transform A of the features for the whole corpus, the maximum-likelihood linear transform of semi-tied
// covariances (Gales 1999), estimated from resident posteriors and statistics.  The step between LDA (frame_lda.hip) and fMLLR
// (frame_adapt.hip): an LDA projection does not decorrelate the classes it separates, and every Gaussian here is diagonal.
//   pcl_mllt_zero              the context's statistics F (D, D, D) and beta made and cleared, state_keep stored with them
//   pcl_batch_accumulate_mllt  per frame p_i(t), beta(t) (frame_adapt.hip's reduction without q, masked by state_keep) -> F_i += the
//                              split-K float64 GEMM of adapt_common.h over the call's frames, ONE group; beta += the frames' occupancies
//   pcl_mllt_estimate          C_i, the mixture side, by the same GEMM over the kept states' mixtures (each visited twice: two products);
//                              G_i = F_i - C_i; Cholesky of every G_i (one wave each); one wave runs frame_adapt.hip's sweeps with k = 0
// The apply needs no kernel of its own: pcl_frames_transform and pcl_model_transform_means take W = [0 | A].
// The rule and every operation order are stated in include/poccala_hip.h; tests/_mllt_twin.py is its NumPy twin.  Everything is float64;
// no floating-point atomics: two runs give the same bits.  Built with -ffp-contract=off.
// The kernels the two rules share -- the frame reduction, the sweeps, the inversion, the occupancy and pivot statuses -- are
// adapt_frames.h's; their MLLT = true instantiations are compiled HERE, the fMLLR ones in frame_adapt.hip.  The small kernels of
// adapt_frames.h and adapt_common.h that are no templates are emitted into this object too, those this file launches (beta, occupancy
// and pivot statuses) and those it does not (gk_reduce, gk_solve, gk_identity): a few kilobytes of code.
// Every index a kernel forms is bounded by what the host validated: dimensions < Dhost <= 48, frame rows < F, virtual frames < V = the
// frames of the call's kept utterances, kept states < J, mixtures < M, K-elements < 2 x (kept states x M).
#include <math.h>

#include "pcl_internal.h"

namespace {

#include "frame_spans.h"                      // env_positive_ll
#include "adapt_common.h"
#include "adapt_frames.h"

static_assert(PCL_MLLT_OK == PCL_FMLLR_OK && PCL_MLLT_LOW_OCCUPANCY == PCL_FMLLR_LOW_OCCUPANCY &&
                  PCL_MLLT_NOT_POSITIVE_DEFINITE == PCL_FMLLR_NOT_POSITIVE_DEFINITE && PCL_MLLT_SINGULAR == PCL_FMLLR_SINGULAR,
              "the shared kernels write fMLLR's status values");

constexpr double STAT_BIAS = 100.0;           // mean_acc holds sum gamma (o + bias): pcl_launch_mstep_range passes the same constant
// K-elements per chunk when PCL_MLLT_CHUNK is not set.  The frame side is ONE group: at 1024 x 300 frames CHUNK_DEFAULT leaves 5 x D
// workgroups for 256 CUs.  Measured there at D = 39 (tools/mllt_bench.py, profiles/r17_mllt.txt; DESIGN.md section 7 (f13) has the sweep):
// 512 -> 3.84 ms, 1024 -> 3.04, 2048 -> 2.71, 4096 -> 2.59, 8192 -> 2.58, 16384 -> 2.60, 65536 -> 8.28 ms.  4096 .. 16384 are level; 4096
// is taken, which still gives a batch a quarter that size a workgroup per CU.  The mixture side has millions of K-elements and keeps
// CHUNK_DEFAULT, as pcl_mllr_estimate does: a shorter chunk there only multiplies the partials.
constexpr long long MLLT_FRAME_CHUNK_DEFAULT = 4096;

// env PCL_MLLT_CHUNK, read on EVERY call (as PCL_MLLR_CHUNK is): K-elements per chunk of both GEMMs; 0 = not set
long long mllt_chunk_env() { return std::min<long long>(env_positive_ll("PCL_MLLT_CHUNK", 0), 1 << 30); }

// The frame side's operand source: K = the call's kept frames in batch order, chunk c = the virtual frames [c len, + n).  For feature
// dimension i and row / column p of the padded grid:   a = x_t[p],   b = p_i(t) x_t[p]   (p < D; 0 beyond), so that sum a[p] b[q] = F_i[p][q]
struct MlltFrameSrc {
    const double *x64;
    const float *x32;
    const long long *vrow;
    const double *P;
    int V, len, FD, Dh;
    struct Chunk {
        int v0, n;
    };
    __device__ __forceinline__ Chunk chunk(int c) const {
        const long long v0 = (long long)c * len;                  // (< V: the host launched ceil(V / len) chunks)
        return Chunk{(int)v0, (int)min((long long)len, V - v0)};
    }
    __device__ __forceinline__ void operands(const Chunk &ch, int le, int i, int p, double &a, double &b) const {
        a = b = 0.0;
        if (le >= ch.n || p >= Dh) return;
        const size_t v = (size_t)ch.v0 + le;
        const size_t at = (size_t)vrow[v] * FD + p;
        a = x64 ? x64[at] : (double)x32[at];
        b = P[v * Dh + i] * a;
    }
};

// The mixture side's operand source: K = the kept states' mixtures, states in ascending order, M real mixtures each (padding is never
// visited), every mixture TWICE: K-element e is mixture e >> 1 of that walk, and with n = acc, s = mean_acc - bias acc of the mixture
//   e even:   a = s[p],    b = mu[p] / var_i                  the product  s mu^T / var_i
//   e odd:    a = mu[p],   b = (s[p] - n mu[p]) / var_i       the product  mu (s - n mu)^T / var_i
// so that sum a[p] b[q] = C_i[p][q] = sum (s mu^T + mu s^T - n mu mu^T) / var_i.  A mixture whose acc is not finite or not > 0 gives zeros.
struct MlltMixSrc {
    const double *mean, *var, *acc, *macc;
    const int *states;                                            // the kept states, ascending
    long long nel;                                                // 2 x kept states x M
    int len, M, Mpad, Dd, Dh;
    struct Chunk {
        long long e0;
        int n;
    };
    __device__ __forceinline__ Chunk chunk(int c) const {
        const long long e0 = (long long)c * len;
        return Chunk{e0, (int)min((long long)len, nel - e0)};
    }
    __device__ __forceinline__ void operands(const Chunk &ch, int le, int i, int p, double &a, double &b) const {
        a = b = 0.0;
        if (le >= ch.n || p >= Dh) return;
        const long long e = ch.e0 + le, g = e >> 1;
        const int js = (int)(g / M), m = (int)(g - (long long)js * M);
        const size_t jm = (size_t)states[js] * Mpad + m;
        const double oc = acc[jm];
        if (!(oc > 0.0 && oc < INFINITY)) return;
        const double v = var[jm * Dd + i], mu = mean[jm * Dd + p], s = macc[jm * Dd + p] - STAT_BIAS * oc;
        if ((e & 1) == 0) {
            a = s;
            b = mu / v;
        } else {
            a = mu;
            b = (s - oc * mu) / v;
        }
    }
};

// One workgroup per feature dimension i: out[i] = base[i] +- (the chunks' partials summed from 0 in chunk order), element by element of the
// full D x D matrix; the lower triangle reads the upper one's element (a diagonal tile holds both, rounded differently: only its upper half
// is read), so out[i] is symmetric to the bit.  base may be out: a thread reads and writes only its own elements.
__global__ __launch_bounds__(256) void mllt_reduce_kernel(const double *__restrict__ partial, int C, int Dh, int NT, const double *base, double *out,
                                                          bool subtract) {
    const int i = blockIdx.x, ntiles = NT * (NT + 1) / 2;
    for (int x = threadIdx.x; x < Dh * Dh; x += 256) {
        const int p = x / Dh, q = x % Dh, pp = min(p, q), qq = max(p, q);
        const size_t at = (size_t)tile_index(pp >> 4, qq >> 4, NT) * 256 + (pp & 15) * 16 + (qq & 15);
        double sum = 0.0;
        for (int c = 0; c < C; ++c) sum += partial[((size_t)c * Dh + i) * (ntiles * 256) + at];
        const double b0 = base[(size_t)i * Dh * Dh + x];
        out[(size_t)i * Dh * Dh + x] = subtract ? b0 - sum : b0 + sum;
    }
}

// The occupancy of the mixture side: block b adds acc over the mixtures [b per, (b + 1) per) of the kept states' walk that contribute
// (thread t its mixtures t, t + 256, .. in ascending order, then a fixed tree); fmllr_beta_kernel then adds the blocks' sums.
__global__ __launch_bounds__(256) void mllt_occ_kernel(MlltMixSrc g, long long nmix, long long per, double *__restrict__ occ_part) {
    __shared__ double so[256];
    const int tid = threadIdx.x;
    const long long lo = blockIdx.x * per, hi = min(lo + per, nmix);
    double o = 0.0;
    for (long long e = lo + tid; e < hi; e += 256) {
        const int js = (int)(e / g.M), m = (int)(e - (long long)js * g.M);
        const double oc = g.acc[(size_t)g.states[js] * g.Mpad + m];
        if (oc > 0.0 && oc < INFINITY) o += oc;
    }
    so[tid] = o;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) so[tid] += so[tid + w];
        __syncthreads();
    }
    if (tid == 0) occ_part[blockIdx.x] = so[0];
}

// One wave per feature dimension: G_i = L L^T in LDS (gk_solve_kernel's factorisation at order D, nothing to solve behind it).  A pivot
// that is not finite or not > 0 stops the factorisation and flags the dimension.  L_out: [i][D][D] row-major, lower triangle and diagonal.
__global__ __launch_bounds__(64) void mllt_factor_kernel(const double *__restrict__ G, const int *__restrict__ status, int Dh,
                                                         int *__restrict__ pivot_bad, double *__restrict__ L_out) {
    __shared__ double A[ADAPT_D_MAX][ADAPT_D_MAX + 1];
    const int i = blockIdx.x, n = Dh, tid = threadIdx.x;
    if (status[0] != 0) {
        if (tid == 0) pivot_bad[i] = 0;
        return;
    }
    for (int x = tid; x < n * n; x += 64) A[x / n][x % n] = G[(size_t)i * n * n + x];
    __syncthreads();
    const bool bad = chol_factor_lds(A, n, tid);
    if (tid == 0) pivot_bad[i] = bad ? 1 : 0;
    if (bad) return;
    for (int x = tid; x < n * n; x += 64) L_out[(size_t)i * n * n + x] = x % n <= x / n ? A[x / n][x % n] : 0.0;
}

// blocks = chunks x Dh; NT = ceil(Dh / 16) in 1 .. 3: the grid has no offset row and no k column
template <class Src>
void mllt_launch_gk(int NT, int blocks, hipStream_t st, const Src &g, double *partial) {
    const bool valu = mllr_use_valu();
    if (NT == 1) launch_gk_nt<1>(valu, blocks, st, g, partial);
    else if (NT == 2) launch_gk_nt<2>(valu, blocks, st, g, partial);
    else launch_gk_nt<3>(valu, blocks, st, g, partial);
}

const char *mllt_ready(pcl_ctx *ctx) {        // nullptr, or why the statistics cannot be used
    if (!ctx->mean64 || ctx->J <= 0) return "no model uploaded";
    if (!ctx->mllt_F) return "no statistics: pcl_mllt_zero first (a new model or a frame matrix of another dimension dropped them)";
    return nullptr;
}

}  // namespace

void pcl_mllt_release(pcl_ctx *ctx) {
    ctx->mllt_F.release();
    ctx->mllt_beta.release();
    ctx->mllt_keep.release();
    ctx->mllt_keep_host.clear();
}

extern "C" int pcl_mllt_zero(pcl_ctx *ctx, const int32_t *state_keep) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_mllt_zero";
    if (!ctx->mean64 || ctx->J <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no model uploaded (the statistics belong to a model)", who);
    const int Dh = ctx->Dhost, J = ctx->J;
    if (Dh > ADAPT_D_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d, the estimate holds at most %d", who, Dh, ADAPT_D_MAX);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // everything is made in locals and handed to the context when nothing can fail any more: a failed call leaves what was there
    const size_t len = (size_t)Dh * Dh * Dh;
    DevBuf<double> d_F, d_beta;
    DevBuf<int> d_keep;
    std::vector<int32_t> keep;
    TRY(d_F.alloc(ctx, len));
    TRY(d_beta.alloc(ctx, (size_t)1));
    if (state_keep) {
        keep.assign(J, 0);
        for (int j = 0; j < J; ++j) keep[j] = state_keep[j] != 0;
        TRY(d_keep.alloc(ctx, (size_t)J));
        HIPCHK(ctx, pcl_h2d(ctx, d_keep, keep.data(), (size_t)J * sizeof(int32_t)));
    }
    HIPCHK(ctx, hipMemsetAsync(d_F, 0, len * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_beta, 0, sizeof(double), ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mllt_F = std::move(d_F);
    ctx->mllt_beta = std::move(d_beta);
    ctx->mllt_keep = std::move(d_keep);                           // (empty without state_keep: every state is kept)
    ctx->mllt_keep_host = std::move(keep);
    return PCL_OK;
}

// pcl_batch_accumulate_mllt behind its checks of the batch (pcl_batch.hip): the batch has emissions, posteriors and states, is joined, fits
// the current frames and model, and the scoring rows (PCL_LAYOUT_P64) are derived
int pcl_launch_mllt_accumulate(pcl_ctx *ctx, pcl_batch *b, const int32_t *utt_keep) {
    const char *who = "pcl_batch_accumulate_mllt";
    if (const char *why = mllt_ready(ctx)) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: %s", who, why);
    const int U = b->U, Dh = ctx->Dhost;
    if (Dh > ADAPT_D_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d, the estimate holds at most %d", who, Dh, ADAPT_D_MAX);
    std::vector<int> lists(U + 2, -1);                            // one upload: [vbase | 0, V]
    long long V = 0;
    for (int u = 0; u < U; ++u) {
        if (utt_keep && utt_keep[u] == 0) continue;
        if (b->shape.utt[u].frame0 < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d has no frames (the batch was made without frame_begin)", who, u);
        lists[u] = (int)V;
        V += b->shape.utt[u].T;                                         // (V <= sum T < 2^31: pcl_batch_create)
    }
    if (V == 0) return PCL_OK;
    lists[U] = 0;
    lists[U + 1] = (int)V;
    const long long env = mllt_chunk_env(), chunk = env ? env : MLLT_FRAME_CHUNK_DEFAULT;
    const long long C = (V + chunk - 1) / chunk;
    const int NT = (Dh + 15) / 16, ntiles = NT * (NT + 1) / 2;
    if (C * Dh > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %lld chunks x %d dimensions do not fit a grid: raise PCL_MLLT_CHUNK", who, C, Dh);

    hipStream_t st = ctx->stream;
    DevBuf<int> d_lists;
    DevBuf<double> d_P, d_B, d_partial;
    DevBuf<long long> d_vrow;
    TRY(d_lists.alloc(ctx, lists.size()));
    TRY(d_P.alloc(ctx, (size_t)V * Dh));
    TRY(d_B.alloc(ctx, (size_t)V));
    TRY(d_vrow.alloc(ctx, (size_t)V));
    TRY(d_partial.alloc(ctx, (size_t)C * Dh * ntiles * 256));
    HIPCHK(ctx, pcl_h2d(ctx, d_lists, lists.data(), lists.size() * sizeof(int)));

    pcl_timer_begin(ctx, "mllt");                                // the whole call's kernels; "mllt_frames" / "mllt_gk": its two halves
    pcl_timer_begin(ctx, "mllt_frames");
    {
        const unsigned tiles = (unsigned)((b->shape.Tmax + FT - 1) / FT);
        const MlltKeep<true> mk{ctx->mllt_keep.p};
#define FRAMES_CASE(DP)                                                                                                                                  \
    hipLaunchKernelGGL((fmllr_frames_kernel<DP, 1, true>), dim3(tiles, (unsigned)U, 1), dim3(256), 0, st, b->d_utt, b->d_row_state, d_lists, b->Bt, b->lgam, ctx->frames64, \
                       ctx->frames32, ctx->FD, ctx->params64, ctx->row, ctx->w64, ctx->M, ctx->Mpad, Dh, d_P, (double *)nullptr, d_B, d_vrow, mk)
        switch (ctx->D) {                                         // (pcl_device_dim of a dimension <= 48)
            case 13: FRAMES_CASE(13); break;
            case 26: FRAMES_CASE(26); break;
            case 39: FRAMES_CASE(39); break;
            case 47: FRAMES_CASE(47); break;
            default: FRAMES_CASE(48); break;
        }
#undef FRAMES_CASE
    }
    hipLaunchKernelGGL(fmllr_beta_kernel, dim3(1), dim3(256), 0, st, d_B, d_lists + U, ctx->mllt_beta);
    pcl_timer_end(ctx, "mllt_frames");
    pcl_timer_begin(ctx, "mllt_gk");
    MlltFrameSrc g{ctx->frames64, ctx->frames32, d_vrow, d_P, (int)V, (int)chunk, ctx->FD, Dh};
    mllt_launch_gk(NT, (int)(C * Dh), st, g, d_partial);
    hipLaunchKernelGGL(mllt_reduce_kernel, dim3(Dh), dim3(256), 0, st, d_partial, (int)C, Dh, NT, ctx->mllt_F.p, ctx->mllt_F.p, false);
    pcl_timer_end(ctx, "mllt_gk");
    pcl_timer_end(ctx, "mllt");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));                        // (the locals above are free to go)
    return PCL_OK;
}

extern "C" int pcl_mllt_stats_download(pcl_ctx *ctx, double *F, double *beta) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_mllt_stats_download";
    if (const char *why = mllt_ready(ctx)) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: %s", who, why);
    const int Dh = ctx->Dhost;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (F) HIPCHK(ctx, hipMemcpyAsync(F, ctx->mllt_F, (size_t)Dh * Dh * Dh * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (beta) HIPCHK(ctx, hipMemcpyAsync(beta, ctx->mllt_beta, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

extern "C" int pcl_mllt_estimate(pcl_ctx *ctx, int n_iter, double min_occ, double *A_out, double *logdet_out, double *q_trace_out, double *G_out,
                                 double *occ_out, int32_t *status_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_mllt_estimate";
    if (const char *why = mllt_ready(ctx)) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: %s", who, why);
    if (!ctx->stats) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the model has no statistics block", who);
    if (n_iter < 1 || n_iter > 1000) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: n_iter = %d sweeps, need 1 .. 1000", who, n_iter);
    if (!(min_occ >= 0.0) || !std::isfinite(min_occ)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: min_occ = %g is not a finite number >= 0", who, min_occ);
    const int J = ctx->J, M = ctx->M, Dh = ctx->Dhost;
    if (Dh > ADAPT_D_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d, the estimate holds at most %d", who, Dh, ADAPT_D_MAX);
    std::vector<int> states;                                      // the kept states, ascending
    for (int j = 0; j < J; ++j)
        if (ctx->mllt_keep_host.empty() || ctx->mllt_keep_host[j]) states.push_back(j);
    const long long nmix = (long long)states.size() * M, nel = 2 * nmix;
    const long long env = mllt_chunk_env(), chunk = env ? env : CHUNK_DEFAULT;
    const long long C = (nel + chunk - 1) / chunk;
    const int NT = (Dh + 15) / 16, ntiles = NT * (NT + 1) / 2;
    if (C * Dh > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %lld chunks x %d dimensions do not fit a grid: raise PCL_MLLT_CHUNK", who, C, Dh);
    const int nocc = (int)std::min<long long>(1024, (nmix + 255) / 256);   // blocks of the occupancy sum
    const long long per = nocc ? (nmix + nocc - 1) / nocc : 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, pcl_stats_join(ctx));
    hipStream_t st = ctx->stream;

    std::vector<int> lists(states);                               // one upload: [kept states | 0, nocc]
    lists.push_back(0);
    lists.push_back(nocc);
    const size_t nq = (size_t)n_iter + 1, len = (size_t)Dh * Dh * Dh;
    DevBuf<int> d_lists, d_status, d_pivot;
    DevBuf<double> d_partial, d_occ_part, d_occ, d_G, d_L, d_A, d_logdet, d_q;
    TRY(d_lists.alloc(ctx, lists.size()));
    TRY(d_partial.alloc(ctx, (size_t)C * Dh * ntiles * 256));
    TRY(d_occ_part.alloc(ctx, (size_t)std::max(nocc, 1)));
    TRY(d_occ.alloc(ctx, (size_t)1));
    TRY(d_G.alloc(ctx, len));
    TRY(d_L.alloc(ctx, len));
    TRY(d_A.alloc(ctx, (size_t)Dh * Dh));
    TRY(d_logdet.alloc(ctx, (size_t)1));
    TRY(d_q.alloc(ctx, nq));
    TRY(d_status.alloc(ctx, (size_t)1));
    TRY(d_pivot.alloc(ctx, (size_t)Dh));
    HIPCHK(ctx, pcl_h2d(ctx, d_lists, lists.data(), lists.size() * sizeof(int)));
    HIPCHK(ctx, hipMemsetAsync(d_occ, 0, sizeof(double), st));
    MlltMixSrc g{ctx->mean64, ctx->var64, ctx->st_acc, ctx->st_mean, d_lists, nel, (int)chunk, M, ctx->Mpad, ctx->D, Dh};

    pcl_timer_begin(ctx, "mllt");                                // the whole call's kernels; "mllt_gk" / "mllt_solve": its two halves
    pcl_timer_begin(ctx, "mllt_gk");
    if (C > 0) {
        mllt_launch_gk(NT, (int)(C * Dh), st, g, d_partial);
        hipLaunchKernelGGL(mllt_occ_kernel, dim3(nocc), dim3(256), 0, st, g, nmix, per, d_occ_part);
        hipLaunchKernelGGL(fmllr_beta_kernel, dim3(1), dim3(256), 0, st, d_occ_part, d_lists + states.size(), d_occ);
    }
    hipLaunchKernelGGL(mllt_reduce_kernel, dim3(Dh), dim3(256), 0, st, d_partial, (int)C, Dh, NT, ctx->mllt_F.p, d_G.p, true);
    pcl_timer_end(ctx, "mllt_gk");
    pcl_timer_begin(ctx, "mllt_solve");
    hipLaunchKernelGGL(fmllr_occ_kernel, dim3(1), dim3(64), 0, st, ctx->mllt_beta, 1, min_occ, d_status);
    hipLaunchKernelGGL(mllt_factor_kernel, dim3(Dh), dim3(64), 0, st, d_G, d_status, Dh, d_pivot, d_L);
    hipLaunchKernelGGL(fmllr_pivot_kernel, dim3(1), dim3(64), 0, st, d_pivot, 1, Dh, d_status);
    hipLaunchKernelGGL(fmllr_sweep_kernel<true>, dim3(1), dim3(64), 0, st, d_G, d_L, (const double *)nullptr, ctx->mllt_beta, Dh, n_iter, d_status, d_A, d_logdet, d_q);
    pcl_timer_end(ctx, "mllt_solve");
    pcl_timer_end(ctx, "mllt");
    HIPCHK(ctx, hipGetLastError());
    if (A_out) HIPCHK(ctx, hipMemcpyAsync(A_out, d_A, (size_t)Dh * Dh * sizeof(double), hipMemcpyDeviceToHost, st));
    if (logdet_out) HIPCHK(ctx, hipMemcpyAsync(logdet_out, d_logdet, sizeof(double), hipMemcpyDeviceToHost, st));
    if (q_trace_out) HIPCHK(ctx, hipMemcpyAsync(q_trace_out, d_q, nq * sizeof(double), hipMemcpyDeviceToHost, st));
    if (G_out) HIPCHK(ctx, hipMemcpyAsync(G_out, d_G, len * sizeof(double), hipMemcpyDeviceToHost, st));
    if (occ_out) {
        HIPCHK(ctx, hipMemcpyAsync(occ_out, ctx->mllt_beta, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(occ_out + 1, d_occ, sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (status_out) HIPCHK(ctx, hipMemcpyAsync(status_out, d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return PCL_OK;
}
