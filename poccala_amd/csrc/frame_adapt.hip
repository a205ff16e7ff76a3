// fMLLR (row f11): per-speaker affine transforms of the FEATURES, y = b + A x, estimated from resident posteriors and applied in place to the
// resident frame matrix.  The model is never touched.
//   pcl_fmllr_zero              the context's per-speaker statistics [G | k] (S, D, D+1, D+2) and beta (S) made and cleared
//   pcl_batch_accumulate_fmllr  per frame p_i(t), q_i(t), beta(t) (the reduction over rows and mixtures) -> [G | k] += the split-K float64
//                               GEMM of adapt_common.h over the speaker's frames, beta += the frames' occupancies
//   pcl_fmllr_estimate          Cholesky of every G[s,i] (one wave per pair), then one wave per speaker runs the row-by-row sweeps in LDS
//   pcl_frames_transform        y = b + A x in place on the float64 copy (when held) and the float32 rows
// The rule and every operation order are stated in include/poccala_hip.h; tests/_fmllr_twin.py is its NumPy twin.  Everything is float64;
// no floating-point atomics: two runs give the same bits.  Built with -ffp-contract=off: the estimate and the apply kernels run one
// rounded operation at a time (the reduction's posterior uses explicit fused multiply-adds, as gmm_accumulate_kernel's float64 path does).
// Every index a kernel forms is bounded by what the host validated: speakers < S, dimensions < Dhost <= 48, frame rows < F, virtual
// frames < V = the frames of the call's utterances that have a speaker, states < J, mixtures < M.
// The frame reduction, the statuses, the inversion and the sweeps are adapt_frames.h's, shared with MLLT (frame_mllt.hip): this file
// compiles their MLLT = false instantiations, and its own copy of that header's three small kernels that are no templates.
#include <math.h>

#include "pcl_internal.h"

namespace {

#include "frame_spans.h"                      // the checks and the upload of a call's utterances, the chunk plan
#include "adapt_common.h"
#include "adapt_frames.h"

constexpr int APPLY_TF = 32;                  // frames per workgroup of the apply kernel

// The GEMM's operand source: virtual frame v of chunk c for feature dimension i and row / column p of the padded (D + 2) grid:
//   a = zeta[p]                      zeta = (1, x_1 .. x_D), 0 beyond
//   b = p_i(t) zeta[p]  (p <= D),    q_i(t)  (p = D + 1: the column that sums to k),  0 beyond
struct FrameSrc {
    const double *x64;
    const float *x32;
    const long long *vrow;
    const double *P, *Q;
    const int *chunk_v0, *chunk_n;
    int FD, Dh;
    struct Chunk {
        int v0, n;
    };
    __device__ __forceinline__ Chunk chunk(int c) const { return Chunk{chunk_v0[c], chunk_n[c]}; }
    __device__ __forceinline__ void operands(const Chunk &ch, int le, int i, int p, double &a, double &b) const {
        a = b = 0.0;
        if (le >= ch.n || p > Dh + 1) return;
        const size_t v = (size_t)ch.v0 + le;
        if (p == Dh + 1) {
            b = Q[v * Dh + i];
            return;
        }
        if (p == 0) a = 1.0;
        else {
            const size_t at = (size_t)vrow[v] * FD + (p - 1);
            a = x64 ? x64[at] : (double)x32[at];
        }
        b = P[v * Dh + i] * a;
    }
};

// ---------------------------------------------------------------- apply
// y = b + A x for the frames of utterance u, one workgroup per (32-frame tile, utterance): W of the speaker and the tile's rows are staged
// in LDS, so the update is in place.  The sum runs b, then the terms in ascending feature order, one rounded product and one rounded sum each.
__global__ __launch_bounds__(256) void fmllr_apply_kernel(const int *__restrict__ T, const long long *__restrict__ begin, const int *__restrict__ spk,
                                                          const double *__restrict__ W, const int *__restrict__ skip, double *__restrict__ x64,
                                                          float *__restrict__ x32, int FD, int Dh) {
    __shared__ double Wl[ADAPT_D_MAX * (ADAPT_D_MAX + 1)], xs[APPLY_TF * ADAPT_D_MAX];
    const int u = blockIdx.y, t0 = blockIdx.x * APPLY_TF, n = Dh + 1, tid = threadIdx.x;
    const int s = spk[u];
    if (s < 0 || skip[s] || t0 >= T[u]) return;                   // (uniform in the workgroup)
    const int nf = min(APPLY_TF, T[u] - t0);
    const size_t row0 = (size_t)(begin[u] + t0);
    for (int x = tid; x < Dh * n; x += 256) Wl[x] = W[(size_t)s * Dh * n + x];
    for (int x = tid; x < nf * Dh; x += 256) {
        const size_t at = (row0 + x / Dh) * FD + x % Dh;
        xs[x] = x64 ? x64[at] : (double)x32[at];
    }
    __syncthreads();
    for (int x = tid; x < nf * Dh; x += 256) {
        const int f = x / Dh, d = x % Dh;
        double y = Wl[d * n];
        for (int e = 0; e < Dh; ++e) y = y + Wl[d * n + 1 + e] * xs[f * Dh + e];
        const size_t at = (row0 + f) * FD + d;
        if (x64) x64[at] = y;
        x32[at] = (float)y;
    }
}

const char *fmllr_ready(pcl_ctx *ctx) {       // nullptr, or why the statistics cannot be used
    if (!ctx->mean64 || ctx->J <= 0) return "no model uploaded";
    if (!ctx->fmllr_Gk || ctx->fmllr_S <= 0) return "no statistics: pcl_fmllr_zero first (a new model or a frame matrix of another dimension dropped them)";
    return nullptr;
}

}  // namespace

void pcl_fmllr_release(pcl_ctx *ctx) {
    ctx->fmllr_Gk.release();
    ctx->fmllr_beta.release();
    ctx->fmllr_W.release();
    ctx->fmllr_S = 0;
}

extern "C" int pcl_fmllr_zero(pcl_ctx *ctx, int S) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_fmllr_zero";
    if (!ctx->mean64 || ctx->J <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no model uploaded (the statistics belong to a model)", who);
    const int Dh = ctx->Dhost, n = Dh + 1;
    if (Dh > ADAPT_D_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d, the estimate holds at most %d", who, Dh, ADAPT_D_MAX);
    const unsigned long long per = 8ull * Dh * n * (n + 1);
    if (S < 1 || S > 65535 || (unsigned long long)S * per > (1ull << 32))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: S = %d speakers, need 1 .. min(65535, 2^32 / %llu bytes per speaker = %llu)", who, S, per, (1ull << 32) / per);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t len = (size_t)S * Dh * n * (n + 1);
    if (ctx->fmllr_S != S || !ctx->fmllr_Gk) {
        pcl_fmllr_release(ctx);
        TRY(ctx->fmllr_Gk.alloc(ctx, len));
        TRY(ctx->fmllr_beta.alloc(ctx, (size_t)S));
        ctx->fmllr_S = S;
    }
    ctx->fmllr_W.release();                                       // an estimate describes the statistics it was made from
    HIPCHK(ctx, hipMemsetAsync(ctx->fmllr_Gk, 0, len * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->fmllr_beta, 0, (size_t)S * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

// pcl_batch_accumulate_fmllr behind its checks of the batch (pcl_batch.hip): the batch has emissions, posteriors and states, is joined, fits
// the current frames and model, and the scoring rows (PCL_LAYOUT_P64) are derived
int pcl_launch_fmllr_accumulate(pcl_ctx *ctx, pcl_batch *b, const int32_t *utt_speaker) {
    const char *who = "pcl_batch_accumulate_fmllr";
    if (const char *why = fmllr_ready(ctx)) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: %s", who, why);
    const int S = ctx->fmllr_S, U = b->U, Dh = ctx->Dhost;
    TRY(speakers_check(ctx, who, U, utt_speaker, S));
    for (int u = 0; u < U; ++u)
        if (utt_speaker[u] >= 0 && b->shape.utt[u].frame0 < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d has no frames (the batch was made without frame_begin)", who, u);
    // virtual frame order: speakers ascending, a speaker's utterances in batch order; a speaker's frames cut into chunks
    const long long chunk = std::min<long long>(mllr_chunk(), 1 << 30);
    std::vector<int> vbase(U, -1), spk_v0(S + 1, 0), spk_frames(S, 0);
    long long V = 0;
    for (int s = 0; s < S; ++s) {
        spk_v0[s] = (int)V;
        for (int u = 0; u < U; ++u)
            if (utt_speaker[u] == s) {
                vbase[u] = (int)V;
                V += b->shape.utt[u].T;
            }
        spk_frames[s] = (int)(V - spk_v0[s]);
    }
    spk_v0[S] = (int)V;                                           // (V <= sum T < 2^31: pcl_batch_create)
    if (V == 0) return PCL_OK;
    ChunkLists plan;                                              // one upload: [vbase | spk_v0 | spk_chunk0 | chunk_v0 | chunk_n]
    plan.plan({&vbase, &spk_v0}, spk_frames, chunk);
    const int C = plan.C;
    const int NT = (Dh + 2 + 15) / 16, ntiles = NT * (NT + 1) / 2;
    if ((long long)C * Dh > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %d chunks x %d dimensions do not fit a grid: raise PCL_MLLR_CHUNK", who, C, Dh);

    hipStream_t st = ctx->stream;
    DevBuf<double> d_P, d_Q, d_B, d_partial;
    DevBuf<long long> d_vrow;
    TRY(plan.upload(ctx));
    const int *d_lists = plan.d_lists;
    TRY(d_P.alloc(ctx, (size_t)V * Dh));
    TRY(d_Q.alloc(ctx, (size_t)V * Dh));
    TRY(d_B.alloc(ctx, (size_t)V));
    TRY(d_vrow.alloc(ctx, (size_t)V));
    TRY(d_partial.alloc(ctx, (size_t)C * Dh * ntiles * 256));

    pcl_timer_begin(ctx, "fmllr");                               // the whole call's kernels; "fmllr_frames" / "fmllr_gk": its two halves
    pcl_timer_begin(ctx, "fmllr_frames");
    {
        const unsigned tiles = (unsigned)((b->shape.Tmax + FT - 1) / FT);
#define FRAMES_CASE(DP, NH)                                                                                                                              \
    hipLaunchKernelGGL((fmllr_frames_kernel<DP, NH, false>), dim3(tiles, (unsigned)U, NH), dim3(256), 0, st, b->d_utt, b->d_row_state, d_lists, b->Bt, b->lgam, ctx->frames64, ctx->frames32, \
                       ctx->FD, ctx->params64, ctx->row, ctx->w64, ctx->M, ctx->Mpad, Dh, d_P, d_Q, d_B, d_vrow, MlltKeep<false>{})
        switch (ctx->D) {                                         // (pcl_device_dim of a dimension <= 48)
            case 13: FRAMES_CASE(13, 1); break;
            case 26: FRAMES_CASE(26, 1); break;
            case 39: FRAMES_CASE(39, 2); break;
            case 47: FRAMES_CASE(47, 2); break;
            default: FRAMES_CASE(48, 2); break;
        }
#undef FRAMES_CASE
    }
    hipLaunchKernelGGL(fmllr_beta_kernel, dim3(S), dim3(256), 0, st, d_B, d_lists + U, ctx->fmllr_beta);
    pcl_timer_end(ctx, "fmllr_frames");
    pcl_timer_begin(ctx, "fmllr_gk");
    FrameSrc g{ctx->frames64, ctx->frames32, d_vrow, d_P, d_Q, plan.chunk_v0(), plan.chunk_n(), ctx->FD, Dh};
    launch_gk(mllr_use_valu(), NT, C * Dh, st, g, d_partial);
    hipLaunchKernelGGL(gk_reduce_kernel, dim3(S * Dh), dim3(256), 0, st, d_partial, plan.chunk0(), Dh, NT, ctx->fmllr_Gk, true);
    pcl_timer_end(ctx, "fmllr_gk");
    pcl_timer_end(ctx, "fmllr");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));                        // (the locals above are free to go)
    return PCL_OK;
}

extern "C" int pcl_fmllr_stats_download(pcl_ctx *ctx, double *G, double *k, double *beta) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_fmllr_stats_download";
    if (const char *why = fmllr_ready(ctx)) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: %s", who, why);
    const int S = ctx->fmllr_S, Dh = ctx->Dhost, n = Dh + 1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (G || k) {
        std::vector<double> host((size_t)S * Dh * n * (n + 1));
        HIPCHK(ctx, hipMemcpyAsync(host.data(), ctx->fmllr_Gk, host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t pair = 0; pair < (size_t)S * Dh; ++pair)
            for (int p = 0; p < n; ++p) {
                const double *src = &host[(pair * n + p) * (n + 1)];
                if (G) memcpy(G + (pair * n + p) * n, src, (size_t)n * sizeof(double));
                if (k) k[pair * n + p] = src[n];
            }
    }
    if (beta) {
        HIPCHK(ctx, hipMemcpyAsync(beta, ctx->fmllr_beta, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PCL_OK;
}

extern "C" int pcl_fmllr_estimate(pcl_ctx *ctx, int n_iter, double min_occ, double *W_out, double *logdet_out, double *q_trace_out, int32_t *status_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_fmllr_estimate";
    if (const char *why = fmllr_ready(ctx)) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: %s", who, why);
    if (n_iter < 1 || n_iter > 1000) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: n_iter = %d sweeps, need 1 .. 1000", who, n_iter);
    if (!(min_occ >= 0.0) || !std::isfinite(min_occ)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: min_occ = %g is not a finite number >= 0", who, min_occ);
    const int S = ctx->fmllr_S, Dh = ctx->Dhost, n = Dh + 1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<double> d_L, d_gk, d_W, d_logdet, d_q;
    DevBuf<int> d_status, d_pivot;
    TRY(d_L.alloc(ctx, (size_t)S * Dh * n * n));
    TRY(d_gk.alloc(ctx, (size_t)S * Dh * n));
    TRY(d_W.alloc(ctx, (size_t)S * Dh * n));
    TRY(d_logdet.alloc(ctx, (size_t)S));
    TRY(d_q.alloc(ctx, (size_t)S * n_iter));
    TRY(d_status.alloc(ctx, (size_t)S));
    TRY(d_pivot.alloc(ctx, (size_t)S * Dh));
    pcl_timer_begin(ctx, "fmllr");
    pcl_timer_begin(ctx, "fmllr_solve");
    hipLaunchKernelGGL(fmllr_occ_kernel, dim3((S + 63) / 64), dim3(64), 0, st, ctx->fmllr_beta, S, min_occ, d_status);
    hipLaunchKernelGGL(gk_solve_kernel, dim3(S * Dh), dim3(64), 0, st, ctx->fmllr_Gk, d_status, Dh, d_gk, d_pivot, d_L);
    hipLaunchKernelGGL(fmllr_pivot_kernel, dim3((S + 63) / 64), dim3(64), 0, st, d_pivot, S, Dh, d_status);
    hipLaunchKernelGGL(fmllr_sweep_kernel<false>, dim3(S), dim3(64), 0, st, ctx->fmllr_Gk, d_L, d_gk, ctx->fmllr_beta, Dh, n_iter, d_status, d_W, d_logdet, d_q);
    pcl_timer_end(ctx, "fmllr_solve");
    pcl_timer_end(ctx, "fmllr");
    HIPCHK(ctx, hipGetLastError());
    if (W_out) HIPCHK(ctx, hipMemcpyAsync(W_out, d_W, (size_t)S * Dh * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (logdet_out) HIPCHK(ctx, hipMemcpyAsync(logdet_out, d_logdet, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
    if (q_trace_out) HIPCHK(ctx, hipMemcpyAsync(q_trace_out, d_q, (size_t)S * n_iter * sizeof(double), hipMemcpyDeviceToHost, st));
    if (status_out) HIPCHK(ctx, hipMemcpyAsync(status_out, d_status, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->fmllr_W = std::move(d_W);                               // the resident estimate: goes with the statistics it was made from
    return PCL_OK;
}

extern "C" int pcl_frames_transform(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *utt_speaker, int S, const double *W) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_frames_transform";
    TRY(frames_loaded_check(ctx, who));
    TRY(spans_args_check(ctx, who, U, T, utt_speaker ? frame_begin : nullptr));   // (utt_speaker = NULL is refused as the other two are)
    const int Dh = ctx->FDhost, n = Dh + 1;
    if (Dh > ADAPT_D_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d, the kernel holds at most %d", who, Dh, ADAPT_D_MAX);
    if (S < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: S = %d speakers, need at least 1", who, S);
    if (!W && (!ctx->fmllr_W || ctx->fmllr_S != S || ctx->Dhost != Dh))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: W is NULL and the context holds no estimate of %d speakers in %d dimensions (pcl_fmllr_estimate first)", who, S, Dh);
    int Tmax = 0;
    TRY(speakers_check(ctx, who, U, utt_speaker, S));
    TRY(spans_check(ctx, who, "a frame is transformed ONCE", U, T, frame_begin, &Tmax));
    if (Tmax == 0) return PCL_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevSpans d;
    DevBuf<int> d_skip;
    DevBuf<double> d_W;
    TRY(d.upload(ctx, U, T, frame_begin, utt_speaker));
    TRY(d_skip.alloc(ctx, (size_t)S));
    if (W) {
        TRY(d_W.alloc(ctx, (size_t)S * Dh * n));
        HIPCHK(ctx, pcl_h2d(ctx, d_W, W, (size_t)S * Dh * n * sizeof(double)));
    }
    const double *dW = W ? d_W.p : ctx->fmllr_W.p;
    pcl_timer_begin(ctx, "fmllr");
    hipLaunchKernelGGL(gk_identity_kernel, dim3(S), dim3(64), 0, st, dW, Dh, d_skip);
    hipLaunchKernelGGL(fmllr_apply_kernel, dim3((unsigned)((Tmax + APPLY_TF - 1) / APPLY_TF), (unsigned)U), dim3(256), 0, st, d.T, d.begin, d.spk, dW, d_skip,
                       ctx->frames64.p, ctx->frames32, ctx->FD, Dh);
    pcl_timer_end(ctx, "fmllr");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    return PCL_OK;
}
