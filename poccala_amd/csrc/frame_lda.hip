// LDA (row f12): class statistics of SPLICED frames and the projection of the resident frame matrix to a new width.
//   pcl_lda_zero               the context's class statistics (R, n, n), n = Ds + 1, made and cleared
//   pcl_lda_accumulate         host class labels per frame row -> the statistics
//   pcl_batch_accumulate_lda   the batch's Viterbi owner map (pcl_batch.hip runs the alignment; the map never leaves the device) -> the statistics
//   pcl_lda_stats_download     n_r, s_r, S_r taken apart on the host, S mirrored from the upper triangle
//   pcl_frames_splice_project  y = b + A splice(x) into new buffers that replace the resident frame matrix (another width)
//   pcl_frames_download        the resident frames as held, unpadded
// The rule and every operation order are stated in include/poccala_hip.h; tests/_lda_twin.py is its NumPy twin.  The statistics are one
// product [x | 1][x | 1]^T per class in float64: frame_keyed.h's pass sorts the kept rows by class and cuts a class's rows into
// K-chunks of PCL_LDA_CHUNK rows, one workgroup per (chunk, tile group) forms the chunk's upper-triangular 16 x 16 tiles on
// v_mfma_f64_16x16x4_f64 (or on the VALU under PCL_LDA_VALU=1), and the chunks' partials are added onto the running statistics in chunk
// order.  No floating-point atomics: two runs give the same bits.  Built with -ffp-contract=off: the projection runs one rounded operation at a time.
// Every index a kernel forms is bounded by what the host validated: classes < R, rows < F, a spliced row inside its utterance's
// [lo, hi) within [0, F), operand columns < 16 NT <= 128, output columns < D_out <= the new row stride.
#include <math.h>

#include "pcl_internal.h"

namespace {

#include "frame_spans.h"                      // the checks and the upload of a call's utterances and row labels, the chunk plan
#include "frame_keyed.h"                      // the keys, the counting sort and the chunks of the kept rows

constexpr int LDA_N_MAX = 128;                // order Ds + 1 of the statistics: 8 x 8 tiles of 16
constexpr int KB = 32;                        // K-elements (rows) staged in LDS per step: 8 MFMA k-steps, two per wave
constexpr long long LDA_CHUNK_DEFAULT = 1024; // rows per chunk: 300 chunks x 4 tile groups at 1024 x 300 frames
constexpr int LDA_ROUND = 1024;               // chunks per launch: the partials of a round are 1024 x 36 x 2 KB = 75 MB at order 128
constexpr int PROJ_TF = 16;                   // frames per workgroup of the projection

typedef double d4 __attribute__((ext_vector_type(4)));

// Chunk length in rows, env PCL_LDA_CHUNK, read on EVERY call (as PCL_MLLR_CHUNK is): tests force several chunks on a small input.
long long lda_chunk() { return std::min<long long>(env_positive_ll("PCL_LDA_CHUNK", LDA_CHUNK_DEFAULT), 1 << 30); }
bool lda_use_valu() {                         // env PCL_LDA_VALU=1 (read on every call): the float64 VALU form of the product (A/B, tools/lda_bench.py)
    const char *e = getenv("PCL_LDA_VALU");
    return e && atoi(e) != 0;
}

__device__ __forceinline__ int lda_tile_index(int tp, int tq, int NT) { return tp * NT - tp * (tp - 1) / 2 + (tq - tp); }

// What the product kernels read: the sorted rows, their utterances' spans, the frames, the splice.
struct LdaSrc {
    const double *x64;
    const float *x32;
    const int *order;                         // the kept rows, class by class, each class in ascending row order
    const int2 *span;                         // [row] -> its utterance's rows [lo, hi)
    const int *chunk_v0, *chunk_n;            // chunk c = positions [v0, v0 + n) of order
    int FD, D, left, Ds;
};

// KB rows of chunk positions [v0 + k0, ..) as augmented spliced vectors in LDS: xs[k][p] = column p of [x | 1], 0 for p > Ds and for
// positions beyond the chunk.  The splice: block j = p / D of the vector is row clamp(row + j - left, lo, hi - 1).
template <int P, int S>
__device__ __forceinline__ void lda_stage(const LdaSrc &g, int v0, int n, int k0, double *xs, int *srow, int *slo, int *shi) {
    const int tid = threadIdx.x;
    if (tid < KB) {
        int row = -1, lo = 0, hi = 0;
        if (k0 + tid < n) {
            row = g.order[(size_t)v0 + k0 + tid];
            const int2 sp = g.span[row];
            lo = sp.x;
            hi = sp.y;
        }
        srow[tid] = row;
        slo[tid] = lo;
        shi[tid] = hi;
    }
    __syncthreads();
    for (int e = tid; e < KB * P; e += 256) {
        const int k = e / P, p = e - k * P, row = srow[k];
        double x = 0.0;
        if (row >= 0) {
            if (p < g.Ds) {
                const int j = p / g.D, d = p - j * g.D;
                const int r = min(max(row + j - g.left, slo[k]), shi[k] - 1);
                const size_t at = (size_t)r * g.FD + d;
                x = g.x64 ? g.x64[at] : (double)g.x32[at];
            } else if (p == g.Ds) {
                x = 1.0;
            }
        }
        xs[k * S + p] = x;
    }
    __syncthreads();
}

// The tiles of a workgroup: tile row grp and, from the other end, tile row NT - 1 - grp -- NT + 1 tiles for every group (the middle row of
// an odd NT alone: (NT + 1) / 2), so (NT + 1) / 2 groups share a chunk's NT (NT + 1) / 2 tiles evenly.  Slot s -> (tile row, tile column).
struct LdaGroup {
    int rowA, rowB, nA, nslots;
    __device__ __forceinline__ LdaGroup(int grp, int NT) : rowA(grp), rowB(NT - 1 - grp), nA(NT - grp), nslots(rowA == rowB ? nA : nA + grp + 1) {}
    __device__ __forceinline__ int row(int s) const { return s < nA ? rowA : rowB; }
    __device__ __forceinline__ int col(int s) const { return s < nA ? rowA + s : rowB + (s - nA); }
};

// One workgroup (4 waves) per (chunk, tile group).  Every step stages KB rows' operands in LDS once for the four waves; wave w runs the
// MFMA k-steps w and w + 4 of the step (4 rows each): lane l holds column / row l & 15 of row l >> 4 (the 16x16x4 operand map, one double
// per lane); the outer products exist only in the accumulators, (NT + 1) x 4 doubles per lane.  C/D of the f64 form: col = l & 15,
// row = (l >> 4) + 4 reg.  The waves' sums are added through LDS in wave order, ((w0 + w1) + w2) + w3.
// partial: [chunk - c0][tile][row * 16 + col]
template <int NT>
__global__ __launch_bounds__(256) void lda_mfma_kernel(LdaSrc g, int c0, double *__restrict__ partial) {
    constexpr int P = NT * 16, S = (P % 32 == 0) ? P + 16 : P, NS = NT + 1, NTILES = NT * (NT + 1) / 2;
    __shared__ double xs[KB * S], red[NS * 256];
    __shared__ int srow[KB], slo[KB], shi[KB];
    const int c = c0 + blockIdx.x, v0 = g.chunk_v0[c], n = g.chunk_n[c];
    const LdaGroup grp(blockIdx.y, NT);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, kk = lane >> 4, c16 = lane & 15;
    d4 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += KB) {
        __syncthreads();                                          // (the step before is read)
        lda_stage<P, S>(g, v0, n, k0, xs, srow, slo, shi);
        for (int st = wave; st < KB / 4; st += 4) {               // (uniform in the wave: every lane reaches every MFMA)
            if (k0 + 4 * st >= n) break;                          // only exact zeros from here on
            const double *xk = xs + (4 * st + kk) * S + c16;
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (s < grp.nslots) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xk[16 * grp.row(s)], xk[16 * grp.col(s)], acc[s], 0, 0, 0);
        }
    }
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (s < grp.nslots) {
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int at = s * 256 + reg * 64 + lane;
                        red[at] = w == 0 ? acc[s][reg] : red[at] + acc[s][reg];
                    }
                }
        }
    }
    __syncthreads();
    double *out = partial + (size_t)blockIdx.x * (NTILES * 256);
    for (int e = tid; e < grp.nslots * 256; e += 256) {
        const int s = e >> 8, x = e & 255, reg = x >> 6, ln = x & 63;
        out[lda_tile_index(grp.row(s), grp.col(s), NT) * 256 + ((ln >> 4) + 4 * reg) * 16 + (ln & 15)] = red[e];
    }
}

// The same partials on the float64 VALU (PCL_LDA_VALU=1): thread t owns element (t >> 4, t & 15) of every tile of the group and adds the
// chunk's rows in ascending order.
template <int NT>
__global__ __launch_bounds__(256) void lda_valu_kernel(LdaSrc g, int c0, double *__restrict__ partial) {
    constexpr int P = NT * 16, S = (P % 32 == 0) ? P + 16 : P, NS = NT + 1, NTILES = NT * (NT + 1) / 2;
    __shared__ double xs[KB * S];
    __shared__ int srow[KB], slo[KB], shi[KB];
    const int c = c0 + blockIdx.x, v0 = g.chunk_v0[c], n = g.chunk_n[c];
    const LdaGroup grp(blockIdx.y, NT);
    const int tid = threadIdx.x, r16 = tid >> 4, c16 = tid & 15;
    double sum[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) sum[s] = 0.0;
    for (int k0 = 0; k0 < n; k0 += KB) {
        __syncthreads();
        lda_stage<P, S>(g, v0, n, k0, xs, srow, slo, shi);
        const int kn = min(KB, n - k0);
        for (int k = 0; k < kn; ++k) {
#pragma unroll
            for (int s = 0; s < NS; ++s)
                if (s < grp.nslots) sum[s] += xs[k * S + 16 * grp.row(s) + r16] * xs[k * S + 16 * grp.col(s) + c16];
        }
    }
    double *out = partial + (size_t)blockIdx.x * (NTILES * 256);
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (s < grp.nslots) out[lda_tile_index(grp.row(s), grp.col(s), NT) * 256 + tid] = sum[s];
}

template <int NT>
void launch_lda_nt(bool valu, int chunks, int c0, hipStream_t st, const LdaSrc &g, double *partial) {
    const dim3 grid((unsigned)chunks, (NT + 1) / 2);
    if (valu) hipLaunchKernelGGL((lda_valu_kernel<NT>), grid, dim3(256), 0, st, g, c0, partial);
    else hipLaunchKernelGGL((lda_mfma_kernel<NT>), grid, dim3(256), 0, st, g, c0, partial);
}
void launch_lda(bool valu, int NT, int chunks, int c0, hipStream_t st, const LdaSrc &g, double *partial) {
    switch (NT) {
        case 1: launch_lda_nt<1>(valu, chunks, c0, st, g, partial); break;
        case 2: launch_lda_nt<2>(valu, chunks, c0, st, g, partial); break;
        case 3: launch_lda_nt<3>(valu, chunks, c0, st, g, partial); break;
        case 4: launch_lda_nt<4>(valu, chunks, c0, st, g, partial); break;
        case 5: launch_lda_nt<5>(valu, chunks, c0, st, g, partial); break;
        case 6: launch_lda_nt<6>(valu, chunks, c0, st, g, partial); break;
        case 7: launch_lda_nt<7>(valu, chunks, c0, st, g, partial); break;
        default: launch_lda_nt<8>(valu, chunks, c0, st, g, partial); break;
    }
}

// One workgroup per (class r0 + blockIdx.x, slice of the matrix): the class's chunks inside the round [c0, c1) added in chunk order onto
// the running statistics' upper triangle (a diagonal tile holds both halves, rounded differently: only its upper half is read).
__global__ __launch_bounds__(256) void lda_reduce_kernel(const double *__restrict__ partial, const int *__restrict__ cls_chunk0, int r0, int c0, int c1, int n,
                                                         int NT, double *__restrict__ stats) {
    const int r = r0 + blockIdx.x, ntiles = NT * (NT + 1) / 2;
    const int lo = max(cls_chunk0[r], c0), hi = min(cls_chunk0[r + 1], c1);
    if (lo >= hi) return;
    double *Sr = stats + (size_t)r * n * n;
    for (int x = blockIdx.y * 256 + threadIdx.x; x < n * n; x += gridDim.y * 256) {
        const int p = x / n, q = x - p * n;
        if (p > q) continue;
        const size_t at = (size_t)lda_tile_index(p >> 4, q >> 4, NT) * 256 + (p & 15) * 16 + (q & 15);
        double sum = Sr[x];
        for (int c = lo; c < hi; ++c) sum += partial[(size_t)(c - c0) * ntiles * 256 + at];
        Sr[x] = sum;
    }
}

// y = b + A splice(x) for the frames of utterance u, one workgroup per (16-frame tile, utterance): the tile's spliced vectors are staged in
// LDS, thread (f, i) runs b_i, then the terms in ascending index order, one rounded product and one rounded sum each.  At: A transposed,
// (Ds, D_out), so that neighbouring threads read neighbouring coefficients.
__global__ __launch_bounds__(256) void lda_project_kernel(const int *__restrict__ T, const long long *__restrict__ begin, const double *__restrict__ x64,
                                                          const float *__restrict__ x32, int FD, int D, int left, int Ds, const double *__restrict__ At,
                                                          const double *__restrict__ bias, int Dout, int FDn, double *__restrict__ y64, float *__restrict__ y32) {
    __shared__ double xs[PROJ_TF * (LDA_N_MAX - 1)];
    const int u = blockIdx.y, Tu = T[u], t0 = blockIdx.x * PROJ_TF, tid = threadIdx.x;
    if (t0 >= Tu) return;                                         // (uniform in the workgroup)
    const int nf = min(PROJ_TF, Tu - t0);
    const long long lo = begin[u], hi = lo + Tu;
    for (int e = tid; e < nf * Ds; e += 256) {
        const int f = e / Ds, p = e - f * Ds, j = p / D, d = p - j * D;
        const long long r = min(max(lo + t0 + f + j - left, lo), hi - 1);
        const size_t at = (size_t)r * FD + d;
        xs[e] = x64 ? x64[at] : (double)x32[at];
    }
    __syncthreads();
    for (int e = tid; e < nf * Dout; e += 256) {
        const int f = e / Dout, i = e - f * Dout;
        double y = bias[i];
        for (int p = 0; p < Ds; ++p) y = y + At[(size_t)p * Dout + i] * xs[f * Ds + p];
        const size_t at = (size_t)(lo + t0 + f) * FDn + i;
        if (y64) y64[at] = y;
        y32[at] = (float)y;
    }
}

// T / frame_begin of a call: inside the frame matrix, disjoint (a row has ONE utterance: its splice clamps are the utterance's)
int lda_check_ranges(pcl_ctx *ctx, const char *who, int U, const int32_t *T, const int64_t *frame_begin, int *Tmax_out) {
    TRY(spans_args_check(ctx, who, U, T, frame_begin));           // (before the frames: the order of the LDA launcher's row in pcl_internal.h's table)
    TRY(frames_loaded_check(ctx, who));
    if (ctx->F > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: frame matrix of %lld rows", who, (long long)ctx->F);
    return spans_check(ctx, who, "a frame is spliced inside ONE utterance", U, T, frame_begin, Tmax_out);
}

}  // namespace

extern "C" int pcl_lda_zero(pcl_ctx *ctx, int R, int left, int right) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_lda_zero";
    if (!ctx->frames32 || ctx->F <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no frames loaded (the statistics' order comes from the frame matrix's dimension)", who);
    if (left < 0 || right < 0 || left > LDA_N_MAX || right > LDA_N_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: context (%d, %d), need 0 <= left, right", who, left, right);
    const int D = ctx->FDhost;
    const long long Ds = (long long)(left + right + 1) * D;
    if (Ds + 1 > LDA_N_MAX)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: spliced dimension %lld = (%d + %d + 1) x %d: the statistics hold an order Ds + 1 of at most %d", who, Ds, left, right, D, LDA_N_MAX);
    const unsigned long long per = 8ull * (Ds + 1) * (Ds + 1);
    if (R < 1 || R > 65535 || (unsigned long long)R * per > (1ull << 32))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: R = %d classes, need 1 .. min(65535, 2^32 / %llu bytes per class = %llu)", who, R, per, (1ull << 32) / per);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t len = (size_t)R * (Ds + 1) * (Ds + 1);
    LdaStats fresh{{}, R, left, right, D};                        // the statistics in place stay until the new set is there and cleared
    TRY(fresh.stats.alloc(ctx, len));
    HIPCHK(ctx, hipMemsetAsync(fresh.stats, 0, len * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->lda = std::move(fresh);
    return PCL_OK;
}

// Both accumulate entries behind their checks: d_src (F entries on the device) holds per row a class in [-1, R), or (state_class given,
// J entries on the host, validated here) an owner state in [-1, J).  Rows outside the U utterances are not kept.
int pcl_launch_lda_accumulate(pcl_ctx *ctx, const char *who, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *d_src,
                              const int32_t *state_class, int J) {
    const LdaStats &lda = ctx->lda;
    TRY(stats_fits(ctx, who, lda));
    const int R = lda.R, n = lda.n();
    int Tmax = 0;
    TRY(lda_check_ranges(ctx, who, U, T, frame_begin, &Tmax));
    if (state_class)
        for (int j = 0; j < J; ++j)
            if (state_class[j] < -1 || state_class[j] >= R) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: state %d has class %d, outside [-1, %d)", who, j, (int)state_class[j], R);
    if (Tmax == 0) return PCL_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<int> d_sc;
    KeyedRows rows;
    DevBuf<double> d_partial;
    if (state_class) {
        TRY(d_sc.alloc(ctx, (size_t)J));
        HIPCHK(ctx, pcl_h2d(ctx, d_sc, state_class, (size_t)J * sizeof(int32_t)));
    }
    TRY(rows.build<true>(ctx, "lda_sort", U, T, frame_begin, Tmax, d_src, d_sc.p, R, lda_chunk()));
    const int C = rows.C;
    if (C == 0) return PCL_OK;
    const std::vector<int> &cls_chunk0 = rows.group_chunk0;
    const int NT = (n + 15) / 16, ntiles = NT * (NT + 1) / 2;
    TRY(d_partial.alloc(ctx, (size_t)std::min(C, LDA_ROUND) * ntiles * 256));
    pcl_timer_begin(ctx, "lda_stats");                           // pcl_kernel_time groups: "lda_sort" (keys and counting sort), "lda_stats" (product and reduction)
    const LdaSrc g{ctx->frames64, ctx->frames32, rows.d_order, rows.d_span, rows.chunk_v0(), rows.chunk_n(), ctx->FD, lda.D, lda.left, lda.Ds()};
    const bool valu = lda_use_valu();
    int r_lo = 0;
    for (int c0 = 0; c0 < C; c0 += LDA_ROUND) {                   // (the rounds add in the same chunk order as one launch would)
        const int c1 = std::min(C, c0 + LDA_ROUND);
        while (cls_chunk0[r_lo + 1] <= c0) ++r_lo;                // the first and the last class with a chunk in the round
        int r_hi = r_lo;
        while (r_hi + 1 < R && cls_chunk0[r_hi + 1] < c1) ++r_hi;
        launch_lda(valu, NT, c1 - c0, c0, st, g, d_partial);
        hipLaunchKernelGGL(lda_reduce_kernel, dim3((unsigned)(r_hi - r_lo + 1), (unsigned)std::min(8, (n * n + 255) / 256)), dim3(256), 0, st, d_partial,
                           rows.chunk0(), r_lo, c0, c1, n, NT, lda.stats.p);
    }
    pcl_timer_end(ctx, "lda_stats");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));                        // (the locals above are free to go)
    return PCL_OK;
}

extern "C" int pcl_lda_accumulate(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *frame_class) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_lda_accumulate";
    TRY(stats_have(ctx, who, ctx->lda));
    DevBuf<int32_t> d_cls;
    TRY(upload_row_labels(ctx, who, "frame_class", "class", frame_class, ctx->lda.R, &d_cls));
    return pcl_launch_lda_accumulate(ctx, who, U, T, frame_begin, d_cls, nullptr, 0);
}

extern "C" int pcl_lda_stats_download(pcl_ctx *ctx, double *n_out, double *s_out, double *S_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_lda_stats_download";
    TRY(stats_have(ctx, who, ctx->lda));
    const int R = ctx->lda.R, Ds = ctx->lda.Ds(), n = ctx->lda.n();
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> host((size_t)R * n * n);
    HIPCHK(ctx, hipMemcpyAsync(host.data(), ctx->lda.stats, host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < R; ++r) {
        const double *src = &host[(size_t)r * n * n];
        if (n_out) n_out[r] = src[(size_t)Ds * n + Ds];
        for (int p = 0; p < Ds; ++p) {
            if (s_out) s_out[(size_t)r * Ds + p] = src[(size_t)p * n + Ds];
            if (S_out)
                for (int q = 0; q < Ds; ++q) S_out[((size_t)r * Ds + p) * Ds + q] = p <= q ? src[(size_t)p * n + q] : src[(size_t)q * n + p];
        }
    }
    return PCL_OK;
}

extern "C" int pcl_frames_splice_project(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, int left, int right, int D_out, const double *A,
                                         const double *b) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_frames_splice_project";
    int Tmax = 0;
    TRY(lda_check_ranges(ctx, who, U, T, frame_begin, &Tmax));
    if (!A || !b) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: A or b is NULL", who);
    if (left < 0 || right < 0 || left > LDA_N_MAX || right > LDA_N_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: context (%d, %d), need 0 <= left, right", who, left, right);
    const int D = ctx->FDhost;
    const long long Dsl = (long long)(left + right + 1) * D;
    if (Dsl + 1 > LDA_N_MAX)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: spliced dimension %lld = (%d + %d + 1) x %d: at most %d", who, Dsl, left, right, D, LDA_N_MAX - 1);
    const int Ds = (int)Dsl;
    if (D_out < 1 || D_out > Ds) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: D_out = %d output dimensions, need 1 .. the spliced dimension %d", who, D_out, Ds);
    const int FDn = pcl_device_dim(D_out);
    if (FDn < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: D_out = %d > 64 is not a frame dimension the kernels hold", who, D_out);
    for (size_t x = 0; x < (size_t)D_out * Ds; ++x)
        if (!std::isfinite(A[x])) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: A[%zu] is not finite", who, x);
    for (int i = 0; i < D_out; ++i)
        if (!std::isfinite(b[i])) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: b[%d] is not finite", who, i);
    if (ctx->live_batches > 0 || ctx->live_segs > 0)
        PCL_FAIL(ctx, PCL_ERR_STATE, "%s: %d batches and %d pcl_seg objects made on the current frame matrix are alive: destroy them first (the matrix changes its width, not its rows)",
                 who, ctx->live_batches, ctx->live_segs);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)ctx->F * FDn;
    std::vector<double> At((size_t)Ds * D_out);
    for (int i = 0; i < D_out; ++i)
        for (int p = 0; p < Ds; ++p) At[(size_t)p * D_out + i] = A[(size_t)i * Ds + p];
    DevBuf<float> n32;
    DevBuf<double> n64, d_At, d_b;
    DevSpans d;
    TRY(n32.alloc(ctx, nn));
    if (ctx->frames64) TRY(n64.alloc(ctx, nn));
    TRY(d_At.alloc(ctx, At.size()));
    TRY(d_b.alloc(ctx, (size_t)D_out));
    HIPCHK(ctx, pcl_h2d(ctx, d_At, At.data(), At.size() * sizeof(double)));
    HIPCHK(ctx, pcl_h2d(ctx, d_b, b, (size_t)D_out * sizeof(double)));
    TRY(d.upload(ctx, U, T, frame_begin, nullptr));
    pcl_timer_begin(ctx, "lda_project");
    HIPCHK(ctx, hipMemsetAsync(n32, 0, nn * sizeof(float), st));  // rows of no utterance and the padding columns: zero
    if (n64) HIPCHK(ctx, hipMemsetAsync(n64, 0, nn * sizeof(double), st));
    if (Tmax > 0)
        hipLaunchKernelGGL(lda_project_kernel, dim3((unsigned)((Tmax + PROJ_TF - 1) / PROJ_TF), (unsigned)U), dim3(256), 0, st, d.T, d.begin, ctx->frames64.p,
                           ctx->frames32, ctx->FD, D, left, Ds, d_At, d_b, D_out, FDn, n64.p, n32.p);
    pcl_timer_end(ctx, "lda_project");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    pcl_frames_adopt(ctx, std::move(n32), std::move(n64), ctx->F, D_out);
    return PCL_OK;
}

extern "C" int pcl_frames_download(pcl_ctx *ctx, double *f64, float *f32) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_frames_download";
    if (!ctx->frames32 || ctx->F <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no frames loaded", who);
    if (f64 && !ctx->frames64) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the context holds no float64 copy of the frames (uploaded as float32)", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t D = (size_t)ctx->FDhost, FD = (size_t)ctx->FD, F = (size_t)ctx->F;
    if (f64)
        HIPCHK(ctx, hipMemcpy2DAsync(f64, D * sizeof(double), ctx->frames64, FD * sizeof(double), D * sizeof(double), F, hipMemcpyDeviceToHost, ctx->stream));
    if (f32)
        HIPCHK(ctx, hipMemcpy2DAsync(f32, D * sizeof(float), ctx->frames32, FD * sizeof(float), D * sizeof(float), F, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}
