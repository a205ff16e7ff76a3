// Phonetic decision tree (row f16): per-context single-Gaussian statistics from an alignment, top-down greedy clustering over phonetic
// questions, the tied-state map, and a one-Gaussian-per-leaf seed model written where the model lives.
//   pcl_tree_zero               the context's statistics n (R) int64, s (R, D), q (R, D) made and cleared: ONE pool block of 8 R (2 D + 1) bytes
//   pcl_tree_accumulate         a host map frame row -> statistics row -> the statistics
//   pcl_batch_accumulate_tree   the batch's Viterbi owner map and the caller's label position -> event list (pcl_batch.hip runs the alignment;
//                               the map never leaves the device) -> the statistics
//   pcl_tree_stats_shape / pcl_tree_stats_download / pcl_tree_stats_upload
//   pcl_tree_build              greedy growth; optionally the (J_t, 1, D) model
// The rule and every summation order are stated in include/poccala_hip.h; tests/_tree_twin.py is its NumPy twin.  Everything is float64;
// no floating-point atomics: two runs give the same bits.  Built with -ffp-contract=off: every kernel runs one rounded operation at a time.
// STATISTICS: frame_keyed.h's pass sorts the kept frame rows by statistics row and cuts a row's frames into chunks of PCL_TREE_CHUNK,
// a group of 64 / G lanes adds a chunk's frames in ascending order from 0 (G columns a lane, one 16-byte load a frame), and the chunks'
// partials are added onto the resident sums in chunk order.
// BUILD: the rows of a leaf are a segment of ONE device list, ascending; an evaluation workgroup owns (leaf, 8 candidates) and walks the
// segment once, lane j adding column j of [s | q] onto the yes- or the no-sum of each of its candidates under the event's answer bit --
// the masked product of the issue in its VALU form: adding +0.0 leaves a sum's bits, so a side's sum IS the sum of its rows in ascending
// order from +0.0, whichever candidate asks.  The gains, the arg-max inside the workgroup and across a leaf's workgroups run on the
// device; the host picks the leaf (a loop over the current leaves' bests), partitions its segment -- the answers are the caller's tables,
// the host has them -- and sends the segment back in place.
// Every index a kernel forms is bounded by what the host validated: statistics rows < R, frame rows < F (a 16-byte load that would end
// beyond the matrix is taken element by element), columns < D <= 64, events < E, answer bytes < E NCB, nodes < the capacity the build
// allocated, segments inside [0, R).
#include <math.h>

#include "pcl_internal.h"

namespace {

#include "frame_spans.h"                      // the checks and the upload of a call's utterances and row labels, the chunk plan
#include "frame_keyed.h"                      // the keys, the counting sort and the chunks of the kept rows

constexpr long long TREE_CHUNK_DEFAULT = 256; // frames per chunk of a statistics row
constexpr int CG = 8;                         // candidates per evaluation workgroup: one answer byte per (event, group)
constexpr int EVAL_T = 128;                   // its lanes: the columns of [s | q], 2 D <= 128
constexpr int NSUM = 2 * CG + 1;              // its sums: yes[CG], no[CG], the leaf
constexpr int TREE_Q_MAX = 4096;              // candidates 3 Q
constexpr double ONE_PLUS_LN_2PI = 2.8378770664093453;   // 1 + ln 2 pi, the double the rule names

// Chunk length in frames, env PCL_TREE_CHUNK, read on EVERY call (as PCL_MLLR_CHUNK is): tests force several chunks on a small input.
long long tree_chunk() { return std::min<long long>(env_positive_ll("PCL_TREE_CHUNK", TREE_CHUNK_DEFAULT), 1 << 30); }

// Source (b): frame_state = the owner map of pcl_batch_align_segments (unit * P + slice, -1: not kept, a dropped utterance).  The label
// position of a frame is the one its path row belongs to (hmm_align_segments_kernel's row -> position map), its slice the owner map's.
// frame_row was set to -1 everywhere before.
__global__ __launch_bounds__(256) void tree_label_rows_kernel(const UttDesc *__restrict__ utts, const int32_t *__restrict__ path, const int *__restrict__ label_off,
                                                              const int32_t *__restrict__ label_event, int P, const int32_t *__restrict__ frame_state,
                                                              int32_t *__restrict__ frame_row) {
    const UttDesc d = utts[blockIdx.y];
    const int lo = label_off[blockIdx.y], L = label_off[blockIdx.y + 1] - lo;
    if (L <= 0) return;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < d.T; t += gridDim.x * 256) {
        const int fs = frame_state[d.frame0 + t];
        if (fs < 0) continue;
        const int row = path[d.path_off + t];
        const int p = row <= 0 ? 0 : min((row - 1) / P, L - 1);
        const int ev = label_event[lo + p];
        if (ev >= 0) frame_row[d.frame0 + t] = ev * P + fs % P;
    }
}

// 256 / LPC chunks per workgroup, LPC = 64 / G lanes each: lane g owns the columns [G g, G g + G) and adds the chunk's frames in ascending
// order, x and x x (rounded, then added), from 0.  A frame's G columns are ONE 16-byte load (G = 4 float32 widened, G = 2 of the float64
// copy); columns beyond D are loaded and dropped.  partial[c][0][d] = the sum of x, [c][1][d] of x^2.
template <typename X, int G>
__global__ __launch_bounds__(256) void tree_partial_kernel(const X *__restrict__ x, long long n_elems, int FD, int Dh, const int *__restrict__ order,
                                                           const int *__restrict__ chunk_v0, const int *__restrict__ chunk_n, int C,
                                                           double *__restrict__ partial) {
    static_assert(G * sizeof(X) == 16, "one 16-byte load per frame and lane");
    constexpr int LPC = 64 / G;
    const int c = blockIdx.x * (256 / LPC) + threadIdx.x / LPC, d0 = (threadIdx.x % LPC) * G;
    if (c >= C || d0 >= Dh) return;
    const int v0 = chunk_v0[c], n = chunk_n[c];
    double s[G], q[G];
#pragma unroll
    for (int e = 0; e < G; ++e) s[e] = q[e] = 0.0;
    for (int k = 0; k < n; ++k) {
        const long long at = (long long)order[(size_t)v0 + k] * FD + d0;
        X v[G];
        if (at + G <= n_elems) {
            __builtin_memcpy(v, x + at, 16);                      // (a row of an odd width starts anywhere: no alignment is claimed)
        } else {
#pragma unroll
            for (int e = 0; e < G; ++e) v[e] = at + e < n_elems ? x[at + e] : (X)0;
        }
#pragma unroll
        for (int e = 0; e < G; ++e) {
            const double xd = (double)v[e];
            s[e] = s[e] + xd;
            q[e] = q[e] + xd * xd;
        }
    }
    double *p = partial + (size_t)c * 2 * Dh;
#pragma unroll
    for (int e = 0; e < G; ++e)
        if (d0 + e < Dh) {
            p[d0 + e] = s[e];
            p[Dh + d0 + e] = q[e];
        }
}

// One thread per (statistics row, column of [s | q | n]): the row's chunks of this call added in chunk order onto the resident value.
__global__ __launch_bounds__(256) void tree_reduce_kernel(const double *__restrict__ partial, const int *__restrict__ row_chunk0, const int *__restrict__ chunk_n,
                                                          int R, int Dh, long long *__restrict__ n_res, double *__restrict__ s_res,
                                                          double *__restrict__ q_res) {
    const int W = 2 * Dh + 1;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)R * W) return;
    const int r = (int)(idx / W), x = (int)(idx - (long long)r * W);
    const int lo = row_chunk0[r], hi = row_chunk0[r + 1];
    if (lo >= hi) return;
    if (x == 2 * Dh) {
        long long n = n_res[r];
        for (int c = lo; c < hi; ++c) n += chunk_n[c];
        n_res[r] = n;
        return;
    }
    double *dst = (x < Dh ? s_res + x : q_res + (x - Dh)) + (size_t)r * Dh;
    double sum = *dst;
    for (int c = lo; c < hi; ++c) sum = sum + partial[(size_t)c * 2 * Dh + x];
    *dst = sum;
}

// ---------------------------------------------------------------- build
struct EvalLeaf {
    int lo, hi;                               // the leaf's rows: rows[lo, hi), ascending
    int node, pad;
};
struct EvalBest {
    double gain;
    long long n_yes, n_no;
    int cand, pad;                            // -1: no valid candidate
};

// The log-likelihood of a pooled set: L = -0.5 n (D (1 + ln 2 pi) + sum_d ln v_d), d ascending; 0 for n = 0.  sq = [s | q], stride 1.
__device__ __forceinline__ double tree_loglike(long long n, const double *sq, int Dh, double var_floor) {
    if (n <= 0) return 0.0;
    const double nn = (double)n;
    double acc = 0.0;
    for (int d = 0; d < Dh; ++d) {
        const double m = sq[d] / nn;
        const double t = sq[Dh + d] / nn - m * m;
        acc = acc + log(t > var_floor ? t : var_floor);
    }
    return -0.5 * nn * ((double)Dh * ONE_PLUS_LN_2PI + acc);
}

// One workgroup per (leaf, group of CG candidates).  Lane j < 2 D owns column j of [s | q]; the rows of the leaf are walked once in
// ascending order, the row's answer byte (one bit per candidate of the group) steering x onto the yes- or the no-sum; every lane keeps the
// counts (the byte and n are uniform).  Then lane i < NSUM forms the likelihood of sum i, and lane 0 the gains and the group's best: the
// largest valid gain, the lowest candidate among equals.  Group 0 also leaves the leaf's own sums at its node.
__global__ __launch_bounds__(EVAL_T) void tree_eval_kernel(const EvalLeaf *__restrict__ leaves, const int *__restrict__ rows, const long long *__restrict__ n_res,
                                                           const double *__restrict__ s_res, const double *__restrict__ q_res, int Dh, int P,
                                                           const unsigned char *__restrict__ ansb, int NCB, int NC, long long min_count, double min_gain,
                                                           double var_floor, EvalBest *__restrict__ gbest, long long *__restrict__ node_n,
                                                           double *__restrict__ node_sq) {
    __shared__ double sums[NSUM][EVAL_T];
    __shared__ double like[NSUM];
    __shared__ long long cnt[NSUM];
    const EvalLeaf leaf = leaves[blockIdx.x];
    const int cg = blockIdx.y, j = threadIdx.x, W = 2 * Dh;
    const bool col = j < W;
    const double *src = j < Dh ? s_res + j : q_res + (col ? j - Dh : 0);
    double yes[CG], no[CG], tot = 0.0;
    long long cy[CG], nt = 0;
#pragma unroll
    for (int i = 0; i < CG; ++i) {
        yes[i] = no[i] = 0.0;
        cy[i] = 0;
    }
    for (int k = leaf.lo; k < leaf.hi; ++k) {
        const int row = rows[k];
        const unsigned bits = ansb[(size_t)(row / P) * NCB + cg];
        const long long nr = n_res[row];
        const double x = col ? src[(size_t)row * Dh] : 0.0;
        tot = tot + x;
        nt += nr;
#pragma unroll
        for (int i = 0; i < CG; ++i) {
            const bool on = (bits >> i) & 1u;
            yes[i] = yes[i] + (on ? x : 0.0);
            no[i] = no[i] + (on ? 0.0 : x);
            cy[i] += on ? nr : 0;
        }
    }
#pragma unroll
    for (int i = 0; i < CG; ++i) {
        sums[i][j] = yes[i];
        sums[CG + i][j] = no[i];
    }
    sums[2 * CG][j] = tot;
    if (j == 0) {
#pragma unroll
        for (int i = 0; i < CG; ++i) {
            cnt[i] = cy[i];
            cnt[CG + i] = nt - cy[i];
        }
        cnt[2 * CG] = nt;
    }
    if (cg == 0) {
        if (col) node_sq[(size_t)leaf.node * W + j] = tot;
        if (j == 0) node_n[leaf.node] = nt;
    }
    __syncthreads();
    if (j < NSUM) like[j] = tree_loglike(cnt[j], sums[j], Dh, var_floor);   // (sums[j] holds [s | q] in its first 2 D entries)
    __syncthreads();
    if (j == 0) {
        EvalBest b{0.0, 0, 0, -1, 0};
        const double l_leaf = like[2 * CG];
        for (int i = 0; i < CG; ++i) {
            const int c = cg * CG + i;
            if (c >= NC) break;
            const double gain = (like[i] + like[CG + i]) - l_leaf;
            const bool valid = cnt[i] >= min_count && cnt[CG + i] >= min_count && gain >= min_gain;
            if (valid && (b.cand < 0 || gain > b.gain)) b = EvalBest{gain, cnt[i], cnt[CG + i], c, 0};
        }
        gbest[(size_t)blockIdx.x * NCB + cg] = b;
    }
}

// One thread per leaf: its groups' bests in ascending group order, a later one only when its gain is larger
__global__ __launch_bounds__(64) void tree_best_kernel(const EvalBest *__restrict__ gbest, int NL, int NCB, EvalBest *__restrict__ best) {
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= NL) return;
    EvalBest b{0.0, 0, 0, -1, 0};
    for (int g = 0; g < NCB; ++g) {
        const EvalBest x = gbest[(size_t)l * NCB + g];
        if (x.cand >= 0 && (b.cand < 0 || x.gain > b.gain)) b = x;
    }
    best[l] = b;
}

// The (J_t, 1, D) model into the float64 master copy: mean = s / n, var = max(q / n - m m, var_floor), weight 1; padding mixtures and
// features mean 0, variance 1, weight 0, as pcl_model_upload leaves them.  One thread per element of a state's (Mpad, Dd) block.
__global__ __launch_bounds__(256) void tree_install_kernel(const int *__restrict__ leaf_node, const long long *__restrict__ node_n, const double *__restrict__ node_sq,
                                                           int Jt, int Mpad, int Dd, int Dh, double var_floor, double *__restrict__ mean64,
                                                           double *__restrict__ var64, double *__restrict__ w64) {
    const int jt = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x;
    if (e >= Mpad * Dd) return;
    const int m = e / Dd, d = e - m * Dd, node = leaf_node[jt];
    double mu = 0.0, vr = 1.0;
    if (m == 0 && d < Dh) {
        const double nn = (double)node_n[node];
        const double *sq = node_sq + (size_t)node * 2 * Dh;
        mu = sq[d] / nn;
        const double t = sq[Dh + d] / nn - mu * mu;
        vr = t > var_floor ? t : var_floor;
    }
    mean64[(size_t)jt * Mpad * Dd + e] = mu;
    var64[(size_t)jt * Mpad * Dd + e] = vr;
    if (d == 0) w64[(size_t)jt * Mpad + m] = m == 0 ? 1.0 : 0.0;
}

}  // namespace

// What both accumulate entries need of the context, in the order the header states: statistics, frames, their width
int pcl_tree_accumulate_ready(pcl_ctx *ctx, const char *who) {
    TRY(stats_have(ctx, who, ctx->tree));
    TRY(frames_loaded_check(ctx, who));
    TRY(stats_fits(ctx, who, ctx->tree));
    if (ctx->F > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: frame matrix of %lld rows", who, (long long)ctx->F);
    return PCL_OK;
}

int pcl_launch_tree_label_rows(pcl_ctx *ctx, pcl_batch *b, const int32_t *d_label_event, int P, const int32_t *d_frame_state, int32_t *d_frame_row) {
    if (b->shape.Tmax <= 0) return PCL_OK;
    hipLaunchKernelGGL(tree_label_rows_kernel, dim3((unsigned)std::min(64, (b->shape.Tmax + 255) / 256), (unsigned)b->U), dim3(256), 0, ctx->stream, b->d_utt.p,
                       b->path.p, b->d_label_off.p, d_label_event, P, d_frame_state, d_frame_row);
    HIPCHK(ctx, hipGetLastError());
    return PCL_OK;
}

// Both accumulate entries behind their checks: d_src (F entries on the device) holds per frame row a statistics row in [-1, R).  Rows outside
// the U utterances are not kept.  The utterances are checked HERE, once for either entry, before anything is queued.  Waits for its kernels.
int pcl_launch_tree_accumulate(pcl_ctx *ctx, const char *who, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *d_src) {
    int Tmax = 0;
    TRY(spans_check(ctx, who, "a frame is counted ONCE", U, T, frame_begin, &Tmax));
    if (Tmax == 0) return PCL_OK;
    const TreeStats &tree = ctx->tree;
    const int R = tree.R, Dh = tree.D;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    KeyedRows rows;
    DevBuf<double> d_partial;
    TRY(rows.build<false>(ctx, "tree_sort", U, T, frame_begin, Tmax, d_src, nullptr, R, tree_chunk()));
    const int C = rows.C;
    if (C == 0) return PCL_OK;
    TRY(d_partial.alloc(ctx, (size_t)C * 2 * Dh));
    pcl_timer_begin(ctx, "tree_stats");                          // pcl_kernel_time groups: "tree_sort" (keys and counting sort), "tree_stats" (partials and reduction)
    const long long n_elems = ctx->F * ctx->FD;
    if (ctx->frames64)
        hipLaunchKernelGGL((tree_partial_kernel<double, 2>), dim3((unsigned)((C + 7) / 8)), dim3(256), 0, st, (const double *)ctx->frames64.p, n_elems, ctx->FD, Dh,
                           rows.d_order.p, rows.chunk_v0(), rows.chunk_n(), C, d_partial.p);
    else
        hipLaunchKernelGGL((tree_partial_kernel<float, 4>), dim3((unsigned)((C + 15) / 16)), dim3(256), 0, st, (const float *)ctx->frames32, n_elems, ctx->FD, Dh,
                           rows.d_order.p, rows.chunk_v0(), rows.chunk_n(), C, d_partial.p);
    const long long cells = (long long)R * (2 * Dh + 1);
    hipLaunchKernelGGL(tree_reduce_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, d_partial.p, rows.chunk0(), rows.chunk_n(), R, Dh, tree.n(),
                       tree.s(), tree.q());
    pcl_timer_end(ctx, "tree_stats");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));                        // (the locals above are free to go)
    return PCL_OK;
}

extern "C" int pcl_tree_zero(pcl_ctx *ctx, int R) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_tree_zero";
    if (!ctx->frames32 || ctx->F <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no frames loaded (the statistics are taken at the frame matrix's dimension)", who);
    const int D = ctx->FDhost;
    const unsigned long long per = 8ull * (2 * D + 1);
    if (R < 1 || (unsigned long long)R * per > (1ull << 32))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: R = %d rows, need 1 .. 2^32 / %llu bytes per row = %llu", who, R, per, (1ull << 32) / per);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t len = (size_t)R * (2 * D + 1);
    TreeStats fresh{{}, R, D};                                    // the statistics in place stay until the new set is there and cleared
    TRY(fresh.stats.alloc(ctx, len));
    HIPCHK(ctx, hipMemsetAsync(fresh.stats, 0, len * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->tree = std::move(fresh);
    return PCL_OK;
}

extern "C" int pcl_tree_accumulate(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *frame_row) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_tree_accumulate";
    TRY(pcl_tree_accumulate_ready(ctx, who));
    DevBuf<int32_t> d_row;                                        // (the utterances are checked by the launcher, before anything resident is touched)
    TRY(upload_row_labels(ctx, who, "frame_row", "row", frame_row, ctx->tree.R, &d_row));
    return pcl_launch_tree_accumulate(ctx, who, U, T, frame_begin, d_row);
}

extern "C" int pcl_tree_stats_shape(pcl_ctx *ctx, int32_t *R, int32_t *D) {
    if (!ctx) return PCL_ERR_INVALID;
    if (R) *R = ctx->tree.R;                                      // (0, 0 without statistics: a set is made and dropped as a whole)
    if (D) *D = ctx->tree.D;
    return PCL_OK;
}

extern "C" int pcl_tree_stats_download(pcl_ctx *ctx, int64_t *n, double *s, double *q) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_tree_stats_download";
    TRY(stats_have(ctx, who, ctx->tree));
    static_assert(sizeof(long long) == sizeof(int64_t), "n travels as it is held");
    const size_t R = (size_t)ctx->tree.R, RD = R * ctx->tree.D;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n) HIPCHK(ctx, hipMemcpyAsync(n, ctx->tree.n(), R * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (s) HIPCHK(ctx, hipMemcpyAsync(s, ctx->tree.s(), RD * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (q) HIPCHK(ctx, hipMemcpyAsync(q, ctx->tree.q(), RD * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

extern "C" int pcl_tree_stats_upload(pcl_ctx *ctx, const int64_t *n, const double *s, const double *q) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_tree_stats_upload";
    TRY(stats_have(ctx, who, ctx->tree));
    if (!n || !s || !q) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: n, s or q is NULL", who);
    const size_t R = (size_t)ctx->tree.R, RD = R * ctx->tree.D;
    for (size_t r = 0; r < R; ++r)
        if (n[r] < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: n[%zu] = %lld is negative", who, r, (long long)n[r]);
    for (size_t x = 0; x < RD; ++x)
        if (!std::isfinite(s[x]) || !std::isfinite(q[x])) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: s[%zu] = %g, q[%zu] = %g: not finite", who, x, s[x], x, q[x]);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, pcl_h2d(ctx, ctx->tree.n(), n, R * sizeof(int64_t)));
    HIPCHK(ctx, pcl_h2d(ctx, ctx->tree.s(), s, RD * sizeof(double)));
    HIPCHK(ctx, pcl_h2d(ctx, ctx->tree.q(), q, RD * sizeof(double)));
    return PCL_OK;
}

extern "C" int pcl_tree_build(pcl_ctx *ctx, int E, int P, const int32_t *event_ctx, int n_units, int Q, const uint8_t *q_member, int R0, const int32_t *root_of,
                              int64_t min_count, double min_gain, int max_leaves, double var_floor, int install, int flags, int32_t *node_cand,
                              int32_t *node_child, int32_t *node_state, int64_t *node_n, double *split_gain, int32_t *row_state, int64_t *leaf_n,
                              double *leaf_s, double *leaf_q, int32_t *n_nodes_out, int32_t *n_states_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_tree_build";
    TRY(stats_have(ctx, who, ctx->tree));
    const int R = ctx->tree.R, Dh = ctx->tree.D;
    if (E < 1 || P < 1 || (long long)E * P != R) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: E = %d events x P = %d positions, the statistics hold %d rows", who, E, P, R);
    if (n_units < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: n_units = %d", who, n_units);
    if (Q < 1 || 3 * (long long)Q > TREE_Q_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: Q = %d questions, need 1 <= Q and 3 Q <= %d", who, Q, TREE_Q_MAX);
    if (!event_ctx || !q_member || !root_of) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: event_ctx, q_member or root_of is NULL", who);
    for (int e = 0; e < E; ++e) {
        const int32_t *c = event_ctx + 3 * (size_t)e;
        if (c[0] < 0 || c[0] > n_units || c[1] < 0 || c[1] >= n_units || c[2] < 0 || c[2] > n_units)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: event %d = (%d, %d, %d): a neighbour is a unit or the edge symbol %d, the centre a unit in [0, %d)", who, e, (int)c[0],
                     (int)c[1], (int)c[2], n_units, n_units);
    }
    if (R0 < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: R0 = %d roots", who, R0);
    {
        std::vector<char> used((size_t)R0, 0);
        for (size_t x = 0; x < (size_t)n_units * P; ++x) {
            if (root_of[x] < 0 || root_of[x] >= R0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: root_of[%zu] = %d is outside [0, %d)", who, x, (int)root_of[x], R0);
            used[root_of[x]] = 1;
        }
        for (int i = 0; i < R0; ++i)
            if (!used[i]) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: no (centre, position) maps to root %d", who, i);
    }
    if (max_leaves < R0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: max_leaves = %d is below the %d roots", who, max_leaves, R0);
    if (!std::isfinite(min_gain) || min_gain < 0.0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: min_gain = %g is not a finite number >= 0", who, min_gain);
    if (!(var_floor > 0.0) || !std::isfinite(var_floor)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: var_floor = %g is not a finite number > 0", who, var_floor);
    if (min_count < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: min_count = %lld, need at least 1", who, (long long)min_count);
    if (install && ctx->frames32 && ctx->F > 0 && ctx->FDhost != Dh)
        PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the statistics were made for %d-dimensional frames; the frame matrix in place has %d: the model would not fit it", who, Dh,
                 ctx->FDhost);
    // a split leaves a row on either side (min_count >= 1): never more leaves than rows
    const int ML = std::min(max_leaves, std::max(R0, R)), Ncap = R0 + 2 * (ML - R0), NC = 3 * Q, NCB = (NC + CG - 1) / CG, W = 2 * Dh;
    // the answers: per (event, group of CG candidates) a byte, candidate c = pos Q + qi at bit c % CG
    std::vector<unsigned char> ansb((size_t)E * NCB, 0);
    for (int e = 0; e < E; ++e)
        for (int pos = 0; pos < 3; ++pos) {
            const int unit = event_ctx[3 * (size_t)e + pos];
            for (int qi = 0; qi < Q; ++qi)
                if (q_member[(size_t)qi * (n_units + 1) + unit]) {
                    const int c = pos * Q + qi;
                    ansb[(size_t)e * NCB + c / CG] |= (unsigned char)(1u << (c % CG));
                }
        }
    auto answers = [&](int row, int c) { return (ansb[(size_t)(row / P) * NCB + c / CG] >> (c % CG)) & 1; };
    // the roots' segments of the row list, each ascending
    struct Node {
        int lo, hi, cand, no, yes;
        EvalBest best;
    };
    std::vector<Node> nodes;
    nodes.reserve((size_t)Ncap);
    std::vector<int> rows((size_t)R), root_row((size_t)R);
    {
        std::vector<int> cnt((size_t)R0 + 1, 0);
        for (int r = 0; r < R; ++r) {
            root_row[r] = root_of[(size_t)event_ctx[3 * (size_t)(r / P) + 1] * P + r % P];
            ++cnt[root_row[r] + 1];
        }
        for (int i = 0; i < R0; ++i) cnt[i + 1] += cnt[i];
        for (int i = 0; i < R0; ++i) nodes.push_back(Node{cnt[i], cnt[i + 1], -1, -1, -1, EvalBest{0.0, 0, 0, -1, 0}});
        for (int r = 0; r < R; ++r) rows[cnt[root_row[r]]++] = r;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int NLmax = std::max(R0, 2);
    DevBuf<int> d_rows, d_leaf_node;
    DevBuf<unsigned char> d_ansb;
    DevBuf<EvalLeaf> d_leaves;
    DevBuf<EvalBest> d_gbest, d_best;
    DevBuf<long long> d_node_n;
    DevBuf<double> d_node_sq;
    TRY(d_rows.alloc(ctx, (size_t)R));
    TRY(d_ansb.alloc(ctx, ansb.size()));
    TRY(d_leaves.alloc(ctx, (size_t)NLmax));
    TRY(d_gbest.alloc(ctx, (size_t)NLmax * NCB));
    TRY(d_best.alloc(ctx, (size_t)NLmax));
    TRY(d_node_n.alloc(ctx, (size_t)Ncap));
    TRY(d_node_sq.alloc(ctx, (size_t)Ncap * W));
    HIPCHK(ctx, pcl_h2d(ctx, d_rows, rows.data(), (size_t)R * sizeof(int)));
    HIPCHK(ctx, pcl_h2d(ctx, d_ansb, ansb.data(), ansb.size()));
    std::vector<EvalLeaf> batch;
    std::vector<EvalBest> bests((size_t)NLmax);
    // the bests of nodes [first, first + count): one evaluation launch over (leaf, candidate group), one arg-max launch, one download
    auto evaluate = [&](int first, int count) -> int {
        batch.clear();
        for (int i = first; i < first + count; ++i) batch.push_back(EvalLeaf{nodes[i].lo, nodes[i].hi, i, 0});
        HIPCHK(ctx, pcl_h2d(ctx, d_leaves, batch.data(), batch.size() * sizeof(EvalLeaf)));
        pcl_timer_begin(ctx, "tree_build");
        hipLaunchKernelGGL(tree_eval_kernel, dim3((unsigned)count, (unsigned)NCB), dim3(EVAL_T), 0, st, d_leaves.p, d_rows.p, ctx->tree.n(), ctx->tree.s(), ctx->tree.q(), Dh,
                           P, d_ansb.p, NCB, NC, (long long)min_count, min_gain, var_floor, d_gbest.p, d_node_n.p, d_node_sq.p);
        hipLaunchKernelGGL(tree_best_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, d_gbest.p, count, NCB, d_best.p);
        pcl_timer_end(ctx, "tree_build");
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, pcl_d2h_queue(ctx, bests.data(), d_best, (size_t)count * sizeof(EvalBest)));
        HIPCHK(ctx, hipStreamSynchronize(st));
        for (int i = 0; i < count; ++i) nodes[first + i].best = bests[i];
        return PCL_OK;
    };
    std::vector<double> gains;
    auto grow = [&]() -> int {
        TRY(evaluate(0, R0));
        std::vector<int> leaves((size_t)R0), part;
        for (int i = 0; i < R0; ++i) leaves[i] = i;
        while ((int)leaves.size() < ML) {
            int at = -1;                                          // the largest gain; the lowest node id among equals (leaves is not sorted)
            for (size_t x = 0; x < leaves.size(); ++x) {
                const Node &nd = nodes[leaves[x]];
                if (nd.best.cand < 0) continue;
                if (at < 0 || nd.best.gain > nodes[leaves[at]].best.gain || (nd.best.gain == nodes[leaves[at]].best.gain && leaves[x] < leaves[at])) at = (int)x;
            }
            if (at < 0) break;
            const int p = leaves[at], c = nodes[p].best.cand, lo = nodes[p].lo, hi = nodes[p].hi;
            part.clear();                                         // stable: the no-rows, then the yes-rows, each ascending
            for (int k = lo; k < hi; ++k)
                if (!answers(rows[k], c)) part.push_back(rows[k]);
            const int mid = lo + (int)part.size();
            for (int k = lo; k < hi; ++k)
                if (answers(rows[k], c)) part.push_back(rows[k]);
            std::copy(part.begin(), part.end(), rows.begin() + lo);
            HIPCHK(ctx, pcl_h2d(ctx, d_rows + lo, rows.data() + lo, (size_t)(hi - lo) * sizeof(int)));
            const int id_no = (int)nodes.size();
            nodes[p].cand = c;
            nodes[p].no = id_no;
            nodes[p].yes = id_no + 1;
            gains.push_back(nodes[p].best.gain);
            nodes.push_back(Node{lo, mid, -1, -1, -1, EvalBest{0.0, 0, 0, -1, 0}});
            nodes.push_back(Node{mid, hi, -1, -1, -1, EvalBest{0.0, 0, 0, -1, 0}});
            leaves[at] = id_no;
            leaves.push_back(id_no + 1);
            TRY(evaluate(id_no, 2));
        }
        return PCL_OK;
    };
    const int rc = grow();
    if (rc != PCL_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    const int N = (int)nodes.size();
    std::vector<long long> h_n((size_t)N);
    std::vector<int> state((size_t)N, -1), leaf_node;
    HIPCHK(ctx, pcl_d2h_queue(ctx, h_n.data(), d_node_n, (size_t)N * sizeof(long long)));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < N; ++i)
        if (nodes[i].cand < 0) {
            state[i] = (int)leaf_node.size();
            leaf_node.push_back(i);
        }
    const int Jt = (int)leaf_node.size();
    if (install)
        for (int j = 0; j < Jt; ++j)
            if (h_n[leaf_node[j]] <= 0)
                PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: leaf node %d (tied state %d) has no frame: no Gaussian to install (the model in place stays)", who, leaf_node[j], j);
    if (leaf_s || leaf_q) {
        std::vector<double> h_sq((size_t)N * W);
        HIPCHK(ctx, pcl_d2h_queue(ctx, h_sq.data(), d_node_sq, h_sq.size() * sizeof(double)));
        HIPCHK(ctx, hipStreamSynchronize(st));
        for (int j = 0; j < Jt; ++j) {
            const double *src = &h_sq[(size_t)leaf_node[j] * W];
            if (leaf_s) memcpy(leaf_s + (size_t)j * Dh, src, (size_t)Dh * sizeof(double));
            if (leaf_q) memcpy(leaf_q + (size_t)j * Dh, src + Dh, (size_t)Dh * sizeof(double));
        }
    }
    for (int i = 0; i < N; ++i) {
        if (node_cand) node_cand[i] = nodes[i].cand;
        if (node_child) {
            node_child[2 * (size_t)i] = nodes[i].no;
            node_child[2 * (size_t)i + 1] = nodes[i].yes;
        }
        if (node_state) node_state[i] = state[i];
        if (node_n) node_n[i] = h_n[i];
        if (row_state && nodes[i].cand < 0)
            for (int k = nodes[i].lo; k < nodes[i].hi; ++k) row_state[rows[k]] = state[i];
    }
    if (split_gain) std::copy(gains.begin(), gains.end(), split_gain);
    if (leaf_n)
        for (int j = 0; j < Jt; ++j) leaf_n[j] = h_n[leaf_node[j]];
    if (n_nodes_out) *n_nodes_out = N;
    if (n_states_out) *n_states_out = Jt;
    if (!install) return PCL_OK;
    // the seed model: pcl_model_flat_start's path -- alloc, fill the float64 master copy on the stream, finish
    TRY(d_leaf_node.alloc(ctx, (size_t)Jt));
    HIPCHK(ctx, pcl_h2d(ctx, d_leaf_node, leaf_node.data(), (size_t)Jt * sizeof(int)));
    TRY(pcl_model_alloc(ctx, Jt, 1, Dh, flags, who));
    const int per = ctx->Mpad * ctx->D;
    pcl_timer_begin(ctx, "tree_build");
    hipLaunchKernelGGL(tree_install_kernel, dim3((unsigned)Jt, (unsigned)((per + 255) / 256)), dim3(256), 0, ctx->stream, d_leaf_node.p, d_node_n.p, d_node_sq.p, Jt,
                       ctx->Mpad, ctx->D, Dh, var_floor, ctx->mean64.p, ctx->var64.p, ctx->w64.p);
    pcl_timer_end(ctx, "tree_build");
    HIPCHK(ctx, hipGetLastError());
    const int rf = pcl_model_finish(ctx);
    (void)hipStreamSynchronize(ctx->stream);                      // (the locals above are free to go)
    return rf;
}
