// tying.hip -- row f17: a decision tree's tying resident on the device, and the walks that turn contexts into tied states.
//
// ContextTree.Tree.lookup walks one tree per (context, state position) in Python; a corpus of 8192 utterances asks for over a million such
// walks per batch.  Here the node arrays live on the device in the two layouts the walk reads, and one kernel maps every label position of a
// batch to its tied states:
//   nodes   one 16-byte record (cand, no, yes, state) per node, in GLOBAL memory: a step of a walk is one dwordx4 load; the arrays of a real
//           tree (tens of thousands of nodes) do not fit the LDS beside anything else, every walk starts at one of a few roots and the
//           levels below them are shared by all walks of the launch, so they are served from L2
//   q bits  q_member as a bit table, ty_W words per question; a step reads ONE word of it.  Staged in LDS by every workgroup when it is
//           at most TY_QBITS_LDS bytes (it is read once per step by every lane, at addresses that differ from lane to lane: the case the
//           LDS is there for), read from global memory above that
// Integer work only.  The validator and the packing of the two layouts: tying_check.h (plain C++, run on the CPU by tests/tying_host_check.cpp).
#include <algorithm>
#include <vector>

#include "pcl_internal.h"
#include "tying_check.h"

static_assert(sizeof(TyingNode) == sizeof(int4), "a node is one 16-byte load");

namespace {

constexpr int TY_QBITS_LDS = 16 * 1024;

// One walk.  Ends because pcl_tying_upload has checked that both children of an inner node lie behind it; stays inside the arrays because it
// has checked cand < 3 Q, children < N, and the caller the context ids <= n_units < 32 W.
__device__ __forceinline__ int tying_walk(const int4 *__restrict__ nodes, const unsigned int *qb, int Q, int W, int node, int left, int centre, int right) {
    for (;;) {
        const int4 nd = nodes[node];
        if (nd.x < 0) return nd.w;
        const int pos = nd.x / Q, qi = nd.x - pos * Q;
        const int u = pos == 0 ? left : pos == 1 ? centre : right;
        node = (qb[qi * W + (u >> 5)] >> (u & 31)) & 1u ? nd.z : nd.y;
    }
}

// The bit table for this workgroup: its LDS copy (LDS = true; dynamic shared memory of Q W words), or the global one
template <bool LDS>
__device__ __forceinline__ const unsigned int *tying_qbits(const unsigned int *__restrict__ qbits, int QW) {
    extern __shared__ unsigned int ty_lds[];
    if (!LDS) return qbits;
    for (int i = threadIdx.x; i < QW; i += blockDim.x) ty_lds[i] = qbits[i];
    __syncthreads();
    return ty_lds;
}

// pcl_tying_lookup: one thread per (context, state position)
template <bool LDS>
__global__ __launch_bounds__(256) void tying_lookup_kernel(const int4 *__restrict__ nodes, const unsigned int *__restrict__ qbits, const int *__restrict__ root_of,
                                                           int P, int Q, int W, long long n_items, const int32_t *__restrict__ ctx3, int32_t *__restrict__ out) {
    const unsigned int *qb = tying_qbits<LDS>(qbits, Q * W);
    for (long long w = blockIdx.x * 256LL + threadIdx.x; w < n_items; w += gridDim.x * 256LL) {
        const long long i = w / P;
        const int k = (int)(w - i * P);
        const int l = ctx3[3 * i], c = ctx3[3 * i + 1], r = ctx3[3 * i + 2];
        out[w] = tying_walk(nodes, qb, Q, W, root_of[c * P + k], l, c, r);
    }
}

// pcl_batch_create_labels_tied: one utterance per workgroup, the lanes stride its (label position, k) pairs.  (left, centre, right) from the
// labels with the edge symbol n_units at both ends, as ContextTree.triphone_events forms them.  Rows of utterance u start at P label_off[u] + 2 u
// (N_u = P L_u + 2 rows each): entry row, the P L_u emitting rows in label order, exit row.
template <bool LDS>
__global__ __launch_bounds__(64) void tied_label_states_kernel(const int4 *__restrict__ nodes, const unsigned int *__restrict__ qbits, const int *__restrict__ root_of,
                                                               int P, int Q, int W, int n_units, const int32_t *__restrict__ labels,
                                                               const int *__restrict__ label_off, int32_t *__restrict__ pos_state, int32_t *__restrict__ row_state) {
    const unsigned int *qb = tying_qbits<LDS>(qbits, Q * W);
    const int u = blockIdx.x, lo = label_off[u], L = label_off[u + 1] - lo;
    int32_t *rows = row_state + (size_t)P * lo + 2 * (size_t)u;
    if (threadIdx.x == 0) {
        rows[0] = PCL_ROW_ENTRY;
        rows[P * L + 1] = PCL_ROW_EXIT;
    }
    for (int w = threadIdx.x; w < P * L; w += 64) {
        const int i = w / P, k = w - i * P;
        const int c = labels[lo + i];
        const int l = i > 0 ? labels[lo + i - 1] : n_units, r = i + 1 < L ? labels[lo + i + 1] : n_units;
        const int st = tying_walk(nodes, qb, Q, W, root_of[c * P + k], l, c, r);
        pos_state[(size_t)P * lo + w] = st;
        rows[1 + w] = st;
    }
}

// The owner map of a tied batch from the monophone one of the same labels and path: frame_state[t] = unit * P + slice where kept.  The
// label position of a frame is the one its path row belongs to (hmm_align_segments_kernel's row -> position map).
__global__ __launch_bounds__(256) void tied_owner_kernel(const UttDesc *__restrict__ utts, const int32_t *__restrict__ path, const int *__restrict__ label_off,
                                                         const int32_t *__restrict__ pos_state, int P, int32_t *__restrict__ frame_state) {
    const UttDesc d = utts[blockIdx.y];
    const int lo = label_off[blockIdx.y], L = label_off[blockIdx.y + 1] - lo;
    if (L <= 0) return;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < d.T; t += gridDim.x * 256) {
        const int fs = frame_state[d.frame0 + t];
        if (fs < 0) continue;
        const int row = path[d.path_off + t];
        const int p = row <= 0 ? 0 : min((row - 1) / P, L - 1);
        frame_state[d.frame0 + t] = pos_state[(size_t)(lo + p) * P + fs % P];
    }
}

// pcl_lexicon_tie: one thread per (lexicon node, unit slot, state position) runs the walk of tying_lookup_kernel on the node's context
// node_ctx (n_nodes, 2, 3); slot 1 of a one-unit node gets -1.  gen (n_nodes, 2 P) is what pcl_lexicon_states returns and the general decode
// kernel reads.
template <bool LDS>
__global__ __launch_bounds__(256) void lexicon_tie_kernel(const int4 *__restrict__ nodes, const unsigned int *__restrict__ qbits, const int *__restrict__ root_of,
                                                          int P, int Q, int W, int n_nodes, const int32_t *__restrict__ node_ctx,
                                                          const int *__restrict__ node_nunits, int *__restrict__ gen) {
    const unsigned int *qb = tying_qbits<LDS>(qbits, Q * W);
    const long long n_items = (long long)n_nodes * 2 * P;
    for (long long w = blockIdx.x * 256LL + threadIdx.x; w < n_items; w += gridDim.x * 256LL) {
        const long long slot = w / P;                              // node * 2 + j
        const int k = (int)(w - slot * P), j = (int)(slot & 1);
        int st = -1;
        if (j < node_nunits[slot >> 1]) {
            const int l = node_ctx[3 * slot], c = node_ctx[3 * slot + 1], r = node_ctx[3 * slot + 2];
            st = tying_walk(nodes, qb, Q, W, root_of[c * P + k], l, c, r);
        }
        gen[w] = st;
    }
}

// ... and the same ids as the left-to-right decode kernel reads them (DecTie::lr; P = 3 there): six 16-bit fields per node, a one-unit
// node repeats slot 0 in slot 1 (the kernel reads both and drops the second).  Zero for another P: that kernel does not apply then.
__global__ __launch_bounds__(256) void lexicon_tie_pack_kernel(int n_nodes, int P, const int *__restrict__ gen, int4 *__restrict__ lr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_nodes) return;
    int4 v = make_int4(0, 0, 0, 0);
    if (P == 3) {
        unsigned int s[6];
#pragma unroll
        for (int x = 0; x < 6; ++x) {
            const int a = gen[(size_t)i * 6 + x];
            s[x] = (unsigned int)(a >= 0 ? a : gen[(size_t)i * 6 + x - 3]) & 0xffffu;
        }
        v = make_int4((int)(s[0] | s[1] << 16), (int)(s[2] | s[3] << 16), (int)(s[4] | s[5] << 16), 0);
    }
    lr[i] = v;
}

size_t qbits_shm(const pcl_ctx *ctx) {
    const size_t bytes = (size_t)ctx->ty_Q * ctx->ty_W * sizeof(unsigned int);
    return bytes <= (size_t)TY_QBITS_LDS ? bytes : 0;
}

}  // namespace

void pcl_tying_release(pcl_ctx *ctx) {
    static_cast<TyingDev &>(*ctx) = {};
    ctx->ty_N = ctx->ty_Q = ctx->ty_W = ctx->ty_R0 = ctx->ty_Jt = ctx->ty_P = ctx->ty_units = 0;
}

void pcl_lexicon_untie_release(pcl_ctx *ctx) {
    ctx->lex_tie_gen.release();
    ctx->lex_tie_lr.release();
    ctx->lex_tie_Jt = ctx->lex_tie_P = 0;
}

int pcl_launch_tied_label_states(pcl_ctx *ctx, pcl_batch *b, int32_t *row_state) {
    const int P = ctx->ty_P;
    const std::vector<int> &loff = b->lab.label_off;
    for (int u = 0; u < b->U; ++u) {
        if (b->shape.utt[u].vec_off != P * loff[u] + 2 * u || b->shape.utt[u].N != P * b->lab.label_len[u] + 2)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_create_labels_tied: utterance %d: rows at %d (%d of them), expected at %d", u, b->shape.utt[u].vec_off, b->shape.utt[u].N,
                     P * loff[u] + 2 * u);
    }
    const size_t tot = b->lab.labels.size();
    TRY(b->d_label_off.alloc(ctx, loff.size()));
    TRY(b->d_labels.alloc(ctx, tot));
    TRY(b->pos_state.alloc(ctx, tot * P));
    HIPCHK(ctx, pcl_h2d(ctx, b->d_label_off, loff.data(), loff.size() * sizeof(int)));
    HIPCHK(ctx, pcl_h2d(ctx, b->d_labels, b->lab.labels.data(), tot * sizeof(int32_t)));
    const size_t shm = qbits_shm(ctx);
    pcl_timer_begin(ctx, "tying");
    // (the batch's d_row_state is the destination: pcl_batch_set_states_impl writes the same values over it afterwards)
    if (shm)
        hipLaunchKernelGGL(tied_label_states_kernel<true>, dim3(b->U), dim3(64), shm, ctx->stream, ctx->ty_nodes.p, ctx->ty_qbits.p, ctx->ty_root.p, P, ctx->ty_Q,
                           ctx->ty_W, ctx->ty_units, b->d_labels.p, b->d_label_off.p, b->pos_state.p, b->d_row_state.p);
    else
        hipLaunchKernelGGL(tied_label_states_kernel<false>, dim3(b->U), dim3(64), 0, ctx->stream, ctx->ty_nodes.p, ctx->ty_qbits.p, ctx->ty_root.p, P, ctx->ty_Q,
                           ctx->ty_W, ctx->ty_units, b->d_labels.p, b->d_label_off.p, b->pos_state.p, b->d_row_state.p);
    pcl_timer_end(ctx, "tying");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, pcl_d2h_queue(ctx, row_state, b->d_row_state, (size_t)b->shape.sumN * sizeof(int32_t)));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

int pcl_launch_tied_owner(pcl_ctx *ctx, pcl_batch *b, int P, int32_t *d_frame_state) {
    if (b->shape.Tmax <= 0) return PCL_OK;
    pcl_timer_begin(ctx, "tying_owner");
    hipLaunchKernelGGL(tied_owner_kernel, dim3((unsigned)std::min(64, (b->shape.Tmax + 255) / 256), (unsigned)b->U), dim3(256), 0, ctx->stream, b->d_utt.p, b->path.p,
                       b->d_label_off.p, b->pos_state.p, P, d_frame_state);
    pcl_timer_end(ctx, "tying_owner");
    HIPCHK(ctx, hipGetLastError());
    return PCL_OK;
}

extern "C" {

int pcl_tying_upload(pcl_ctx *ctx, int n_units, int P, int Q, const uint8_t *q_member, int N, const int32_t *node_cand, const int32_t *node_child,
                     const int32_t *node_state, int R0, const int32_t *root_of, int J_t) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_tying_upload";
    if (!ctx->n_units) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: pcl_units_upload first", who);
    if (P != ctx->S - 2) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: P = %d state positions, the unit inventory has %d emitting states per unit", who, P, ctx->S - 2);
    if (n_units != ctx->n_units) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: n_units = %d, the unit inventory has %d units", who, n_units, ctx->n_units);
    const TyingArrays a{n_units, P, Q, q_member, N, node_cand, node_child, node_state, R0, root_of, J_t};
    char why[256];
    if (!tying_validate(a, why, sizeof(why))) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %s", who, why);
    std::vector<TyingNode> nodes;
    std::vector<uint32_t> qbits;
    tying_pack(a, &nodes, &qbits);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the new tying is complete on the device before the resident one is touched
    TyingDev fresh;
    TRY(fresh.ty_nodes.alloc(ctx, nodes.size()));
    TRY(fresh.ty_qbits.alloc(ctx, qbits.size()));
    TRY(fresh.ty_root.alloc(ctx, (size_t)n_units * P));
    HIPCHK(ctx, pcl_h2d(ctx, fresh.ty_nodes, nodes.data(), nodes.size() * sizeof(TyingNode)));
    HIPCHK(ctx, pcl_h2d(ctx, fresh.ty_qbits, qbits.data(), qbits.size() * sizeof(uint32_t)));
    HIPCHK(ctx, pcl_h2d(ctx, fresh.ty_root, root_of, (size_t)n_units * P * sizeof(int32_t)));
    static_cast<TyingDev &>(*ctx) = std::move(fresh);
    ctx->ty_N = N;
    ctx->ty_Q = Q;
    ctx->ty_W = tying_words(n_units);
    ctx->ty_R0 = R0;
    ctx->ty_Jt = J_t;
    ctx->ty_P = P;
    ctx->ty_units = n_units;
    return PCL_OK;
}

int pcl_tying_drop(pcl_ctx *ctx) {
    if (!ctx) return PCL_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pcl_tying_release(ctx);
    return PCL_OK;
}

int pcl_batch_get_states(pcl_batch *b, int32_t *row_state, int32_t *pos_state) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    const char *who = "pcl_batch_get_states";
    if (!b->have_states) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the batch has no row -> state map yet", who);
    if (pos_state && !b->tied) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: pos_state is kept by batches over tied states only (pcl_batch_create_labels_tied)", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (row_state) HIPCHK(ctx, pcl_d2h_queue(ctx, row_state, b->d_row_state, (size_t)b->shape.sumN * sizeof(int32_t)));
    if (pos_state) HIPCHK(ctx, pcl_d2h_queue(ctx, pos_state, b->pos_state, b->pos_state.cap * sizeof(int32_t)));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

int pcl_lexicon_tie(pcl_ctx *ctx, const int32_t *node_ctx) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_lexicon_tie";
    if (!ctx->lex_nodes) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no resident lexicon: pcl_lexicon_upload first", who);
    if (!ctx->ty_N) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no resident tying: pcl_tying_upload first", who);
    if (!node_ctx) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: node_ctx is NULL", who);
    const int nu = ctx->ty_units, P = ctx->ty_P, n_nodes = ctx->lex_nodes;
    if (P != ctx->S - 2 || nu != ctx->n_units)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the tying has %d units of P = %d state positions, the unit inventory %d units of %d emitting states", who, nu, P,
                 ctx->n_units, ctx->S - 2);
    for (int i = 0; i < n_nodes; ++i)
        for (int j = 0; j < ctx->lex_nunits_host[i]; ++j) {
            const int32_t *c = node_ctx + 3 * (2 * (size_t)i + j);
            if (c[1] != ctx->lex_units_host[2 * (size_t)i + j])
                PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: node %d slot %d: centre %d is not the node's unit %d", who, i, j, c[1], ctx->lex_units_host[2 * (size_t)i + j]);
            if (c[0] < 0 || c[0] > nu || c[2] < 0 || c[2] > nu)
                PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: node %d slot %d: neighbours (%d, %d) outside [0,%d]", who, i, j, c[0], c[2], nu);
        }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream_dp));             // (a decoder may still be reading the old states on the second stream)
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // the new states are complete on the device before the resident ones are touched
    DevBuf<int32_t> d_ctx;
    DevBuf<int> gen;
    DevBuf<int4> lr;
    const size_t items = (size_t)n_nodes * 2 * P;
    auto run = [&]() -> int {
        TRY(d_ctx.alloc(ctx, (size_t)n_nodes * 6));
        TRY(gen.alloc(ctx, items));
        TRY(lr.alloc(ctx, (size_t)n_nodes));
        HIPCHK(ctx, hipMemcpyAsync(d_ctx, node_ctx, (size_t)n_nodes * 6 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        const unsigned grid = (unsigned)std::min<size_t>((items + 255) / 256, 1024);
        const size_t shm = qbits_shm(ctx);
        pcl_timer_begin(ctx, "lexicon_tie");
        if (shm)
            hipLaunchKernelGGL(lexicon_tie_kernel<true>, dim3(grid), dim3(256), shm, ctx->stream, ctx->ty_nodes.p, ctx->ty_qbits.p, ctx->ty_root.p, P, ctx->ty_Q,
                               ctx->ty_W, n_nodes, d_ctx.p, ctx->lex_nunits.p, gen.p);
        else
            hipLaunchKernelGGL(lexicon_tie_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, ctx->ty_nodes.p, ctx->ty_qbits.p, ctx->ty_root.p, P, ctx->ty_Q,
                               ctx->ty_W, n_nodes, d_ctx.p, ctx->lex_nunits.p, gen.p);
        hipLaunchKernelGGL(lexicon_tie_pack_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, ctx->stream, n_nodes, P, gen.p, lr.p);
        pcl_timer_end(ctx, "lexicon_tie");
        HIPCHK(ctx, hipGetLastError());
        return PCL_OK;
    };
    int rc = run();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PCL_OK) {      // (on every path: the frees below rely on it)
        pcl_set_error(ctx, "pcl_lexicon_tie: HIP error");
        rc = PCL_ERR_HIP;
    }
    pcl_free_synced_scope done;
    d_ctx.release();
    if (rc != PCL_OK) return rc;
    ctx->lex_tie_gen = std::move(gen);
    ctx->lex_tie_lr = std::move(lr);
    ctx->lex_tie_Jt = ctx->ty_Jt;
    ctx->lex_tie_P = P;
    return PCL_OK;
}

int pcl_lexicon_untie(pcl_ctx *ctx) {
    if (!ctx) return PCL_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream_dp));             // (a tied decode may still be reading them)
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    pcl_lexicon_untie_release(ctx);
    return PCL_OK;
}

int pcl_lexicon_states(pcl_ctx *ctx, int32_t *node_state) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_lexicon_states";
    if (!ctx->lex_nodes || !ctx->lex_tie_Jt) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the lexicon is not tied (pcl_lexicon_tie first)", who);
    if (!node_state) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: node_state is NULL", who);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, pcl_d2h_queue(ctx, node_state, ctx->lex_tie_gen, (size_t)ctx->lex_nodes * 2 * ctx->lex_tie_P * sizeof(int32_t)));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

int pcl_tying_lookup(pcl_ctx *ctx, int n, const int32_t *ctx3, int32_t *state_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_tying_lookup";
    if (!ctx->ty_N) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no resident tying: pcl_tying_upload first", who);
    if (n < 1 || !ctx3 || !state_out) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: bad arguments (n=%d)", who, n);
    const int nu = ctx->ty_units, P = ctx->ty_P;
    if ((long long)n * P > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %d contexts of %d positions", who, n, P);
    for (int i = 0; i < n; ++i) {
        const int32_t *c = ctx3 + 3 * (size_t)i;
        if (c[1] < 0 || c[1] >= nu) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: context %d has centre %d outside [0,%d)", who, i, c[1], nu);
        if (c[0] < 0 || c[0] > nu || c[2] < 0 || c[2] > nu)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: context %d has neighbours (%d, %d) outside [0,%d]", who, i, c[0], c[2], nu);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long items = (long long)n * P;
    DevBuf<int32_t> d_ctx, d_out;
    auto run = [&]() -> int {
        TRY(d_ctx.alloc(ctx, (size_t)n * 3));
        TRY(d_out.alloc(ctx, (size_t)items));
        HIPCHK(ctx, hipMemcpyAsync(d_ctx, ctx3, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        const unsigned grid = (unsigned)std::min<long long>((items + 255) / 256, 1024);
        const size_t shm = qbits_shm(ctx);
        pcl_timer_begin(ctx, "tying_lookup");
        if (shm)
            hipLaunchKernelGGL(tying_lookup_kernel<true>, dim3(grid), dim3(256), shm, ctx->stream, ctx->ty_nodes.p, ctx->ty_qbits.p, ctx->ty_root.p, P, ctx->ty_Q,
                               ctx->ty_W, items, d_ctx.p, d_out.p);
        else
            hipLaunchKernelGGL(tying_lookup_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, ctx->ty_nodes.p, ctx->ty_qbits.p, ctx->ty_root.p, P, ctx->ty_Q,
                               ctx->ty_W, items, d_ctx.p, d_out.p);
        pcl_timer_end(ctx, "tying_lookup");
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(state_out, d_out, (size_t)items * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        return PCL_OK;
    };
    int rc = run();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PCL_OK) {      // (on every path: the frees below rely on it)
        pcl_set_error(ctx, "pcl_tying_lookup: HIP error");
        rc = PCL_ERR_HIP;
    }
    pcl_free_synced_scope done;
    d_ctx.release();
    d_out.release();
    return rc;
}

}  // extern "C"
