// lattice.hip -- the word lattice of a token-passing decode (gfx950): canonical order, forward-backward and Viterbi over the arcs, arc
// posteriors and word confidences.  pcl_batch_decode_lattice / pcl_batch_lattice_get / _posteriors / _results (the rule in full:
// include/poccala_hip.h).  All float64, compiled with -ffp-contract=off, integer atomics only (counts).
//
// The single tree with one history entry per frame is a time-conditioned search: every word that ends at frame t joins the same
// continuation, the frame's entry.  So the lattice's nodes are START (node 0: history -1, seed 0, frame -1), the history entries (entry k =
// node k + 1; they ascend in frame, so the index order is a topological order) and END (node H + 1); its arcs are the word-end donors the
// decode kernels' LAT instantiations recorded (hmm_decode_common.h: DecLat), from the donor's entry to the entry made at the donor's frame,
// and the closing arcs, the decoder's own ending: the n_final tokens the transfer returned, from their entry to END.
//
// lattice_build_kernel (one workgroup per utterance, behind the decode kernel on its stream; pcl_kernel_time "lattice_build")
//   recorded arcs into ascending (frame, tok) -- the kernels append frame after frame, so only the inside of a frame is sorted: an arc's place
//   is its frame's first place plus the arcs of the frame with a smaller token index; closing arcs behind them in transfer order (frame
//   T - 1, tok = rank, word -1, term 0).  start = hist + 1; end = 1 + the entry whose hist_frame is the arc's frame (binary search).
//   The arcs are then sorted by end node as they stand: in_ptr by binary search.  out_ptr / out_idx: a counting sort by start node, stable --
//   one wave places the arcs 64 at a time, equal keys of a chunk in lane order behind the key's cursor.
// lattice_post_kernel (one workgroup per utterance; "lattice_post"), w(a) = kappa (score(a) - seed(start(a))) + term(a):
//   forward over the nodes in index order, alpha(n) = LSE over the arcs into n of alpha(start) + w, and Viterbi with the earliest arc on
//   ties; backward in descending order over out_idx, beta(n) = LSE of w + beta(end); ln Z = alpha(END); ln p(a) = ((alpha(start) + w) +
//   beta(end)) - ln Z.  Every log-sum-exp is max-then-sum over the node's list: thread i takes arcs i, i + 256, ... of the list in that order,
//   the 64 lanes of a wave combine by a butterfly (partner lane ^ 32, 16, 8, 4, 2, 1), the four waves in ascending order -- hmm_mbr.hip's
//   order; a maximum of +-inf is returned as itself, so a node that cannot be reached (or cannot reach END) holds -inf and so do its arcs.
//   The best path is read back from END through the back-pointers.  A word of it (arc a*, frames (frame(start), frame(a*)]) gets Wessel's
//   C_max: max over the frames tau of its span of P(tau) = sum, in ascending arc order, of exp(ln p(a)) over the arcs a that cover tau and
//   share a*'s identity (the word id when the decode ran with a language model and a* is a recorded arc; the node otherwise, and for the
//   closing arc).  One thread per frame, which starts at the first arc that ends at or after its frame.  An empty span (a closing arc from
//   an entry made at the last frame) gives the arc's own posterior.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "hmm_decode_common.h"

namespace {

constexpr int LT = 256, LNW = LT / 64;      // threads and waves of both kernels
enum { ST_OVERFLOW = 1, ST_NO_FINAL = 2, ST_BAD_RECORD = 4, ST_NO_PATH = 8 };   // lat_status bits
enum { UI_WANTED = 0, UI_NREC, UI_NARCS, UI_NNODES, UI_OVERFLOW, UI_STATUS, UI_BESTN, UI_COUNT };

struct LatArgs {
    int max_arcs, A, NN, Tmax, use_word;
    double kappa;
    const UttDesc *utts;
    const int *raw_frame, *raw_tok, *raw_node, *raw_hist, *raw_word;           // [U][max_arcs]
    const double *raw_score, *raw_term;
    const int *hist_frame;                                                      // [U][Tmax]
    const double *hist_seed;
    PclLatDecEnd end;                                                           // the decoder's own ending
    int *frame, *tok, *node, *hist, *word, *start, *endn;                       // [U][A]
    double *score, *term, *w, *lnp;
    int *out_idx;                                                               // [U][A]
    int *in_ptr, *out_ptr, *bp, *best;                                          // [U][NN]
    double *seed, *alpha, *beta, *vit, *conf;                                   // [U][NN]
    int *utt_i;                                                                 // [UI_COUNT][U]
    double *lnZ, *best_score;                                                   // [U]
    int U;
};

__device__ __forceinline__ int lower_bound_i(const int *v, int n, int key) {   // the first index with v[i] >= key
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(LT) void lattice_build_kernel(LatArgs a) {
    __shared__ int s_bad;
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const size_t ro = (size_t)u * a.max_arcs, co = (size_t)u * a.A, no = (size_t)u * a.NN, ho = (size_t)u * a.Tmax;
    const int wanted = a.utt_i[UI_WANTED * a.U + u], n_rec = min(wanted, a.max_arcs);
    const int H = a.end.hist_n[u], nf = a.end.out_n[u], T = a.utts[u].T, n_arcs = n_rec + nf;
    const int *hf = a.hist_frame + ho;
    if (tid == 0) s_bad = 0;
    // Records that cannot come from a decode (the test entry's, or what lies behind a cut list) may leave places no record reaches:
    // every place holds an empty arc (START -> START, frame -1, score -inf) before the records take theirs
    for (int i = tid; i < n_rec; i += LT) {
        a.frame[co + i] = a.tok[co + i] = a.node[co + i] = a.hist[co + i] = a.word[co + i] = -1;
        a.score[co + i] = -INFINITY;
        a.term[co + i] = 0.0;
        a.start[co + i] = a.endn[co + i] = 0;
    }
    __syncthreads();
    bool bad = false;
    for (int i = tid; i < n_rec; i += LT) {
        const int f = a.raw_frame[ro + i], tk = a.raw_tok[ro + i], hs = a.raw_hist[ro + i];
        int g0 = i, less = 0;                                      // the frame's first place, and the arcs of the frame before this one
        for (int j = i - 1; j >= 0 && a.raw_frame[ro + j] == f; --j) {
            less += a.raw_tok[ro + j] < tk;
            if (a.raw_tok[ro + j] == tk) bad = true;               // (a token ends one word in a frame: two records would share a place)
            g0 = j;
        }
        for (int j = i + 1; j < n_rec && a.raw_frame[ro + j] == f; ++j) {
            less += a.raw_tok[ro + j] < tk;
            if (a.raw_tok[ro + j] == tk) bad = true;
        }
        if (i > 0 && a.raw_frame[ro + i - 1] > f) bad = true;      // (frames ascend)
        const int to = g0 + less, e = lower_bound_i(hf, H, f);
        if (e >= H || hf[e] != f || hs < -1 || hs >= e) bad = true;          // (an arc goes forward: its entry was made before its frame)
        a.frame[co + to] = f;
        a.tok[co + to] = tk;
        a.node[co + to] = a.raw_node[ro + i];
        a.hist[co + to] = hs;
        a.word[co + to] = a.raw_word[ro + i];
        a.score[co + to] = a.raw_score[ro + i];
        a.term[co + to] = a.raw_term[ro + i];
        a.start[co + to] = bad ? 0 : hs + 1;
        a.endn[co + to] = min(e, H - 1) + 1;
    }
    for (int c = tid; c < nf; c += LT) {                           // the closing arcs, in transfer order
        const size_t x = (size_t)u * a.end.candidate + c;
        const int to = n_rec + c, hs = a.end.out_hist[x];
        if (hs < -1 || hs >= H) bad = true;
        a.frame[co + to] = T - 1;
        a.tok[co + to] = c;
        a.node[co + to] = a.end.out_node[x];
        a.hist[co + to] = hs;
        a.word[co + to] = -1;
        a.score[co + to] = a.end.out_score[x];
        a.term[co + to] = 0.0;
        a.start[co + to] = bad ? 0 : hs + 1;
        a.endn[co + to] = H + 1;
    }
    if (bad) atomicOr(&s_bad, 1);
    for (int n = tid; n <= H; n += LT) a.seed[no + n] = n == 0 ? 0.0 : a.hist_seed[ho + n - 1];
    for (int n = tid; n <= H + 2; n += LT) a.out_ptr[no + n] = 0;
    __syncthreads();
    for (int n = tid; n <= H + 2; n += LT) a.in_ptr[no + n] = lower_bound_i(a.endn + co, n_arcs, n);
    // (a flagged utterance may hold places no record reached: whatever lies there is clamped, so that counts and places stay in range)
    auto start_key = [&](int i) { return min(max(a.start[co + i], 0), H); };
    for (int i = tid; i < n_arcs; i += LT) atomicAdd(&a.out_ptr[no + start_key(i) + 1], 1);
    __syncthreads();
    if (tid == 0) {
        for (int n = 1; n <= H + 2; ++n) a.out_ptr[no + n] += a.out_ptr[no + n - 1];
        a.utt_i[UI_NREC * a.U + u] = n_rec;
        a.utt_i[UI_NARCS * a.U + u] = n_arcs;
        a.utt_i[UI_NNODES * a.U + u] = H;
        a.utt_i[UI_OVERFLOW * a.U + u] = wanted > a.max_arcs;
        a.utt_i[UI_STATUS * a.U + u] = (wanted > a.max_arcs ? ST_OVERFLOW : 0) | (nf == 0 ? ST_NO_FINAL : 0) | (s_bad ? ST_BAD_RECORD : 0);
        a.utt_i[UI_BESTN * a.U + u] = 0;
    }
    __syncthreads();
    // the stable placement: wave 0, 64 arcs at a time; the cursors live in the back-pointer row, which the pass behind writes anew
    int *cur = a.bp + no;
    for (int n = tid; n <= H + 1; n += LT) cur[n] = a.out_ptr[no + n];
    __syncthreads();
    if (tid >= 64) return;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    for (int i0 = 0; i0 < n_arcs; i0 += 64) {
        const int i = i0 + lane;
        const bool valid = i < n_arcs;
        const int key = valid ? start_key(i) : -1;
        unsigned long long rem = __ballot(valid);
        while (rem != 0ull) {                                      // (wave-uniform: one round per different key of the chunk)
            const int leader = __ffsll((long long)rem) - 1;
            const int k0 = __shfl(key, leader, 64);
            const bool mine = valid && key == k0;
            const unsigned long long m = __ballot(mine);
            int c = 0;
            if (lane == leader) c = cur[k0];
            c = __shfl(c, leader, 64);
            if (mine) a.out_idx[co + c + __popcll(m & lt_mask)] = i;
            if (lane == leader) cur[k0] = c + __popcll(m);
            __threadfence_block();                                 // (another lane may lead the same key in a later chunk)
            rem &= ~m;
        }
    }
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {            // a butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

struct PostLds {
    double m[2][LNW], s[2][LNW], v[2][LNW];
    int j[2][LNW];
};

// One node's list: value(k) and the Viterbi candidate vvalue(k) of list position k in [0, cnt), arc(k) its arc index.  Returns the LSE;
// vbest / varc = the best candidate and the earliest arc that reaches it (VIT).  Workgroup-collective; `slot` alternates between calls.
template <bool VIT, class Val, class VVal, class Arc>
__device__ __forceinline__ double node_lse(int cnt, Val value, VVal vvalue, Arc arc, PostLds &L, int &slot, double &vbest, int &varc) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double m = -INFINITY, vb = -INFINITY;
    int vj = NONE;
    for (int k = tid; k < cnt; k += LT) {
        m = fmax(m, value(k));
        if constexpr (VIT) {
            const double y = vvalue(k);
            const int j = arc(k);
            if (vj == NONE || y > vb) {                            // (a thread's arcs ascend)
                vb = y;
                vj = j;
            }
        }
    }
    m = wave_max(m);
    if constexpr (VIT) pcl_wave_best(vb, vj);
    if (lane == 0) {
        L.m[slot][wave] = m;
        if constexpr (VIT) {
            L.v[slot][wave] = vb;
            L.j[slot][wave] = vj;
        }
    }
    __syncthreads();
    double M = L.m[slot][0];
    for (int w = 1; w < LNW; ++w) M = fmax(M, L.m[slot][w]);
    if constexpr (VIT) pcl_best_of_waves<LNW>(L.v[slot], L.j[slot], vbest, varc);
    double r = M;
    if (!isinf(M)) {                                               // (uniform; an empty list, or one of -inf only, is -inf)
        double s = 0.0;
        for (int k = tid; k < cnt; k += LT) s = s + exp(value(k) - M);
        s = wave_sum(s);
        if (lane == 0) L.s[slot][wave] = s;
        __syncthreads();
        double S = L.s[slot][0];
        for (int w = 1; w < LNW; ++w) S = S + L.s[slot][w];
        r = M + log(S);
    }
    slot ^= 1;
    return r;
}

__global__ __launch_bounds__(LT) void lattice_post_kernel(LatArgs a) {
    __shared__ PostLds L;
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t co = (size_t)u * a.A, no = (size_t)u * a.NN, ho = (size_t)u * a.Tmax;
    const int n_arcs = a.utt_i[UI_NARCS * a.U + u], H = a.utt_i[UI_NNODES * a.U + u], END = H + 1;
    int status = a.utt_i[UI_STATUS * a.U + u] & ~ST_NO_PATH;
    const int *start = a.start + co, *endn = a.endn + co, *frame = a.frame + co, *in_ptr = a.in_ptr + no, *out_ptr = a.out_ptr + no, *out_idx = a.out_idx + co;
    const int *hf = a.hist_frame + ho;
    double *w = a.w + co, *lnp = a.lnp + co, *alpha = a.alpha + no, *beta = a.beta + no, *vit = a.vit + no;
    int *bp = a.bp + no, *best = a.best + no;
    if (status != 0) {                                             // overflowed, nothing came out of the transfer, or a record out of range
        for (int i = tid; i < n_arcs; i += LT) lnp[i] = NAN;
        if (tid == 0) {
            a.lnZ[u] = NAN;
            a.best_score[u] = NAN;
            a.utt_i[UI_BESTN * a.U + u] = 0;
            a.utt_i[UI_STATUS * a.U + u] = status;
        }
        return;
    }
    for (int i = tid; i < n_arcs; i += LT) {
        const double s = a.score[co + i];
        const double ac = s == -INFINITY ? -INFINITY : s - a.seed[no + start[i]];
        w[i] = a.kappa * ac + a.term[co + i];
    }
    if (tid == 0) {
        alpha[0] = 0.0;
        vit[0] = 0.0;
        bp[0] = -1;
        beta[END] = 0.0;
    }
    __syncthreads();
    int slot = 0;
    // forward and Viterbi.  alpha / vit of node n - 1 are every thread's own copy (the same bits): what thread 0 stored for the nodes
    // before it lies behind at least one barrier
    double a_prev = 0.0, v_prev = 0.0;
    for (int n = 1; n <= END; ++n) {
        const int lo = in_ptr[n], cnt = in_ptr[n + 1] - lo;
        double vb;
        int vj;
        const double an = node_lse<true>(
            cnt, [&](int k) { const int st = start[lo + k]; return (st == n - 1 ? a_prev : alpha[st]) + w[lo + k]; },
            [&](int k) { const int st = start[lo + k]; return (st == n - 1 ? v_prev : vit[st]) + w[lo + k]; }, [&](int k) { return lo + k; }, L, slot, vb, vj);
        if (tid == 0) {
            alpha[n] = an;
            vit[n] = vb;
            bp[n] = vj == NONE ? -1 : vj;
        }
        a_prev = an;
        v_prev = vb;
    }
    const double lnZ = a_prev, vbest = v_prev;
    double b_next = 0.0;
    for (int n = H; n >= 0; --n) {
        const int lo = out_ptr[n], cnt = out_ptr[n + 1] - lo;
        double vb;
        int vj;
        const double bn = node_lse<false>(
            cnt, [&](int k) { const int j = out_idx[lo + k], e = endn[j]; return w[j] + (e == n + 1 ? b_next : beta[e]); }, [](int) { return 0.0; },
            [](int) { return 0; }, L, slot, vb, vj);
        if (tid == 0) beta[n] = bn;
        b_next = bn;
    }
    __syncthreads();
    if (!(lnZ > -INFINITY)) status |= ST_NO_PATH;                  // (every path holds a -inf arc: no posterior, no best path)
    for (int i = tid; i < n_arcs; i += LT) lnp[i] = status ? NAN : ((alpha[start[i]] + w[i]) + beta[endn[i]]) - lnZ;
    int best_n = 0;
    if (tid == 0) {
        if (!status) {
            for (int n = END; n != 0 && best_n < a.NN;) {
                const int j = bp[n];
                if (j < 0) break;
                best[best_n++] = j;
                n = start[j];
            }
            for (int k = 0; k < best_n / 2; ++k) {
                const int x = best[k];
                best[k] = best[best_n - 1 - k];
                best[best_n - 1 - k] = x;
            }
        }
        a.lnZ[u] = status ? NAN : lnZ;
        a.best_score[u] = status ? NAN : vbest;
        a.utt_i[UI_BESTN * a.U + u] = best_n;
        a.utt_i[UI_STATUS * a.U + u] = status;
        L.j[0][0] = best_n;
    }
    __syncthreads();
    best_n = L.j[0][0];
    __syncthreads();
    // confidences: a thread per frame of the word's span
    auto node_frame = [&](int n) { return n == 0 ? -1 : hf[n - 1]; };
    for (int k = 0; k < best_n; ++k) {
        const int as = best[k], fs = node_frame(start[as]), fe = frame[as];
        const bool by_word = a.use_word && a.word[co + as] >= 0;
        const int id = by_word ? a.word[co + as] : a.node[co + as];
        const int *ids = by_word ? a.word + co : a.node + co;
        double pm = fe > fs ? -INFINITY : exp(lnp[as]);
        for (int tau = fs + 1 + tid; tau <= fe; tau += LT) {
            double P = 0.0;
            for (int j = lower_bound_i(frame, n_arcs, tau); j < n_arcs; ++j)
                if (ids[j] == id && node_frame(start[j]) < tau) P = P + exp(lnp[j]);
            pm = fmax(pm, P);
        }
        pm = wave_max(pm);
        if (lane == 0) L.m[slot][wave] = pm;
        __syncthreads();
        double M = L.m[slot][0];
        for (int x = 1; x < LNW; ++x) M = fmax(M, L.m[slot][x]);
        if (tid == 0) a.conf[no + k] = M;
        slot ^= 1;
    }
}

struct LatLayout {
    size_t ra, ca, nn;             // U max_arcs, U A, U NN
};

LatArgs lat_args(const pcl_batch *b) {
    const size_t U = (size_t)b->U, ra = U * b->lat_max_arcs, A = (size_t)b->lat_max_arcs + b->lat_cand, ca = U * A, NN = (size_t)b->shape.Tmax + 3, nn = U * NN;
    LatArgs a = {};
    a.U = b->U;
    a.max_arcs = b->lat_max_arcs;
    a.A = (int)A;
    a.NN = (int)NN;
    a.Tmax = b->shape.Tmax;
    a.use_word = b->lat_lm ? 1 : 0;
    a.kappa = 1.0;
    a.utts = b->d_utt;
    int *ri = b->lat_raw_i;
    a.raw_frame = ri;
    a.raw_tok = ri + ra;
    a.raw_node = ri + 2 * ra;
    a.raw_hist = ri + 3 * ra;
    a.raw_word = ri + 4 * ra;
    double *rf = b->lat_raw_f;
    a.raw_score = rf;
    a.raw_term = rf + ra;
    a.hist_frame = b->lat_hist_frame;
    a.hist_seed = b->lat_hist_seed;
    int *ci = b->lat_arc_i;
    a.frame = ci;
    a.tok = ci + ca;
    a.node = ci + 2 * ca;
    a.hist = ci + 3 * ca;
    a.word = ci + 4 * ca;
    a.start = ci + 5 * ca;
    a.endn = ci + 6 * ca;
    double *cf = b->lat_arc_f;
    a.score = cf;
    a.term = cf + ca;
    a.w = cf + 2 * ca;
    a.lnp = cf + 3 * ca;
    a.out_idx = b->lat_out_idx;
    int *ni = b->lat_node_i;
    a.in_ptr = ni;
    a.out_ptr = ni + nn;
    a.bp = ni + 2 * nn;
    a.best = ni + 3 * nn;
    double *nf = b->lat_node_f;
    a.seed = nf;
    a.alpha = nf + nn;
    a.beta = nf + 2 * nn;
    a.vit = nf + 3 * nn;
    a.conf = b->lat_conf;
    a.utt_i = b->lat_utt_i;
    a.lnZ = b->lat_utt_f;
    a.best_score = b->lat_utt_f.p + U;
    return a;
}

}  // namespace

// the batch's lattice buffers for (max_arcs, candidate): re-made as a group when either changed
int pcl_lattice_reserve(pcl_ctx *ctx, pcl_batch *b, int max_arcs, int candidate) {
    const size_t U = (size_t)b->U, ra = U * max_arcs, ca = U * ((size_t)max_arcs + candidate), nn = U * ((size_t)b->shape.Tmax + 3), fr = U * b->shape.Tmax;
    if (b->lat_max_arcs != max_arcs || b->lat_cand != candidate || !b->lat_raw_i) {
        static_cast<BatchLatDev &>(*b) = {};
        TRY(b->lat_raw_i.alloc(ctx, 5 * ra));
        TRY(b->lat_raw_f.alloc(ctx, 2 * ra));
        TRY(b->lat_arc_i.alloc(ctx, 7 * ca));
        TRY(b->lat_arc_f.alloc(ctx, 4 * ca));
        TRY(b->lat_out_idx.alloc(ctx, ca));
        TRY(b->lat_node_i.alloc(ctx, 4 * nn));
        TRY(b->lat_node_f.alloc(ctx, 4 * nn));
        TRY(b->lat_hist_frame.alloc(ctx, fr));
        TRY(b->lat_hist_seed.alloc(ctx, fr));
        TRY(b->lat_utt_i.alloc(ctx, UI_COUNT * U));
        TRY(b->lat_utt_f.alloc(ctx, 2 * U));
        TRY(b->lat_conf.alloc(ctx, nn));
        b->lat_max_arcs = max_arcs;
        b->lat_cand = candidate;
    }
    b->have_lat = b->have_lat_post = false;
    HIPCHK(ctx, hipMemsetAsync(b->lat_utt_i, 0, UI_COUNT * U * sizeof(int), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(b->lat_hist_frame, 0xff, fr * sizeof(int), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(b->lat_hist_seed, 0, fr * sizeof(double), ctx->stream));
    return PCL_OK;
}

DecLat pcl_lattice_dec_args(const pcl_batch *b) {
    const LatArgs a = lat_args(b);
    DecLat d;
    d.max_arcs = a.max_arcs;
    d.arc_frame = const_cast<int *>(a.raw_frame);
    d.arc_tok = const_cast<int *>(a.raw_tok);
    d.arc_node = const_cast<int *>(a.raw_node);
    d.arc_hist = const_cast<int *>(a.raw_hist);
    d.arc_word = const_cast<int *>(a.raw_word);
    d.arc_score = const_cast<double *>(a.raw_score);
    d.arc_term = const_cast<double *>(a.raw_term);
    d.n_wanted = a.utt_i + UI_WANTED * (size_t)b->U;
    d.hist_frame = b->lat_hist_frame;
    d.hist_seed = b->lat_hist_seed;
    return d;
}

// canonical order and the two CSRs, on ctx->stream (the decode kernel's)
int pcl_lattice_build(pcl_ctx *ctx, pcl_batch *b, const PclLatDecEnd &end, bool with_lm) {
    b->lat_lm = with_lm;
    LatArgs a = lat_args(b);
    a.end = end;
    pcl_timer_begin(ctx, "lattice_build");
    hipLaunchKernelGGL(lattice_build_kernel, dim3(b->U), dim3(LT), 0, ctx->stream, a);
    pcl_timer_end(ctx, "lattice_build");
    HIPCHK(ctx, hipGetLastError());
    return PCL_OK;
}

extern "C" {

int pcl_batch_lattice_get(pcl_batch *b, int32_t *n_arcs, int32_t *n_arcs_wanted, int32_t *lat_overflow, int32_t *arc_frame, int32_t *arc_tok, int32_t *arc_node,
                          int32_t *arc_hist, double *arc_score, double *arc_term, int32_t *arc_word, int32_t *arc_start, int32_t *arc_end, int32_t *hist_frame,
                          double *hist_seed) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_lat) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_lattice_get: run pcl_batch_decode_lattice first (new emissions, transitions, states or another decode drop the lattice)");
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const LatArgs a = lat_args(b);
    const size_t U = (size_t)b->U, ca = U * a.A, fr = U * b->shape.Tmax;
    auto get = [&](void *dst, const void *src, size_t bytes) -> int {
        if (dst) HIPCHK(ctx, pcl_d2h_queue(ctx, dst, src, bytes));
        return PCL_OK;
    };
    TRY(get(n_arcs, a.utt_i + UI_NARCS * U, U * 4));
    TRY(get(n_arcs_wanted, a.utt_i + UI_WANTED * U, U * 4));
    TRY(get(lat_overflow, a.utt_i + UI_OVERFLOW * U, U * 4));
    TRY(get(arc_frame, a.frame, ca * 4));
    TRY(get(arc_tok, a.tok, ca * 4));
    TRY(get(arc_node, a.node, ca * 4));
    TRY(get(arc_hist, a.hist, ca * 4));
    TRY(get(arc_score, a.score, ca * 8));
    TRY(get(arc_term, a.term, ca * 8));
    TRY(get(arc_word, a.word, ca * 4));
    TRY(get(arc_start, a.start, ca * 4));
    TRY(get(arc_end, a.endn, ca * 4));
    TRY(get(hist_frame, a.hist_frame, fr * 4));
    TRY(get(hist_seed, a.hist_seed, fr * 8));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

int pcl_batch_lattice_posteriors(pcl_batch *b, double kappa) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_lat) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_lattice_posteriors: run pcl_batch_decode_lattice first (new emissions, transitions, states or another decode drop the lattice)");
    if (!(kappa > 0.0) || !std::isfinite(kappa)) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_lattice_posteriors: kappa = %g is not a finite number > 0", kappa);
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    b->have_lat_post = false;
    LatArgs a = lat_args(b);
    a.kappa = kappa;
    pcl_timer_begin(ctx, "lattice_post");
    hipLaunchKernelGGL(lattice_post_kernel, dim3(b->U), dim3(LT), 0, ctx->stream, a);
    pcl_timer_end(ctx, "lattice_post");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, pcl_batch_mark(b));
    b->have_lat_post = true;
    return PCL_OK;
}

int pcl_batch_lattice_results(pcl_batch *b, double *lnZ, double *arc_lnpost, int32_t *best_n, int32_t *best_arc, double *best_score, double *best_conf, int32_t *lat_status) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_lat || !b->have_lat_post) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_lattice_results: run pcl_batch_lattice_posteriors first (another decode drops the lattice and its posteriors)");
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const LatArgs a = lat_args(b);
    const size_t U = (size_t)b->U, ca = U * a.A, nn = U * a.NN;
    auto get = [&](void *dst, const void *src, size_t bytes) -> int {
        if (dst) HIPCHK(ctx, pcl_d2h_queue(ctx, dst, src, bytes));
        return PCL_OK;
    };
    TRY(get(lnZ, a.lnZ, U * 8));
    TRY(get(arc_lnpost, a.lnp, ca * 8));
    TRY(get(best_n, a.utt_i + UI_BESTN * U, U * 4));
    TRY(get(best_arc, a.best, nn * 4));
    TRY(get(best_score, a.best_score, U * 8));
    TRY(get(best_conf, a.conf, nn * 8));
    TRY(get(lat_status, a.utt_i + UI_STATUS * U, U * 4));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

// TEST ENTRY: a record set of the caller's in place of a decode's (tests/test_gpu_lattice_edges.py reaches list lengths and node counts
// no decode of a few seconds does).  Arrays as pcl_batch_lattice_get / pcl_batch_decode_get name them, (U, max_arcs) / (U, candidate) /
// (U, Tmax) / (U,); n_arcs_wanted may exceed max_arcs (an overflow).  The build runs on them as it does behind a decode; out-of-range
// records are flagged there (lat_status), nothing is indexed by them.
int pcl_batch_lattice_set_records(pcl_batch *b, int max_arcs, int candidate, int with_words, const int32_t *n_arcs_wanted, const int32_t *arc_frame, const int32_t *arc_tok,
                                  const int32_t *arc_node, const int32_t *arc_hist, const double *arc_score, const double *arc_term, const int32_t *arc_word,
                                  const int32_t *hist_n, const int32_t *hist_frame, const double *hist_seed, const int32_t *n_final, const int32_t *final_node,
                                  const double *final_score, const int32_t *final_hist) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    const char *who = "pcl_batch_lattice_set_records";
    if (max_arcs < 1 || candidate < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: max_arcs %d, candidate %d", who, max_arcs, candidate);
    if (!n_arcs_wanted || !arc_frame || !arc_tok || !arc_node || !arc_hist || !arc_score || !arc_term || !arc_word || !hist_n || !hist_frame || !hist_seed || !n_final ||
        !final_node || !final_score || !final_hist)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: NULL argument", who);
    const size_t U = (size_t)b->U, ra = U * max_arcs, fr = U * b->shape.Tmax, oc = U * candidate;
    for (size_t u = 0; u < U; ++u)
        if (n_arcs_wanted[u] < 0 || hist_n[u] < 0 || hist_n[u] > b->shape.Tmax || n_final[u] < 0 || n_final[u] > candidate)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %zu: n_arcs_wanted %d, hist_n %d (Tmax %d), n_final %d (candidate %d)", who, u, n_arcs_wanted[u], hist_n[u],
                     b->shape.Tmax, n_final[u], candidate);
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TRY(pcl_lattice_reserve(ctx, b, max_arcs, candidate));
    b->launched = true;
    HIPCHK(ctx, pcl_h2d(ctx, b->d_utt, b->shape.utt.data(), U * sizeof(UttDesc)));
    const LatArgs a = lat_args(b);
    DevBuf<int> d_end_i;                                           // hist_n | n_final | final_node | final_hist
    DevBuf<double> d_end_f;
    TRY(d_end_i.alloc(ctx, 2 * U + 2 * oc));
    TRY(d_end_f.alloc(ctx, oc));
    auto up = [&](const void *dst, const void *src, size_t bytes) -> int {
        HIPCHK(ctx, pcl_h2d(ctx, const_cast<void *>(dst), src, bytes));
        return PCL_OK;
    };
    TRY(up(a.utt_i + UI_WANTED * U, n_arcs_wanted, U * 4));
    TRY(up(a.raw_frame, arc_frame, ra * 4));
    TRY(up(a.raw_tok, arc_tok, ra * 4));
    TRY(up(a.raw_node, arc_node, ra * 4));
    TRY(up(a.raw_hist, arc_hist, ra * 4));
    TRY(up(a.raw_word, arc_word, ra * 4));
    TRY(up(a.raw_score, arc_score, ra * 8));
    TRY(up(a.raw_term, arc_term, ra * 8));
    TRY(up(a.hist_frame, hist_frame, fr * 4));
    TRY(up(a.hist_seed, hist_seed, fr * 8));
    TRY(up(d_end_i.p, hist_n, U * 4));
    TRY(up(d_end_i.p + U, n_final, U * 4));
    TRY(up(d_end_i.p + 2 * U, final_node, oc * 4));
    TRY(up(d_end_i.p + 2 * U + oc, final_hist, oc * 4));
    TRY(up(d_end_f.p, final_score, oc * 8));
    const PclLatDecEnd end{d_end_i.p + U, d_end_i.p + 2 * U, d_end_i.p + 2 * U + oc, d_end_i.p, d_end_f.p, candidate};
    TRY(pcl_lattice_build(ctx, b, end, with_words != 0));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                // (the staging goes back to the pool with the work done)
    HIPCHK(ctx, pcl_batch_mark(b));
    b->have_lat = true;
    return PCL_OK;
}

}  // extern "C"
