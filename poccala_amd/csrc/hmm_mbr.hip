// hmm_mbr.hip -- forward-backward under an acoustic scale with an expected frame accuracy beside alpha and beta (row f19): the pass behind
// pcl_batch_mbr, for minimum Bayes risk training (sMBR / MPFE) and for MMI with a scaled denominator.  Not in the reference.
//
// The rule (include/poccala_hip.h states it in full; tests/_mbr_twin.py is the same rule in NumPy, operation for operation).  Per utterance,
// float64, bs_j(t) = kappa B[j,t], A_t(j) = 1 where row j's state and the reference state of frame t fall into the same group, else 0:
//     alpha, beta                 the recursions of hmm_dp.hip on bs (every row may end, quirk Q8; log-sum-exp with quirk Q4)
//     alpha'_t(j), beta'_t(i)     the expected accuracy of the partial paths into (t, j) / out of (t, i): weighted means, the weights are the
//                                 terms of alpha's / beta's own log-sum-exp, so every exp is taken once and used by both sums
//     ln gamma_t(j)               alpha + beta - LSE_i(alpha + beta), per frame
//     c_avg                       sum_j gamma_0(j) (alpha'_0(j) + beta'_0(j)): the expected accuracy of the utterance, taken at frame 0
//     g_t(j)                      kappa gamma_t(j) (alpha'_t(j) + beta'_t(j) - c_avg)
//
// Mapping: one workgroup per utterance, lane i <-> row i, up to 1024 rows, over the batch's CSR / CSC arrays -- any transition structure.
// The BACKWARD pass runs first and stores beta and beta' time-major (the pass's own buffers); frame 0 then gives c_avg, and the FORWARD pass
// keeps alpha and alpha' of the current and the previous frame in LDS only, combines them with the stored pair and writes ln gamma and g as
// it goes.  A row publishes (value, accuracy) as ONE 16-byte LDS element, so a predecessor costs one ds_read_b128.  Two passes per step over
// the row's list: the maximum, then  s = sum e_k,  sp = sum e_k acc_k  with e_k = exp(v_k - max), both in list order (CSC: ascending source
// row; CSR: ascending target row); the value is max + log(s), the accuracy sp / s.  The emission row (and the stored beta pair) of the next
// step is requested before the current step is computed, as hmm_fb_kernel does.
// Sums ACROSS rows (the per-frame normaliser, c_avg, ln P) run in this order, which the twin repeats: the 64 lanes of a wave by a butterfly
// with partner lane ^ 32, 16, 8, 4, 2, 1 (lanes past N hold 0, or -inf under a max), then the waves' sums in ascending order.
// KREG = 2: rows with at most two predecessors and successors (every label-built sentence HMM) keep their lists in registers; a padded entry
// is ln 0, adds exp(-inf) = 0 to both sums and so leaves every bit as the general lists (KREG = 0) give it.
// Built with -ffp-contract=off: one rounded operation at a time, as the twin runs them.  No atomics: two runs give the same bits.
// Every index is bounded by what the host planned: rows < N <= blockDim.x <= 1024, frames < T, list entries inside [ptr[i], ptr[i+1]) of the
// utterance's own CSR / CSC slice; the kernels write the pass's own buffers only (mbr_post_kernel: the batch's lgam).
#include <math.h>

#include "pcl_internal.h"

namespace {

constexpr int MBR_MAXW = 16;                  // waves per workgroup (N <= 1024)

struct MbrArgs {
    const UttDesc *utts;
    const double *Bt;                         // emissions, time-major (read only)
    const int *row_ptr, *col_idx;             // CSR (successors)
    const double *csr_val;
    const int *col_ptr, *row_idx;             // CSC (predecessors, ascending source row)
    const double *csc_val;
    const double *logpi;
    const int32_t *row_state;                 // ragged (N,): state id, or PCL_ROW_ENTRY / PCL_ROW_EXIT
    const int32_t *ref_group;                 // ragged (T,): ref / group, or -1
    double *beta, *betap, *lgam, *g;          // time-major, the pass's own
    double *logp, *cavg;                      // (U,)
    double kappa;
    int group;
};

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
// The workgroup's max / sum of one value per thread, waves in ascending order.  red: [2][MBR_MAXW] doubles of LDS; `slot` alternates, so
// consecutive calls need one barrier each (whoever writes a slot again has passed the barrier of the call in between).
__device__ __forceinline__ double block_max(double v, double *red, int &slot) {
    v = wave_max(v);
    const int nw = blockDim.x >> 6;
    if (nw == 1) return v;
    if ((threadIdx.x & 63) == 0) red[slot * MBR_MAXW + (threadIdx.x >> 6)] = v;
    __syncthreads();
    double r = red[slot * MBR_MAXW];
    for (int k = 1; k < nw; ++k) r = fmax(r, red[slot * MBR_MAXW + k]);
    slot ^= 1;
    return r;
}
__device__ __forceinline__ double block_sum(double v, double *red, int &slot) {
    v = wave_sum(v);
    const int nw = blockDim.x >> 6;
    if (nw == 1) return v;
    if ((threadIdx.x & 63) == 0) red[slot * MBR_MAXW + (threadIdx.x >> 6)] = v;
    __syncthreads();
    double r = red[slot * MBR_MAXW];
    for (int k = 1; k < nw; ++k) r = r + red[slot * MBR_MAXW + k];
    slot ^= 1;
    return r;
}
// util.log_sum_exp over the rows (quirk Q4: a maximum of +-inf is returned as itself)
__device__ __forceinline__ double block_lse(double v, double *red, int &slot) {
    const double m = block_max(v, red, slot);
    if (isinf(m)) return m;
    const double s = block_sum(exp(v - m), red, slot);
    return m + log(s);
}

// One step of either recursion for one row: (value, accuracy) over the row's list.  `from` holds the published pairs of the neighbouring
// frame; idx / val are the row's list (registers for KREG > 0, the batch's arrays from k0 to k1 otherwise).
template <int KREG>
__device__ __forceinline__ void mbr_step(const double2 *__restrict__ from, const int *ridx, const double *rval, const int *__restrict__ gidx,
                                         const double *__restrict__ gval, int k0, int k1, double &value, double &accuracy) {
    constexpr int KR = KREG > 0 ? KREG : 1;
    double m = -INFINITY, s = 0.0, sp = 0.0;
    if (KREG > 0) {
        double v[KR], y[KR];
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            const double2 e = from[ridx[k]];
            v[k] = e.x + rval[k];
            y[k] = e.y;
            m = fmax(m, v[k]);
        }
        if (!isinf(m)) {
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                const double e = exp(v[k] - m);                    // a padded entry: exp(-inf) = 0
                s = s + e;
                sp = sp + e * y[k];
            }
        }
    } else {
        for (int k = k0; k < k1; ++k) m = fmax(m, from[gidx[k]].x + gval[k]);
        if (!isinf(m)) {
            for (int k = k0; k < k1; ++k) {
                const double2 f = from[gidx[k]];
                const double e = exp(f.x + gval[k] - m);
                s = s + e;
                sp = sp + e * f.y;
            }
        }
    }
    if (isinf(m)) {                                                // nothing arrives (or quirk Q4): no path, no accuracy
        value = m;
        accuracy = 0.0;
    } else {
        value = m + log(s);
        accuracy = sp / s;
    }
}

template <int KREG>
__global__ __launch_bounds__(64 * MBR_MAXW) void hmm_mbr_kernel(const MbrArgs a) {
    constexpr int KR = KREG > 0 ? KREG : 1;
    extern __shared__ __attribute__((aligned(16))) double2 mbr_lds[];
    const UttDesc d = a.utts[blockIdx.x];
    const int N = d.N, T = d.T, NP = blockDim.x;
    double2 *vec0 = mbr_lds, *vec1 = mbr_lds + NP;                 // (value, accuracy) of even / odd frames
    double *red = reinterpret_cast<double *>(mbr_lds + 2 * NP);
    const int i = threadIdx.x;
    const bool act = i < N;
    int slot = 0;

    const double *B = a.Bt + d.b_off;
    double *Be = a.beta + d.b_off, *Bp = a.betap + d.b_off, *G = a.lgam + d.b_off, *Gr = a.g + d.b_off;
    const int32_t *ref = a.ref_group + d.path_off;
    const double kappa = a.kappa;

    int pc0 = 0, pc1 = 0, sr0 = 0, sr1 = 0, mine = -1;             // mine: this row's group (-1: entry / exit row, never accurate)
    double lpi = -INFINITY;
    if (act) {
        pc0 = a.col_ptr[d.ptr_off + i] + d.nnz_off;
        pc1 = a.col_ptr[d.ptr_off + i + 1] + d.nnz_off;
        sr0 = a.row_ptr[d.ptr_off + i] + d.nnz_off;
        sr1 = a.row_ptr[d.ptr_off + i + 1] + d.nnz_off;
        const int rs = a.row_state[d.vec_off + i];
        mine = rs >= 0 ? rs / a.group : -1;
        lpi = a.logpi[d.vec_off + i];
    }
    int pidx[KR], sidx[KR];
    double pval[KR], sval[KR];
    if (KREG > 0) {
        const int npred = pc1 - pc0, nsucc = sr1 - sr0;
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            pidx[k] = (k < npred) ? a.row_idx[pc0 + k] : 0;
            pval[k] = (k < npred) ? a.csc_val[pc0 + k] : -INFINITY;
            sidx[k] = (k < nsucc) ? a.col_idx[sr0 + k] : 0;
            sval[k] = (k < nsucc) ? a.csr_val[sr0 + k] : -INFINITY;
        }
    }

    // ---------------------------------------------------------------- backward: beta, beta', stored
    // what a row publishes for step t is  (bs_i(t+1) + beta_{t+1}(i),  beta'_{t+1}(i) + A_{t+1}(i))
    {
        double be = 0.0, bp = 0.0;                                 // beta_{T-1} = 0 (quirk Q8), beta'_{T-1} = 0
        if (act) {
            Be[(long long)(T - 1) * N + i] = 0.0;
            Bp[(long long)(T - 1) * N + i] = 0.0;
        }
        double b_t = act ? B[(long long)(T - 1) * N + i] : 0.0;   // B[i, t+1] and ref[t+1] of the step about to run
        int r_t = ref[T - 1];
        for (int t = T - 2; t >= 0; --t) {
            double2 *cur = ((t + 1) & 1) ? vec1 : vec0;
            const double acc = (mine >= 0 && mine == r_t) ? 1.0 : 0.0;
            cur[i] = act ? make_double2(kappa * b_t + be, bp + acc) : make_double2(-INFINITY, 0.0);
            if (act) b_t = B[(long long)t * N + i];               // the next step's row, in flight during this one
            r_t = ref[t];
            __syncthreads();                                       // (one barrier per step: a buffer is written again two barriers after its last read)
            if (act) {
                mbr_step<KREG>(cur, sidx, sval, a.col_idx, a.csr_val, sr0, sr1, be, bp);
                Be[(long long)t * N + i] = be;
                Bp[(long long)t * N + i] = bp;
            }
        }
    }
    __syncthreads();                                               // everyone is done reading the backward vectors

    // ---------------------------------------------------------------- forward: alpha, alpha' in LDS; ln gamma and g as it goes
    double al = -INFINITY, ap = 0.0, c_avg = 0.0;
    double b_n = act ? B[i] : 0.0, be_n = act ? Be[i] : 0.0, bp_n = act ? Bp[i] : 0.0;
    int r_n = ref[0];
    for (int t = 0; t < T; ++t) {
        const double2 *prev = (t & 1) ? vec0 : vec1;
        double2 *cur = (t & 1) ? vec1 : vec0;
        const double b_t = b_n, be = be_n, bp = bp_n;
        const int r_t = r_n;
        if (t + 1 < T) {                                           // the next step's rows, in flight during this one
            if (act) {
                b_n = B[(long long)(t + 1) * N + i];
                be_n = Be[(long long)(t + 1) * N + i];
                bp_n = Bp[(long long)(t + 1) * N + i];
            }
            r_n = ref[t + 1];
        }
        const double acc = (mine >= 0 && mine == r_t) ? 1.0 : 0.0;
        if (act) {
            if (t == 0) {
                al = lpi + kappa * b_t;
                ap = acc;
            } else {
                double r, y;
                mbr_step<KREG>(prev, pidx, pval, a.row_idx, a.csc_val, pc0, pc1, r, y);
                al = r + kappa * b_t;
                ap = (al == -INFINITY) ? 0.0 : y + acc;
            }
        }
        cur[i] = act ? make_double2(al, ap) : make_double2(-INFINITY, 0.0);
        const double l = act ? al + be : -INFINITY;
        const double norm = block_lse(l, red, slot);
        const double lg = l - norm;
        const double gam = exp(lg);
        const double both = ap + bp;
        if (t == 0) c_avg = block_sum((act && gam > 0.0) ? gam * both : 0.0, red, slot);
        if (act) {
            G[(long long)t * N + i] = lg;
            Gr[(long long)t * N + i] = (gam > 0.0) ? kappa * gam * (both - c_avg) : 0.0;
        }
        __syncthreads();
    }
    const double lp = block_lse(act ? al : -INFINITY, red, slot);  // ln P = LSE_j alpha_{T-1}(j)
    if (i == 0) {
        a.logp[blockIdx.x] = lp;
        a.cavg[blockIdx.x] = c_avg;
    }
}

// which = 0: ln gamma; +1: ln max(g, 0); -1: ln max(-g, 0) -- into the batch's lgam, the layout the accumulate pass reads
__global__ __launch_bounds__(256) void mbr_post_kernel(const double *__restrict__ lg, const double *__restrict__ g, double *__restrict__ out,
                                                       long long n, int which) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        if (which == 0) {
            out[e] = lg[e];
        } else {
            const double v = which > 0 ? g[e] : -g[e];
            out[e] = v > 0.0 ? log(v) : -INFINITY;
        }
    }
}

}  // namespace

// The pass's buffers, the batch's own (BatchMbrDev): made on first use, kept for the next call.
int pcl_mbr_reserve(pcl_ctx *ctx, pcl_batch *b) {
    const size_t nt = (size_t)b->shape.sumNT;
    TRY(b->mbr_beta.reserve(ctx, nt));
    TRY(b->mbr_betap.reserve(ctx, nt));
    TRY(b->mbr_lgam.reserve(ctx, nt));
    TRY(b->mbr_g.reserve(ctx, nt));
    TRY(b->mbr_logp.reserve(ctx, (size_t)b->U));
    TRY(b->mbr_cavg.reserve(ctx, (size_t)b->U));
    TRY(b->mbr_ref.reserve(ctx, (size_t)b->shape.sumT));
    return PCL_OK;
}

int pcl_mbr_max_rows() { return 64 * MBR_MAXW; }

int pcl_launch_mbr(pcl_ctx *ctx, pcl_batch *b, double kappa, int group) {
    const int NP = (b->shape.Nmax + 63) / 64 * 64;
    if (NP > 64 * MBR_MAXW) PCL_FAIL(ctx, PCL_ERR_INVALID, "HMM with %d states exceeds the %d-state limit", b->shape.Nmax, 64 * MBR_MAXW);
    const size_t shm = (size_t)2 * NP * sizeof(double2) + (size_t)2 * MBR_MAXW * sizeof(double);   // 32.25 KiB at 1024 rows
    const MbrArgs a{b->d_utt, b->Bt, b->row_ptr, b->col_idx, b->csr_val, b->col_ptr, b->row_idx, b->csc_val, b->logpi, b->d_row_state, b->mbr_ref,
                    b->mbr_beta, b->mbr_betap, b->mbr_lgam, b->mbr_g, b->mbr_logp, b->mbr_cavg, kappa, group};
    pcl_timer_begin(ctx, "mbr");
    if (b->trans.max_indeg <= 2 && b->trans.max_outdeg <= 2)
        hipLaunchKernelGGL(hmm_mbr_kernel<2>, dim3(b->U), dim3(NP), shm, ctx->stream, a);
    else
        hipLaunchKernelGGL(hmm_mbr_kernel<0>, dim3(b->U), dim3(NP), shm, ctx->stream, a);
    pcl_timer_end(ctx, "mbr");
    HIPCHK(ctx, hipGetLastError());
    return PCL_OK;
}

int pcl_launch_mbr_posteriors(pcl_ctx *ctx, pcl_batch *b, int which) {
    const long long n = b->shape.sumNT;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 2048);
    pcl_timer_begin(ctx, "mbr_post");
    if (blocks > 0) hipLaunchKernelGGL(mbr_post_kernel, dim3(blocks), dim3(256), 0, ctx->stream, b->mbr_lgam, b->mbr_g, b->lgam, n, which);
    pcl_timer_end(ctx, "mbr_post");
    HIPCHK(ctx, hipGetLastError());
    return PCL_OK;
}
