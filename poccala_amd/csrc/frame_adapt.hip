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
#include <math.h>

#include "pcl_internal.h"

namespace {

#include "adapt_common.h"

constexpr int FT = 64;                        // frames per tile of the reduction: one per lane
constexpr int APPLY_TF = 32;                  // frames per workgroup of the apply kernel

// ---------------------------------------------------------------- the frame-side reduction
// One workgroup (4 waves) per (utterance, 64-frame tile).  Lane l of every wave owns frame t0 + l; wave w takes the mixtures m = w, w + 4, ...
// of every GMM row of the utterance, rows in ascending order, and keeps its partial sums of all 2 D + 1 outputs in registers.  The four
// waves' partials are then added through LDS in wave order: ((w0 + w1) + w2) + w3.  The posterior is gmm_accumulate_kernel's float64 form
// on the scoring row [s_d c_d .. k2] (s = sqrt(log2 e / (2 var)), c = -mu s, log2 domain):
//     g = exp2((k2 - sum_d (x_d s_d + c_d)^2) + (ln gamma_t(row) - ln b_t(row)) log2 e)
// and 1 / var = 2 ln2 s^2, mu / var = -2 ln2 c s are taken from the same row: sum g s^2 and sum g c s are accumulated and scaled once.
// DP = the model's padded device dimension (its rows hold s = c = 0 beyond D).  NH = 2 (D >= 39): blockIdx.z picks the half of the feature
// dimensions whose sums the workgroup keeps -- all 2 D + 1 sums of a frame beside the posterior's operands need more than 256 VGPRs per lane,
// and hipcc's AGPR spill code for 64-bit values is what gmm_accumulate_kernel's float64 path had to avoid; each half forms the posterior
// itself, with the same bits.  Outputs at the frame's VIRTUAL index v = vbase[u] + t (the call's frames in speaker order): P[v][i], Q[v][i], B[v], vrow[v] = its row.
// MLLT (compile time; row f13, frame_mllt.hip): the same reduction without q -- a frame's D + 1 sums fit the registers, so NH = 1 -- and
// with a mask over the states: a row whose state has keep[j] == 0 is passed over like an entry row.  MLLT = false does not read `keep`.
// The MLLT = true instantiations are compiled in a translation unit of their own (frame_mllt.hip defines PCL_FRAME_MLLT and includes this
// file), so the fMLLR kernels come out as they did before there was a switch.
template <bool MLLT>
struct MlltKeep {};
template <>
struct MlltKeep<true> {
    const int32_t *keep;                      // J entries, or nullptr = every state
};
template <int DP, int NH, bool MLLT>
__global__ __launch_bounds__(256) void fmllr_frames_kernel(const UttDesc *__restrict__ utt, const int32_t *__restrict__ row_state,
                                                           const int *__restrict__ vbase, const double *__restrict__ Bt,
                                                           const double *__restrict__ lgam, const double *__restrict__ x64,
                                                           const float *__restrict__ x32, int FD, const double *__restrict__ params,
                                                           int prow, const double *__restrict__ w64, int M, int Mpad, int Dh,
                                                           double *__restrict__ P, double *__restrict__ Q, double *__restrict__ Bv,
                                                           long long *__restrict__ vrow, MlltKeep<MLLT> mk) {
    constexpr int DH = (DP + NH - 1) / NH, NOUT = (MLLT ? DH : 2 * DH) + 1;
    static_assert(!MLLT || NH == 1, "without q one workgroup keeps every sum of its frames");
    static_assert(2 * (NH * DH) <= (2 * DP + 1 + 3) / 4 * 4, "the last half may read the row's constant and padding as if they were s and c (never stored)");
    static_assert(NOUT >= DP, "the frames share the sums' LDS");
    const int d0 = blockIdx.z * DH;
    __shared__ double sh[NOUT * FT];                             // first the tile's frames xs[d][lane], then the waves' sum
    const int u = blockIdx.y, vb = vbase[u];
    if (vb < 0) return;                                          // (uniform)
    const UttDesc ud = utt[u];
    const int t0 = blockIdx.x * FT;
    if (t0 >= ud.T) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = t0 + lane;
    const bool valid = t < ud.T;
    for (int e = tid; e < FT * DP; e += 256) {                   // (the padded dimensions hold 0, as their s and c do)
        const int f = e / DP, d = e - f * DP;
        double x = 0.0;
        if (d < Dh && t0 + f < ud.T) {
            const size_t at = (size_t)(ud.frame0 + t0 + f) * FD + d;
            x = x64 ? x64[at] : (double)x32[at];
        }
        sh[d * FT + f] = x;
    }
    __syncthreads();
    constexpr double LOG2E = 1.4426950408889634074;
    double ap[DH], aq[DH], ab = 0.0;
#pragma unroll
    for (int d = 0; d < DH; ++d) ap[d] = aq[d] = 0.0;
    for (int n = 0; n < ud.N; ++n) {
        const int j = __builtin_amdgcn_readfirstlane(row_state[ud.vec_off + n]);
        if (j < 0) continue;                                      // entry / exit rows
        if constexpr (MLLT)
            if (mk.keep && mk.keep[j] == 0) continue;             // (uniform: j is)
        double cf = -INFINITY;
        if (valid) {
            const double lg = lgam[ud.b_off + (long long)t * ud.N + n], lb = Bt[ud.b_off + (long long)t * ud.N + n];
            if (lg > -INFINITY && lb > -INFINITY) cf = (lg - lb) * LOG2E;
        }
        if (__ballot(cf > -INFINITY) == 0ull) continue;           // (uniform in the wave; adding exact zeros would change no bit)
        for (int m = wave; m < M; m += 4) {
            const size_t jm = (size_t)j * Mpad + m;
            const double wt = w64[jm];
            if (!(wt > 0.0 && wt < INFINITY)) continue;           // weight 0 / not finite: contributes exactly nothing
            const double *__restrict__ pr = params + jm * prow;
            double q = 0.0;
#pragma unroll
            for (int d = 0; d < DP; ++d) {
                const double y = __builtin_fma(sh[d * FT + lane], pr[2 * d], pr[2 * d + 1]);
                q = __builtin_fma(y, y, q);
            }
            const double g = exp2((pr[2 * DP] - q) + cf);
            ab += g;
#pragma unroll
            for (int d = 0; d < DH; ++d) {
                const double gs = g * pr[2 * (d0 + d)];
                ap[d] = __builtin_fma(gs, pr[2 * (d0 + d)], ap[d]);
                if constexpr (!MLLT) aq[d] = __builtin_fma(gs, pr[2 * (d0 + d) + 1], aq[d]);
            }
        }
    }
    // the waves' sums, in wave order
    for (int w = 0; w < 4; ++w) {
        __syncthreads();                                          // (the first one: every wave is done with the frames in sh)
        if (wave == w) {
            if (w == 0) {
#pragma unroll
                for (int d = 0; d < DH; ++d) {
                    sh[d * FT + lane] = ap[d];
                    if constexpr (!MLLT) sh[(DH + d) * FT + lane] = aq[d];
                }
                sh[(NOUT - 1) * FT + lane] = ab;
            } else {
#pragma unroll
                for (int d = 0; d < DH; ++d) {
                    ap[d] = sh[d * FT + lane] + ap[d];
                    if constexpr (!MLLT) aq[d] = sh[(DH + d) * FT + lane] + aq[d];
                }
                ab = sh[(NOUT - 1) * FT + lane] + ab;
                if (w < 3) {
#pragma unroll
                    for (int d = 0; d < DH; ++d) {
                        sh[d * FT + lane] = ap[d];
                        if constexpr (!MLLT) sh[(DH + d) * FT + lane] = aq[d];
                    }
                    sh[(NOUT - 1) * FT + lane] = ab;
                }
            }
        }
    }
    if (wave == 3 && valid) {
        constexpr double TWO_LN2 = 1.3862943611198906188;
        const size_t v = (size_t)vb + t;
#pragma unroll
        for (int d = 0; d < DH; ++d)
            if (d0 + d < Dh) {
                P[v * Dh + d0 + d] = TWO_LN2 * ap[d];
                if constexpr (!MLLT) Q[v * Dh + d0 + d] = -(TWO_LN2 * aq[d]);
            }
        if (blockIdx.z == 0) {
            Bv[v] = ab;
            vrow[v] = ud.frame0 + t;
        }
    }
}

// beta[s] += sum of B over the speaker's virtual frames [spk_v0[s], spk_v0[s + 1]): thread t adds its frames t, t + 256, .. in ascending
// order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void fmllr_beta_kernel(const double *__restrict__ Bv, const int *__restrict__ spk_v0, double *__restrict__ beta) {
    __shared__ double so[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    double o = 0.0;
    for (int v = spk_v0[s] + tid; v < spk_v0[s + 1]; v += 256) o += Bv[v];
    so[tid] = o;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) so[tid] += so[tid + w];
        __syncthreads();
    }
    if (tid == 0 && spk_v0[s + 1] > spk_v0[s]) beta[s] = beta[s] + so[0];
}

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

// ---------------------------------------------------------------- the estimate
// Before any factorisation: status = LOW_OCCUPANCY where beta < min_occ
__global__ void fmllr_occ_kernel(const double *__restrict__ beta, int S, double min_occ, int *__restrict__ status) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) status[s] = beta[s] < min_occ ? PCL_FMLLR_LOW_OCCUPANCY : PCL_FMLLR_OK;
}
// ... and after them: a failed pivot in any of the speaker's D factorisations
__global__ void fmllr_pivot_kernel(const int *__restrict__ pivot_bad, int S, int Dh, int *__restrict__ status) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S || status[s] != PCL_FMLLR_OK) return;
    for (int i = 0; i < Dh; ++i)
        if (pivot_bad[s * Dh + i]) {
            status[s] = PCL_FMLLR_NOT_POSITIVE_DEFINITE;
            return;
        }
}

// In-place Gauss-Jordan inversion with row pivoting of the Dh x Dh matrix Ai (LDS, one wave, lane c owns column c); the header states the
// steps.  -> false: a pivot is 0 or not finite.  *logdet = sum ln |pivot|.
constexpr int LDA = ADAPT_D_MAX + 1;
__device__ bool invert_in_place(double (*Ai)[LDA], int Dh, double *colk, int *perm, double *logdet) {
    const int c = threadIdx.x;
    double ld = 0.0;
    bool ok = true;
    for (int k = 0; k < Dh; ++k) {
        int r = k;                                                // (every lane scans the same values: uniform)
        double best = fabs(Ai[k][k]);
        for (int q = k + 1; q < Dh; ++q) {
            const double v = fabs(Ai[q][k]);
            if (v > best) {
                best = v;
                r = q;
            }
        }
        __syncthreads();
        if (c == 0) perm[k] = r;
        if (r != k && c < Dh) {
            const double tmp = Ai[k][c];
            Ai[k][c] = Ai[r][c];
            Ai[r][c] = tmp;
        }
        __syncthreads();
        const double piv = Ai[k][k];
        if (!(fabs(piv) > 0.0 && fabs(piv) < INFINITY)) {
            ok = false;
            break;
        }
        ld = ld + log(fabs(piv));
        if (c < Dh) colk[c] = Ai[c][k];                           // column k before it is rewritten (lane c copies row c's element)
        __syncthreads();
        if (c < Dh) {
            const double rk = (c == k ? 1.0 : Ai[k][c]) / piv;
            for (int q = 0; q < Dh; ++q) {
                if (q == k) continue;
                const double old = c == k ? 0.0 : Ai[q][c];
                Ai[q][c] = old - colk[q] * rk;
            }
            Ai[k][c] = rk;
        }
        __syncthreads();
    }
    if (ok)
        for (int k = Dh - 1; k >= 0; --k) {                       // the row swaps become column swaps of the inverse, undone in reverse
            const int r = perm[k];
            if (r != k && c < Dh) {                               // (lane c owns ROW c here)
                const double tmp = Ai[c][k];
                Ai[c][k] = Ai[c][r];
                Ai[c][r] = tmp;
            }
            __syncthreads();
        }
    *logdet = ld;
    return ok;
}

// One wave per speaker: the sweeps, in LDS.  L[s][i] (the Cholesky factor of G[s,i]) is staged per row update; Gk is read through L2 for Q.
// MLLT (compile time; row f13): the same sweeps with k = 0 and no offset column -- W is the square A (n = D), G[s,i] is D x D with no k
// column behind its rows, g = G^-1 k is 0 and is not read -- and a trace of n_iter + 1 entries whose first is Q at the start, A = I.
// Instantiated in frame_mllt.hip, as the frame reduction's MLLT form is.
template <bool MLLT>
__global__ __launch_bounds__(64) void fmllr_sweep_kernel(const double *__restrict__ Gk, const double *__restrict__ Lall, const double *__restrict__ gkall,
                                                         const double *__restrict__ beta_all, int Dh, int n_iter, int *__restrict__ status,
                                                         double *__restrict__ W_out, double *__restrict__ logdet_out, double *__restrict__ qtrace) {
    __shared__ double Ls[LDA][LDA + 1], Ai[ADAPT_D_MAX][LDA], Wl[ADAPT_D_MAX][LDA + 1];
    __shared__ double vv[64], pv[64], gki[64], wn[64], ucol[64], zrow[64], colk[64];
    __shared__ int perm[64];
    constexpr int O = MLLT ? 0 : 1;                               // columns in front of A in a row of W
    const int s = blockIdx.x, n = Dh + O, gs = MLLT ? n : n + 1, nq = MLLT ? n_iter + 1 : n_iter, tid = threadIdx.x;
    int st = status[s];
    const double beta = beta_all[s];
    double logdet = 0.0;
    for (int x = tid; x < Dh * n; x += 64) Wl[x / n][x % n] = (x % n == x / n + O) ? 1.0 : 0.0;
    for (int x = tid; x < Dh * Dh; x += 64) Ai[x / Dh][x % Dh] = (x % Dh == x / Dh) ? 1.0 : 0.0;
    __syncthreads();
    for (int it = MLLT ? -1 : 0; it < n_iter && st == PCL_FMLLR_OK; ++it) {   // (MLLT: pass -1 only forms Q of the start)
        for (int i = 0; it >= 0 && i < Dh && st == PCL_FMLLR_OK; ++i) {
            const size_t pair = (size_t)s * Dh + i;
            for (int x = tid; x < n * n; x += 64) Ls[x / n][x % n] = Lall[pair * n * n + x];
            if (tid < n) {
                const double p = (O && tid == 0) ? 0.0 : Ai[tid - O][i];   // p = (0, column i of A^-1)
                pv[tid] = p;
                vv[tid] = p;
                gki[tid] = MLLT ? 0.0 : gkall[pair * n + tid];
                if (tid >= O) ucol[tid - O] = p;
            }
            __syncthreads();
            for (int j = 0; j < n; ++j) {                         // L y = p
                const double y = vv[j] / Ls[j][j];
                __syncthreads();
                if (tid == j) vv[j] = y;
                else if (tid > j && tid < n) vv[tid] -= Ls[tid][j] * y;
                __syncthreads();
            }
            for (int j = n - 1; j >= 0; --j) {                    // L^T v = y
                const double v = vv[j] / Ls[j][j];
                __syncthreads();
                if (tid == j) vv[j] = v;
                else if (tid < j) vv[tid] -= Ls[j][tid] * v;
                __syncthreads();
            }
            double a = 0.0, c = 0.0;                              // (every lane: the same sums in ascending order)
            for (int q = 0; q < n; ++q) {
                a = a + pv[q] * vv[q];
                c = c + pv[q] * gki[q];
            }
            const double disc = c * c + 4.0 * a * beta;
            if (!(a > 0.0 && a < INFINITY) || !(disc >= 0.0 && disc < INFINITY)) {
                st = PCL_FMLLR_SINGULAR;
                break;
            }
            const double sq = sqrt(disc);
            const double a1 = (-c + sq) / (2.0 * a), a2 = (-c - sq) / (2.0 * a);
            const double f1 = beta * log(fabs(a1 * a + c)) - 0.5 * a * a1 * a1, f2 = beta * log(fabs(a2 * a + c)) - 0.5 * a * a2 * a2;
            const double alpha = (f1 >= f2 || !(f2 == f2)) ? a1 : a2;                              // ties go to the + root
            if (!(fabs(alpha) < INFINITY)) {
                st = PCL_FMLLR_SINGULAR;
                break;
            }
            if (tid < n) wn[tid] = alpha * vv[tid] + gki[tid];
            __syncthreads();
            double denom = 0.0;                                   // w_new . (column i of A^-1) = det A_new / det A
            for (int q = 0; q < Dh; ++q) denom = denom + wn[O + q] * ucol[q];
            if (!(fabs(denom) > 0.0 && fabs(denom) < INFINITY)) {
                st = PCL_FMLLR_SINGULAR;
                break;
            }
            if (tid < Dh) {                                       // z = (w_new - w_old) A^-1, then A^-1 <- A^-1 - u z / denom
                double z = 0.0;
                for (int q = 0; q < Dh; ++q) z = z + (wn[O + q] - Wl[i][O + q]) * Ai[q][tid];
                zrow[tid] = z / denom;
            }
            __syncthreads();
            if (tid < Dh)
                for (int q = 0; q < Dh; ++q) Ai[q][tid] = Ai[q][tid] - ucol[q] * zrow[tid];
            if (tid < n) Wl[i][tid] = wn[tid];
            __syncthreads();
        }
        if (st != PCL_FMLLR_OK) break;
        if (it >= 0) {
            for (int x = tid; x < Dh * Dh; x += 64) Ai[x / Dh][x % Dh] = Wl[x / Dh][O + x % Dh];   // the full re-inversion that ends every sweep
            __syncthreads();
            if (!invert_in_place(Ai, Dh, colk, perm, &logdet)) {
                st = PCL_FMLLR_SINGULAR;
                break;
            }
        }
        double quad = 0.0;                                        // Q = beta ln|det A| - 1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T)
        for (int i = 0; i < Dh; ++i) {
            const double *G = Gk + ((size_t)s * Dh + i) * n * gs;
            __syncthreads();
            if (tid < n) {
                double t = 0.0;
                for (int q = 0; q < n; ++q) t = t + G[tid * gs + q] * Wl[i][q];
                vv[tid] = MLLT ? Wl[i][tid] * t : Wl[i][tid] * t - 2.0 * (Wl[i][tid] * G[tid * gs + n]);
            }
            __syncthreads();
            for (int q = 0; q < n; ++q) quad = quad + vv[q];
        }
        if (tid == 0) qtrace[(size_t)s * nq + it + (MLLT ? 1 : 0)] = beta * logdet - 0.5 * quad;
    }
    __syncthreads();
    // statuses are decided: now, and only now, the outputs are written
    if (tid == 0) {
        status[s] = st;
        logdet_out[s] = st == PCL_FMLLR_OK ? logdet : 0.0;
    }
    if (st != PCL_FMLLR_OK)
        for (int x = tid; x < nq; x += 64) qtrace[(size_t)s * nq + x] = NAN;
    for (int x = tid; x < Dh * n; x += 64)
        W_out[(size_t)s * Dh * n + x] = st == PCL_FMLLR_OK ? Wl[x / n][x % n] : ((x % n == x / n + O) ? 1.0 : 0.0);
}

#ifndef PCL_FRAME_MLLT
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
#endif  // PCL_FRAME_MLLT

}  // namespace

#ifndef PCL_FRAME_MLLT
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

// pcl_batch_accumulate_fmllr behind its checks of the batch (pcl_api.hip): the batch has emissions, posteriors and states, is joined, fits
// the current frames and model, and the scoring rows (PCL_LAYOUT_P64) are derived
int pcl_launch_fmllr_accumulate(pcl_ctx *ctx, pcl_batch *b, const int32_t *utt_speaker) {
    const char *who = "pcl_batch_accumulate_fmllr";
    if (const char *why = fmllr_ready(ctx)) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: %s", who, why);
    if (!utt_speaker) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utt_speaker is NULL", who);
    const int S = ctx->fmllr_S, U = b->U, Dh = ctx->Dhost;
    for (int u = 0; u < U; ++u) {
        if (utt_speaker[u] < -1 || utt_speaker[u] >= S)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d has speaker %d, outside [-1, %d)", who, u, (int)utt_speaker[u], S);
        if (utt_speaker[u] >= 0 && b->utt[u].frame0 < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d has no frames (the batch was made without frame_begin)", who, u);
    }
    // virtual frame order: speakers ascending, a speaker's utterances in batch order; a speaker's frames cut into chunks
    const long long chunk = std::min<long long>(mllr_chunk(), 1 << 30);
    std::vector<int> vbase(U, -1), spk_v0(S + 1, 0), spk_chunk0(S + 1, 0), chunk_v0, chunk_n;
    long long V = 0;
    for (int s = 0; s < S; ++s) {
        spk_v0[s] = (int)V;
        for (int u = 0; u < U; ++u)
            if (utt_speaker[u] == s) {
                vbase[u] = (int)V;
                V += b->utt[u].T;
            }
        for (long long v0 = spk_v0[s]; v0 < V; v0 += chunk) {
            chunk_v0.push_back((int)v0);
            chunk_n.push_back((int)std::min(chunk, V - v0));
        }
        spk_chunk0[s + 1] = (int)chunk_v0.size();
    }
    spk_v0[S] = (int)V;                                           // (V <= sum T < 2^31: pcl_batch_create)
    if (V == 0) return PCL_OK;
    const int C = (int)chunk_v0.size();
    const int NT = (Dh + 2 + 15) / 16, ntiles = NT * (NT + 1) / 2;
    if ((long long)C * Dh > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %d chunks x %d dimensions do not fit a grid: raise PCL_MLLR_CHUNK", who, C, Dh);
    std::vector<int> lists;                                       // one upload: [vbase | spk_v0 | spk_chunk0 | chunk_v0 | chunk_n]
    const size_t o_v0 = U, o_chunk0 = o_v0 + S + 1, o_cv0 = o_chunk0 + S + 1, o_cn = o_cv0 + C;
    lists.insert(lists.end(), vbase.begin(), vbase.end());
    lists.insert(lists.end(), spk_v0.begin(), spk_v0.end());
    lists.insert(lists.end(), spk_chunk0.begin(), spk_chunk0.end());
    lists.insert(lists.end(), chunk_v0.begin(), chunk_v0.end());
    lists.insert(lists.end(), chunk_n.begin(), chunk_n.end());

    hipStream_t st = ctx->stream;
    DevBuf<int> d_lists;
    DevBuf<double> d_P, d_Q, d_B, d_partial;
    DevBuf<long long> d_vrow;
    TRY(d_lists.alloc(ctx, lists.size()));
    TRY(d_P.alloc(ctx, (size_t)V * Dh));
    TRY(d_Q.alloc(ctx, (size_t)V * Dh));
    TRY(d_B.alloc(ctx, (size_t)V));
    TRY(d_vrow.alloc(ctx, (size_t)V));
    TRY(d_partial.alloc(ctx, (size_t)C * Dh * ntiles * 256));
    HIPCHK(ctx, pcl_h2d(ctx, d_lists, lists.data(), lists.size() * sizeof(int)));

    pcl_timer_begin(ctx, "fmllr");                               // the whole call's kernels; "fmllr_frames" / "fmllr_gk": its two halves
    pcl_timer_begin(ctx, "fmllr_frames");
    {
        const unsigned tiles = (unsigned)((b->Tmax + FT - 1) / FT);
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
    hipLaunchKernelGGL(fmllr_beta_kernel, dim3(S), dim3(256), 0, st, d_B, d_lists + o_v0, ctx->fmllr_beta);
    pcl_timer_end(ctx, "fmllr_frames");
    pcl_timer_begin(ctx, "fmllr_gk");
    FrameSrc g{ctx->frames64, ctx->frames32, d_vrow, d_P, d_Q, d_lists + o_cv0, d_lists + o_cn, ctx->FD, Dh};
    launch_gk(mllr_use_valu(), NT, C * Dh, st, g, d_partial);
    hipLaunchKernelGGL(gk_reduce_kernel, dim3(S * Dh), dim3(256), 0, st, d_partial, d_lists + o_chunk0, Dh, NT, ctx->fmllr_Gk, true);
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
    if (!ctx->frames32 || ctx->F <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no frames loaded", who);
    if (U < 1 || U > 65535 || !T || !frame_begin || !utt_speaker) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: U = %d utterances (1 .. 65535), or a NULL argument", who, U);
    const int Dh = ctx->FDhost, n = Dh + 1;
    if (Dh > ADAPT_D_MAX) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d, the kernel holds at most %d", who, Dh, ADAPT_D_MAX);
    if (S < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: S = %d speakers, need at least 1", who, S);
    if (!W && (!ctx->fmllr_W || ctx->fmllr_S != S || ctx->Dhost != Dh))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: W is NULL and the context holds no estimate of %d speakers in %d dimensions (pcl_fmllr_estimate first)", who, S, Dh);
    std::vector<std::pair<long long, long long>> spans;
    int Tmax = 0;
    for (int u = 0; u < U; ++u) {
        if (utt_speaker[u] < -1 || utt_speaker[u] >= S) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d has speaker %d, outside [-1, %d)", who, u, (int)utt_speaker[u], S);
        if (T[u] < 0 || frame_begin[u] < 0 || frame_begin[u] + T[u] > ctx->F)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d covers rows [%lld, %lld) of a frame matrix of %lld rows", who, u, (long long)frame_begin[u],
                     (long long)frame_begin[u] + T[u], (long long)ctx->F);
        if (T[u] > 0) spans.emplace_back((long long)frame_begin[u], (long long)frame_begin[u] + T[u]);
        Tmax = std::max(Tmax, (int)T[u]);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); ++i)
        if (spans[i].first < spans[i - 1].second)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the utterances overlap in the frame matrix at row %lld (a frame is transformed ONCE)", who, spans[i].first);
    if (Tmax == 0) return PCL_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<long long> begin(frame_begin, frame_begin + U);
    DevBuf<int> d_T, d_spk, d_skip;
    DevBuf<long long> d_begin;
    DevBuf<double> d_W;
    TRY(d_T.alloc(ctx, (size_t)U));
    TRY(d_spk.alloc(ctx, (size_t)U));
    TRY(d_skip.alloc(ctx, (size_t)S));
    TRY(d_begin.alloc(ctx, (size_t)U));
    HIPCHK(ctx, pcl_h2d(ctx, d_T, T, (size_t)U * sizeof(int32_t)));
    HIPCHK(ctx, pcl_h2d(ctx, d_spk, utt_speaker, (size_t)U * sizeof(int32_t)));
    HIPCHK(ctx, pcl_h2d(ctx, d_begin, begin.data(), (size_t)U * sizeof(long long)));
    if (W) {
        TRY(d_W.alloc(ctx, (size_t)S * Dh * n));
        HIPCHK(ctx, pcl_h2d(ctx, d_W, W, (size_t)S * Dh * n * sizeof(double)));
    }
    const double *dW = W ? d_W.p : ctx->fmllr_W.p;
    pcl_timer_begin(ctx, "fmllr");
    hipLaunchKernelGGL(gk_identity_kernel, dim3(S), dim3(64), 0, st, dW, Dh, d_skip);
    hipLaunchKernelGGL(fmllr_apply_kernel, dim3((unsigned)((Tmax + APPLY_TF - 1) / APPLY_TF), (unsigned)U), dim3(256), 0, st, d_T, d_begin, d_spk, dW, d_skip,
                       ctx->frames64.p, ctx->frames32, ctx->FD, Dh);
    pcl_timer_end(ctx, "fmllr");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    return PCL_OK;
}
#endif  // PCL_FRAME_MLLT
