// What fMLLR (frame_adapt.hip, row f11) and MLLT (frame_mllt.hip, row f13) share on the frame side: the reduction over rows and mixtures
// that gives every frame its p_i(t), q_i(t), beta(t), the sum of beta per group, the occupancy and pivot statuses, the Gauss-Jordan
// inversion, and the row-by-row sweeps.  The two rules differ at compile time (template parameter MLLT): an instantiation is compiled in
// the translation unit that launches it, so frame_adapt.hip holds the MLLT = false kernels and frame_mllt.hip the MLLT = true ones.  The
// three small kernels that are no templates (fmllr_beta_kernel, fmllr_occ_kernel, fmllr_pivot_kernel) are launched by both files and are
// emitted into both objects.
// Included inside the including file's unnamed namespace, after adapt_common.h; built with -ffp-contract=off.
#pragma once

constexpr int FT = 64;                        // frames per tile of the reduction: one per lane

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
            chol_solve_lds([&](int r, int c) -> double & { return Ls[r][c]; }, [&](int r) -> double & { return vv[r]; }, n, tid);   // L y = p, L^T v = y
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
