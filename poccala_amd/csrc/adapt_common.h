// What the adaptation files share (model_adapt.hip: MLLR over the mixtures, row f10; frame_adapt.hip: fMLLR over the frames, row f11;
// frame_mllt.hip: MLLT, row f13):
// the split-K float64 GEMM that forms [G | k] per (group, feature dimension) on v_mfma_f64_16x16x4_f64 or on the VALU, the reduction of the
// chunks' partials in chunk order, the in-LDS Cholesky factorisation and the two solves behind it (chol_factor_lds, chol_solve_lds: the ONE
// copy of each), the solve of one [G | k] and the test for W == [0 | I].  The kernels are templates over the
// operand SOURCE, which knows where chunk c's K-range lies and what element `le` of it contributes:
//     int Dh;                                                         feature dimension: row / column p of the padded grid runs over D + 2
//     struct Chunk { ...; int n; };   Chunk chunk(int c) const;       chunk c and its length
//     void operands(const Chunk &, int le, int i, int p, double &a, double &b) const;
// with sum_le a[p] b[q] = G[i][p][q] (q <= D) and k[i][p] (q = D + 1); an element that contributes nothing gives exact zeros.
// Included inside the including file's unnamed namespace; built with -ffp-contract=off.
#pragma once
#include <math.h>

#include "pcl_internal.h"

constexpr int ADAPT_D_MAX = 48;               // order D + 1 <= 49 (the solve's LDS matrix)
constexpr long long CHUNK_DEFAULT = 65536;    // K-elements per chunk: 93 chunks x 39 dimensions = 3600 workgroups at config 4's shape

typedef double d4 __attribute__((ext_vector_type(4)));

// Chunk length in K-elements (mixtures for MLLR, frames for fMLLR), env PCL_MLLR_CHUNK, read on EVERY call (as PCL_PCM_CHUNK is): tests
// force several chunks on a small input.
static long long mllr_chunk() { return env_positive_ll("PCL_MLLR_CHUNK", CHUNK_DEFAULT); }
static bool mllr_use_valu() {                 // env PCL_MLLR_VALU=1 (read on every call): the float64 VALU form of the GEMM (A/B, tools/adapt_bench.py)
    const char *e = getenv("PCL_MLLR_VALU");
    return e && atoi(e) != 0;
}

// One workgroup per (chunk, feature dimension): the upper-triangular 16 x 16 tiles (tp <= tq) of the chunk's contribution to [G | k].
// A wave takes every fourth k-step of 4 elements; lane l holds row / column l & 15 of element l >> 4 (the f32 16x16x4 operand map, one
// double per lane); the outer products exist only in the accumulators.  C/D of the f64 form: col = l & 15, row = (l >> 4) + 4 reg.
// partial: [chunk][i][tile][row * 16 + col]
template <int NT, class Src>
__global__ __launch_bounds__(256) void gk_mfma_kernel(Src g, double *__restrict__ partial) {
    constexpr int NTILES = NT * (NT + 1) / 2;
    __shared__ double red[4][NTILES][256];
    const int i = blockIdx.x % g.Dh, c = blockIdx.x / g.Dh;
    const typename Src::Chunk ch = g.chunk(c);
    const int n = ch.n;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kk = lane >> 4, c16 = lane & 15;
    d4 accv[NTILES];
#pragma unroll
    for (int t = 0; t < NTILES; ++t) accv[t] = d4{0.0, 0.0, 0.0, 0.0};
    const int nsteps = (n + 3) / 4;
    for (int s = wave; s < nsteps; s += 4) {                      // (uniform in the wave: every lane reaches every MFMA)
        double a[NT], b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) g.operands(ch, 4 * s + kk, i, 16 * t + c16, a[t], b[t]);
        int idx = 0;
#pragma unroll
        for (int tp = 0; tp < NT; ++tp)
#pragma unroll
            for (int tq = tp; tq < NT; ++tq, ++idx) accv[idx] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[tp], b[tq], accv[idx], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NTILES; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) red[wave][t][reg * 64 + lane] = accv[t][reg];
    __syncthreads();
    double *out = partial + ((size_t)c * g.Dh + i) * (NTILES * 256);
    for (int e = tid; e < NTILES * 256; e += 256) {
        const int t = e >> 8, x = e & 255, reg = x >> 6, ln = x & 63;
        const double sum = ((red[0][t][x] + red[1][t][x]) + red[2][t][x]) + red[3][t][x];      // wave order
        out[t * 256 + ((ln >> 4) + 4 * reg) * 16 + (ln & 15)] = sum;
    }
}

// The same partials on the float64 VALU (PCL_MLLR_VALU=1): 64 elements of operands staged in LDS, thread t owns element t of every tile.
template <int NT, class Src>
__global__ __launch_bounds__(256) void gk_valu_kernel(Src g, double *__restrict__ partial) {
    constexpr int NTILES = NT * (NT + 1) / 2, P = NT * 16;
    __shared__ double xa[64][P], xb[64][P];
    const int i = blockIdx.x % g.Dh, c = blockIdx.x / g.Dh;
    const typename Src::Chunk ch = g.chunk(c);
    const int n = ch.n;
    const int tid = threadIdx.x, row = tid >> 4, col = tid & 15;
    double sum[NTILES];
#pragma unroll
    for (int t = 0; t < NTILES; ++t) sum[t] = 0.0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        __syncthreads();
        for (int x = tid; x < 64 * P; x += 256) g.operands(ch, k0 + x / P, i, x % P, xa[x / P][x % P], xb[x / P][x % P]);
        __syncthreads();
        for (int k = 0; k < 64; ++k) {
            int idx = 0;
#pragma unroll
            for (int tp = 0; tp < NT; ++tp)
#pragma unroll
                for (int tq = tp; tq < NT; ++tq, ++idx) sum[idx] += xa[k][16 * tp + row] * xb[k][16 * tq + col];
        }
    }
    double *out = partial + ((size_t)c * g.Dh + i) * (NTILES * 256);
#pragma unroll
    for (int t = 0; t < NTILES; ++t) out[t * 256 + tid] = sum[t];
}

template <int NT, class Src>
static void launch_gk_nt(bool valu, int blocks, hipStream_t st, const Src &g, double *partial) {
    if (valu) hipLaunchKernelGGL((gk_valu_kernel<NT, Src>), dim3(blocks), dim3(256), 0, st, g, partial);
    else hipLaunchKernelGGL((gk_mfma_kernel<NT, Src>), dim3(blocks), dim3(256), 0, st, g, partial);
}
// blocks = chunks x Dh; NT = ceil((Dh + 2) / 16) in 1 .. 4
template <class Src>
static void launch_gk(bool valu, int NT, int blocks, hipStream_t st, const Src &g, double *partial) {
    if (NT == 1) launch_gk_nt<1>(valu, blocks, st, g, partial);
    else if (NT == 2) launch_gk_nt<2>(valu, blocks, st, g, partial);
    else if (NT == 3) launch_gk_nt<3>(valu, blocks, st, g, partial);
    else launch_gk_nt<4>(valu, blocks, st, g, partial);
}

__device__ __forceinline__ int tile_index(int tp, int tq, int NT) { return tp * NT - tp * (tp - 1) / 2 + (tq - tp); }

// One workgroup per (group, dimension): the group's chunks [grp_chunk0[r], grp_chunk0[r + 1]) summed in chunk order into the full symmetric
// [G | k], n x (n + 1), n = D + 1.  The lower triangle mirrors the upper one (a diagonal tile holds both, rounded differently: only its
// upper half is read).  add: the sum starts from what Gk holds (statistics that grow over calls) instead of from 0.
static __global__ __launch_bounds__(256) void gk_reduce_kernel(const double *__restrict__ partial, const int *__restrict__ grp_chunk0, int Dh, int NT,
                                                               double *__restrict__ Gk, bool add) {
    const int r = blockIdx.x / Dh, i = blockIdx.x % Dh, n = Dh + 1, ntiles = NT * (NT + 1) / 2;
    const int c_lo = grp_chunk0[r], c_hi = grp_chunk0[r + 1];
    for (int x = threadIdx.x; x < n * (n + 1); x += 256) {
        const int p = x / (n + 1), q = x % (n + 1);
        const int pp = q == n ? p : min(p, q), qq = q == n ? n : max(p, q);
        const size_t at = (size_t)tile_index(pp >> 4, qq >> 4, NT) * 256 + (pp & 15) * 16 + (qq & 15);
        double sum = add ? Gk[(size_t)blockIdx.x * n * (n + 1) + x] : 0.0;
        for (int c = c_lo; c < c_hi; ++c) sum += partial[((size_t)c * Dh + i) * (ntiles * 256) + at];
        Gk[(size_t)blockIdx.x * n * (n + 1) + x] = sum;
    }
}

// A = L L^T in place in LDS, one wave, thread t owns row t: the n x n matrix in the top left of A (rows of LD doubles) becomes L in its
// lower triangle and diagonal.  -> bad: a pivot is not finite or not > 0, and the factorisation stopped there (uniform).  Three barriers
// per column; the caller's barrier stands before the call.
template <int LD>
__device__ __forceinline__ bool chol_factor_lds(double (*A)[LD], int n, int tid) {
    for (int j = 0; j < n; ++j) {
        const double piv = A[j][j];
        if (!(piv > 0.0 && piv < INFINITY)) return true;          // (every thread reads the same value: uniform)
        const double d = sqrt(piv);
        __syncthreads();
        if (tid == j) A[j][j] = d;
        if (tid > j && tid < n) A[tid][j] = A[tid][j] / d;
        __syncthreads();
        if (tid > j && tid < n)
            for (int q = j + 1; q <= tid; ++q) A[tid][q] -= A[tid][j] * A[q][j];
        __syncthreads();
    }
    return false;
}

// The two solves behind the factorisation, in LDS, one wave, column by column: L y = rhs, then L^T w = y; rhs ends as w = (L L^T)^-1 rhs.
// L(r, c) and rhs(r) give references into the caller's arrays (lambdas: the address arithmetic is the caller's own).
template <class Mat, class Vec>
__device__ __forceinline__ void chol_solve_lds(Mat L, Vec rhs, int n, int tid) {
    for (int j = 0; j < n; ++j) {                                 // L y = rhs
        const double y = rhs(j) / L(j, j);
        __syncthreads();
        if (tid == j) rhs(j) = y;
        else if (tid > j && tid < n) rhs(tid) -= L(tid, j) * y;
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; --j) {                            // L^T w = y
        const double w = rhs(j) / L(j, j);
        __syncthreads();
        if (tid == j) rhs(j) = w;
        else if (tid < j) rhs(tid) -= L(j, tid) * w;
        __syncthreads();
    }
}

// One workgroup (one wave) per (group, dimension): G = L L^T in LDS, L y = k, L^T w = y; w = G^-1 k goes to W.  A pivot that is not finite
// or not > 0 stops the factorisation and flags the pair.  L_out (or NULL): the factor, [pair][n][n] row-major, lower triangle and diagonal.
static __global__ __launch_bounds__(64) void gk_solve_kernel(const double *__restrict__ Gk, const int *__restrict__ status, int Dh, double *__restrict__ W,
                                                             int *__restrict__ pivot_bad, double *__restrict__ L_out) {
    __shared__ double A[ADAPT_D_MAX + 1][ADAPT_D_MAX + 3];
    const int r = blockIdx.x / Dh, n = Dh + 1, tid = threadIdx.x;
    if (status[r] != 0) {
        if (tid == 0) pivot_bad[blockIdx.x] = 0;
        return;
    }
    for (int x = tid; x < n * (n + 1); x += 64) A[x / (n + 1)][x % (n + 1)] = Gk[(size_t)blockIdx.x * n * (n + 1) + x];
    __syncthreads();
    const bool bad = chol_factor_lds(A, n, tid);
    if (tid == 0) pivot_bad[blockIdx.x] = bad ? 1 : 0;
    if (bad) return;
    if (L_out)
        for (int x = tid; x < n * n; x += 64) L_out[(size_t)blockIdx.x * n * n + x] = x % n <= x / n ? A[x / n][x % n] : 0.0;
    chol_solve_lds([&](int r, int c) -> double & { return A[r][c]; }, [&](int r) -> double & { return A[r][n]; }, n, tid);   // k sits in column n
    if (tid < n) W[(size_t)blockIdx.x * n + tid] = A[tid][n];
}

// skip[r] = 1 when W[r] is exactly [0 | I]: the apply kernels leave such a group alone, bit for bit
static __global__ __launch_bounds__(64) void gk_identity_kernel(const double *__restrict__ W, int Dh, int *__restrict__ skip) {
    __shared__ int same;
    const int r = blockIdx.x, n = Dh + 1;
    if (threadIdx.x == 0) same = 1;
    __syncthreads();
    for (int x = threadIdx.x; x < Dh * n; x += 64)
        if (!(W[(size_t)r * Dh * n + x] == ((x % n == x / n + 1) ? 1.0 : 0.0))) same = 0;
    __syncthreads();
    if (threadIdx.x == 0) skip[r] = same;
}
