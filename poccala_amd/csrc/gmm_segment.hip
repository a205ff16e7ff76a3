// Segmental GMM training (training scheme 1 of the reference, AcousticModel.training mode 1, AcousticModel.py:771-840): after forced
// alignment every frame belongs to ONE GMM state, and every state's GMM is made from its own frames -- ClusterInitialization.kmeans
// (Clustering.py:838-1044) when the model is new or its mixture count changed, then the stand-alone GMM.em (Clustering.py:583-651,
// 695-719).  Here all J states go through every step together:
//   pcl_seg_create   counting sort of the frame indices by owner state (stable in frame order) + a gathered copy of the frames in
//                    segment order, so that a state's frames are one contiguous block of rows
//   pcl_seg_kmeans   k-means++ seeding (one workgroup per state) + Lloyd sweeps (one workgroup per state x 256-frame tile), the cluster
//                    sums taken in a fixed order over a cluster-sorted frame list (no floating-point atomics: same bits every run)
//   pcl_seg_em       the E-step IS the library's scoring + accumulate pass over a batch in which state j is a three-row "utterance"
//                    [entry, j, exit] of n_j frames with ln gamma = 0 on the middle row (what Clustering.GMM.update_acc does for one
//                    state), reading the gathered frames; the M-step + Q kernel below is new (GMM.maximization + q_function)
// Every kernel indexes frames through (off[j], counts[j]) built here from a validated owner array; a state outside [0, J) never
// reaches the device.
#include <math.h>

#include <limits>
#include <memory>

#include "pcl_internal.h"

struct pcl_seg {
    pcl_ctx *ctx = nullptr;
    int J = 0, FD = 0, FDhost = 0;
    long long F = 0, Ntot = 0;
    std::vector<int> counts, off;      // off: J + 1 entries
    DevBuf<int> d_counts, d_off, d_order;   // order[off[j] + i] = frame row of the i-th frame of state j
    DevBuf<float> G32;                 // (Ntot, FD) frames in segment order
    DevBuf<double> G64;                // ... float64 (made when first needed)
    int K = 0;                         // of the last pcl_seg_kmeans
    DevBuf<int> d_assign, d_corder, d_coff, d_seed;
    DevBuf<double> d_centres;          // (J, K, FD)
};

namespace {

constexpr int SEG_T = 256;

// The generator of the seeding draws (also in include/poccala_hip.h): SplitMix64's finaliser over a counter.
__host__ __device__ inline double seg_uniform(unsigned long long seed, int j, int k) {
    unsigned long long x = seed * 0x9E3779B97F4A7C15ULL + (((unsigned long long)(unsigned)j) << 32) + (unsigned long long)(unsigned)k + 1ULL;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}

// ---------------------------------------------------------------- segment build
__global__ __launch_bounds__(SEG_T) void seg_hist_kernel(const int *__restrict__ state, long long F, int J, int tile, int *__restrict__ tilecnt) {
    const long long lo = (long long)blockIdx.x * tile, hi = min(F, lo + tile);
    for (long long f = lo + threadIdx.x; f < hi; f += SEG_T) {
        const int s = state[f];
        if (s >= 0 && s < J) atomicAdd(&tilecnt[(size_t)blockIdx.x * J + s], 1);
    }
}

// per state: tilecnt[tile][j] -> the state's frames in earlier tiles; counts[j] = all of them
__global__ void seg_colscan_kernel(int *__restrict__ tilecnt, int n_tiles, int J, int *__restrict__ counts) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J) return;
    int run = 0;
    for (int t = 0; t < n_tiles; ++t) {
        const int c = tilecnt[(size_t)t * J + j];
        tilecnt[(size_t)t * J + j] = run;
        run += c;
    }
    counts[j] = run;
}

// rank of this thread's key among the equal keys of the round's lower threads, and how many threads hold the key
__device__ __forceinline__ void seg_round_rank(const int *keys, int key, int &rank, int &total) {
    rank = 0;
    total = 0;
    for (int t = 0; t < SEG_T; ++t) {
        const int same = keys[t] == key;
        total += same;
        rank += same & (t < (int)threadIdx.x);
    }
}

__global__ __launch_bounds__(SEG_T) void seg_scatter_kernel(const int *__restrict__ state, long long F, int J, int tile, int *tilecnt,
                                                            const int *__restrict__ off, int *__restrict__ order) {
    __shared__ int keys[SEG_T];
    const long long lo = (long long)blockIdx.x * tile, hi = min(F, lo + tile);
    int *base = tilecnt + (size_t)blockIdx.x * J;
    for (long long r0 = lo; r0 < hi; r0 += SEG_T) {
        const long long f = r0 + threadIdx.x;
        int key = -1;
        if (f < hi) {
            key = state[f];
            if (key < 0 || key >= J) key = -1;
        }
        keys[threadIdx.x] = key;
        __syncthreads();
        int rank = 0, total = 0;
        if (key >= 0) {
            seg_round_rank(keys, key, rank, total);
            order[off[key] + base[key] + rank] = (int)f;
        }
        __syncthreads();
        if (key >= 0 && rank == total - 1) base[key] += total;
        __threadfence_block();
        __syncthreads();
    }
}

template <typename T>
__global__ void seg_gather_kernel(const T *__restrict__ frames, const int *__restrict__ order, long long Ntot, int FD, T *__restrict__ G) {
    const long long total = Ntot * FD;
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const long long p = g / FD;
        const int d = (int)(g - p * FD);
        G[g] = frames[(long long)order[p] * FD + d];
    }
}

// ---------------------------------------------------------------- k-means++ seeding: one workgroup per state
template <typename T>
__global__ __launch_bounds__(SEG_T) void seg_seed_kernel(const T *__restrict__ G, int DD, const int *__restrict__ off, const int *__restrict__ counts,
                                                         const int *__restrict__ flags, int K, unsigned long long seed, double *mind2,
                                                         double *__restrict__ centres, int *__restrict__ seed_idx) {
    const int j = blockIdx.x, tid = threadIdx.x;
    if (!flags[j]) return;
    const int n = counts[j];
    const long long o = off[j];
    __shared__ double cen[64], part[SEG_T], s_total;
    __shared__ int s_idx, s_best, s_last;
    const int chunk = (n + SEG_T - 1) / SEG_T;
    const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    for (int k = 0; k < K; ++k) {
        if (k == 0) {
            if (tid == 0) s_idx = min((int)(seg_uniform(seed, j, 0) * (double)n), n - 1);
        } else {
            double local = 0.0;
            for (int i = lo; i < hi; ++i) local += mind2[o + i];
            part[tid] = local;
            if (tid == 0) {
                s_best = 0x7fffffff;
                s_last = -1;
            }
            __syncthreads();
            if (tid == 0) {
                double run = 0.0;
                for (int t = 0; t < SEG_T; ++t) {
                    const double v = part[t];
                    part[t] = run;
                    run += v;
                }
                s_total = run;
            }
            __syncthreads();
            const double total = s_total, u = seg_uniform(seed, j, k), target = u * total;
            if (total > 0.0) {
                double run = part[tid];
                int lastpos = -1;
                for (int i = lo; i < hi; ++i) {
                    const double v = mind2[o + i];
                    run += v;
                    if (v > 0.0) lastpos = i;
                    if (v > 0.0 && run > target) {           // (v > 0: a frame that IS a seed is never drawn, whatever the rounding at a chunk boundary)
                        atomicMin(&s_best, i);
                        break;
                    }
                }
                if (lastpos >= 0) atomicMax(&s_last, lastpos);
            }
            __syncthreads();
            if (tid == 0) {
                int idx = (total > 0.0) ? (s_best != 0x7fffffff ? s_best : s_last) : -1;
                if (idx < 0) idx = min((int)(u * (double)n), n - 1);      // every frame sits on a chosen centre: any row will do
                s_idx = idx;
            }
        }
        __syncthreads();
        const int idx = s_idx;
        if (tid < DD) {
            const double v = (double)G[(o + idx) * DD + tid];
            cen[tid] = v;
            centres[((size_t)j * K + k) * DD + tid] = v;
        }
        if (tid == 0) seed_idx[(size_t)j * K + k] = idx;
        __syncthreads();
        if (k == K - 1) break;
        for (int i = tid; i < n; i += SEG_T) {
            const T *x = G + (o + i) * DD;
            double d2 = 0.0;
            for (int d = 0; d < DD; ++d) {
                const double t = (double)x[d] - cen[d];
                d2 += t * t;
            }
            mind2[o + i] = (k == 0) ? d2 : fmin(mind2[o + i], d2);
        }
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------- Lloyd: assignment, one workgroup per (state, 256-frame tile)
template <typename T, int DD>
__global__ __launch_bounds__(SEG_T) void seg_assign_kernel(const T *__restrict__ G, const int2 *__restrict__ tiles, const int *__restrict__ off,
                                                           const int *__restrict__ counts, const int *__restrict__ active,
                                                           const double *__restrict__ centres, int K, int *__restrict__ assign, int *changed) {
    constexpr int KC = 32;
    __shared__ T c[KC * DD];
    const int2 tl = tiles[blockIdx.x];
    const int j = tl.x;
    if (!active[j]) return;
    const int n = counts[j], i = tl.y + (int)threadIdx.x;
    const bool valid = i < n;
    const long long p = (long long)off[j] + (valid ? i : 0);
    T x[DD];
#pragma unroll
    for (int d = 0; d < DD; ++d) x[d] = G[p * DD + d];
    T best = std::numeric_limits<T>::infinity();
    int bk = 0;
    for (int k0 = 0; k0 < K; k0 += KC) {
        __syncthreads();
        for (int e = threadIdx.x; e < KC * DD; e += SEG_T) {
            const int kk = k0 + e / DD;
            c[e] = kk < K ? (T)centres[((size_t)j * K + kk) * DD + e % DD] : (T)0;
        }
        __syncthreads();
        const int kc = min(KC, K - k0);
        for (int kk = 0; kk < kc; ++kk) {
            T acc = 0;
#pragma unroll
            for (int d = 0; d < DD; ++d) {
                const T t = x[d] - c[kk * DD + d];
                acc += t * t;
            }
            if (acc < best) {                 // strict: the lowest index wins a tie
                best = acc;
                bk = k0 + kk;
            }
        }
    }
    if (valid && assign[p] != bk) {
        assign[p] = bk;
        atomicAdd(&changed[j], 1);            // an integer count: the same whatever the order
    }
}

// a state's frames sorted by cluster, stable (counting sort inside one workgroup): corder[off + .] = row of G, coff[j][k] = first of cluster k
__global__ __launch_bounds__(SEG_T) void seg_cluster_sort_kernel(const int *__restrict__ off, const int *__restrict__ counts, const int *__restrict__ flags,
                                                                 const int *__restrict__ assign, int K, int *__restrict__ corder, int *__restrict__ coff) {
    extern __shared__ int sh[];               // K running offsets, then the round's keys
    int *keys = sh + K;
    const int j = blockIdx.x, tid = threadIdx.x;
    if (!flags[j]) return;
    const int n = counts[j], o = off[j];
    for (int k = tid; k < K; k += SEG_T) sh[k] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += SEG_T) atomicAdd(&sh[assign[o + i]], 1);
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int k = 0; k < K; ++k) {
            const int cnt = sh[k];
            sh[k] = run;
            coff[(size_t)j * (K + 1) + k] = run;
            run += cnt;
        }
        coff[(size_t)j * (K + 1) + K] = run;
    }
    __syncthreads();
    for (int r0 = 0; r0 < n; r0 += SEG_T) {
        const int i = r0 + tid;
        const int key = i < n ? assign[o + i] : -1;
        keys[tid] = key;
        __syncthreads();
        int rank = 0, total = 0;
        if (key >= 0) {
            seg_round_rank(keys, key, rank, total);
            corder[o + sh[key] + rank] = o + i;
        }
        __syncthreads();
        if (key >= 0 && rank == total - 1) sh[key] += total;
        __syncthreads();
    }
}

// sum over one cluster's run in a fixed order: wave w takes the w-th quarter, lane d one feature; ((p0 + p1) + p2) + p3
template <typename T, bool SQ>
__device__ __forceinline__ double seg_cluster_sum(const T *__restrict__ G, int DD, const int *__restrict__ rows, int cnt, double centre, double *part) {
    const int w = threadIdx.x >> 6, d = threadIdx.x & 63;
    const int q = (cnt + 3) / 4, lo = min(cnt, w * q), hi = min(cnt, lo + q);
    double s = 0.0;
    if (d < DD)
        for (int p = lo; p < hi; ++p) {
            const double v = (double)G[(long long)rows[p] * DD + d];
            if (SQ) s += (v - centre) * (v - centre);
            else s += v;
        }
    __syncthreads();
    part[threadIdx.x] = s;
    __syncthreads();
    return ((part[d] + part[64 + d]) + part[128 + d]) + part[192 + d];
}

// centres <- cluster means (an empty cluster keeps its centre); FINAL: also write the model as the reference does after clustering
// (ClusterInitialization.cal_variance, Clustering.py:807-832: mean squared deviation floored at 1e-4; weight n_jk / n_j)
template <typename T, bool FINAL>
__global__ __launch_bounds__(SEG_T) void seg_centre_kernel(const T *__restrict__ G, int DD, int Dhost, const int *__restrict__ off, const int *__restrict__ counts,
                                                           const int *__restrict__ flags, const int *__restrict__ corder, const int *__restrict__ coff, int K,
                                                           double *__restrict__ centres, int Mpad, double *__restrict__ mean64, double *__restrict__ var64,
                                                           double *__restrict__ w64) {
    __shared__ double part[SEG_T];
    const int k = blockIdx.x, j = blockIdx.y;
    if (!flags[j]) return;
    const int c0 = coff[(size_t)j * (K + 1) + k], cnt = coff[(size_t)j * (K + 1) + k + 1] - c0;
    const int *rows = corder + off[j] + c0;
    const int d = threadIdx.x & 63;
    const size_t ci = ((size_t)j * K + k) * DD + d;
    double mean = (d < DD) ? centres[ci] : 0.0;
    const double sum = seg_cluster_sum<T, false>(G, DD, rows, cnt, 0.0, part);
    if (cnt > 0) mean = sum / (double)cnt;
    if (threadIdx.x < DD && cnt > 0) centres[ci] = mean;
    if (FINAL) {
        const double sq = seg_cluster_sum<T, true>(G, DD, rows, cnt, mean, part);
        if (threadIdx.x < Dhost) {
            double v = cnt > 0 ? sq / (double)cnt : 0.0;
            if (!(v >= 1e-4)) v = 1e-4;
            const size_t mi = ((size_t)j * Mpad + k) * DD + d;
            mean64[mi] = mean;
            var64[mi] = v;
        }
        if (threadIdx.x == 0) w64[(size_t)j * Mpad + k] = (double)cnt / (double)counts[j];
    }
}

// ---------------------------------------------------------------- EM
// ln gamma of the three-row segments: entry / exit rows ln 0, the state's row ln 1 (time-major (t, n), N = 3 everywhere)
__global__ void seg_posterior_kernel(double *__restrict__ lgam, long long n) {
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x)
        lgam[g] = (g % 3 == 1) ? 0.0 : -INFINITY;
}

// GMM.maximization (Clustering.py:624-651) + q_function (:607-616) for every running state, from the statistics of this iteration's
// E-step, which are centred on the mean c the E-step used:  mu = sum gamma (x + bias) / Gamma - bias;  s2 = sum gamma (x - c)^2 / Gamma
// - (mu - c)^2 is the variance about the NEW mean (:638);  var = max(s2, floor);  w = Gamma / n_j.  Q with the gamma of this E-step and the
// parameters after the M-step needs no second pass over the data:
//   Q = sum_m Gamma_m [ ln w_m - 1/2 sum_d ( ln 2 pi + g(var_md) + s2_md / var_md ) ],   g(v) = v as util.gaussian_function has it
//   (util.py:29, quirk Q1; ln v under PCL_MODEL_LOGDET).  A mixture nobody reached (Gamma = 0) gets weight 0, keeps its mean and variance
//   and adds nothing to Q (0 ln 0 taken as 0; the reference gives NaN there).
__global__ __launch_bounds__(SEG_T) void seg_mstep_q_kernel(const double *__restrict__ st_acc, const double *__restrict__ st_mean, const double *__restrict__ st_cov,
                                                            const int *__restrict__ counts, const int *__restrict__ active, int M, int Mpad, int D, int Dhost,
                                                            double bias, double floor_var, int logdet, double *__restrict__ mean64, double *__restrict__ var64,
                                                            double *__restrict__ w64, double *__restrict__ q_out) {
    __shared__ double part[SEG_T];
    const int j = blockIdx.x;
    if (!active[j]) return;
    const double n = (double)counts[j], ln2pi = 1.8378770664093454836;
    double q = 0.0;
    for (int m = threadIdx.x; m < M; m += SEG_T) {
        const size_t jm = (size_t)j * Mpad + m;
        const double g = st_acc[jm], w = g / n;
        w64[jm] = w;
        if (!(g > 0.0)) continue;
        double qd = 0.0;
        for (int d = 0; d < Dhost; ++d) {
            const size_t i = jm * D + d;
            const double c = mean64[i], mu = st_mean[i] / g - bias;
            double s2 = st_cov[i] / g - (mu - c) * (mu - c);
            if (!(s2 > 0.0)) s2 = 0.0;
            const double v = s2 >= floor_var ? s2 : floor_var;
            mean64[i] = mu;
            var64[i] = v;
            qd += ln2pi + (logdet ? log(v) : v) + s2 / v;
        }
        q += g * (log(w) - 0.5 * qd);
    }
    part[threadIdx.x] = q;
    __syncthreads();
    for (int s = SEG_T / 2; s > 0; s >>= 1) {                 // a fixed tree: the same bits every run
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) q_out[j] = part[0];
}

template <typename T>
int launch_assign(pcl_seg *s, const T *G, const int2 *tiles, int n_tiles, const int *active, int *changed) {
    pcl_ctx *ctx = s->ctx;
#define SEG_ASSIGN(DDV)                                                                                                                        \
    case DDV:                                                                                                                                  \
        hipLaunchKernelGGL((seg_assign_kernel<T, DDV>), dim3(n_tiles), dim3(SEG_T), 0, ctx->stream, G, tiles, s->d_off, s->d_counts, active, \
                           s->d_centres, s->K, s->d_assign, changed);                                                                          \
        break;
    switch (s->FD) {
        SEG_ASSIGN(13)
        SEG_ASSIGN(26)
        SEG_ASSIGN(39)
        SEG_ASSIGN(47)
        SEG_ASSIGN(48)
        SEG_ASSIGN(64)
        default: PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_kmeans: no kernel for the device feature dimension %d", s->FD);
    }
#undef SEG_ASSIGN
    HIPCHK(ctx, hipGetLastError());
    return PCL_OK;
}

int seg_ensure_g64(pcl_seg *s) {
    if (s->G64) return PCL_OK;
    const size_t n = (size_t)s->Ntot * s->FD;
    TRY(s->G64.alloc(s->ctx, n));
    return pcl_launch_cast(s->ctx, nullptr, s->G32, s->G64, n);          // float -> double is exact
}

// While a segment call runs the library's scoring / accumulate pass, the context's frame matrix IS the gathered copy: the f32 view points
// at it, the f64 matrices change hands for the duration (so one the pass derives meanwhile is the segment set's to keep).
struct FrameSwap {
    pcl_ctx *ctx;
    pcl_seg *seg;
    float *f32;
    DevBuf<double> f64;
    int64_t F;
    int FD, FDhost;
    FrameSwap(pcl_ctx *c, pcl_seg *s) : ctx(c), seg(s), f32(c->frames32), f64(std::move(c->frames64)), F(c->F), FD(c->FD), FDhost(c->FDhost) {
        c->frames32 = s->G32;
        c->frames64 = std::move(s->G64);
        c->F = s->Ntot;
        c->FD = s->FD;
        c->FDhost = s->FDhost;
    }
    ~FrameSwap() {
        ctx->frames32 = f32;
        seg->G64 = std::move(ctx->frames64);
        ctx->frames64 = std::move(f64);
        ctx->F = F;
        ctx->FD = FD;
        ctx->FDhost = FDhost;
    }
};

int upload_flags(pcl_ctx *ctx, int *d, const std::vector<int> &h) {
    HIPCHK(ctx, pcl_h2d(ctx, d, h.data(), h.size() * sizeof(int)));
    return PCL_OK;
}

}  // namespace

extern "C" {

int pcl_seg_create(pcl_ctx *ctx, int64_t n_frames_total, int J, const int32_t *frame_state, pcl_seg **out) {
    if (!ctx || !out) return PCL_ERR_INVALID;
    *out = nullptr;
    if (!frame_state || J <= 0 || J > 65535 || n_frames_total <= 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_create: bad arguments (J=%d, at most 65535 states)", J);
    if (!ctx->frames32 || ctx->F == 0) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_seg_create: no frames uploaded");
    if (n_frames_total != ctx->F || n_frames_total > 0x7fffffffLL)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_create: %lld owner entries for a frame matrix of %lld rows", (long long)n_frames_total, (long long)ctx->F);
    for (int64_t t = 0; t < n_frames_total; ++t)
        if (frame_state[t] < -1 || frame_state[t] >= J)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_create: frame_state[%lld] = %d is neither -1 nor a state in [0,%d)", (long long)t, frame_state[t], J);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf<int> d_state;
    TRY(d_state.alloc(ctx, (size_t)n_frames_total));
    HIPCHK(ctx, pcl_h2d(ctx, d_state, frame_state, (size_t)n_frames_total * sizeof(int)));
    return pcl_seg_create_device(ctx, n_frames_total, J, d_state, out);
}

}  // extern "C"

// The owner array is on the device already (pcl_seg_create above; pcl_uniform_segments, bootstrap.hip; pcl_batch_align_segments, pcl_batch.hip):
// counting sort (timer "seg_count") + scatter and gather (timer "seg_gather").
int pcl_seg_create_device(pcl_ctx *ctx, int64_t n_frames_total, int J, const int32_t *d_state, pcl_seg **out) {
    *out = nullptr;
    if (J <= 0 || J > 65535) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_create: bad arguments (J=%d, at most 65535 states)", J);
    if (!ctx->frames32 || ctx->F == 0) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_seg_create: no frames uploaded");
    if (n_frames_total != ctx->F || n_frames_total > 0x7fffffffLL)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_create: %lld owner entries for a frame matrix of %lld rows", (long long)n_frames_total, (long long)ctx->F);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long F = n_frames_total;
    std::unique_ptr<pcl_seg> s(new pcl_seg());                   // (a failure below gives back whatever the set holds by then)
    s->ctx = ctx;
    s->J = J;
    s->F = F;
    s->FD = ctx->FD;
    s->FDhost = ctx->FDhost;
    // tiles of at least 2048 frames, at most 4096 of them and at most 2^26 entries (256 MB) in the tile x state count matrix
    const long long per_tile = std::max<long long>(std::max<long long>(2048, (F + 4095) / 4096), (F * (long long)J + (1LL << 26) - 1) >> 26);
    const int tile = (int)((per_tile + SEG_T - 1) / SEG_T * SEG_T);
    const int n_tiles = (int)((F + tile - 1) / tile);
    DevBuf<int> d_tilecnt;
    TRY(d_tilecnt.alloc(ctx, (size_t)n_tiles * J));
    TRY(s->d_counts.alloc(ctx, (size_t)J));
    TRY(s->d_off.alloc(ctx, (size_t)J + 1));
    HIPCHK(ctx, hipMemsetAsync(d_tilecnt, 0, (size_t)n_tiles * J * sizeof(int), ctx->stream));
    pcl_timer_begin(ctx, "seg_count");
    hipLaunchKernelGGL(seg_hist_kernel, dim3(n_tiles), dim3(SEG_T), 0, ctx->stream, d_state, F, J, tile, d_tilecnt);
    hipLaunchKernelGGL(seg_colscan_kernel, dim3((J + 255) / 256), dim3(256), 0, ctx->stream, d_tilecnt, n_tiles, J, s->d_counts);
    pcl_timer_end(ctx, "seg_count");
    HIPCHK(ctx, hipGetLastError());
    s->counts.resize(J);
    HIPCHK(ctx, hipMemcpyAsync(s->counts.data(), s->d_counts, (size_t)J * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    s->off.assign(J + 1, 0);
    for (int j = 0; j < J; ++j) s->off[j + 1] = s->off[j] + s->counts[j];
    s->Ntot = s->off[J];
    HIPCHK(ctx, pcl_h2d(ctx, s->d_off, s->off.data(), (size_t)(J + 1) * sizeof(int)));
    TRY(s->d_order.alloc(ctx, (size_t)s->Ntot));
    TRY(s->G32.alloc(ctx, (size_t)s->Ntot * s->FD));
    if (ctx->frames64) TRY(s->G64.alloc(ctx, (size_t)s->Ntot * s->FD));
    if (s->Ntot > 0) {
        pcl_timer_begin(ctx, "seg_gather");
        hipLaunchKernelGGL(seg_scatter_kernel, dim3(n_tiles), dim3(SEG_T), 0, ctx->stream, d_state, F, J, tile, d_tilecnt, s->d_off, s->d_order);
        const unsigned gb = (unsigned)std::min<long long>(8192, (s->Ntot * s->FD + 255) / 256);
        hipLaunchKernelGGL(seg_gather_kernel<float>, dim3(gb), dim3(256), 0, ctx->stream, ctx->frames32, s->d_order, s->Ntot, s->FD, s->G32);
        if (s->G64) hipLaunchKernelGGL(seg_gather_kernel<double>, dim3(gb), dim3(256), 0, ctx->stream, ctx->frames64, s->d_order, s->Ntot, s->FD, s->G64);
        pcl_timer_end(ctx, "seg_gather");
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ++ctx->live_segs;
    *out = s.release();
    return PCL_OK;
}

// The histogram / scan / stable scatter above without a pcl_seg around them (frame_lda.hip sorts rows by class)
int pcl_count_sort_device(pcl_ctx *ctx, long long F, int J, const int *d_key, std::vector<int> *counts, DevBuf<int> *d_order) {
    const long long per_tile = std::max<long long>(std::max<long long>(2048, (F + 4095) / 4096), (F * (long long)J + (1LL << 26) - 1) >> 26);
    const int tile = (int)((per_tile + SEG_T - 1) / SEG_T * SEG_T);
    const int n_tiles = (int)((F + tile - 1) / tile);
    DevBuf<int> d_tilecnt, d_counts, d_off;
    TRY(d_tilecnt.alloc(ctx, (size_t)n_tiles * J));
    TRY(d_counts.alloc(ctx, (size_t)J));
    TRY(d_off.alloc(ctx, (size_t)J + 1));
    HIPCHK(ctx, hipMemsetAsync(d_tilecnt, 0, (size_t)n_tiles * J * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(seg_hist_kernel, dim3(n_tiles), dim3(SEG_T), 0, ctx->stream, d_key, F, J, tile, d_tilecnt);
    hipLaunchKernelGGL(seg_colscan_kernel, dim3((J + 255) / 256), dim3(256), 0, ctx->stream, d_tilecnt, n_tiles, J, d_counts);
    HIPCHK(ctx, hipGetLastError());
    counts->resize(J);
    HIPCHK(ctx, hipMemcpyAsync(counts->data(), d_counts, (size_t)J * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> off(J + 1, 0);
    for (int j = 0; j < J; ++j) off[j + 1] = off[j] + (*counts)[j];
    HIPCHK(ctx, pcl_h2d(ctx, d_off, off.data(), (size_t)(J + 1) * sizeof(int)));
    TRY(d_order->alloc(ctx, (size_t)off[J]));
    if (off[J] > 0) {
        hipLaunchKernelGGL(seg_scatter_kernel, dim3(n_tiles), dim3(SEG_T), 0, ctx->stream, d_key, F, J, tile, d_tilecnt, d_off, d_order->p);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

extern "C" {

int pcl_seg_destroy(pcl_seg *seg) {
    if (!seg) return PCL_ERR_INVALID;
    (void)hipSetDevice(seg->ctx->device);
    --seg->ctx->live_segs;
    delete seg;                                                  // (every block with its device-wide wait: nothing says the GPU is done with them)
    return PCL_OK;
}

int pcl_seg_get(pcl_seg *seg, int what, void *host) {
    if (!seg) return PCL_ERR_INVALID;
    pcl_ctx *ctx = seg->ctx;
    if (!host) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_get: NULL destination");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const void *src = nullptr;
    size_t bytes = 0;
    switch (what) {
        case PCL_SEG_COUNTS:
            memcpy(host, seg->counts.data(), (size_t)seg->J * sizeof(int));
            return PCL_OK;
        case PCL_SEG_ORDER: src = seg->d_order, bytes = (size_t)seg->Ntot * sizeof(int); break;
        case PCL_SEG_ASSIGN: src = seg->d_assign, bytes = (size_t)seg->Ntot * sizeof(int); break;
        case PCL_SEG_SEEDS: src = seg->d_seed, bytes = (size_t)seg->J * seg->K * sizeof(int); break;
        default: PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_get: selector %d", what);
    }
    if (!src && bytes) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_seg_get: run pcl_seg_kmeans first");
    if (bytes) {
        HIPCHK(ctx, hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PCL_OK;
}

int pcl_seg_kmeans(pcl_seg *seg, int K, uint64_t seed, int max_sweeps, int precision, const double *init_centres, int32_t *sweeps_done) {
    if (!seg) return PCL_ERR_INVALID;
    pcl_ctx *ctx = seg->ctx;
    const int J = seg->J, DD = seg->FD, Dh = seg->FDhost;
    if (K < 1 || K > 8192 || max_sweeps < 1 || !sweeps_done) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_kmeans: K=%d (1..8192), max_sweeps=%d (>= 1)", K, max_sweeps);
    if (precision != PCL_F32 && precision != PCL_F64) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_kmeans: precision %d", precision);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the model the clusters are written into: (J, K, D).  A context that holds another shape (or none) gets a neutral one first
    // (mean 0, variance 1, uniform weights): that is what the states with fewer than K frames keep.
    if (ctx->J != J || ctx->M != K || ctx->Dhost != Dh) {
        const size_t nm = (size_t)J * K * Dh;
        std::vector<double> m0(nm, 0.0), v0(nm, 1.0), w0((size_t)J * K, 1.0 / K);
        TRY(pcl_model_upload(ctx, J, K, Dh, m0.data(), v0.data(), w0.data(), ctx->model_flags));
    }
    if (ctx->D != DD) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_seg_kmeans: model and frames disagree on the device feature dimension");
    if (precision == PCL_F64) TRY(seg_ensure_g64(seg));
    // per-call buffers (K may differ from the last call)
    seg->d_assign.release();
    seg->d_corder.release();
    seg->d_coff.release();
    seg->d_seed.release();
    seg->d_centres.release();
    seg->K = K;
    TRY(seg->d_assign.alloc(ctx, (size_t)seg->Ntot));
    TRY(seg->d_corder.alloc(ctx, (size_t)seg->Ntot));
    TRY(seg->d_coff.alloc(ctx, (size_t)J * (K + 1)));
    TRY(seg->d_seed.alloc(ctx, (size_t)J * K));
    TRY(seg->d_centres.alloc(ctx, (size_t)J * K * DD));
    HIPCHK(ctx, hipMemsetAsync(seg->d_assign, 0xff, (size_t)seg->Ntot * sizeof(int), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(seg->d_seed, 0xff, (size_t)J * K * sizeof(int), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(seg->d_centres, 0, (size_t)J * K * DD * sizeof(double), ctx->stream));

    std::vector<int> train(J), active(J), changed(J);
    std::vector<int2> tiles;
    int n_train = 0;
    for (int j = 0; j < J; ++j) {
        train[j] = seg->counts[j] >= K && seg->counts[j] > 0;      // __cal_gmm skips a state with fewer frames than mixtures (AcousticModel.py:549-551)
        sweeps_done[j] = train[j] ? 0 : -1;
        n_train += train[j];
        if (train[j])
            for (int t0 = 0; t0 < seg->counts[j]; t0 += SEG_T) tiles.push_back(make_int2(j, t0));
    }
    if (n_train == 0) return PCL_OK;
    DevBuf<int> d_train, d_active, d_changed;                    // (call-scoped: released, each with its device-wide wait, on every way out)
    DevBuf<int2> d_tiles;
    DevBuf<double> d_mind2;
    auto run = [&]() -> int {
    TRY(d_train.alloc(ctx, (size_t)J));
    TRY(d_active.alloc(ctx, (size_t)J));
    TRY(d_changed.alloc(ctx, (size_t)J));
    TRY(d_tiles.alloc(ctx, tiles.size()));
    TRY(upload_flags(ctx, d_train, train));
    HIPCHK(ctx, pcl_h2d(ctx, d_tiles, tiles.data(), tiles.size() * sizeof(int2)));
    const bool f64 = precision == PCL_F64;
    // ---- seeds
    if (init_centres) {
        std::vector<double> c((size_t)J * K * DD, 0.0);
        for (size_t jk = 0; jk < (size_t)J * K; ++jk)
            for (int d = 0; d < Dh; ++d) c[jk * DD + d] = init_centres[jk * Dh + d];
        HIPCHK(ctx, pcl_h2d(ctx, seg->d_centres, c.data(), c.size() * sizeof(double)));
    } else {
        TRY(d_mind2.alloc(ctx, (size_t)seg->Ntot));
        if (f64) hipLaunchKernelGGL(seg_seed_kernel<double>, dim3(J), dim3(SEG_T), 0, ctx->stream, seg->G64, DD, seg->d_off, seg->d_counts, d_train, K,
                                    (unsigned long long)seed, d_mind2, seg->d_centres, seg->d_seed);
        else hipLaunchKernelGGL(seg_seed_kernel<float>, dim3(J), dim3(SEG_T), 0, ctx->stream, seg->G32, DD, seg->d_off, seg->d_counts, d_train, K,
                                (unsigned long long)seed, d_mind2, seg->d_centres, seg->d_seed);
        HIPCHK(ctx, hipGetLastError());
    }
    // ---- Lloyd sweeps: a state leaves the loop when none of its frames changed cluster
    const size_t sort_shm = (size_t)(K + SEG_T) * sizeof(int);
    auto sort_and_centres = [&](const int *d_flags, bool final) -> int {
        hipLaunchKernelGGL(seg_cluster_sort_kernel, dim3(J), dim3(SEG_T), sort_shm, ctx->stream, seg->d_off, seg->d_counts, d_flags, seg->d_assign, K,
                           seg->d_corder, seg->d_coff);
#define SEG_CENTRE(T, G, FIN)                                                                                                                         \
    hipLaunchKernelGGL((seg_centre_kernel<T, FIN>), dim3(K, J), dim3(SEG_T), 0, ctx->stream, G, DD, Dh, seg->d_off, seg->d_counts, d_flags, seg->d_corder, \
                       seg->d_coff, K, seg->d_centres, ctx->Mpad, ctx->mean64, ctx->var64, ctx->w64)
        if (f64) {
            if (final) SEG_CENTRE(double, seg->G64, true);
            else SEG_CENTRE(double, seg->G64, false);
        } else {
            if (final) SEG_CENTRE(float, seg->G32, true);
            else SEG_CENTRE(float, seg->G32, false);
        }
#undef SEG_CENTRE
        HIPCHK(ctx, hipGetLastError());
        return PCL_OK;
    };
    active = train;
    int n_active = n_train;
    for (int sweep = 0; sweep < max_sweeps && n_active > 0; ++sweep) {
        TRY(upload_flags(ctx, d_active, active));
        HIPCHK(ctx, hipMemsetAsync(d_changed, 0, (size_t)J * sizeof(int), ctx->stream));
        TRY(f64 ? launch_assign<double>(seg, seg->G64, d_tiles, (int)tiles.size(), d_active, d_changed)
              : launch_assign<float>(seg, seg->G32, d_tiles, (int)tiles.size(), d_active, d_changed));
        HIPCHK(ctx, hipMemcpyAsync(changed.data(), d_changed, (size_t)J * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        n_active = 0;
        for (int j = 0; j < J; ++j)
            if (active[j]) {
                ++sweeps_done[j];
                if (changed[j] == 0) active[j] = 0;
                n_active += active[j];
            }
        if (n_active > 0) {
            TRY(upload_flags(ctx, d_active, active));
            TRY(sort_and_centres(d_active, false));
        }
    }
    // ---- the model: cluster mean, floored mean squared deviation, n_jk / n_j; then every scoring layout, as pcl_mstep does
    TRY(sort_and_centres(d_train, true));
    TRY(pcl_launch_derive(ctx));
    return PCL_OK;
    };
    int rc = run();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PCL_OK) PCL_FAIL(ctx, PCL_ERR_HIP, "pcl_seg_kmeans: HIP error");
    return rc;
}

int pcl_seg_centres(pcl_seg *seg, double *centres) {
    if (!seg) return PCL_ERR_INVALID;
    pcl_ctx *ctx = seg->ctx;
    if (!centres) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_centres: NULL destination");
    if (!seg->d_centres) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_seg_centres: run pcl_seg_kmeans first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> c((size_t)seg->J * seg->K * seg->FD);
    HIPCHK(ctx, hipMemcpyAsync(c.data(), seg->d_centres, c.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t jk = 0; jk < (size_t)seg->J * seg->K; ++jk)
        for (int d = 0; d < seg->FDhost; ++d) centres[jk * seg->FDhost + d] = c[jk * seg->FD + d];
    return PCL_OK;
}

int pcl_seg_em(pcl_seg *seg, double c_covariance, double q_threshold, int max_iters, int precision, int32_t *iters, double *q,
               double *q_trace) {
    if (!seg) return PCL_ERR_INVALID;
    pcl_ctx *ctx = seg->ctx;
    const int J = seg->J;
    if (!iters || !q || max_iters < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_em: bad arguments");
    if (precision != PCL_F32 && precision != PCL_F64) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_seg_em: precision %d", precision);
    if (ctx->J != J || !ctx->stats) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_seg_em: the context's model has %d states, the segments %d", ctx->J, J);
    if (ctx->Dhost != seg->FDhost) PCL_FAIL(ctx, PCL_ERR_INVALID, "data dimension %d does not match model dimension %d", seg->FDhost, ctx->Dhost);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (precision == PCL_F64) TRY(seg_ensure_g64(seg));
    const int M = ctx->M;
    std::vector<int> active(J);
    std::vector<double> q_old(J, -INFINITY), q_new(J);
    int n_active = 0;
    for (int j = 0; j < J; ++j) {
        active[j] = seg->counts[j] >= M && seg->counts[j] > 0;       // AcousticModel.py:549-551
        iters[j] = active[j] ? 0 : -1;
        q[j] = active[j] ? -INFINITY : NAN;
        n_active += active[j];
    }
    if (q_trace)
        for (size_t i = 0; i < (size_t)J * max_iters; ++i) q_trace[i] = NAN;
    if (n_active == 0) return PCL_OK;
    FrameSwap swap(ctx, seg);
    DevBuf<int> d_active;                                        // (call-scoped: released, each with its device-wide wait, on every way out)
    DevBuf<double> d_q;
    pcl_batch *b = nullptr;
    auto run = [&]() -> int {
    TRY(d_active.alloc(ctx, (size_t)J));
    TRY(d_q.alloc(ctx, (size_t)J));
    bool rebuild = true;
    for (int it = 0; it < max_iters && n_active > 0; ++it) {
        if (rebuild) {
            // the running states as three-row utterances over the gathered frames; a converged state is not scored again
            if (b) TRY(pcl_batch_destroy(b));
            b = nullptr;
            std::vector<int32_t> N, T, rows;
            std::vector<int64_t> begin;
            for (int j = 0; j < J; ++j)
                if (active[j]) {
                    N.push_back(3);
                    T.push_back(seg->counts[j]);
                    begin.push_back(seg->off[j]);
                    rows.push_back(PCL_ROW_ENTRY);
                    rows.push_back(j);
                    rows.push_back(PCL_ROW_EXIT);
                }
            TRY(pcl_batch_create(ctx, (int)N.size(), N.data(), T.data(), begin.data(), &b));
            TRY(pcl_batch_set_states(b, rows.data()));
            TRY(b->lgam.alloc(ctx, (size_t)b->shape.sumNT));
            {
                hipLaunchKernelGGL(seg_posterior_kernel, dim3((unsigned)std::min<long long>(4096, (b->shape.sumNT + 255) / 256)), dim3(256), 0, ctx->stream, b->lgam,
                                   b->shape.sumNT);
                HIPCHK(ctx, hipGetLastError());
                b->have_post = true;
            }
            TRY(upload_flags(ctx, d_active, active));
            rebuild = false;
        }
        TRY(pcl_batch_score(b, precision));                         // GMM.expectation: the per-frame normaliser ln b_j(o_t) ...
        TRY(pcl_stats_zero(ctx));
        TRY(pcl_batch_accumulate(b, precision));  // ... and the responsibilities summed into Gamma, sum gamma (x + bias), sum gamma (x - c)^2
        HIPCHK(ctx, pcl_stats_join(ctx));
        hipLaunchKernelGGL(seg_mstep_q_kernel, dim3(J), dim3(SEG_T), 0, ctx->stream, ctx->st_acc, ctx->st_mean, ctx->st_cov, seg->d_counts, d_active, M, ctx->Mpad,
                           ctx->D, ctx->Dhost, 100.0, c_covariance, ctx->model_flags & PCL_MODEL_LOGDET, ctx->mean64, ctx->var64, ctx->w64, d_q);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(q_new.data(), d_q, (size_t)J * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TRY(pcl_launch_derive(ctx));              // (waits for the stream: q_new has landed)
        for (int j = 0; j < J; ++j) {
            if (!active[j]) continue;
            ++iters[j];
            if (q_trace) q_trace[(size_t)j * max_iters + it] = q_new[j];
            if (q_new[j] - q_old[j] > q_threshold) {              // Clustering.py:706; the parameters of a refused step are kept (:704)
                q_old[j] = q_new[j];
                q[j] = q_new[j];
            } else {
                active[j] = 0;
                --n_active;
                rebuild = true;
            }
        }
    }
    return PCL_OK;
    };
    int rc = run();
    if (b) (void)pcl_batch_destroy(b);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PCL_OK) PCL_FAIL(ctx, PCL_ERR_HIP, "pcl_seg_em: HIP error");
    return rc;
}

}  // extern "C"
