// Starting from nothing (row f7): the two steps of the reference that need no model, on the resident frames.
//   pcl_frames_moments     global mean / variance of a sub-sample of the corpus: AcousticModel.__flat_start's p_data and the k = 1 clustering
//                          it feeds it to (AcousticModel.py:479-501; Clustering.py:807-832, :955-960)
//   pcl_model_flat_start   every mixture of every state set to that Gaussian, the means pushed apart by one coefficient per mixture
//                          (AcousticModel.py:504-516), written into the float64 master copy on the device
//   pcl_uniform_segments   multi_process_data(init=True): __eq_segment mode 'e' per utterance, then __get_gmmdata's mode 'g' per chunk
//                          (AcousticModel.py:605-625, 629-644, 734-735), as the owner map pcl_seg_create sorts by
// Built with -ffp-contract=off: a product and a sum are two rounded operations, as in NumPy.
// Every index a kernel forms comes from host-validated descriptors: utterance ranges lie inside the frame matrix and do not overlap, label ids
// lie inside the inventory, and the sample's row offsets are the prefix sums the kernels search.
#include <math.h>

#include <numeric>

#include "pcl_internal.h"

namespace {

constexpr int MOM_T = 256;                 // threads of a moments workgroup: MOM_LANES row lanes x 64 feature lanes
constexpr int MOM_LANES = MOM_T / 64;
constexpr int MOM_ROWS = 1024;             // sample rows of one workgroup: the fixed partition the summation order is defined on
constexpr double VAR_FLOOR = 1e-4;         // cal_variance, Clustering.py:829-830

// Partial sums of one workgroup over its MOM_ROWS sample rows.  SQ: squared deviations about mean[] instead of the values.
// sample row g of utterance u (roff[u] <= g < roff[u + 1]) is frame row begin[u] + (g - roff[u]) * step.
template <typename T, bool SQ>
__global__ __launch_bounds__(MOM_T) void moments_partial_kernel(const T *__restrict__ frames, int FD, int Dh, const long long *__restrict__ roff,
                                                                const long long *__restrict__ begin, int n_utts, long long n, int step,
                                                                const double *__restrict__ mean, double *__restrict__ partial) {
    __shared__ double lane_sum[MOM_LANES][64];
    const int d = threadIdx.x & 63, r = threadIdx.x >> 6;
    const long long lo = (long long)blockIdx.x * MOM_ROWS, hi = min(n, lo + MOM_ROWS);
    double acc = 0.0;
    if (d < Dh && lo + r < hi) {
        const double mu = SQ ? mean[d] : 0.0;
        int u = 0;                                       // the utterance of the first row: the last u with roff[u] <= g
        for (int a = 0, b = n_utts - 1; a <= b;) {
            const int mid = (a + b) >> 1;
            if (roff[mid] <= lo + r) u = mid, a = mid + 1;
            else b = mid - 1;
        }
        for (long long g = lo + r; g < hi; g += MOM_LANES) {
            while (u + 1 < n_utts && roff[u + 1] <= g) ++u;      // (utterances without a sample row have roff[u + 1] == roff[u])
            const long long row = begin[u] + (g - roff[u]) * (long long)step;
            const double x = (double)frames[row * FD + d];
            if (SQ) {
                const double dv = x - mu;
                acc += dv * dv;
            } else {
                acc += x;
            }
        }
    }
    lane_sum[r][d] = acc;
    __syncthreads();
    if (r == 0) {
        double s = lane_sum[0][d];
#pragma unroll
        for (int k = 1; k < MOM_LANES; ++k) s += lane_sum[k][d];
        partial[(size_t)blockIdx.x * 64 + d] = s;
    }
}

// One workgroup: the workgroups' partial sums in ascending index order, then the mean, or the floored variance through sqrt and square.
template <bool VAR>
__global__ __launch_bounds__(64) void moments_final_kernel(const double *__restrict__ partial, int n_blocks, long long n, int Dh, double *__restrict__ out) {
    const int d = threadIdx.x;
    if (d >= Dh) return;
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b) s += partial[(size_t)b * 64 + d];
    double v = s / (double)n;
    if (VAR) {
        if (v < VAR_FLOOR) v = VAR_FLOOR;
        const double sd = sqrt(v);
        v = sd * sd;
    }
    out[d] = v;
}

// The master copy of a flat-start model.  One state's block of Mpad * Dd doubles is the same for every state: a thread forms one pair of
// neighbouring elements once and stores it into the block of every state of its grid row (16-byte stores, consecutive lanes consecutive).
__global__ __launch_bounds__(256) void flat_fill_kernel(const double *__restrict__ mean, const double *__restrict__ var, const double *__restrict__ coeff,
                                                        int J, int M, int Mpad, int Dd, int Dh, double *__restrict__ mean64, double *__restrict__ var64) {
    const int pairs = Mpad * Dd / 2;                     // Mpad is a multiple of 4: the block has an even number of elements
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    double mu[2], vr[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = 2 * p + k, m = e / Dd, d = e - m * Dd;
        const bool real = m < M && d < Dh;               // padding mixtures / features: mean 0, variance 1, as pcl_model_upload leaves them
        vr[k] = real ? var[d] : 1.0;
        mu[k] = real ? (coeff ? mean[d] + coeff[m] * var[d] : mean[d]) : 0.0;
    }
    const double2 mu2 = make_double2(mu[0], mu[1]), vr2 = make_double2(vr[0], vr[1]);
    const size_t block = (size_t)Mpad * Dd;
    for (int j = blockIdx.y; j < J; j += gridDim.y) {
        *reinterpret_cast<double2 *>(mean64 + (size_t)j * block + 2 * (size_t)p) = mu2;
        *reinterpret_cast<double2 *>(var64 + (size_t)j * block + 2 * (size_t)p) = vr2;
    }
}

__global__ void flat_weight_kernel(int J, int M, int Mpad, double *__restrict__ w64) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)J * Mpad) return;
    w64[i] = (int)(i % Mpad) < M ? 1.0 / (double)M : 0.0;
}

// Owner state of every frame of the batch's utterances (the rest of the map was set to -1 before): one workgroup row per utterance.
__global__ __launch_bounds__(256) void uniform_map_kernel(const int *__restrict__ label_len, const long long *__restrict__ label_off, const int *__restrict__ labels,
                                                          const int *__restrict__ T, const long long *__restrict__ begin, int gmm_num, int *__restrict__ frame_state) {
    const int u = blockIdx.y;
    const int L = label_len[u], Tu = T[u];
    if (L <= 0) return;
    const int chunk = Tu / L;                            // __eq_segment mode 'e' (:606)
    if (chunk == 0) return;
    const int used = chunk * L, c2 = chunk / gmm_num;    // mode 'g' (:614)
    const int *lab = labels + label_off[u];
    int *dst = frame_state + begin[u];
    for (int t = blockIdx.x * 256 + threadIdx.x; t < used; t += gridDim.x * 256) {
        const int i = t / chunk, rr = t - i * chunk;
        const int k = c2 > 0 ? min(rr / c2, gmm_num - 1) : gmm_num - 1;
        dst[t] = lab[i] * gmm_num + k;
    }
}

// utterance ranges against the current frame matrix; begin_out = frame_begin, or the utterances back to back
int check_ranges(pcl_ctx *ctx, const char *who, int U, const int32_t *T, const int64_t *frame_begin, std::vector<long long> &begin_out) {
    begin_out.resize(U);
    long long run = 0;
    for (int u = 0; u < U; ++u) {
        const long long b = frame_begin ? (long long)frame_begin[u] : run;
        if (T[u] < 0 || b < 0 || b + T[u] > (long long)ctx->F)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d (rows %lld .. %lld) lies outside the uploaded frame matrix of %lld rows", who, u, b, b + T[u],
                     (long long)ctx->F);
        begin_out[u] = b;
        run += T[u];
    }
    return PCL_OK;
}

// The moments of the sample into d_mean / d_var (device, 64 doubles each), complete on return.
int moments_device(pcl_ctx *ctx, const char *who, int U, const int32_t *T, const int64_t *frame_begin, int n_utts, int step, double *d_mean, double *d_var,
                   long long *n_out) {
    if (U < 1 || !T) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: no utterances", who);
    if (n_utts < 1 || n_utts > U) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: n_utts = %d, need 1 .. %d (int(file_count * proportion) of the caller)", who, n_utts, U);
    if (step < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: step = %d, need >= 1", who, step);
    if (!ctx->frames32 || ctx->F == 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: no frames uploaded", who);
    std::vector<long long> begin;
    TRY(check_ranges(ctx, who, n_utts, T, frame_begin, begin));
    std::vector<long long> roff(n_utts + 1, 0);
    for (int u = 0; u < n_utts; ++u) roff[u + 1] = roff[u] + ((long long)T[u] + step - 1) / step;      // len(data[::step])
    const long long n = roff[n_utts];
    if (n == 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the first %d utterances have no frame: empty sample", who, n_utts);
    const long long n_blocks_ll = (n + MOM_ROWS - 1) / MOM_ROWS;
    if (n_blocks_ll > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: sample of %lld rows is too large", who, n);
    const int n_blocks = (int)n_blocks_ll;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf<long long> d_roff, d_begin;
    DevBuf<double> d_partial;
    TRY(d_roff.alloc(ctx, roff.size()));
    TRY(d_begin.alloc(ctx, begin.size()));
    TRY(d_partial.alloc(ctx, (size_t)n_blocks * 64));
    HIPCHK(ctx, pcl_h2d(ctx, d_roff, roff.data(), roff.size() * sizeof(long long)));
    HIPCHK(ctx, pcl_h2d(ctx, d_begin, begin.data(), begin.size() * sizeof(long long)));
    const int FD = ctx->FD, Dh = ctx->FDhost;
    hipStream_t st = ctx->stream;
#define MOM_PARTIAL(TY, SQ, FR)                                                                                                                     \
    hipLaunchKernelGGL((moments_partial_kernel<TY, SQ>), dim3(n_blocks), dim3(MOM_T), 0, st, FR, FD, Dh, d_roff, d_begin, \
                       n_utts, n, step, d_mean, d_partial)
    const bool f64 = ctx->frames64 != nullptr;
    pcl_timer_begin(ctx, "moments");
    if (f64) MOM_PARTIAL(double, false, ctx->frames64);
    else MOM_PARTIAL(float, false, ctx->frames32);
    hipLaunchKernelGGL(moments_final_kernel<false>, dim3(1), dim3(64), 0, st, d_partial, n_blocks, n, Dh, d_mean);
    if (f64) MOM_PARTIAL(double, true, ctx->frames64);
    else MOM_PARTIAL(float, true, ctx->frames32);
    hipLaunchKernelGGL(moments_final_kernel<true>, dim3(1), dim3(64), 0, st, d_partial, n_blocks, n, Dh, d_var);
#undef MOM_PARTIAL
    pcl_timer_end(ctx, "moments");
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    *n_out = n;
    return PCL_OK;
}

int moments_to_host(pcl_ctx *ctx, const double *d_mean, const double *d_var, double *mean_out, double *var_out) {
    const size_t bytes = (size_t)ctx->FDhost * sizeof(double);
    if (mean_out) HIPCHK(ctx, hipMemcpyAsync(mean_out, d_mean, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (var_out) HIPCHK(ctx, hipMemcpyAsync(var_out, d_var, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

// The model from mean / var / coeff ON THE DEVICE (D, D, M doubles; coeff may be nullptr).
int flat_start_device(pcl_ctx *ctx, const char *who, int J, int M, int D, const double *d_mean, const double *d_var, const double *d_coeff, int flags) {
    TRY(pcl_model_alloc(ctx, J, M, D, flags, who));
    const int Mpad = ctx->Mpad, Dd = ctx->D;
    const int pairs = Mpad * Dd / 2;
    const int gx = (pairs + 255) / 256;
    const int gy = std::max(1, std::min(J, 16384 / gx));
    pcl_timer_begin(ctx, "flat_fill");
    hipLaunchKernelGGL(flat_fill_kernel, dim3(gx, gy), dim3(256), 0, ctx->stream, d_mean, d_var, d_coeff, J, M, Mpad, Dd, D, ctx->mean64, ctx->var64);
    const size_t nw = (size_t)J * Mpad;
    hipLaunchKernelGGL(flat_weight_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, ctx->stream, J, M, Mpad, ctx->w64);
    pcl_timer_end(ctx, "flat_fill");
    HIPCHK(ctx, hipGetLastError());
    return pcl_model_finish(ctx);
}

int check_coeff(pcl_ctx *ctx, const char *who, int M, const double *coeff) {
    if (coeff)
        for (int m = 0; m < M; ++m)
            if (!std::isfinite(coeff[m])) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: coeff[%d] = %g is not finite", who, m, coeff[m]);
    return PCL_OK;
}

int check_shape(pcl_ctx *ctx, const char *who, int J, int M, int D) {
    if (J <= 0 || M <= 0 || D <= 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: bad shape J=%d M=%d D=%d", who, J, M, D);
    if (pcl_device_dim(D) < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d > 64 is not supported", who, D);
    return PCL_OK;
}

}  // namespace

extern "C" {

int pcl_frames_moments(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, int n_utts, int step, double *mean_out, double *var_out,
                       int64_t *n_rows_out) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!mean_out || !var_out) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_frames_moments: NULL destination");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf<double> d_mv;
    TRY(d_mv.alloc(ctx, 128));
    long long n = 0;
    TRY(moments_device(ctx, "pcl_frames_moments", U, T, frame_begin, n_utts, step, d_mv, d_mv + 64, &n));
    TRY(moments_to_host(ctx, d_mv, d_mv + 64, mean_out, var_out));
    if (n_rows_out) *n_rows_out = n;
    return PCL_OK;
}

int pcl_model_flat_start(pcl_ctx *ctx, int J, int M, int D, const double *mean, const double *var, const double *coeff, int flags) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_model_flat_start";
    if (!mean || !var) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: NULL mean / var", who);
    TRY(check_shape(ctx, who, J, M, D));
    for (int d = 0; d < D; ++d) {
        if (!(var[d] > 0.0) || !std::isfinite(var[d])) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: variance[%d] = %g is not positive and finite", who, d, var[d]);
        if (!std::isfinite(mean[d])) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: mean[%d] = %g is not finite", who, d, mean[d]);
    }
    TRY(check_coeff(ctx, who, M, coeff));
    if (ctx->frames32 && ctx->F > 0 && ctx->FDhost != D)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: D = %d, the frame matrix in place has %d features", who, D, ctx->FDhost);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf<double> d_in;
    TRY(d_in.alloc(ctx, (size_t)(2 * D + M)));
    double *d_mean = d_in, *d_var = d_mean + D, *d_coeff = coeff ? d_var + D : nullptr;
    HIPCHK(ctx, pcl_h2d(ctx, d_mean, mean, (size_t)D * sizeof(double)));
    HIPCHK(ctx, pcl_h2d(ctx, d_var, var, (size_t)D * sizeof(double)));
    if (coeff) HIPCHK(ctx, pcl_h2d(ctx, d_coeff, coeff, (size_t)M * sizeof(double)));
    return flat_start_device(ctx, who, J, M, D, d_mean, d_var, d_coeff, flags);
}

int pcl_flat_start(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, int n_utts, int step, int J, int M, const double *coeff, int flags,
                   double *mean_out, double *var_out, int64_t *n_rows_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_flat_start";
    if (!ctx->frames32 || ctx->F == 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: no frames uploaded", who);
    const int D = ctx->FDhost;
    TRY(check_shape(ctx, who, J, M, D));
    TRY(check_coeff(ctx, who, M, coeff));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf<double> d_mv, d_c;
    TRY(d_mv.alloc(ctx, 128));
    TRY(d_c.alloc(ctx, (size_t)M));
    long long n = 0;
    TRY(moments_device(ctx, who, U, T, frame_begin, n_utts, step, d_mv, d_mv + 64, &n));
    // (a non-finite frame makes the moments NaN: they are read back before the model in place is given up)
    std::vector<double> mv(2 * (size_t)D);
    TRY(moments_to_host(ctx, d_mv, d_mv + 64, mv.data(), mv.data() + D));
    for (int d = 0; d < D; ++d)
        if (!std::isfinite(mv[d]) || !std::isfinite(mv[D + d]))
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature %d of the sample has mean %g, variance %g (non-finite frames)", who, d, mv[d], mv[D + d]);
    if (coeff) HIPCHK(ctx, pcl_h2d(ctx, d_c, coeff, (size_t)M * sizeof(double)));
    TRY(flat_start_device(ctx, who, J, M, D, d_mv, d_mv + 64, coeff ? d_c : nullptr, flags));
    if (mean_out) memcpy(mean_out, mv.data(), (size_t)D * sizeof(double));
    if (var_out) memcpy(var_out, mv.data() + D, (size_t)D * sizeof(double));
    if (n_rows_out) *n_rows_out = n;
    return PCL_OK;
}

int pcl_uniform_segments(pcl_ctx *ctx, int U, const int32_t *label_len, const int32_t *labels, const int32_t *T, const int64_t *frame_begin, int gmm_num,
                         int J, int32_t *frame_state_out, pcl_seg **out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_uniform_segments";
    if (out) *out = nullptr;
    if (!frame_state_out && !out) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: neither frame_state_out nor out is given", who);
    if (U < 1 || U > 65535 || !label_len || !labels || !T) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: bad arguments (U=%d, 1 .. 65535 utterances)", who, U);
    if (gmm_num < 1 || J < 1 || J > 65535 || J % gmm_num != 0)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: J = %d must be a multiple of gmm_num = %d (and at most 65535)", who, J, gmm_num);
    if (!ctx->frames32 || ctx->F == 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: no frames uploaded", who);
    if (ctx->F > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: frame matrix of %lld rows", who, (long long)ctx->F);
    const int n_units = J / gmm_num;
    std::vector<long long> begin, loff(U + 1, 0);
    TRY(check_ranges(ctx, who, U, T, frame_begin, begin));
    for (int u = 0; u < U; ++u) {
        if (label_len[u] < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: label_len[%d] = %d", who, u, label_len[u]);
        loff[u + 1] = loff[u] + label_len[u];
    }
    for (long long i = 0; i < loff[U]; ++i)
        if (labels[i] < 0 || labels[i] >= n_units)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: label %lld = %d is not a unit in [0,%d) (J / gmm_num)", who, i, labels[i], n_units);
    {   // a frame has one owner: the utterances' row ranges are disjoint
        std::vector<int> by(U);
        std::iota(by.begin(), by.end(), 0);
        std::sort(by.begin(), by.end(), [&](int a, int b) { return begin[a] != begin[b] ? begin[a] < begin[b] : a < b; });
        long long end = 0;
        int prev = -1;
        for (int u : by) {
            if (T[u] == 0) continue;
            if (begin[u] < end) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterances %d and %d overlap in the frame matrix", who, prev, u);
            end = begin[u] + T[u];
            prev = u;
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long F = ctx->F;
    DevBuf<int> d_state, d_ll, d_lab, d_T;
    DevBuf<long long> d_lo, d_begin;
    TRY(d_state.alloc(ctx, (size_t)F));
    TRY(d_ll.alloc(ctx, (size_t)U));
    TRY(d_lo.alloc(ctx, (size_t)(U + 1)));
    TRY(d_lab.alloc(ctx, (size_t)std::max<long long>(1, loff[U])));
    TRY(d_T.alloc(ctx, (size_t)U));
    TRY(d_begin.alloc(ctx, (size_t)U));
    HIPCHK(ctx, pcl_h2d(ctx, d_ll, label_len, (size_t)U * sizeof(int)));
    HIPCHK(ctx, pcl_h2d(ctx, d_lo, loff.data(), (size_t)(U + 1) * sizeof(long long)));
    HIPCHK(ctx, pcl_h2d(ctx, d_lab, labels, (size_t)loff[U] * sizeof(int)));
    HIPCHK(ctx, pcl_h2d(ctx, d_T, T, (size_t)U * sizeof(int)));
    HIPCHK(ctx, pcl_h2d(ctx, d_begin, begin.data(), (size_t)U * sizeof(long long)));
    HIPCHK(ctx, hipMemsetAsync(d_state, 0xff, (size_t)F * sizeof(int), ctx->stream));
    int Tmax = 1;
    for (int u = 0; u < U; ++u) Tmax = std::max(Tmax, (int)T[u]);
    hipLaunchKernelGGL(uniform_map_kernel, dim3(std::min(64, (Tmax + 255) / 256), U), dim3(256), 0, ctx->stream, d_ll, d_lo, d_lab,
                       d_T, d_begin, gmm_num, d_state);
    HIPCHK(ctx, hipGetLastError());
    if (frame_state_out) HIPCHK(ctx, hipMemcpyAsync(frame_state_out, d_state, (size_t)F * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (out) TRY(pcl_seg_create_device(ctx, F, J, d_state, out));
    return PCL_OK;
}

}  // extern "C"
