// Mix-up (row f9): a resident model of M mixtures per state grows to M_new by splitting its heaviest mixtures, on the device.
//   pcl_model_mixup   plan (weights only, one workgroup per state) -> a new master copy through pcl_model_alloc -> fill through the plan's
//                     origin map -> pcl_model_finish, as bootstrap.hip makes a flat-start model.  Nothing sized by M is patched in place.
// The rule (include/poccala_hip.h states it in full): per state, rounds of "the n heaviest live mixtures each give birth to one child"; parent
// and child share the halved weight and the variance, the child's mean is the parent's + perturb * sqrt(var), the parent's moves by - that.
// Built with -ffp-contract=off: perturb * sqrt(var) is one rounded product, the sum that follows another, as in NumPy.
// Every index a kernel forms is bounded by the shape the host validated: slots < M_new <= CAP, origins < M, rounds <= PLAN_MAX_ROUNDS.
#include <math.h>

#include "pcl_internal.h"

namespace {

constexpr int PLAN_T = 256;                // threads of a plan workgroup
constexpr int PLAN_Q = 4;                  // slots a thread ranks per sweep over the state's weights
constexpr int PLAN_MAX_ROUNDS = 16;        // two bits of a 32-bit word per round
constexpr int PLAN_M_MAX = 8192;           // 64 KB of weights + 9 bytes of plan per slot: 136 KB of the CU's 160 KB of LDS
enum { PLAN_OK = 0, PLAN_NO_LIVE = 1, PLAN_ROUNDS = 2 };
enum { CODE_MINUS = 1u, CODE_PLUS = 2u };  // a round's two bits: 0 = not split, the parent took -delta, the child was born with +delta

// The rounds of one state, on its weights alone.  Rank by counting: the rank of live mixture i = (live mixtures heavier than it) + (equally
// heavy ones before it), so equal weights go to the lower index; a mixture whose weight is not > 0 (zero, negative, NaN) is never counted
// and never a parent.  No atomics: two runs give the same bits.
// origin / code: [J][Mpad_new] (padding slots: origin -1, code 0), halvings: [J][Mpad_new], status: [J][2] = (PLAN_*, rounds run).
template <int CAP>
__global__ __launch_bounds__(PLAN_T) void mixup_plan_kernel(const double *__restrict__ w64, int M, int Mpad_old, int M_new, int Mpad_new, int max_rounds,
                                                            int *__restrict__ origin, unsigned int *__restrict__ code, unsigned char *__restrict__ halvings,
                                                            int *__restrict__ status) {
    __shared__ double w[CAP];
    __shared__ unsigned int cd[CAP];
    __shared__ unsigned short org[CAP], rnk[CAP];
    __shared__ unsigned char kh[CAP];
    __shared__ int wave_live[PLAN_T / 64];
    const int j = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < M_new; i += PLAN_T) {
        w[i] = i < M ? w64[(size_t)j * Mpad_old + i] : 0.0;
        org[i] = (unsigned short)(i < M ? i : 0);
        cd[i] = 0u;
        kh[i] = 0;
    }
    __syncthreads();
    int cur = M, round = 0, st = PLAN_OK;
    while (cur < M_new) {
        if (round >= max_rounds) {
            st = PLAN_ROUNDS;
            break;
        }
        // ranks of the live mixtures below cur
        int live = 0;
        for (int i0 = tid; i0 < cur; i0 += PLAN_T * PLAN_Q) {
            double key[PLAN_Q];
            int idx[PLAN_Q], r[PLAN_Q];
#pragma unroll
            for (int q = 0; q < PLAN_Q; ++q) {
                idx[q] = i0 + q * PLAN_T;
                const double v = idx[q] < cur ? w[idx[q]] : 0.0;
                key[q] = v > 0.0 ? v : -1.0;             // (-1: not live -- no weight compares equal to it, every live one lies above it)
                r[q] = 0;
            }
            for (int k = 0; k < cur; ++k) {
                const double v = w[k];                    // (the same address in every lane: a broadcast)
#pragma unroll
                for (int q = 0; q < PLAN_Q; ++q) r[q] += (v > key[q] || (v == key[q] && k < idx[q])) ? 1 : 0;
            }
#pragma unroll
            for (int q = 0; q < PLAN_Q; ++q)
                if (idx[q] < cur) {
                    const bool is_live = key[q] > 0.0;
                    rnk[idx[q]] = (unsigned short)(is_live ? r[q] : 0xffff);      // (a live rank is < cur <= 8191)
                    live += is_live ? 1 : 0;
                }
        }
        for (int o = 32; o > 0; o >>= 1) live += __shfl_down(live, o);
        if ((tid & 63) == 0) wave_live[tid >> 6] = live;
        __syncthreads();
        int n_live = 0;
#pragma unroll
        for (int k = 0; k < PLAN_T / 64; ++k) n_live += wave_live[k];
        if (n_live == 0) {                                // (uniform: every thread read the same sums)
            st = PLAN_NO_LIVE;
            break;
        }
        const int n = min(M_new - cur, n_live);
        // the n heaviest split: parent i stays in its slot, child cur + rank is new.  Slot i is written by the thread that owns i alone,
        // slot cur + rank by the one thread whose mixture has that rank.
        for (int i = tid; i < cur; i += PLAN_T) {
            const int r = rnk[i];
            if (r < n) {
                const int c = cur + r;
                const double h = 0.5 * w[i];
                const unsigned int before = cd[i];
                w[i] = h;
                w[c] = h;
                org[c] = org[i];
                kh[c] = kh[i] = (unsigned char)(kh[i] + 1);
                cd[i] = before | (CODE_MINUS << (2 * round));
                cd[c] = before | (CODE_PLUS << (2 * round));
            }
        }
        cur += n;
        ++round;
        __syncthreads();
    }
    if (tid == 0) {
        status[2 * j] = st;
        status[2 * j + 1] = round;
    }
    if (st != PLAN_OK) return;
    for (int i = tid; i < Mpad_new; i += PLAN_T) {
        const size_t o = (size_t)j * Mpad_new + i;
        const bool real = i < M_new;
        origin[o] = real ? (int)org[i] : -1;
        code[o] = real ? cd[i] : 0u;
        halvings[o] = real ? kh[i] : (unsigned char)0;
    }
}

// The new master copy's means and variances.  As the flat-start fill: a thread forms one pair of neighbouring elements of a state's block of
// Mpad_new * Dd doubles and stores it with one 16-byte store per array, consecutive lanes consecutive.  An element's source is the OLD
// model's row origin[j, m]; its mean then takes the slot's rounds in order, delta = perturb * sqrt(var) being the same in every round
// because variances are copied.  Padding mixtures / features: mean 0, variance 1, as pcl_model_upload leaves them.
__global__ __launch_bounds__(256) void mixup_fill_kernel(const double *__restrict__ old_mean, const double *__restrict__ old_var, int Mpad_old,
                                                         const int *__restrict__ origin, const unsigned int *__restrict__ code, int M_new, int Mpad_new,
                                                         int J, int Dd, int Dh, double perturb, double *__restrict__ mean64, double *__restrict__ var64) {
    const int pairs = Mpad_new * Dd / 2;                 // Mpad_new is a multiple of 4: the block has an even number of elements
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    for (int j = blockIdx.y; j < J; j += gridDim.y) {
        double mu[2], vr[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int e = 2 * p + k, m = e / Dd, d = e - m * Dd;
            mu[k] = 0.0;
            vr[k] = 1.0;
            if (m < M_new && d < Dh) {
                const size_t slot = (size_t)j * Mpad_new + m;
                const size_t src = ((size_t)j * Mpad_old + origin[slot]) * Dd + d;
                const double v = old_var[src];
                double x = old_mean[src];
                unsigned int c = code[slot];
                if (c) {
                    const double delta = perturb * sqrt(v);
                    for (; c; c >>= 2) {
                        const unsigned int bits = c & 3u;
                        if (bits == CODE_MINUS) x = x - delta;
                        else if (bits == CODE_PLUS) x = x + delta;
                    }
                }
                mu[k] = x;
                vr[k] = v;
            }
        }
        const size_t at = (size_t)j * Mpad_new * Dd + 2 * (size_t)p;
        *reinterpret_cast<double2 *>(mean64 + at) = make_double2(mu[0], mu[1]);
        *reinterpret_cast<double2 *>(var64 + at) = make_double2(vr[0], vr[1]);
    }
}

// weight = the origin's, halved once per split the slot went through (one rounded product each, as the rule does it); padding: 0
__global__ void mixup_weight_kernel(const double *__restrict__ old_w, int Mpad_old, const int *__restrict__ origin, const unsigned char *__restrict__ halvings,
                                    int J, int M_new, int Mpad_new, double *__restrict__ w64) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)J * Mpad_new) return;
    const int m = (int)(i % Mpad_new);
    double w = 0.0;
    if (m < M_new) {
        w = old_w[(i / Mpad_new) * Mpad_old + origin[i]];
        for (int k = halvings[i]; k > 0; --k) w = 0.5 * w;
    }
    w64[i] = w;
}

int ceil_log2(int n) {
    int k = 0;
    while ((1 << k) < n) ++k;
    return k;
}

}  // namespace

extern "C" int pcl_model_mixup(pcl_ctx *ctx, int M_new, double perturb, int32_t *origin_out) {
    if (!ctx) return PCL_ERR_INVALID;
    const char *who = "pcl_model_mixup";
    if (!ctx->mean64 || ctx->J <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no model uploaded", who);
    const int J = ctx->J, M = ctx->M, Mpad_old = ctx->Mpad, Dh = ctx->Dhost, flags = ctx->model_flags;
    if (M_new <= M || M_new > PLAN_M_MAX)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: M_new = %d, need more than the model's %d mixtures and at most %d", who, M_new, M, PLAN_M_MAX);
    if (!(perturb >= 0.0) || !std::isfinite(perturb)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: perturb = %g is not a finite number >= 0", who, perturb);
    // the live mixtures at least double every round until the remainder caps them: more rounds than this mean no state can be finished
    const int max_rounds = ceil_log2(M_new) + 1;
    if (max_rounds > PLAN_MAX_ROUNDS) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %d rounds do not fit the plan's %d", who, max_rounds, PLAN_MAX_ROUNDS);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int Mpad_new = (M_new + 3) / 4 * 4;
    const size_t nslot = (size_t)J * Mpad_new;
    hipStream_t st = ctx->stream;

    // the plan, and with it the check that every state can grow: nothing of the model has changed when it fails
    DevBuf<int> d_origin, d_status;
    DevBuf<unsigned int> d_code;
    DevBuf<unsigned char> d_halvings;
    TRY(d_origin.alloc(ctx, nslot));
    TRY(d_code.alloc(ctx, nslot));
    TRY(d_halvings.alloc(ctx, nslot));
    TRY(d_status.alloc(ctx, (size_t)2 * J));
    pcl_timer_begin(ctx, "mixup");
#define MIXUP_PLAN(CAP)                                                                                                                          \
    hipLaunchKernelGGL(mixup_plan_kernel<CAP>, dim3(J), dim3(PLAN_T), 0, st, ctx->w64, M, Mpad_old, M_new, Mpad_new, max_rounds, d_origin, d_code, \
                       d_halvings, d_status)
    if (M_new <= 512) MIXUP_PLAN(512);
    else if (M_new <= 2048) MIXUP_PLAN(2048);
    else MIXUP_PLAN(PLAN_M_MAX);
#undef MIXUP_PLAN
    pcl_timer_end(ctx, "mixup");
    HIPCHK(ctx, hipGetLastError());
    std::vector<int> status((size_t)2 * J);
    HIPCHK(ctx, hipMemcpyAsync(status.data(), d_status, status.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int j = 0; j < J; ++j) {
        if (status[2 * j] == PLAN_NO_LIVE)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: state %d has no mixture with a weight > 0 left to split (round %d): it cannot grow", who, j, status[2 * j + 1]);
        if (status[2 * j] != PLAN_OK) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: state %d is not finished after %d rounds", who, j, max_rounds);
    }
    std::vector<int32_t> origin_host;
    if (origin_out) {
        origin_host.resize(nslot);
        HIPCHK(ctx, hipMemcpyAsync(origin_host.data(), d_origin, nslot * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }

    // the old master copy leaves the context (pcl_model_alloc drops whatever the context holds) and lives until this call returns
    DevBuf<double> old_mean = std::move(ctx->mean64), old_var = std::move(ctx->var64), old_w = std::move(ctx->w64);
    TRY(pcl_model_alloc(ctx, J, M_new, Dh, flags, who));       // (on a failure the context has no model, as after a failed upload)
    const int Dd = ctx->D;
    const int pairs = Mpad_new * Dd / 2;
    pcl_timer_begin(ctx, "mixup");
    hipLaunchKernelGGL(mixup_fill_kernel, dim3((pairs + 255) / 256, std::min(J, 65535)), dim3(256), 0, st, old_mean, old_var, Mpad_old, d_origin, d_code, M_new, Mpad_new, J, Dd, Dh,
                       perturb, ctx->mean64, ctx->var64);
    hipLaunchKernelGGL(mixup_weight_kernel, dim3((unsigned)((nslot + 255) / 256)), dim3(256), 0, st, old_w, Mpad_old, d_origin, d_halvings, J, M_new, Mpad_new,
                       ctx->w64);
    pcl_timer_end(ctx, "mixup");
    HIPCHK(ctx, hipGetLastError());
    TRY(pcl_model_finish(ctx));                                  // (waits for the stream: the fill has read the old copy)
    if (origin_out)
        for (int j = 0; j < J; ++j) memcpy(origin_out + (size_t)j * M_new, origin_host.data() + (size_t)j * Mpad_new, (size_t)M_new * sizeof(int32_t));
    return PCL_OK;
}
