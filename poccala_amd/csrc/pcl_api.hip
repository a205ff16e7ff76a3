// pcl_api.hip -- host side of the C-ABI declared in include/poccala_hip.h.
// Owns device memory, builds the state-major scoring work lists and the sparse transition
// structure, and launches the kernels in gmm_score.hip / hmm_dp.hip / gmm_accumulate.hip.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>

#include "pcl_internal.h"

static std::string g_init_error;

void pcl_set_error(pcl_ctx *ctx, const char *msg) {
    if (ctx) ctx->err = msg;
    else g_init_error = msg;
}

// ---------------------------------------------------------------- timers (HIP events on ctx->stream)
// Opt-in (pcl_timing_enable / env PCL_TIMERS=1): a training run that never asks for kernel times must not pay two
// hipEventCreate per launch nor keep the events alive until the context dies.
void pcl_timer_begin(pcl_ctx *ctx, const char *which) {
    if (!ctx->timing) return;
    TimedEventPair p;
    if (p.make() != hipSuccess) return;
    hipEventRecord(p.first, ctx->stream);
    ctx->timers[which].ev.push_back(std::move(p));
}
void pcl_timer_end(pcl_ctx *ctx, const char *which) {
    if (!ctx->timing) return;
    auto &t = ctx->timers[which];
    if (!t.ev.empty()) hipEventRecord(t.ev.back().second, ctx->stream);
}

void pcl_timer_host(pcl_ctx *ctx, const char *which, double ms) {
    if (!ctx->timing) return;
    auto &t = ctx->timers[which];
    t.host_ms += ms;
    ++t.host_n;
}

// ================================================================ device memory pool
// Size classes: powers of two up to 1 MiB, eighths of a power of two above (a block wastes < 12.5 %), so that batches of
// similar shape -- the chunks of a ragged stream, the one-utterance batches of the drop-in classes -- reuse each other's
// blocks.  The cache is trimmed (largest blocks first) when it exceeds PCL_POOL_MAX_MB (default 65536), and released
// altogether before an allocation is reported as failed.
thread_local int pcl_tls_free_synced = 0;
namespace {
struct PoolBlock { size_t bytes; int device; };
std::mutex g_pool_mu;
std::unordered_map<void *, PoolBlock> g_pool_live;                 // every block handed out or cached
std::multimap<std::pair<int, size_t>, void *> g_pool_free;           // (device, class bytes) -> cached block
size_t g_pool_cached = 0;
uint64_t g_pool_device_allocs = 0, g_pool_device_waits = 0;         // successful hipMalloc calls / device-wide waits of pcl_pool_free (pcl_pool_stats)
size_t pool_class(size_t n) {
    if (n <= 256) return 256;
    size_t p2 = 256;
    while (p2 < n) p2 <<= 1;
    if (p2 <= (1u << 20)) return p2;
    const size_t step = p2 >> 4;                                    // eighths of the lower power of two
    return (n + step - 1) / step * step;
}
size_t pool_limit() {
    static const size_t lim = (size_t)(getenv("PCL_POOL_MAX_MB") ? atol(getenv("PCL_POOL_MAX_MB")) : 65536) << 20;
    return lim;
}
void pool_release_locked(size_t keep) {                              // hipFree cached blocks, largest first, down to `keep` bytes
    while (g_pool_cached > keep && !g_pool_free.empty()) {
        auto best = g_pool_free.begin();
        for (auto it = g_pool_free.begin(); it != g_pool_free.end(); ++it)
            if (it->first.second > best->first.second) best = it;
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != best->first.first) (void)hipSetDevice(best->first.first);
        (void)hipFree(best->second);
        if (cur != best->first.first) (void)hipSetDevice(cur);
        g_pool_cached -= best->first.second;
        g_pool_live.erase(best->second);
        g_pool_free.erase(best);
    }
}
}  // namespace

void *pcl_pool_alloc(int device, size_t bytes) {
    const size_t cls = pool_class(bytes);
    std::lock_guard<std::mutex> lock(g_pool_mu);
    auto it = g_pool_free.find(std::make_pair(device, cls));
    if (it != g_pool_free.end()) {
        void *p = it->second;
        g_pool_free.erase(it);
        g_pool_cached -= cls;
        return p;
    }
    void *p = nullptr;
    if (hipMalloc(&p, cls) != hipSuccess) {
        (void)hipGetLastError();
        pool_release_locked(0);                                      // give the cache back and try once more
        if (hipMalloc(&p, cls) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
    }
    ++g_pool_device_allocs;
    g_pool_live[p] = PoolBlock{cls, device};                        // (overwrites a stale entry, should a block ever have left the pool by a raw hipFree)
    return p;
}

void pcl_pool_free(void *p) {
    if (!p) return;
    const bool wait = pcl_tls_free_synced <= 0;
    if (wait) (void)hipDeviceSynchronize();                         // what hipFree did: nobody on the device still uses the block
    std::lock_guard<std::mutex> lock(g_pool_mu);
    if (wait) ++g_pool_device_waits;
    auto it = g_pool_live.find(p);
    if (it == g_pool_live.end()) {                                   // not ours (never happens): the runtime's problem
        (void)hipFree(p);
        return;
    }
    g_pool_free.emplace(std::make_pair(it->second.device, it->second.bytes), p);
    g_pool_cached += it->second.bytes;
    if (g_pool_cached > pool_limit()) pool_release_locked(pool_limit() / 2);
}

extern "C" int pcl_pool_stats(size_t *handed_out_blocks, size_t *handed_out_bytes, size_t *cached_bytes, uint64_t *device_allocs, uint64_t *device_waits) {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    size_t live_bytes = 0;
    for (const auto &kv : g_pool_live) live_bytes += kv.second.bytes;
    if (handed_out_blocks) *handed_out_blocks = g_pool_live.size() - g_pool_free.size();
    if (handed_out_bytes) *handed_out_bytes = live_bytes - g_pool_cached;
    if (cached_bytes) *cached_bytes = g_pool_cached;
    if (device_allocs) *device_allocs = g_pool_device_allocs;
    if (device_waits) *device_waits = g_pool_device_waits;
    return PCL_OK;
}

// ---------------------------------------------------------------- descriptor uploads (pcl_desc_group, pcl_internal.h)
namespace {
__global__ void desc_copy_kernel(DescCopyArgs a, const char *__restrict__ stage) {
    const int e = blockIdx.y;
    if (e >= a.n) return;
    const unsigned long long n = a.bytes[e];                          // (0: the entry was superseded by a later upload of the same array)
    if (n == 0) return;
    const char *src = stage + a.off[e];
    char *dst = (char *)a.dst[e];
    const unsigned long long n16 = n / 16;                            // (staging offsets and pool blocks are 256-byte aligned)
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n16; i += (unsigned long long)gridDim.x * blockDim.x)
        ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
    if (blockIdx.x == 0)
        for (unsigned long long i = n16 * 16 + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}
}  // namespace

hipError_t pcl_desc_launch(pcl_ctx *ctx, const DescCopyArgs &a, const char *pin) {
    void *dev_stage = nullptr;
    hipError_t e = hipHostGetDevicePointer(&dev_stage, const_cast<char *>(pin), 0);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(desc_copy_kernel, dim3(32, a.n), dim3(256), 0, ctx->stream_desc, a, (const char *)dev_stage);
    e = hipGetLastError();
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream_desc);
}

static int pcl_batch_reap(pcl_ctx *ctx, bool wait);   // frees the destroyed batches the GPU is done with (wait: all of them); returns how many are left

extern "C" {

// ================================================================ context
static void free_model(pcl_ctx *ctx) {
    pcl_accumulate_release(ctx);                                 // (sized for the model's states and mixtures)
    pcl_coarse_release(ctx);
    ctx->nbad.clear();
    if (ctx->zero_pending && ctx->ev_zero) (void)hipEventSynchronize(ctx->ev_zero);
    ctx->zero_pending = false;
    static_cast<ModelDev &>(*ctx) = {};                          // the master copy, every derived layout, the statistics block
    ctx->st_acc = ctx->st_alpha = ctx->st_mean = ctx->st_cov = nullptr;
    ctx->J = ctx->M = ctx->Mpad = 0;
}

// frames32 is a view of either the plain upload (which goes) or a streaming slot (which stays)
static void release_frames32(pcl_ctx *ctx) {
    if (ctx->frames_front < 0) ctx->frames_up.release();
    ctx->frames32 = nullptr;
    ctx->frames_front = -1;
}

// The streams and the environment's knobs of a fresh context.  On a failure the caller unwinds through ctx_teardown.
static int ctx_setup(pcl_ctx *ctx) {
    HIPCHK(nullptr, hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess) ctx->cus = prop.multiProcessorCount;
    // (compute units set aside for the second stream with hipExtStreamCreateWithCUMask were tried in round 4: 8 of 256 cost the scoring
    //  kernel 20 %, 16 cost 70 %, and the posterior kernel's in-loop span did not move -- it waits for registers, not for CUs)
    HIPCHK(nullptr, ctx->stream_main.make(StreamKind::Plain));
    ctx->stream = ctx->stream_main;
    HIPCHK(nullptr, ctx->stream_dp.make(StreamKind::HighPriority));                            // (priority 0 measured: no difference)
    HIPCHK(nullptr, ctx->stream_aux.make(StreamKind::Plain));
    HIPCHK(nullptr, ctx->stream_desc.make(StreamKind::NonBlocking));
    HIPCHK(nullptr, ctx->stream_d2h.make(StreamKind::NonBlocking));
    // PCL_SCORE_VARIANT: 7 (default) = f32-class contraction on the f16 matrix pipe, 3 = strict f32 on the f32-input MFMA,
    // 1 = direct form on the VALU (the kernels states leave the matrix pipe for: fix-up, ill-conditioned models)
    const char *var = getenv("PCL_SCORE_VARIANT");
    ctx->score_variant = var ? atoi(var) : 7;
    if (ctx->score_variant != 1 && ctx->score_variant != 3 && ctx->score_variant != 7)
        PCL_FAIL(nullptr, PCL_ERR_INVALID, "pcl_init: PCL_SCORE_VARIANT must be 1, 3 or 7");
    if (const char *cm = getenv("PCL_MFMA_COND_MAX")) ctx->cond_max = (float)atof(cm);
    if (const char *sm = getenv("PCL_SPLIT_MAX")) {
        ctx->split_frac = std::min(1.0f, std::max(0.0f, (float)atof(sm)));
        ctx->split_frac_set = true;
    }
    if (const char *ds = getenv("PCL_DP_STREAM")) ctx->dp_async = atoi(ds) != 0;
    if (const char *co = getenv("PCL_COARSE")) ctx->coarse_on = atoi(co) != 0;
    if (const char *cm2 = getenv("PCL_COMPACT_MAIN")) ctx->compact_main = atoi(cm2) != 0;
    if (const char *cs = getenv("PCL_COARSE_STATS")) ctx->coarse_stats = atoi(cs) != 0;
    if (const char *cp = getenv("PCL_COARSE_PASSES")) ctx->coarse_np = atoi(cp) == 3 ? 3 : 1;
    if (const char *cm_ = getenv("PCL_COARSE_SPLIT_MAX")) ctx->coarse_split_frac = std::min(1.0f, std::max(0.0f, (float)atof(cm_)));   // (scoring only: A/B, tests)
    if (const char *tm = getenv("PCL_TIMERS")) ctx->timing = atoi(tm) != 0;
    return PCL_OK;
}

// Everything a context holds goes.  Spelled out, in this order, are the steps whose order is a decision: the communicator (collectives and the
// pipelined exchange run on the context's streams and stream_comm; rounds 1-5 destroyed it first), the buried batches, and zero_pending
// (round 6, tools/lifecycle_stress.py: a context destroyed with an asynchronous pcl_stats_zero still un-joined had ev_zero destroyed here
// and then synchronised on by free_model: a use of a dead event, SIGSEGV inside the runtime -- nothing may wait on an event from here on).
// Everything else is given back by its owner when `delete ctx` destroys the members, the streams last (see pcl_ctx).  The caller has DRAINED
// the streams (pcl_destroy); a context pcl_init gives up on has queued nothing.  Every handle may be null.
static void ctx_teardown(pcl_ctx *ctx) {
    pcl_comm_destroy(ctx);
    pcl_batch_reap(ctx, true);
    ctx->zero_pending = false;
    delete ctx;
}

int pcl_init(int device, pcl_ctx **out) {
    if (!out) PCL_FAIL(nullptr, PCL_ERR_INVALID, "pcl_init: out is NULL");
    *out = nullptr;
    // five streams per context on the runtime's default of four hardware queues would make two of them share one (see poccala_amd/_lib.py);
    // honoured only if the HIP runtime has not started yet -- a C caller that initialises HIP first exports GPU_MAX_HW_QUEUES=8 itself
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        PCL_FAIL(nullptr, PCL_ERR_HIP, "pcl_init: no HIP device (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) PCL_FAIL(nullptr, PCL_ERR_INVALID, "pcl_init: device %d out of range [0,%d)", device, n);
    pcl_ctx *ctx = new pcl_ctx();
    ctx->device = device;
    const int rc = ctx_setup(ctx);
    if (rc != PCL_OK) {
        ctx_teardown(ctx);                                       // (the message is pcl_last_error(NULL)'s)
        return rc;
    }
    *out = ctx;
    return PCL_OK;
}

int pcl_destroy(pcl_ctx *ctx) {
    if (!ctx) return PCL_OK;
    hipSetDevice(ctx->device);
    // Drain first, release second: every stream of the context (twice -- a stream drained early may have been handed work by an event
    // of one drained later only in the sense that its wait completes; nothing new is queued, so the second round returns at once and
    // is there for the reader), THEN ctx_teardown.  No member of the context gives anything back before this point.
    for (int round = 0; round < 2; ++round) {
        for (hipStream_t s : ctx->streams())
            if (s) hipStreamSynchronize(s);
    }
    ctx_teardown(ctx);
    return PCL_OK;
}

const char *pcl_last_error(pcl_ctx *ctx) { return ctx ? ctx->err.c_str() : g_init_error.c_str(); }

// the two streams kernels are timed on
static int sync_main_and_dp(pcl_ctx *ctx) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream_dp));
    return PCL_OK;
}

int pcl_sync(pcl_ctx *ctx) {
    if (!ctx) return PCL_ERR_INVALID;
    TRY(sync_main_and_dp(ctx));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream_aux));
    if (ctx->stream_d2h) HIPCHK(ctx, hipStreamSynchronize(ctx->stream_d2h));
    pcl_batch_reap(ctx, false);
    return PCL_OK;
}

// The dynamic-programming kernels of a batch run on a second, higher-priority stream (one wave per utterance, no
// matrix work: they fit beside another batch's scoring).  Anything else that touches the batch on the main stream
// first orders the main stream behind them.
static int batch_join(pcl_batch *b) {
    if (b->dp_pending) {
        HIPCHK(b->ctx, hipStreamWaitEvent(b->ctx->stream, b->ev_dp, 0));
        b->dp_pending = false;
    }
    if (b->fetch_pending) {                                  // result copies still reading this batch's buffers (pcl_batch_fetch_async)
        HIPCHK(b->ctx, hipStreamWaitEvent(b->ctx->stream, b->ev_fetch, 0));
        b->fetch_pending = false;
    }
    return PCL_OK;
}

int pcl_device_info(pcl_ctx *ctx, char *name, int cap, int *cus, size_t *hbm_bytes) {
    if (!ctx) return PCL_ERR_INVALID;
    hipDeviceProp_t prop;
    HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
    if (name && cap > 0) snprintf(name, cap, "%s (%s)", prop.name, prop.gcnArchName);
    if (cus) *cus = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return PCL_OK;
}

int pcl_timing_enable(pcl_ctx *ctx, int on) {
    if (!ctx) return PCL_ERR_INVALID;
    TRY(sync_main_and_dp(ctx));
    if (!on) ctx->timers.clear();                                // (every group's event pairs and host-clock entries)
    ctx->timing = on != 0;
    return PCL_OK;
}

int pcl_kernel_time(pcl_ctx *ctx, const char *which, float *total_ms, int *launches) {
    if (!ctx || !which) return PCL_ERR_INVALID;
    TRY(sync_main_and_dp(ctx));
    float tot = 0.f;
    int n = 0;
    auto it = ctx->timers.find(which);
    if (it != ctx->timers.end()) {
        for (auto &p : it->second.ev) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
                tot += ms;
                ++n;
            }
        }
        it->second.ev.clear();
        tot += (float)it->second.host_ms;
        n += it->second.host_n;
        it->second.host_ms = 0.0;
        it->second.host_n = 0;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
    return PCL_OK;
}

// ================================================================ model
// Device feature dimension.  Up to 47 it is one of 13 / 26 / 39 / 47 -- the sizes with a spare K slot in their last k-step of
// 8, which the matrix-pipe kernels need for the folded constants -- so that EVERY model of up to 47 features is scored and
// accumulated on the matrix pipe (the padding features are zero in the frames and carry zero coefficients; round 2 padded
// e.g. D = 20 to 24 and silently dropped it to the 4-5x slower VALU kernels).  Above: 48 / 64 on the VALU kernels.
static int device_dim(int D) {
    const int pipe[] = {13, 26, 39, 47};
    for (int o : pipe)
        if (D <= o) return o;
    const int opts[] = {48, 64};
    for (int o : opts)
        if (D <= o) return o;
    return -1;
}

int pcl_device_dim(int D) { return device_dim(D); }

// The front-end (vad.hip) built the frame matrix on the device: make it the current one, as pcl_frames_upload does with a host matrix.
void pcl_frames_adopt(pcl_ctx *ctx, DevBuf<float> &&f32, DevBuf<double> &&f64, int64_t F, int D) {
    release_frames32(ctx);
    ctx->frames64.release();
    ctx->frames_up = std::move(f32);
    ctx->frames32 = ctx->frames_up;
    ctx->frames64 = std::move(f64);
    ctx->F = F;
    ctx->FD = device_dim(D);
    ctx->FDhost = D;
    if (ctx->fmllr_Gk && D != ctx->Dhost) pcl_fmllr_release(ctx);
    if (ctx->mllt_F && D != ctx->Dhost) pcl_mllt_release(ctx);
}

// The first half of pcl_model_upload (also bootstrap.hip: a model made on the device): the old model goes, the master copy and every derived
// buffer of a (J, M, D) model are allocated, the shape fields set.  The master copy's contents are the caller's to write.
int pcl_model_alloc(pcl_ctx *ctx, int J, int M, int D, int flags, const char *who) {
    if (J <= 0 || M <= 0 || D <= 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: bad shape J=%d M=%d D=%d", who, J, M, D);
    const int Dd = device_dim(D);
    if (Dd < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: feature dimension %d > 64 is not supported", who, D);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    free_model(ctx);
    const int Mpad = (M + 3) / 4 * 4;
    const int row = (2 * Dd + 1 + 3) / 4 * 4;
    const int Mp32 = (M + 31) / 32 * 32, KS4 = (Dd + 1 + 3) / 4;
    const size_t nm = (size_t)J * Mpad * Dd, nw = (size_t)J * Mpad;
    const size_t npm = (size_t)J * (Mp32 / 32) * KS4 * 64 * 4;
    // (params32 / params64 / mean32: allocated when first derived, model_derive.hip)
    TRY(ctx->mean64.alloc(ctx, nm));
    TRY(ctx->var64.alloc(ctx, nm));
    TRY(ctx->w64.alloc(ctx, nw));
    TRY(ctx->pm32.alloc(ctx, npm));
    TRY(ctx->pm16f.alloc(ctx, (size_t)J * (Mp32 / 32) * 2 * ((Dd + 7) / 8) * 64 * 8));
    TRY(ctx->kzero.alloc(ctx, (size_t)J));
    TRY(ctx->fscale.alloc(ctx, (size_t)J * 2 * ((Dd + 7) / 8) * 8));
    TRY(ctx->centers32.alloc(ctx, (size_t)J * Dd));
    TRY(ctx->d_cond.alloc(ctx, (size_t)J));
    TRY(ctx->d_bad.alloc(ctx, (size_t)J * Mpad));
    TRY(ctx->d_bad_idx.alloc(ctx, (size_t)J * Mpad));
    TRY(ctx->d_nbad.alloc(ctx, (size_t)J));
    TRY(ctx->d_non.alloc(ctx, (size_t)J));
    TRY(ctx->d_good_idx.alloc(ctx, (size_t)J * Mpad));
    TRY(ctx->d_npt.alloc(ctx, (size_t)J));
    // with the coarse pass (gmm_score_coarse.hip) a state's off-pipe mixtures cost the scoring about what they would cost on the pipe, so
    // states stay split for scoring up to coarse_split_frac (0.99) of their mixtures.  Beyond it the route stops paying: tens of pairs per
    // frame and state pass the bound (many of a state's broader mixtures have by then crossed cond_max themselves and sit, off-pipe,
    // within reach of most frames) for a pass that evaluates a pair per lane, and the whole-state direct form with its
    // partial-distance test is the cheaper route.  Config 4's EM iterations 5 / 6 / 7 (98.8 / 99.7 / 99.8 % off-pipe) at
    // the limits 0.95, 0.99, 0.998: 274 / 256 / 275, 206 / 260 / 306 and 160 / 276 / 362 ms (profiles/r06_coarse_rework.txt).  PCL_SPLIT_MAX overrides both limits; the accumulate pass keeps the round 4-5 half
    ctx->acc_split_max = (int)((ctx->split_frac_set ? ctx->split_frac : 0.5f) * (float)M);
    ctx->split_max = (int)(((ctx->split_frac_set || !pcl_coarse_enabled_for(ctx, Dd)) ? ctx->split_frac : ctx->coarse_split_frac) * (float)M);
    ctx->J = J;
    ctx->M = M;
    ctx->Mpad = Mpad;
    ctx->Mpad32 = Mp32;
    ctx->D = Dd;
    ctx->Dhost = D;
    ctx->row = row;
    ctx->model_flags = flags;
    return PCL_OK;
}

// The second half: from the master copy on the device to a model every scoring path can use.
int pcl_model_finish(pcl_ctx *ctx) {
    const int J = ctx->J, Mpad = ctx->Mpad;
    const size_t nm = (size_t)J * Mpad * ctx->D;
    pcl_timer_begin(ctx, "derive");
    const int rc_derive = pcl_launch_derive(ctx);
    pcl_timer_end(ctx, "derive");
    TRY(rc_derive);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // statistics: [acc J*Mpad | alpha J | mean J*Mpad*Dd | cov J*Mpad*Dd]
    ctx->stats_len = (size_t)J * Mpad + J + 2 * nm;
    TRY(ctx->stats.alloc(ctx, ctx->stats_len));
    ctx->st_acc = ctx->stats;
    ctx->st_alpha = ctx->st_acc + (size_t)J * Mpad;
    ctx->st_mean = ctx->st_alpha + J;
    ctx->st_cov = ctx->st_mean + nm;
    HIPCHK(ctx, hipMemset(ctx->stats, 0, ctx->stats_len * sizeof(double)));
    return PCL_OK;
}

int pcl_model_upload(pcl_ctx *ctx, int J, int M, int D, const double *mean, const double *var, const double *weight,
                     int flags) {
    if (!ctx) return PCL_ERR_INVALID;
    if (J <= 0 || M <= 0 || D <= 0 || !mean || !var || !weight) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_model_upload: bad shape J=%d M=%d D=%d", J, M, D);
    const int Dd = device_dim(D);
    if (Dd < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_model_upload: feature dimension %d > 64 is not supported", D);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    free_model(ctx);                                              // (as always: a rejected variance below leaves the context without a model)
    const int Mpad = (M + 3) / 4 * 4;
    const size_t nm = (size_t)J * Mpad * Dd, nw = (size_t)J * Mpad;
    // float64 master copy in the padded device layout; every derived layout is built on the device
    std::vector<double> m64(nm, 0.0), v64(nm, 1.0), w64(nw, 0.0);
    for (int j = 0; j < J; ++j)
        for (int m = 0; m < M; ++m) {
            w64[(size_t)j * Mpad + m] = weight[(size_t)j * M + m];
            for (int d = 0; d < D; ++d) {
                const double vr = var[((size_t)j * M + m) * D + d];
                if (!(vr > 0.0)) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_model_upload: variance[%d,%d,%d] = %g is not positive", j, m, d, vr);
                m64[((size_t)j * Mpad + m) * Dd + d] = mean[((size_t)j * M + m) * D + d];
                v64[((size_t)j * Mpad + m) * Dd + d] = vr;
            }
        }
    TRY(pcl_model_alloc(ctx, J, M, D, flags, "pcl_model_upload"));
    HIPCHK(ctx, hipMemcpy(ctx->mean64, m64.data(), nm * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->var64, v64.data(), nm * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->w64, w64.data(), nw * sizeof(double), hipMemcpyHostToDevice));
    return pcl_model_finish(ctx);
}

// ================================================================ frames
int pcl_frames_upload(pcl_ctx *ctx, int64_t F, int D, const void *frames, int dtype) {
    if (!ctx) return PCL_ERR_INVALID;
    if (F <= 0 || D <= 0 || !frames) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_frames_upload: bad shape F=%lld D=%d", (long long)F, D);
    const int Dd = device_dim(D);
    if (Dd < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_frames_upload: feature dimension %d > 64 is not supported", D);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    release_frames32(ctx);
    ctx->frames64.release();
    const size_t n = (size_t)F * Dd;
    // Direct PCIe copy in the host element type (padded on the host only when D has no exact kernel);
    // the other precision is derived on the device: f32 now (every mode reads it), f64 lazily (parity mode).
    const size_t esz = (dtype == PCL_F64) ? sizeof(double) : sizeof(float);
    const void *src = frames;
    std::vector<char> padded;
    if (Dd != D) {
        padded.assign(n * esz, 0);
        for (int64_t f = 0; f < F; ++f) memcpy(&padded[(size_t)f * Dd * esz], (const char *)frames + (size_t)f * D * esz, (size_t)D * esz);
        src = padded.data();
    }
    TRY(ctx->frames_up.alloc(ctx, n));
    ctx->frames32 = ctx->frames_up;
    if (dtype == PCL_F64) {
        TRY(ctx->frames64.alloc(ctx, n));
        HIPCHK(ctx, hipMemcpy(ctx->frames64, src, n * esz, hipMemcpyHostToDevice));
        TRY(pcl_launch_cast(ctx, ctx->frames64, ctx->frames32, nullptr, n));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        HIPCHK(ctx, hipMemcpy(ctx->frames32, src, n * esz, hipMemcpyHostToDevice));
    }
    ctx->F = F;
    ctx->FD = Dd;
    ctx->FDhost = D;
    if (ctx->fmllr_Gk && D != ctx->Dhost) pcl_fmllr_release(ctx);   // fMLLR statistics describe frames of the model's dimension
    if (ctx->mllt_F && D != ctx->Dhost) pcl_mllt_release(ctx);      // ... and so do MLLT's
    return PCL_OK;
}

// Streaming (BASELINE config 5: the corpus does not fit a batch): the next chunk's frames travel on the copy stream
// into the slot that is not being scored, so the H2D leg runs beside the scoring / decoding of the current chunk.
int pcl_frames_stage(pcl_ctx *ctx, int64_t F, int D, const float *frames) {
    if (!ctx) return PCL_ERR_INVALID;
    if (F <= 0 || D <= 0 || !frames) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_frames_stage: bad shape F=%lld D=%d", (long long)F, D);
    const int Dd = device_dim(D);
    if (Dd < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_frames_stage: feature dimension %d > 64 is not supported", D);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int back = ctx->frames_front == 0 ? 1 : 0;
    const size_t n = (size_t)F * Dd;
    TRY(ctx->frames_slot[back].reserve(ctx, n));                   // (grows only: a steady stream of equal chunks allocates twice)
    HIPCHK(ctx, ctx->ev_stage.make());
    if (ctx->have_slot_free) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream_aux, ctx->ev_slot_free, 0));   // its last readers
    if (Dd == D) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->frames_slot[back], frames, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream_aux));
    } else {
        // a dimension without a kernel instance of its own (D = 8, 20, 40, ...): rows are padded to the device dimension on the way
        // in -- the pad columns zeroed, the rows copied with a pitch -- as pcl_frames_upload pads on the host
        HIPCHK(ctx, hipMemsetAsync(ctx->frames_slot[back], 0, n * sizeof(float), ctx->stream_aux));
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->frames_slot[back], (size_t)Dd * sizeof(float), frames, (size_t)D * sizeof(float), (size_t)D * sizeof(float),
                                     (size_t)F, hipMemcpyHostToDevice, ctx->stream_aux));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev_stage, ctx->stream_aux));
    ctx->staged_slot = back;
    ctx->staged_F = F;
    ctx->staged_D = D;
    return PCL_OK;
}

int pcl_frames_swap(pcl_ctx *ctx) {
    if (!ctx) return PCL_ERR_INVALID;
    if (ctx->staged_slot < 0) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_frames_swap: nothing staged (pcl_frames_stage first)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize(ctx->ev_stage));               // the copy is done: the caller's buffer is free again
    release_frames32(ctx);
    ctx->frames64.release();
    HIPCHK(ctx, ctx->ev_slot_free.make());
    HIPCHK(ctx, hipEventRecord(ctx->ev_slot_free, ctx->stream));   // everything queued so far read the old slot
    ctx->have_slot_free = true;
    ctx->frames_front = ctx->staged_slot;
    ctx->frames32 = ctx->frames_slot[ctx->frames_front];
    ctx->F = ctx->staged_F;
    ctx->FDhost = ctx->staged_D;
    if (ctx->fmllr_Gk && ctx->FDhost != ctx->Dhost) pcl_fmllr_release(ctx);
    if (ctx->mllt_F && ctx->FDhost != ctx->Dhost) pcl_mllt_release(ctx);
    ctx->FD = device_dim(ctx->staged_D);
    ctx->staged_slot = -1;
    return PCL_OK;
}

int pcl_host_alloc(pcl_ctx *ctx, size_t bytes, void **out) {
    if (!ctx || !out || !bytes) return PCL_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostMalloc(out, bytes, hipHostMallocDefault));
    return PCL_OK;
}

// hipHostFree does not wait for copies that still read or write the block: a result set queued by pcl_batch_fetch_async on stream_d2h
// (or a chunk staged by pcl_frames_stage) and never waited for would be DMA into unmapped host memory -- a GPU-side fault at the next
// teardown (round 5 saw one at a fixture's engine.close(), which freed its page-locked result buffers before pcl_destroy drained the
// streams).  Freeing page-locked memory is rare (engine close, a staging buffer outgrown): drain every stream of the context first.
int pcl_host_free(pcl_ctx *ctx, void *ptr) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ptr) return PCL_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t all[] = {ctx->stream_d2h, ctx->stream_aux, ctx->stream_dp, ctx->stream, ctx->stream_desc, ctx->stream_comm};
    for (hipStream_t s : all)
        if (s) HIPCHK(ctx, hipStreamSynchronize(s));
    HIPCHK(ctx, hipHostFree(ptr));
    return PCL_OK;
}

// ================================================================ batch
int pcl_batch_create(pcl_ctx *ctx, int U, const int32_t *N, const int32_t *T, const int64_t *frame_begin, pcl_batch **out) {
    if (!ctx || !out) return PCL_ERR_INVALID;
    *out = nullptr;
    BatchShape shape;
    TRY(plan_batch_shape(ctx, U, N, T, frame_begin, ctx->F, &shape));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pcl_batch_reap(ctx, false);                              // destroyed batches the GPU has finished with: their blocks first
    std::unique_ptr<pcl_batch> b(new pcl_batch());           // (a failed allocation below gives back what the batch holds by then: nothing was launched on it)
    b->ctx = ctx;
    b->U = U;
    b->shape = std::move(shape);
    TRY(b->d_utt.alloc(ctx, (size_t)U));
    TRY(b->Bt.alloc(ctx, (size_t)b->shape.sumNT));
    TRY(b->logpi.alloc(ctx, (size_t)b->shape.sumN));
    TRY(b->d_row_state.alloc(ctx, (size_t)b->shape.sumN));
    b->counted = true;
    ++ctx->live_batches;
    *out = b.release();
    return PCL_OK;
}

// Everything a batch owns goes back to the pool.  The caller has made sure the GPU is done with the batch.
static void batch_free_now(pcl_batch *b) {
    pcl_free_synced_scope done;                              // the members' frees skip their device-wide wait
    delete b;
}

// has the GPU finished the batch's own work on every stream it used?  (wait: block until it has)
static bool batch_work_done(pcl_batch *b, bool wait) {
    hipEvent_t evs[3] = {b->ev_mark, b->ev_dp, b->ev_fetch};
    bool done = true;
    for (hipEvent_t ev : evs) {
        if (!ev) continue;
        const hipError_t e = wait ? hipEventSynchronize(ev) : hipEventQuery(ev);      // (an event never recorded reads as complete)
        if (e != hipSuccess) done = false;
        if (!done && !wait) break;
    }
    (void)hipGetLastError();                                 // (hipErrorNotReady is not an error)
    return done;
}

static int pcl_batch_reap(pcl_ctx *ctx, bool wait) {
    size_t keep = 0;
    for (size_t g = 0; g < ctx->graves.size(); ++g) {
        pcl_batch *b = ctx->graves[g];
        if (batch_work_done(b, wait)) batch_free_now(b);
        else ctx->graves[keep++] = b;
    }
    ctx->graves.resize(keep);
    return (int)keep;
}

// The reference drops an utterance's objects when its worker returns (AcousticModel.py:884-916); a corpus sweep here drops the batch
// of step k - 3 while the GPU works on step k.  Waiting for the streams at that point (what this function did through round 4:
// 38 ms per call inside a sweep, tools/fresh_batch_probe.py) stalls the host that should be queueing step k + 1.  So the batch
// is freed at once when ITS OWN last work has completed -- the events it left behind its main-stream work (pcl_batch_mark), its
// recursion on the second stream and its result copies, not what later batches queued behind them -- and otherwise waits in the
// context's list until it has (pcl_batch_reap).  The handle is dead for the caller either way.
int pcl_batch_destroy(pcl_batch *b) {
    if (!b) return PCL_OK;
    pcl_ctx *ctx = b->ctx;
    hipSetDevice(ctx->device);
    if (b->counted) --ctx->live_batches;
    b->counted = false;
    pcl_batch_reap(ctx, false);
    static const bool sync_destroy = getenv("PCL_DESTROY_SYNC") && atoi(getenv("PCL_DESTROY_SYNC")) != 0;   // A/B: rounds 1-4 (wait here)
    if (batch_work_done(b, sync_destroy)) batch_free_now(b);
    else ctx->graves.push_back(b);
    return PCL_OK;
}

// Upload the sparse transition structure of every utterance (SparseTrans, batch_plan.h; the UttDesc nnz_off fields are set) and ln pi.
int pcl_batch_upload_sparse(pcl_batch *b, const SparseTrans &t, const double *logpi) {
    pcl_ctx *ctx = b->ctx;
    b->trans = t.shape;
    b->row_ptr.release(); b->col_idx.release(); b->csr_val.release();
    b->col_ptr.release(); b->row_idx.release(); b->csc_val.release();
    b->xi_m.release(); b->xi_s.release(); b->nz_tmp.release();
    const size_t nz = (size_t)t.shape.nnz, np = t.row_ptr.size();
    TRY(b->row_ptr.alloc(ctx, np));
    TRY(b->col_ptr.alloc(ctx, np));
    TRY(b->col_idx.alloc(ctx, nz));
    TRY(b->row_idx.alloc(ctx, nz));
    TRY(b->csr_val.alloc(ctx, nz));
    TRY(b->csc_val.alloc(ctx, nz));
    TRY(b->xi_m.alloc(ctx, nz));
    TRY(b->xi_s.alloc(ctx, nz));
    // (a batch that has launched nothing: its buffers are fresh, the copies need not queue behind the main stream's kernels)
    auto up = b->launched ? pcl_h2d : pcl_h2d_fresh;
    HIPCHK(ctx, up(ctx, b->row_ptr, t.row_ptr.data(), np * sizeof(int)));
    HIPCHK(ctx, up(ctx, b->col_ptr, t.col_ptr.data(), np * sizeof(int)));
    if (nz) {
        HIPCHK(ctx, up(ctx, b->col_idx, t.col_idx.data(), nz * sizeof(int)));
        HIPCHK(ctx, up(ctx, b->row_idx, t.row_idx.data(), nz * sizeof(int)));
        HIPCHK(ctx, up(ctx, b->csr_val, t.csr_val.data(), nz * sizeof(double)));
        HIPCHK(ctx, up(ctx, b->csc_val, t.csc_val.data(), nz * sizeof(double)));
    }
    HIPCHK(ctx, up(ctx, b->logpi, logpi, (size_t)b->shape.sumN * sizeof(double)));
    HIPCHK(ctx, up(ctx, b->d_utt, b->shape.utt.data(), (size_t)b->U * sizeof(UttDesc)));
    b->have_trans = true;
    b->have_fb = b->have_vit = b->have_mbr = false;
    return PCL_OK;
}

int pcl_batch_set_transitions(pcl_batch *b, const double *logA, const double *logpi) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    TRY(batch_join(b));
    if (!logA || !logpi) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_set_transitions: NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SparseTrans t;                                                 // an entry is stored unless ln A == -inf
    TRY(plan_sparse_trans(ctx, "pcl_batch_set_transitions", b->shape.utt, dense_trans_rows(b->shape.utt, logA), &t));
    return pcl_batch_upload_sparse(b, t, logpi);
}

int pcl_batch_set_states(pcl_batch *b, const int32_t *row_state) {
    if (!b) return PCL_ERR_INVALID;
    TRY(batch_join(b));
    if (!row_state) PCL_FAIL(b->ctx, PCL_ERR_INVALID, "pcl_batch_set_states: NULL argument");
    return pcl_batch_set_states_impl(b, row_state);
}

int pcl_batch_set_states_impl(pcl_batch *b, const int32_t *row_state) {
    pcl_ctx *ctx = b->ctx;
    if (ctx->J == 0) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_set_states: upload a model first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ScorePlan plan;
    TRY(plan_score(ctx, b->shape.utt, row_state, ctx->J, &plan));   // (refused: the batch keeps the lists it had, on the host as on the device)
    b->plan = std::move(plan);
    b->d_dups.release();
    if (!b->plan.dups.empty()) {
        TRY(b->d_dups.alloc(ctx, b->plan.dups.size()));
        HIPCHK(ctx, pcl_h2d_fresh(ctx, b->d_dups, b->plan.dups.data(), b->plan.dups.size() * sizeof(DupRow)));
    }
    b->d_segs.release();
    b->d_tiles.release();
    b->d_tiles_v.release();
    b->d_tiles_s.release();
    b->d_tiles_c.release();
    b->d_tile_flags_c.release();
    b->n_tiles_s = b->n_tiles_c = 0;
    b->tile_frames = 0;
    TRY(b->d_segs.alloc(ctx, (size_t)b->plan.n_segs));
    if (b->plan.n_segs) HIPCHK(ctx, pcl_h2d_fresh(ctx, b->d_segs, b->plan.segs.data(), (size_t)b->plan.n_segs * sizeof(ScoreSeg)));
    b->d_seg_of_row.release();
    TRY(b->d_seg_of_row.alloc(ctx, (size_t)b->shape.sumN));
    if (b->shape.sumN) HIPCHK(ctx, pcl_h2d_fresh(ctx, b->d_seg_of_row, b->plan.seg_of_row.data(), (size_t)b->shape.sumN * sizeof(int)));
    auto up = b->launched ? pcl_h2d : pcl_h2d_fresh;             // (batch-lifetime buffers: fresh only while nothing was launched)
    HIPCHK(ctx, up(ctx, b->d_row_state, row_state, (size_t)b->shape.sumN * sizeof(int32_t)));
    HIPCHK(ctx, up(ctx, b->d_utt, b->shape.utt.data(), (size_t)b->U * sizeof(UttDesc)));
    b->have_states = true;
    b->have_mbr = false;                                           // (pcl_batch_mbr's accuracy was taken against the map that just went)
    b->virt_rows_filled = false;
    b->model_J = ctx->J;
    return PCL_OK;
}

// A batch outlives pcl_frames_upload / pcl_model_upload calls (the drop-in classes re-upload on the shared engine all
// the time): its frame rows and state ids were checked against the buffers of THEN.  Re-check against the buffers of
// NOW before any kernel indexes them.
static int batch_revalidate(pcl_batch *b, const char *who) {
    pcl_ctx *ctx = b->ctx;
    if (b->shape.max_frame_end > ctx->F)
        PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the batch refers to frame rows up to %lld but the frame matrix now has %lld rows (re-uploaded after the batch was created)",
                 who, b->shape.max_frame_end, (long long)ctx->F);
    if (b->have_states && (b->plan.max_state >= ctx->J || b->model_J != ctx->J))
        PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the batch was laid out for a model of %d states (largest id used %d) but the model now has %d (re-uploaded after pcl_batch_set_states)",
                 who, b->model_J, b->plan.max_state, ctx->J);
    return PCL_OK;
}

static int ensure_tmp(pcl_batch *b) {
    if (!b->tmp) TRY(b->tmp.alloc(b->ctx, (size_t)b->shape.sumNT));
    return PCL_OK;
}

int pcl_batch_set_emissions(pcl_batch *b, const double *B) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    TRY(batch_join(b));
    if (!B) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_set_emissions: NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TRY(ensure_tmp(b));
    b->launched = true;
    HIPCHK(ctx, pcl_h2d(ctx, b->d_utt, b->shape.utt.data(), (size_t)b->U * sizeof(UttDesc)));
    HIPCHK(ctx, hipMemcpyAsync(b->tmp, B, (size_t)b->shape.sumNT * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TRY(pcl_launch_transpose(ctx, b, b->tmp, b->Bt, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    b->have_B = true;
    b->virt_rows_filled = false;                                   // (the caller's matrix is in the buffer now)
    b->have_fb = b->have_vit = b->have_mbr = false;
    return PCL_OK;
}

int pcl_batch_set_posteriors(pcl_batch *b, const double *lgamma) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    TRY(batch_join(b));
    if (!lgamma) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_set_posteriors: NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TRY(ensure_tmp(b));
    if (!b->lgam) TRY(b->lgam.alloc(ctx, (size_t)b->shape.sumNT));
    HIPCHK(ctx, pcl_h2d(ctx, b->d_utt, b->shape.utt.data(), (size_t)b->U * sizeof(UttDesc)));
    HIPCHK(ctx, hipMemcpyAsync(b->tmp, lgamma, (size_t)b->shape.sumNT * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TRY(pcl_launch_transpose(ctx, b, b->tmp, b->lgam, 1));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    b->have_post = true;
    return PCL_OK;
}

static int ensure_frames64(pcl_ctx *ctx) {
    if (ctx->frames64 || !ctx->frames32) return PCL_OK;
    const size_t n = (size_t)ctx->F * ctx->FD;
    TRY(ctx->frames64.alloc(ctx, n));
    return pcl_launch_cast(ctx, nullptr, ctx->frames32, ctx->frames64, n);   // float -> double is exact
}

static int build_tiles(pcl_batch *b, int precision) {
    pcl_ctx *ctx = b->ctx;
    const int route = pcl_route(ctx, precision, ctx->D);
    const bool mfma = route != PCL_ROUTE_DIRECT;
    const int tf = route == PCL_ROUTE_SPLIT16 ? pcl_score_split16_tile_frames()
                 : route == PCL_ROUTE_MFMA32 ? pcl_score_mfma_tile_frames() : pcl_score_tile_frames(ctx->D, precision);
    if (b->d_tiles && b->tile_frames == tf && b->tile_gen == ctx->model_gen) return PCL_OK;
    // MFMA mode: states whose centred expansion is ill conditioned go to the direct-form VALU kernel
    std::vector<size_t> good, bad;
    for (size_t k = 0; k < b->plan.work_states.size(); ++k) (mfma && pcl_state_uses_valu(ctx, b->plan.work_states[k]) ? bad : good).push_back(k);
    const std::vector<ScoreTile> tiles = plan_tiles(b->plan, good, tf);
    const std::vector<ScoreTile> tiles_v = bad.empty() ? std::vector<ScoreTile>() : plan_tiles(b->plan, bad, pcl_score_tile_frames(ctx->D, PCL_F32));
    // split states: on the matrix pipe (in `good`) AND, for their off-pipe mixtures, in a list of their own at the direct-form tile size
    std::vector<size_t> split;
    if (mfma)
        for (size_t k : good)
            if (pcl_state_is_split(ctx, b->plan.work_states[k])) split.push_back(k);
    // ... at the direct-form tile size (the subset launch, rounds 4-5) or, with the coarse pass, at the matrix pipe's
    const bool coarse = route == PCL_ROUTE_SPLIT16 && pcl_coarse_enabled(ctx);
    const std::vector<ScoreTile> tiles_s = (split.empty() || coarse) ? std::vector<ScoreTile>() : plan_tiles(b->plan, split, pcl_score_subset_tile_frames(ctx->D));
    const std::vector<ScoreTile> tiles_c = (split.empty() || !coarse) ? std::vector<ScoreTile>() : plan_tiles(b->plan, split, pcl_coarse_tile_frames());
    b->d_tiles.release();
    b->d_tiles_v.release();
    b->d_tiles_s.release();
    b->d_tiles_c.release();
    b->d_tile_flags_c.release();
    pcl_desc_group uploads(ctx);                                   // the tile lists: staged, one wait at the end
    b->n_tiles_s = (int)tiles_s.size();
    if (!tiles_s.empty()) {
        TRY(b->d_tiles_s.alloc(ctx, tiles_s.size()));
        HIPCHK(ctx, pcl_h2d_fresh(ctx, b->d_tiles_s, tiles_s.data(), tiles_s.size() * sizeof(ScoreTile)));
    }
    b->n_tiles_c = (int)tiles_c.size();
    if (!tiles_c.empty()) {
        TRY(b->d_tiles_c.alloc(ctx, tiles_c.size()));
        TRY(b->d_tile_flags_c.alloc(ctx, tiles_c.size()));
        HIPCHK(ctx, pcl_h2d_fresh(ctx, b->d_tiles_c, tiles_c.data(), tiles_c.size() * sizeof(ScoreTile)));
    }
    b->d_tile_flags.release();
    TRY(b->d_tile_flags.alloc(ctx, tiles.size()));
    b->n_tiles = (int)tiles.size();
    b->n_tiles_v = (int)tiles_v.size();
    b->tile_frames = tf;
    b->tile_gen = ctx->model_gen;
    TRY(b->d_tiles.alloc(ctx, tiles.size()));
    if (!tiles.empty()) HIPCHK(ctx, pcl_h2d_fresh(ctx, b->d_tiles, tiles.data(), tiles.size() * sizeof(ScoreTile)));
    if (!tiles_v.empty()) {
        TRY(b->d_tiles_v.alloc(ctx, tiles_v.size()));
        HIPCHK(ctx, pcl_h2d_fresh(ctx, b->d_tiles_v, tiles_v.data(), tiles_v.size() * sizeof(ScoreTile)));
    }
    HIPCHK(ctx, uploads.finish());
    return PCL_OK;
}

int pcl_batch_score(pcl_batch *b, int precision) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    TRY(batch_join(b));
    if (precision != PCL_F32 && precision != PCL_F64) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_score: precision %d", precision);
    if (ctx->J == 0) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_score: no model uploaded");
    if (ctx->F == 0) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_score: no frames uploaded");
    if (!b->have_states) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_score: pcl_batch_set_states was not called");
    if (ctx->FDhost != ctx->Dhost)  // DataDimensionError, Clustering.py:749-751
        PCL_FAIL(ctx, PCL_ERR_INVALID, "data dimension %d does not match model dimension %d", ctx->FDhost, ctx->Dhost);
    TRY(batch_revalidate(b, "pcl_batch_score"));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (precision == PCL_F64) {
        TRY(ensure_frames64(ctx));
        TRY(pcl_ensure_layouts(ctx, PCL_LAYOUT_P64));
    }
    TRY(build_tiles(b, precision));
    b->launched = true;
    if (!b->virt_rows_filled) {                                    // entry row ln 1, exit row ln 0 (AcousticModel.py:218-219): constants,
        TRY(pcl_launch_fill_virtual_rows(ctx, b));                // written once per row map, not once per scoring pass
        b->virt_rows_filled = true;
    }
    const int route = pcl_route(ctx, precision, ctx->D);
    if (route != PCL_ROUTE_DIRECT) {
        if (route == PCL_ROUTE_SPLIT16) {
            TRY(pcl_launch_score_split16(ctx, b, b->d_tiles, b->n_tiles));
#ifndef PCL_DIAG_NOFIXUP
            TRY(pcl_launch_score_fixup(ctx, b, b->d_tiles, b->n_tiles, b->d_tile_flags));   // tiles with out-of-range features
#endif
        } else TRY(pcl_launch_score_mfma(ctx, b, b->d_tiles, b->n_tiles));
        if (b->n_tiles_c) {                                                       // split states: their off-pipe mixtures, log-added --
            TRY(pcl_launch_score_coarse(ctx, b));                                 // proven negligible by a bound on the matrix pipe, or evaluated exactly
            TRY(pcl_launch_score_subset_flagged(ctx, b, b->d_tiles_c, b->n_tiles_c, b->d_tile_flags_c));   // (tiles with features out of the f16 range)
        }
        TRY(pcl_launch_score_subset(ctx, b, b->d_tiles_s, b->n_tiles_s));         // ... or all of them in direct form (PCL_COARSE=0)
        TRY(pcl_launch_score(ctx, b, PCL_F32, b->d_tiles_v, b->n_tiles_v));      // ill-conditioned states, direct form
    } else {
        TRY(pcl_launch_score(ctx, b, precision, b->d_tiles, b->n_tiles));
    }
    TRY(pcl_launch_dup_rows(ctx, b));                              // rows of a state an utterance's label names again
    HIPCHK(ctx, pcl_batch_mark(b));
    b->mark_is_score = true;
    b->have_B = true;
    b->have_fb = b->have_vit = b->have_mbr = false;
    return PCL_OK;
}

int pcl_batch_forward_backward(pcl_batch *b, int fix_pi, double threshold) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_trans) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_forward_backward: no transitions set");
    if (!b->have_B) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_forward_backward: no emissions (score or set_emissions first)");  // LHMM.py:69
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool after_fetch = b->fetch_pending;
    if (b->fetch_pending) {                                  // the copies of the previous results read lgam / ksai: main stream first (stream_dp waits for them below)
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, b->ev_fetch, 0));
        b->fetch_pending = false;
    }
    if (!b->alpha) {
        TRY(b->alpha.alloc(ctx, (size_t)b->shape.sumNT));
        TRY(b->beta.alloc(ctx, (size_t)b->shape.sumNT));
        if (!b->lgam) TRY(b->lgam.alloc(ctx, (size_t)b->shape.sumNT));
        TRY(b->pi_out.alloc(ctx, (size_t)b->shape.sumN));
        TRY(b->gamma_out.alloc(ctx, (size_t)b->shape.sumN));
        TRY(b->ksai.alloc(ctx, (size_t)b->shape.sumNN));
        TRY(b->logp.alloc(ctx, (size_t)b->U));
        TRY(b->qtrace.alloc(ctx, (size_t)b->U * PCL_MAX_PASS));
        TRY(b->npass.alloc(ctx, (size_t)b->U));
    }
    if (ctx->dp_async) {
        // stream_dp waits for everything queued on the main stream so far (the scoring of this batch), runs the
        // recursion, and leaves an event for whoever touches the batch next
        TRY(pcl_run_on_dp_stream(b, after_fetch, [&] { return pcl_launch_forward_backward(ctx, b, fix_pi ? 1 : 0, threshold); }));
    } else {
        TRY(pcl_launch_forward_backward(ctx, b, fix_pi ? 1 : 0, threshold));
        HIPCHK(ctx, pcl_batch_mark(b));
        b->mark_is_score = false;
    }
    b->have_fb = true;
    b->have_post = true;
    return PCL_OK;
}

int pcl_batch_viterbi(pcl_batch *b, int end_state_back) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_trans) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_viterbi: no transitions set");
    if (!b->have_B) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_viterbi: no emissions (score or set_emissions first)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool after_fetch = b->fetch_pending;
    if (b->fetch_pending) {                                  // result copies still reading this batch's path / point buffers
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, b->ev_fetch, 0));
        b->fetch_pending = false;
    }
    if (!b->bp) {
        TRY(b->bp.alloc(ctx, (size_t)b->shape.sumNT));
        TRY(b->path.alloc(ctx, (size_t)b->shape.sumT));
        TRY(b->point.alloc(ctx, (size_t)b->U));
    }
    if (ctx->dp_async) {
        // like the forward-backward: on the second stream, behind everything the main stream has queued (this batch's scoring), beside
        // the NEXT batch's scoring; in order with a forward-backward of the same batch already queued there (round 4: on the main
        // stream the 0.35 ms recursion sat between two scoring kernels -- config 3's step is score + Viterbi)
        TRY(pcl_run_on_dp_stream(b, after_fetch, [&] { return pcl_launch_viterbi(ctx, b, end_state_back ? 1 : 0); }));
    } else {
        TRY(batch_join(b));
        TRY(pcl_launch_viterbi(ctx, b, end_state_back ? 1 : 0));
        HIPCHK(ctx, pcl_batch_mark(b));
        b->mark_is_score = false;
    }
    b->have_vit = true;
    return PCL_OK;
}

// Minimum Bayes risk: one forward-backward under kappa with the expected accuracy against frame_ref (hmm_mbr.hip; the rule: poccala_hip.h).
// On the main stream, behind whatever the batch has queued on either stream; it reads Bt, the transitions and the row map and writes the
// pass's own buffers only.
int pcl_batch_mbr(pcl_batch *b, const int32_t *frame_ref, double kappa, int group) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    const char *who = "pcl_batch_mbr";
    if (!b->have_trans) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no transitions set", who);
    if (!b->have_states) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: pcl_batch_set_states was not called (the accuracy compares row states)", who);
    if (!b->have_B) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no emissions (score or set_emissions first)", who);
    if (!frame_ref) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: NULL argument", who);
    if (!(kappa > 0.0) || !std::isfinite(kappa)) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: kappa = %g is not a finite number > 0", who, kappa);
    if (group < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: group = %d", who, group);
    if (b->shape.Nmax > pcl_mbr_max_rows()) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: HMM with %d states exceeds the %d-state limit", who, b->shape.Nmax, pcl_mbr_max_rows());
    std::vector<int32_t> ref_group((size_t)b->shape.sumT);
    for (size_t t = 0; t < ref_group.size(); ++t) {
        const int32_t r = frame_ref[t];
        if (r < -1 || r >= b->model_J) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: frame_ref[%zu] = %d is outside [-1, %d)", who, t, (int)r, b->model_J);
        ref_group[t] = r < 0 ? -1 : r / group;
    }
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    b->have_mbr = false;                                           // (from here on the buffers are being rewritten)
    TRY(pcl_mbr_reserve(ctx, b));
    b->launched = true;
    HIPCHK(ctx, pcl_h2d(ctx, b->mbr_ref, ref_group.data(), ref_group.size() * sizeof(int32_t)));
    TRY(pcl_launch_mbr(ctx, b, kappa, group));
    HIPCHK(ctx, pcl_batch_mark(b));                                // (the pass writes nothing a recursion reads: mark_is_score stays)
    b->have_mbr = true;
    return PCL_OK;
}

int pcl_batch_mbr_get(pcl_batch *b, double *logp, double *c_avg, double *lgamma, double *g) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_mbr) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_mbr_get: run pcl_batch_mbr first (new emissions, transitions or states drop its results)");
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (lgamma || g) TRY(ensure_tmp(b));
    const size_t nt = (size_t)b->shape.sumNT * sizeof(double);
    if (logp) HIPCHK(ctx, pcl_d2h_queue(ctx, logp, b->mbr_logp, (size_t)b->U * sizeof(double)));
    if (c_avg) HIPCHK(ctx, pcl_d2h_queue(ctx, c_avg, b->mbr_cavg, (size_t)b->U * sizeof(double)));
    const double *mats[2] = {b->mbr_lgam, b->mbr_g};
    double *hosts[2] = {lgamma, g};
    for (int k = 0; k < 2; ++k) {
        if (!hosts[k]) continue;
        TRY(pcl_launch_transpose(ctx, b, mats[k], b->tmp, 0));     // time-major -> the reference's (N_u, T_u); in stream order with the copy before it
        HIPCHK(ctx, pcl_d2h_queue(ctx, hosts[k], b->tmp, nt));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

int pcl_batch_mbr_posteriors(pcl_batch *b, int which) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_mbr) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_mbr_posteriors: run pcl_batch_mbr first (new emissions, transitions or states drop its results)");
    if (which < -1 || which > 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_mbr_posteriors: which = %d is not -1, 0 or +1", which);
    TRY(batch_join(b));                                            // (a forward-backward queued on the second stream writes lgam too)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!b->lgam) TRY(b->lgam.alloc(ctx, (size_t)b->shape.sumNT));
    TRY(pcl_launch_mbr_posteriors(ctx, b, which));
    HIPCHK(ctx, pcl_batch_mark(b));
    b->mark_is_score = false;                                      // lgam changed behind the scoring: a later recursion waits for a fresh event
    b->have_post = true;
    return PCL_OK;
}

int pcl_batch_regroup(pcl_batch *b, const int32_t *row_unit, int gmm_num, int32_t *frame_unit, int32_t *frame_k) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    TRY(batch_join(b));
    if (!row_unit || !frame_unit || !frame_k || gmm_num < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_regroup: bad arguments");
    if (!b->have_vit) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_regroup: run pcl_batch_viterbi first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf<int32_t> d_ru, d_fu, d_fk;                       // (released with the device-wide wait, as ever, on every path)
    TRY(d_ru.alloc(ctx, (size_t)b->shape.sumN));
    TRY(d_fu.alloc(ctx, (size_t)b->shape.sumT));
    TRY(d_fk.alloc(ctx, (size_t)b->shape.sumT));
    HIPCHK(ctx, hipMemcpyAsync(d_ru, row_unit, (size_t)b->shape.sumN * 4, hipMemcpyHostToDevice, ctx->stream));
    TRY(pcl_launch_regroup(ctx, b, d_ru, gmm_num, d_fu, d_fk));
    HIPCHK(ctx, hipMemcpyAsync(frame_unit, d_fu, (size_t)b->shape.sumT * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(frame_k, d_fk, (size_t)b->shape.sumT * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

// What the owner map of a batch's Viterbi paths needs (pcl_batch_align_segments, pcl_batch_accumulate_lda), checked before anything is queued
static int align_precheck(pcl_batch *b, const char *who) {
    pcl_ctx *ctx = b->ctx;
    if (!b->from_labels) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the batch was not created from labels (pcl_batch_create_labels)", who);
    if (!b->have_vit) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: run pcl_batch_viterbi first", who);
    const int e = ctx->S - 2;
    if (b->tied) {                                    // owners are the tied states the batch was made with (pcl_batch_create_labels_tied)
        if (ctx->n_units < 1 || e < 1 || ctx->J != b->tied_J)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the model has %d GMM states, the batch was made over %d tied states", who, ctx->J, b->tied_J);
    } else if (ctx->n_units < 1 || e < 1 || ctx->J != ctx->n_units * e)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the model has %d GMM states, %d units x %d emitting states need %d", who, ctx->J, ctx->n_units, e, ctx->n_units * e);
    if (b->lab.label_max >= ctx->n_units) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the batch names unit %d, the inventory now has %d units", who, b->lab.label_max, ctx->n_units);
    for (int u = 0; u < b->U; ++u)
        if (b->shape.utt[u].N != e * b->lab.label_len[u] + 2)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d has %d rows for %d label units, the inventory now has %d emitting states per unit", who, u,
                     b->shape.utt[u].N, b->lab.label_len[u], e);
    if (!ctx->frames32 || ctx->F == 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: no frames uploaded", who);
    if (b->shape.max_frame_end > ctx->F)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the batch refers to frame rows up to %lld but the frame matrix now has %lld rows (re-uploaded after the batch was created)",
                 who, b->shape.max_frame_end, (long long)ctx->F);
    if (ctx->F > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: frame matrix of %lld rows", who, (long long)ctx->F);
    {   // a frame has one owner: the utterances' row ranges are disjoint
        std::vector<int> by(b->U);
        for (int u = 0; u < b->U; ++u) by[u] = u;
        std::sort(by.begin(), by.end(), [&](int x, int y) { return b->shape.utt[x].frame0 != b->shape.utt[y].frame0 ? b->shape.utt[x].frame0 < b->shape.utt[y].frame0 : x < y; });
        long long end = 0;
        int prev = -1;
        for (int u : by) {
            if (b->shape.utt[u].frame0 < end) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterances %d and %d overlap in the frame matrix", who, prev, u);
            end = b->shape.utt[u].frame0 + b->shape.utt[u].T;
            prev = u;
        }
    }
    return PCL_OK;
}

// the batch's labels and the U + 1 offsets into them on the device: once per batch
static int align_labels_up(pcl_batch *b) {
    pcl_ctx *ctx = b->ctx;
    if (!b->d_labels) {
        const std::vector<int> &loff = b->lab.label_off;
        b->d_label_off.release();                                   // (left by a call whose second allocation failed)
        TRY(b->d_label_off.alloc(ctx, loff.size()));
        TRY(b->d_labels.alloc(ctx, b->lab.labels.size()));
        HIPCHK(ctx, pcl_h2d(ctx, b->d_label_off, loff.data(), loff.size() * sizeof(int)));
        HIPCHK(ctx, pcl_h2d(ctx, b->d_labels, b->lab.labels.data(), b->lab.labels.size() * sizeof(int32_t)));
    }
    return PCL_OK;
}

int pcl_batch_align_segments(pcl_batch *b, int32_t *frame_state_out, int32_t *dropped_out, pcl_seg **out) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    const char *who = "pcl_batch_align_segments";
    if (out) *out = nullptr;
    if (!frame_state_out && !out) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: neither frame_state_out nor out is given", who);
    TRY(align_precheck(b, who));
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long F = ctx->F;
    const int e = ctx->S - 2;
    TRY(align_labels_up(b));
    DevBuf<int32_t> d_state, d_drop;
    auto align = [&]() -> int {
        TRY(d_state.alloc(ctx, (size_t)F));
        TRY(d_drop.alloc(ctx, (size_t)b->U));
        HIPCHK(ctx, hipMemsetAsync(d_state, 0xff, (size_t)F * sizeof(int32_t), ctx->stream));
        TRY(pcl_launch_align_segments(ctx, b, b->lab.label_len_max, e, d_state, d_drop));
        if (b->tied) TRY(pcl_launch_tied_owner(ctx, b, e, d_state));            // unit * P + slice -> the position's tied state of that slice
        if (frame_state_out) HIPCHK(ctx, hipMemcpyAsync(frame_state_out, d_state, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (dropped_out) HIPCHK(ctx, hipMemcpyAsync(dropped_out, d_drop, (size_t)b->U * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, pcl_batch_mark(b));
        return PCL_OK;
    };
    int rc = align();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PCL_OK) {      // (on every path: the frees below rely on it)
        pcl_set_error(ctx, "pcl_batch_align_segments: HIP error");
        rc = PCL_ERR_HIP;
    }
    if (rc == PCL_OK && out) rc = pcl_seg_create_device(ctx, F, ctx->J, d_state, out);
    pcl_free_synced_scope done;                                     // the stream these two were used on has been waited for
    d_state.release();
    d_drop.release();
    return rc;
}

// LDA class statistics from the batch's Viterbi paths (frame_lda.hip): the owner map pcl_batch_align_segments makes stays on the device
int pcl_batch_accumulate_lda(pcl_batch *b, const int32_t *state_class) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    const char *who = "pcl_batch_accumulate_lda";
    if (!ctx->lda_stats || ctx->lda_R <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no statistics: pcl_lda_zero first", who);
    TRY(align_precheck(b, who));
    if (!state_class && ctx->J > ctx->lda_R)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: state_class is NULL (every state its own class) but the model has %d states and the statistics %d classes", who, ctx->J, ctx->lda_R);
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long F = ctx->F;
    TRY(align_labels_up(b));
    DevBuf<int32_t> d_state, d_drop;
    auto align = [&]() -> int {
        TRY(d_state.alloc(ctx, (size_t)F));
        TRY(d_drop.alloc(ctx, (size_t)b->U));
        HIPCHK(ctx, hipMemsetAsync(d_state, 0xff, (size_t)F * sizeof(int32_t), ctx->stream));
        TRY(pcl_launch_align_segments(ctx, b, b->lab.label_len_max, ctx->S - 2, d_state, d_drop));
        if (b->tied) TRY(pcl_launch_tied_owner(ctx, b, ctx->S - 2, d_state));
        HIPCHK(ctx, pcl_batch_mark(b));
        return PCL_OK;
    };
    int rc = align();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PCL_OK) {      // (on every path: the frees below rely on it)
        pcl_set_error(ctx, "pcl_batch_accumulate_lda: HIP error");
        rc = PCL_ERR_HIP;
    }
    if (rc == PCL_OK) {
        std::vector<int32_t> T(b->U);
        std::vector<int64_t> begin(b->U);
        for (int u = 0; u < b->U; ++u) {
            T[u] = b->shape.utt[u].T;
            begin[u] = b->shape.utt[u].frame0;
        }
        rc = pcl_launch_lda_accumulate(ctx, who, b->U, T.data(), begin.data(), d_state, state_class, ctx->J);   // (waits for its kernels)
        if (rc != PCL_OK) (void)hipStreamSynchronize(ctx->stream);  // ... unless it gave up half-way
    }
    pcl_free_synced_scope done;
    d_state.release();
    d_drop.release();
    return rc;
}

// Decision-tree context statistics from the batch's Viterbi paths (tree_cluster.hip): the owner map pcl_batch_align_segments makes and the
// statistics row of every frame stay on the device
int pcl_batch_accumulate_tree(pcl_batch *b, const int32_t *label_event) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    const char *who = "pcl_batch_accumulate_tree";
    TRY(pcl_tree_accumulate_ready(ctx, who));
    TRY(align_precheck(b, who));
    const int P = ctx->S - 2;
    if (ctx->tree_R % P != 0)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the statistics hold %d rows, no multiple of the inventory's %d emitting states per unit", who, ctx->tree_R, P);
    const int E = ctx->tree_R / P;
    if (!label_event) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: label_event is NULL", who);
    for (size_t i = 0; i < b->lab.labels.size(); ++i)
        if (label_event[i] < -1 || label_event[i] >= E)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: label_event[%zu] = %d is neither -1 nor an event in [0, %d)", who, i, (int)label_event[i], E);
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long F = ctx->F;
    TRY(align_labels_up(b));
    DevBuf<int32_t> d_state, d_drop, d_row, d_event;
    auto align = [&]() -> int {
        TRY(d_state.alloc(ctx, (size_t)F));
        TRY(d_row.alloc(ctx, (size_t)F));
        TRY(d_drop.alloc(ctx, (size_t)b->U));
        TRY(d_event.alloc(ctx, b->lab.labels.size()));
        HIPCHK(ctx, pcl_h2d(ctx, d_event, label_event, b->lab.labels.size() * sizeof(int32_t)));
        HIPCHK(ctx, hipMemsetAsync(d_state, 0xff, (size_t)F * sizeof(int32_t), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_row, 0xff, (size_t)F * sizeof(int32_t), ctx->stream));
        TRY(pcl_launch_align_segments(ctx, b, b->lab.label_len_max, P, d_state, d_drop));
        TRY(pcl_launch_tree_label_rows(ctx, b, d_event, P, d_state, d_row));
        HIPCHK(ctx, pcl_batch_mark(b));
        return PCL_OK;
    };
    int rc = align();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PCL_OK) {      // (on every path: the frees below rely on it)
        pcl_set_error(ctx, "pcl_batch_accumulate_tree: HIP error");
        rc = PCL_ERR_HIP;
    }
    if (rc == PCL_OK) {
        std::vector<int32_t> T(b->U);
        std::vector<int64_t> begin(b->U);
        for (int u = 0; u < b->U; ++u) {
            T[u] = b->shape.utt[u].T;
            begin[u] = b->shape.utt[u].frame0;
        }
        rc = pcl_launch_tree_accumulate(ctx, who, b->U, T.data(), begin.data(), d_row);   // (waits for its kernels)
        if (rc != PCL_OK) (void)hipStreamSynchronize(ctx->stream);  // ... unless it gave up half-way
    }
    pcl_free_synced_scope done;
    d_state.release();
    d_drop.release();
    d_row.release();
    d_event.release();
    return rc;
}

int pcl_batch_get(pcl_batch *b, int what, void *host) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    TRY(batch_join(b));
    if (!host) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_get: NULL host buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double *mat = nullptr;
    switch (what) {
        case PCL_GET_B:
            if (!b->have_B) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_get: no emissions yet");
            mat = b->Bt;
            break;
        case PCL_GET_ALPHA: mat = b->alpha; break;
        case PCL_GET_BETA: mat = b->beta; break;
        case PCL_GET_LGAMMA: mat = b->lgam; break;
        default: break;
    }
    if (((what >= PCL_GET_ALPHA && what <= PCL_GET_QTRACE) || what == PCL_GET_KSAI_NZ) && !b->have_fb) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_get: run pcl_batch_forward_backward first");
    if ((what == PCL_GET_PATH || what == PCL_GET_POINT) && !b->have_vit) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_get: run pcl_batch_viterbi first");
    if (mat) {
        TRY(ensure_tmp(b));
        DevBuf<double> logs;
        if ((what == PCL_GET_ALPHA || what == PCL_GET_BETA) && b->fb_linear) {
            // the scaled forward-backward keeps (mantissa, exponent) pairs; the logarithms the reference holds are made here, on demand
            TRY(logs.alloc(ctx, (size_t)b->shape.sumNT));
            TRY(pcl_launch_fb_to_log(ctx, b, mat, what == PCL_GET_ALPHA ? b->alpha_e : b->beta_e, logs));
            mat = logs;
        }
        const int rt = pcl_launch_transpose(ctx, b, mat, b->tmp, 0);
        if (logs) {
            hipStreamSynchronize(ctx->stream);
            pcl_free_synced_scope done;
            logs.release();
        }
        TRY(rt);
        HIPCHK(ctx, hipMemcpyAsync(host, b->tmp, (size_t)b->shape.sumNT * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return PCL_OK;
    }
    const void *src = nullptr;
    size_t bytes = 0;
    switch (what) {
        case PCL_GET_KSAI: src = b->ksai; bytes = (size_t)b->shape.sumNN * 8; break;
        case PCL_GET_KSAI_NZ:
            if (!b->nz_tmp) TRY(b->nz_tmp.alloc(ctx, (size_t)b->trans.nnz));
            TRY(pcl_launch_ksai_gather(ctx, b, b->nz_tmp));
            src = b->nz_tmp; bytes = (size_t)b->trans.nnz * 8;
            break;
        case PCL_GET_GAMMA: src = b->gamma_out; bytes = (size_t)b->shape.sumN * 8; break;
        case PCL_GET_PI: src = b->pi_out; bytes = (size_t)b->shape.sumN * 8; break;
        case PCL_GET_LOGP: src = b->logp; bytes = (size_t)b->U * 8; break;
        case PCL_GET_NPASS: src = b->npass; bytes = (size_t)b->U * 4; break;
        case PCL_GET_QTRACE: src = b->qtrace; bytes = (size_t)b->U * PCL_MAX_PASS * 8; break;
        case PCL_GET_PATH: src = b->path; bytes = (size_t)b->shape.sumT * 4; break;
        case PCL_GET_POINT: src = b->point; bytes = (size_t)b->U * 8; break;
        default: PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_get: unknown selector %d", what);
    }
    HIPCHK(ctx, hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

int pcl_batch_sizes(pcl_batch *b, int64_t *sum_nt, int64_t *sum_n, int64_t *sum_t, int64_t *nnz) {
    if (!b) return PCL_ERR_INVALID;
    if (sum_nt) *sum_nt = b->shape.sumNT;
    if (sum_n) *sum_n = b->shape.sumN;
    if (sum_t) *sum_t = b->shape.sumT;
    if (nnz) *nnz = b->trans.nnz;
    return PCL_OK;
}

int pcl_batch_fetch_async(pcl_batch *b, double *logp, double *lgamma_tm, double *ksai_nz, int32_t *path, double *point) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if ((logp || lgamma_tm || ksai_nz) && !b->have_fb) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_fetch_async: run pcl_batch_forward_backward first");
    if ((path || point) && !b->have_vit) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_fetch_async: run pcl_batch_viterbi first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, b->ev_fetch.make());
    HIPCHK(ctx, b->ev_fetch_src.make());
    hipStream_t ds = ctx->stream_d2h;
    // behind what the batch has queued: the second stream's recursion (which itself waited for the batch's scoring) when one is
    // pending -- no packet on the main stream then --, else the main stream as of now
    if (b->dp_pending && pcl_fewer_markers()) {
        HIPCHK(ctx, hipStreamWaitEvent(ds, b->ev_dp, 0));
    } else {
        HIPCHK(ctx, hipEventRecord(b->ev_fetch_src, ctx->stream));
        HIPCHK(ctx, hipStreamWaitEvent(ds, b->ev_fetch_src, 0));
        if (b->dp_pending) HIPCHK(ctx, hipStreamWaitEvent(ds, b->ev_dp, 0));
    }
    if (ksai_nz) {
        if (!b->nz_tmp) TRY(b->nz_tmp.alloc(ctx, (size_t)b->trans.nnz));
        {
            pcl_stream_scope on_d2h(ctx, ds);
            TRY(pcl_launch_ksai_gather(ctx, b, b->nz_tmp));
        }
        HIPCHK(ctx, hipMemcpyAsync(ksai_nz, b->nz_tmp, (size_t)b->trans.nnz * 8, hipMemcpyDeviceToHost, ds));
    }
    if (logp) HIPCHK(ctx, hipMemcpyAsync(logp, b->logp, (size_t)b->U * 8, hipMemcpyDeviceToHost, ds));
    if (lgamma_tm) HIPCHK(ctx, hipMemcpyAsync(lgamma_tm, b->lgam, (size_t)b->shape.sumNT * 8, hipMemcpyDeviceToHost, ds));
    if (path) HIPCHK(ctx, hipMemcpyAsync(path, b->path, (size_t)b->shape.sumT * 4, hipMemcpyDeviceToHost, ds));
    if (point) HIPCHK(ctx, hipMemcpyAsync(point, b->point, (size_t)b->U * 8, hipMemcpyDeviceToHost, ds));
    HIPCHK(ctx, hipEventRecord(b->ev_fetch, ds));
    b->fetch_pending = true;
    return PCL_OK;
}

int pcl_batch_fetch_wait(pcl_batch *b) {
    if (!b) return PCL_ERR_INVALID;
    if (!b->ev_fetch) PCL_FAIL(b->ctx, PCL_ERR_STATE, "pcl_batch_fetch_wait: nothing was fetched");
    HIPCHK(b->ctx, hipEventSynchronize(b->ev_fetch));
    b->fetch_pending = false;
    return PCL_OK;
}

int pcl_clock_probe(pcl_ctx *ctx, int spin_us, double *shader_mhz) {
    if (!ctx || !shader_mhz || spin_us < 1 || spin_us > 1000000) return PCL_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long h[4] = {0, 0, 0, 0};
    DevBuf<unsigned long long> d;
    TRY(d.alloc(ctx, (size_t)4));
    int rc = pcl_launch_clock_probe(ctx, spin_us, d);
    if (rc == PCL_OK && hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream_aux) != hipSuccess) rc = PCL_ERR_HIP;
    if (rc == PCL_OK && hipStreamSynchronize(ctx->stream_aux) != hipSuccess) rc = PCL_ERR_HIP;
    {
        pcl_free_synced_scope done;                           // (the probe is the only user of d and it has finished)
        d.release();
    }
    if (rc != PCL_OK) PCL_FAIL(ctx, rc, "pcl_clock_probe: HIP error");
    const double cyc = (double)(h[1] - h[0]), ref = (double)(h[3] - h[2]);
    *shader_mhz = ref > 0 ? cyc / ref * 100.0 : 0.0;          // s_memrealtime counts at 100 MHz
    return PCL_OK;
}

// ================================================================ E-step statistics
int pcl_stats_zero(pcl_ctx *ctx) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ctx->stats) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_stats_zero: no model uploaded");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    static const bool zero_async = !(getenv("PCL_ZERO_ASYNC") && atoi(getenv("PCL_ZERO_ASYNC")) == 0);      // 0: on the main stream (rounds 1-4; A/B)
    // (a small block -- the one-unit models of the per-object drop-in route -- is cleared in microseconds where it is: the hop to another
    //  queue and back costs more than that)
    if (zero_async && ctx->stream_aux && ctx->stats_len * sizeof(double) >= ((size_t)64 << 20)) {
        // beside whatever the main stream does next (an E-step starts with the scoring of its first batch, which does not touch the block):
        // behind everything queued so far (the block's last readers), on the auxiliary stream
        HIPCHK(ctx, ctx->ev_zero.make());
        HIPCHK(ctx, ctx->ev_zero_src.make());
        HIPCHK(ctx, hipEventRecord(ctx->ev_zero_src, ctx->stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream_aux, ctx->ev_zero_src, 0));
        HIPCHK(ctx, hipMemsetAsync(ctx->stats, 0, ctx->stats_len * sizeof(double), ctx->stream_aux));
        HIPCHK(ctx, hipEventRecord(ctx->ev_zero, ctx->stream_aux));
        ctx->zero_pending = true;
    } else {
        HIPCHK(ctx, hipMemsetAsync(ctx->stats, 0, ctx->stats_len * sizeof(double), ctx->stream));
    }
    ctx->stats_fresh = true;
    if (ctx->hmm_ksai) return pcl_hmm_acc_zero(ctx);      // the per-unit transition accumulators restart at ln 0 (LHMM.py:84-85)
    return PCL_OK;
}

// what pcl_batch_accumulate needs of the batch and the context (checked before anything is queued; pcl_batch_accumulate_exchange checks
// it BEFORE it opens the pipe: a pass that cannot run must not be followed by an exchange of incomplete statistics)
static int accumulate_precheck(pcl_batch *b, int precision, const char *who) {
    pcl_ctx *ctx = b->ctx;
    if (precision != PCL_F32 && precision != PCL_F64) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: precision %d", who, precision);
    if (!b->have_post) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: run pcl_batch_forward_backward (or set_posteriors) first", who);
    if (!b->have_B) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no emissions", who);
    if (!b->have_states) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: pcl_batch_set_states was not called", who);
    if (ctx->F == 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no frames uploaded", who);
    if (ctx->FDhost != ctx->Dhost) PCL_FAIL(ctx, PCL_ERR_INVALID, "data dimension %d does not match model dimension %d", ctx->FDhost, ctx->Dhost);
    return batch_revalidate(b, who);
}

int pcl_batch_accumulate(pcl_batch *b, int precision) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    TRY(batch_join(b));
    TRY(accumulate_precheck(b, precision, "pcl_batch_accumulate"));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (precision == PCL_F64) {
        TRY(ensure_frames64(ctx));
        TRY(pcl_ensure_layouts(ctx, PCL_LAYOUT_P64));
    }
    HIPCHK(ctx, pcl_stats_join(ctx));
    const int rc = pcl_launch_accumulate(ctx, b, precision);
    ctx->stats_fresh = false;
    if (rc == PCL_OK) HIPCHK(ctx, pcl_batch_mark(b));
    return rc;                                               // (accumulate writes nothing the recursion reads: mark_is_score stays)
}

// fMLLR statistics of the batch's utterances (frame_adapt.hip): what pcl_batch_accumulate needs of the batch, in float64
int pcl_batch_accumulate_fmllr(pcl_batch *b, const int32_t *utt_speaker) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    TRY(batch_join(b));
    TRY(accumulate_precheck(b, PCL_F64, "pcl_batch_accumulate_fmllr"));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TRY(pcl_ensure_layouts(ctx, PCL_LAYOUT_P64));
    const int rc = pcl_launch_fmllr_accumulate(ctx, b, utt_speaker);
    if (rc == PCL_OK) HIPCHK(ctx, pcl_batch_mark(b));
    return rc;
}

// MLLT statistics of the batch's utterances (frame_mllt.hip): the frame side of G_i, from the posteriors pcl_batch_accumulate reads
int pcl_batch_accumulate_mllt(pcl_batch *b, const int32_t *utt_keep) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    TRY(batch_join(b));
    TRY(accumulate_precheck(b, PCL_F64, "pcl_batch_accumulate_mllt"));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TRY(pcl_ensure_layouts(ctx, PCL_LAYOUT_P64));
    const int rc = pcl_launch_mllt_accumulate(ctx, b, utt_keep);
    if (rc == PCL_OK) HIPCHK(ctx, pcl_batch_mark(b));
    return rc;
}

int pcl_batch_accumulate_exchange(pcl_batch *b, int precision, double c_covariance, int payload, int update_transitions, int n_chunks) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!ctx->stats) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_accumulate_exchange: no model uploaded");
    HIPCHK(ctx, pcl_stats_join(ctx));
    if (payload != PCL_F64 && payload != PCL_F32) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_accumulate_exchange: payload %d", payload);
    if (n_chunks < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_accumulate_exchange: n_chunks %d", n_chunks);
    if (ctx->transport == 0 && ctx->nranks != 1) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_accumulate_exchange: pcl_comm_init was not called");
    if (update_transitions && !ctx->hmm_ksai) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_accumulate_exchange: update_transitions without pcl_units_upload");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TRY(accumulate_precheck(b, precision, "pcl_batch_accumulate_exchange"));   // nothing is exchanged for a pass that cannot run
    TRY(pcl_pipe_begin(ctx, c_covariance, payload, n_chunks));
    int rc = pcl_batch_accumulate(b, precision);                 // releases chunks as its state groups finish
    // (a failure from here on is a HIP / allocation error in the middle of the pass: the pipe is closed -- the collectives stay
    //  matched across the ranks -- and the error is returned; the caller must treat the model as undefined)
    const int rf = pcl_pipe_finish(ctx, update_transitions);     // (always: closes the pipe)
    if (rc == PCL_OK) rc = rf;
    if (rc != PCL_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

int pcl_accumulate_exchange_idle(pcl_ctx *ctx, double c_covariance, int payload, int update_transitions, int n_chunks) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ctx->stats) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_accumulate_exchange_idle: no model uploaded");
    HIPCHK(ctx, pcl_stats_join(ctx));
    if (payload != PCL_F64 && payload != PCL_F32) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_accumulate_exchange_idle: payload %d", payload);
    if (n_chunks < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_accumulate_exchange_idle: n_chunks %d", n_chunks);
    if (ctx->transport == 0 && ctx->nranks != 1) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_accumulate_exchange_idle: pcl_comm_init was not called");
    if (update_transitions && !ctx->hmm_ksai) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_accumulate_exchange_idle: update_transitions without pcl_units_upload");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TRY(pcl_pipe_begin(ctx, c_covariance, payload, n_chunks));
    TRY(pcl_pipe_finish(ctx, update_transitions));               // every chunk, in order: the collectives the other ranks' passes release
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PCL_OK;
}

int pcl_mstep(pcl_ctx *ctx, double c_covariance) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ctx->stats) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_mstep: no model uploaded");
    HIPCHK(ctx, pcl_stats_join(ctx));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return pcl_launch_mstep(ctx, c_covariance);
}

int pcl_model_conditioning(pcl_ctx *ctx, float *cond, float *cond_max) {
    if (!ctx) return PCL_ERR_INVALID;
    if (ctx->cond.empty()) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_model_conditioning: no model uploaded");
    if (cond) memcpy(cond, ctx->cond.data(), ctx->cond.size() * sizeof(float));
    if (cond_max) *cond_max = ctx->cond_max;
    return PCL_OK;
}

int pcl_score_occupancy(pcl_ctx *ctx, int workgroups_per_cu) {
    if (!ctx) return PCL_ERR_INVALID;
    if (workgroups_per_cu != 0 && workgroups_per_cu != 2) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_score_occupancy: 0 (default) or 2");
    ctx->score_wgs_per_cu = workgroups_per_cu;
    return PCL_OK;
}

int pcl_model_split_info(pcl_ctx *ctx, int *n_off, int *limit) {
    if (!ctx) return PCL_ERR_INVALID;
    if (ctx->nbad.empty()) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_model_split_info: no model uploaded");
    if (n_off) memcpy(n_off, ctx->nbad.data(), ctx->nbad.size() * sizeof(int));
    if (limit) *limit = ctx->split_max;
    return PCL_OK;
}

int pcl_model_download(pcl_ctx *ctx, double *mean, double *var, double *weight) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ctx->mean64) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_model_download: no model uploaded");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->J * ctx->M * ctx->Dhost;
    DevBuf<double> tmp;                                      // (released with the device-wide wait, on every path)
    TRY(tmp.alloc(ctx, n));
    const double *srcs[3] = {ctx->mean64, ctx->var64, ctx->w64};
    double *dsts[3] = {mean, var, weight};
    for (int k = 0; k < 3; ++k) {
        if (!dsts[k]) continue;
        const int inner = (k == 2) ? 1 : ctx->Dhost;
        TRY(pcl_launch_pack(ctx, srcs[k], k != 2, tmp));
        HIPCHK(ctx, hipMemcpyAsync(dsts[k], tmp, (size_t)ctx->J * ctx->M * inner * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return PCL_OK;
}

int pcl_accumulate_prune(pcl_ctx *ctx, double log2_threshold) {
    if (!ctx) return PCL_ERR_INVALID;
    if (log2_threshold > 0.0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_accumulate_prune: threshold 2^%g > 1", log2_threshold);
    ctx->acc_prune_log2 = log2_threshold;
    return PCL_OK;
}

int pcl_stats_download(pcl_ctx *ctx, double *acc, double *alpha_acc, double *mean_acc, double *cov_acc) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ctx->stats) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_stats_download: no model uploaded");
    HIPCHK(ctx, pcl_stats_join(ctx));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return pcl_stats_block_download(ctx, ctx->stats, acc, alpha_acc, mean_acc, cov_acc);
}

}  // extern "C"

// A statistics block [acc | alpha | mean | cov] of the current model's shape -> the caller's dense arrays (NULLs are skipped): the live block
// (pcl_stats_download) or the held numerator set (pcl_ebw_stats_download, model_ebw.hip)
int pcl_stats_block_download(pcl_ctx *ctx, const double *block, double *acc, double *alpha_acc, double *mean_acc, double *cov_acc) {
    const int J = ctx->J, M = ctx->M, Mp = ctx->Mpad, D = ctx->Dhost, Dd = ctx->D;
    const size_t o_alpha = (size_t)J * Mp, o_mean = o_alpha + J, o_cov = o_mean + (size_t)J * Mp * Dd;
    // only as far as the caller asks (the two moment blocks are 99 % of the bytes)
    const size_t need = cov_acc ? ctx->stats_len : mean_acc ? o_cov : o_mean;
    std::vector<double> h(need);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), block, need * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const double *a = h.data(), *al = a + o_alpha, *me = a + o_mean, *co = a + o_cov;
    for (int j = 0; j < J; ++j) {
        if (alpha_acc) alpha_acc[j] = al[j];
        for (int m = 0; m < M; ++m) {
            if (acc) acc[(size_t)j * M + m] = a[(size_t)j * Mp + m];
            for (int d = 0; d < D; ++d) {
                if (mean_acc) mean_acc[((size_t)j * M + m) * D + d] = me[((size_t)j * Mp + m) * Dd + d];
                if (cov_acc) cov_acc[((size_t)j * M + m) * D + d] = co[((size_t)j * Mp + m) * Dd + d];
            }
        }
    }
    return PCL_OK;
}
