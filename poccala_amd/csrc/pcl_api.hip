// pcl_api.hip -- host side of the C-ABI declared in include/poccala_hip.h: the context (streams, timers, teardown), the model and frame
// uploads, page-locked host memory and the context-level statistics calls.  The batches are pcl_batch.hip's, the device memory pool
// pcl_pool.hip's; the kernels are launched by the files that hold them.
#include <math.h>
#include <stdio.h>

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

int ensure_frames64(pcl_ctx *ctx) {
    if (ctx->frames64 || !ctx->frames32) return PCL_OK;
    const size_t n = (size_t)ctx->F * ctx->FD;
    TRY(ctx->frames64.alloc(ctx, n));
    return pcl_launch_cast(ctx, nullptr, ctx->frames32, ctx->frames64, n);   // float -> double is exact
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

// what a statistics exchange needs of the context, in `who`'s name, before the pipe is opened (the main stream goes behind a pending pcl_stats_zero)
int exchange_precheck(pcl_ctx *ctx, const char *who, int payload, int n_chunks, int update_transitions) {
    if (!ctx->stats) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no model uploaded", who);
    HIPCHK(ctx, pcl_stats_join(ctx));
    if (payload != PCL_F64 && payload != PCL_F32) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: payload %d", who, payload);
    if (n_chunks < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: n_chunks %d", who, n_chunks);
    if (ctx->transport == 0 && ctx->nranks != 1) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: pcl_comm_init was not called", who);
    if (update_transitions && !ctx->hmm_ksai) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: update_transitions without pcl_units_upload", who);
    return PCL_OK;
}

int pcl_accumulate_exchange_idle(pcl_ctx *ctx, double c_covariance, int payload, int update_transitions, int n_chunks) {
    if (!ctx) return PCL_ERR_INVALID;
    TRY(exchange_precheck(ctx, "pcl_accumulate_exchange_idle", payload, n_chunks, update_transitions));
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
