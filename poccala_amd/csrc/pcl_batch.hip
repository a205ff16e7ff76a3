// pcl_batch.hip -- every entry point that takes a pcl_batch *: the batch's lifecycle, what is set on it, the scoring, the recursions on
// the second stream, the owner-map passes over its Viterbi paths, the result downloads and the batch-level accumulate calls.  (C linkage
// comes with the declarations: include/poccala_hip.h, and pcl_internal.h for what other files of the library call.)
#include <math.h>

#include <memory>

#include "pcl_internal.h"

// The dynamic-programming kernels of a batch run on a second, higher-priority stream (one wave per utterance, no
// matrix work: they fit beside another batch's scoring).  Anything else that touches the batch on the main stream
// first orders the main stream behind them.
int batch_join(pcl_batch *b) {
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

int pcl_batch_reap(pcl_ctx *ctx, bool wait) {
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
    b->have_fb = b->have_vit = b->have_mbr = b->have_lat = false;
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
    b->have_mbr = b->have_lat = false;                             // (pcl_batch_mbr's accuracy was taken against the map that just went; the lattice's decode too)
    b->virt_rows_filled = false;
    b->model_J = ctx->J;
    return PCL_OK;
}

// A batch outlives pcl_frames_upload / pcl_model_upload calls (the drop-in classes re-upload on the shared engine all
// the time): its frame rows and state ids were checked against the buffers of THEN.  Re-check against the buffers of
// NOW before any kernel indexes them.
static int batch_revalidate(pcl_batch *b, const char *who) {
    pcl_ctx *ctx = b->ctx;
    if (!shape_fits_frames(b->shape, ctx->F))
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
    b->have_fb = b->have_vit = b->have_mbr = b->have_lat = false;
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
    b->have_fb = b->have_vit = b->have_mbr = b->have_lat = false;
    return PCL_OK;
}

int pcl_batch_forward_backward(pcl_batch *b, int fix_pi, double threshold) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_trans) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_forward_backward: no transitions set");
    if (!b->have_B) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_forward_backward: no emissions (score or set_emissions first)");  // LHMM.py:69
    HIPCHK(ctx, hipSetDevice(ctx->device));
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
    // stream_dp waits for everything queued on the main stream so far (the scoring of this batch), runs the recursion, and leaves an event
    // for whoever touches the batch next.  AFTER_FETCH: copies of the previous results read lgam / ksai / logp, which the pass rewrites
    TRY(pcl_run_recursion(b, PCL_REC_AFTER_FETCH | PCL_REC_RETIRES_MARK, [&] { return pcl_launch_forward_backward(ctx, b, fix_pi ? 1 : 0, threshold); }));
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
    if (!b->bp) {
        TRY(b->bp.alloc(ctx, (size_t)b->shape.sumNT));
        TRY(b->path.alloc(ctx, (size_t)b->shape.sumT));
        TRY(b->point.alloc(ctx, (size_t)b->U));
    }
    // like the forward-backward: on the second stream, behind everything the main stream has queued (this batch's scoring), beside
    // the NEXT batch's scoring; in order with a forward-backward of the same batch already queued there (round 4: on the main
    // stream the 0.35 ms recursion sat between two scoring kernels -- config 3's step is score + Viterbi).  AFTER_FETCH: copies of the
    // previous results read path / point
    TRY(pcl_run_recursion(b, PCL_REC_AFTER_FETCH | PCL_REC_JOIN_ON_MAIN | PCL_REC_RETIRES_MARK, [&] { return pcl_launch_viterbi(ctx, b, end_state_back ? 1 : 0); }));
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

// What the owner map of a batch's Viterbi paths needs (BatchOwnerMap's three callers), checked before anything is queued
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
    if (!shape_fits_frames(b->shape, ctx->F))
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the batch refers to frame rows up to %lld but the frame matrix now has %lld rows (re-uploaded after the batch was created)",
                 who, b->shape.max_frame_end, (long long)ctx->F);
    if (ctx->F > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: frame matrix of %lld rows", who, (long long)ctx->F);
    const UttOverlap o = shape_overlap(b->shape);     // a frame has one owner
    if (o.found) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterances %d and %d overlap in the frame matrix", who, o.first, o.second);
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

// The owner map of a label batch's Viterbi paths, on the device for the length of one entry point (the caller has run align_precheck and
// batch_join): d_state[f] = the state that owns row f of the frame matrix (-1: none), d_drop[u] = utterance u was dropped.  `queue` adds
// the caller's own main-stream work on the two ahead of the batch's mark; `consume` runs on the finished map with the utterances' lengths
// and first rows, as the frame-level accumulate launchers take them.  The stream is waited for on EVERY path, a failed one included:
// the map goes back to the pool without the device-wide wait.  The error text of that wait is `who`'s.
template <typename Queue, typename Consume>
static int with_owner_map(pcl_batch *b, const char *who, bool tied_owner, Queue queue, Consume consume) {
    pcl_ctx *ctx = b->ctx;
    const long long F = ctx->F;
    const int e = ctx->S - 2;
    DevBuf<int32_t> d_state, d_drop;
    int rc = [&]() -> int {
        TRY(align_labels_up(b));
        TRY(d_state.alloc(ctx, (size_t)F));
        TRY(d_drop.alloc(ctx, (size_t)b->U));
        HIPCHK(ctx, hipMemsetAsync(d_state, 0xff, (size_t)F * sizeof(int32_t), ctx->stream));
        TRY(pcl_launch_align_segments(ctx, b, b->lab.label_len_max, e, d_state, d_drop));
        if (tied_owner && b->tied) TRY(pcl_launch_tied_owner(ctx, b, e, d_state));   // unit * P + slice -> the position's tied state of that slice
        TRY(queue(d_state, d_drop));
        HIPCHK(ctx, pcl_batch_mark(b));
        return PCL_OK;
    }();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PCL_OK) {
        pcl_set_error(ctx, (std::string(who) + ": HIP error").c_str());
        rc = PCL_ERR_HIP;
    }
    if (rc == PCL_OK) {
        std::vector<int32_t> T(b->U);
        std::vector<int64_t> begin(b->U);
        for (int u = 0; u < b->U; ++u) {
            T[u] = b->shape.utt[u].T;
            begin[u] = b->shape.utt[u].frame0;
        }
        rc = consume(d_state, T.data(), begin.data());              // (waits for its kernels)
        if (rc != PCL_OK) (void)hipStreamSynchronize(ctx->stream);  // ... unless it gave up half-way
    }
    pcl_free_synced_scope done;
    d_state.release();
    d_drop.release();
    return rc;
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
    // tied owners: the caller's owners are the model's states.  This pass alone hands the map to the host: the copies are complete with the scope's wait
    return with_owner_map(b, who, true, [&](const int32_t *d_state, const int32_t *d_drop) -> int {
        if (frame_state_out) HIPCHK(ctx, hipMemcpyAsync(frame_state_out, d_state, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (dropped_out) HIPCHK(ctx, hipMemcpyAsync(dropped_out, d_drop, (size_t)b->U * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        return PCL_OK;
    }, [&](const int32_t *d_state, const int32_t *, const int64_t *) { return out ? pcl_seg_create_device(ctx, F, ctx->J, d_state, out) : PCL_OK; });
}

// LDA class statistics from the batch's Viterbi paths (frame_lda.hip): the owner map pcl_batch_align_segments makes stays on the device
int pcl_batch_accumulate_lda(pcl_batch *b, const int32_t *state_class) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    const char *who = "pcl_batch_accumulate_lda";
    TRY(stats_have(ctx, who, ctx->lda));
    TRY(align_precheck(b, who));
    if (!state_class && ctx->J > ctx->lda.R)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: state_class is NULL (every state its own class) but the model has %d states and the statistics %d classes", who, ctx->J, ctx->lda.R);
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // tied owners: state_class maps the model's states
    return with_owner_map(b, who, true, [](const int32_t *, const int32_t *) { return PCL_OK; }, [&](const int32_t *d_state, const int32_t *T, const int64_t *begin) {
        return pcl_launch_lda_accumulate(ctx, who, b->U, T, begin, d_state, state_class, ctx->J);
    });
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
    if (ctx->tree.R % P != 0)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the statistics hold %d rows, no multiple of the inventory's %d emitting states per unit", who, ctx->tree.R, P);
    const int E = ctx->tree.R / P;
    if (!label_event) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: label_event is NULL", who);
    for (size_t i = 0; i < b->lab.labels.size(); ++i)
        if (label_event[i] < -1 || label_event[i] >= E)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: label_event[%zu] = %d is neither -1 nor an event in [0, %d)", who, i, (int)label_event[i], E);
    TRY(batch_join(b));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // this pass's own two: the statistics row of every frame, from the caller's event of every label position.  (Until the memset is queued
    // an early return lets them go with the device-wide wait; from then on with_owner_map waits on every path.)
    DevBuf<int32_t> d_row, d_event;
    TRY(d_row.alloc(ctx, (size_t)ctx->F));
    TRY(d_event.alloc(ctx, b->lab.labels.size()));
    HIPCHK(ctx, pcl_h2d(ctx, d_event, label_event, b->lab.labels.size() * sizeof(int32_t)));
    HIPCHK(ctx, hipMemsetAsync(d_row, 0xff, (size_t)ctx->F * sizeof(int32_t), ctx->stream));
    // no tied owners: the rows are read off unit * P + slice
    const int rc = with_owner_map(b, who, false, [&](const int32_t *d_state, const int32_t *) { return pcl_launch_tree_label_rows(ctx, b, d_event, P, d_state, d_row); },
                                  [&](const int32_t *, const int32_t *T, const int64_t *begin) { return pcl_launch_tree_accumulate(ctx, who, b->U, T, begin, d_row); });
    pcl_free_synced_scope done;
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
    TRY(exchange_precheck(ctx, "pcl_batch_accumulate_exchange", payload, n_chunks, update_transitions));
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
