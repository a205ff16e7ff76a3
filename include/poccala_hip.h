/*
 * poccala_hip.h  --  C-ABI of libpoccala_hip.so, the MI355X (gfx950) engine for the
 * GMM-HMM hot path of Byshx/Poccala.
 *
 * The reference has no FFI layer: its boundary is the Python class surface
 * (StatisticalModel/LHMM.py, StatisticalModel/Clustering.py, AcousticModel/AcousticModel.py).
 * Every entry point below names the reference function(s) it replaces.  The Python
 * drop-in classes in poccala_amd/ call these through ctypes and nothing else.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  Return 0 on success, a negative
 *     pcl_status on failure; pcl_last_error() gives the message.  Nothing throws
 *     across the ABI.
 *   - The caller owns every host buffer (C-contiguous NumPy arrays).  The library
 *     owns all device memory (inside pcl_ctx / pcl_batch).
 *   - One pcl_ctx = one GPU.  Calls on a ctx are serialised by the caller (one process or
 *     thread per GPU).  Internally a ctx owns two HIP streams: pcl_batch_forward_backward and
 *     pcl_batch_viterbi run on the second one, ordered after everything queued before them, so that they
 *     overlap the scoring of ANOTHER batch queued after them; any later call on the same
 *     batch, pcl_sync and every download wait for it (env PCL_DP_STREAM=0: one stream).  Uploads, downloads (pcl_batch_get,
 *     pcl_*_download) and pcl_stats_allreduce are synchronous at return.  The compute
 *     calls -- pcl_batch_score / _forward_backward / _viterbi / _accumulate,
 *     pcl_stats_zero, pcl_mstep -- are ASYNCHRONOUS: they enqueue kernels in call order
 *     and return; pcl_sync() or any download completes them.
 *   - Host-side matrices use the REFERENCE layout: (N,T) row-major emission /
 *     alpha / beta matrices, float64, log domain, -inf for impossible.
 *   - log A and log pi are passed ALREADY LOGGED by the caller (np.log), because
 *     bit-exact Viterbi is defined on those values (LHMM.py:571,577).
 */
#ifndef POCCALA_HIP_H
#define POCCALA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: what this header declares is what libpoccala_hip.so exports, nothing else
 * (tests/test_cabi_loads.py holds exported pcl_* == declared). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct pcl_ctx pcl_ctx;
typedef struct pcl_batch pcl_batch;
typedef struct pcl_seg pcl_seg;     /* segmental GMM training, below */

typedef enum {
    PCL_OK = 0,
    PCL_ERR_INVALID = -1,  /* bad argument / shape (reference: DataDimensionError, AssertionError) */
    PCL_ERR_HIP = -2,      /* HIP runtime error */
    PCL_ERR_STATE = -3,    /* call order (e.g. score before model upload) */
    PCL_ERR_NOMEM = -4,
    PCL_ERR_COMM = -5      /* RCCL error */
} pcl_status;

/* arithmetic of the scoring / accumulate kernels */
#define PCL_F32 0 /* f32 Gaussian arithmetic, f64 dynamic programming (headline mode) */
#define PCL_F64 1 /* everything float64 (alignment-parity mode)            */

/* pcl_model_upload flags */
#define PCL_MODEL_Q1_SUMVAR 0 /* reference constant: -D/2 ln2pi - 1/2 sum(var)   (util.py:29, quirk Q1) */
#define PCL_MODEL_LOGDET 1    /* textbook constant:  -D/2 ln2pi - 1/2 sum(ln var) (opt-in, not parity)  */
/* The flag belongs to the RESIDENT MODEL, not to a call: only pcl_model_upload and the flat starts (pcl_model_flat_start,
 * pcl_flat_start) set it, and everything that rewrites the resident model afterwards keeps it -- pcl_mstep, pcl_em_exchange and
 * pcl_batch_accumulate_exchange (state ranges re-derived on their own), pcl_model_mixup, pcl_model_transform_means, pcl_mstep_map and
 * the re-upload after pcl_seg_kmeans.  Scoring, the accumulate pass and segmental EM all read it from there; uploading the same arrays
 * with the other flag is a new model (tests/test_gpu_logdet.py). */

/* row kinds in pcl_batch_set_states: >=0 is a GMM state id */
#define PCL_ROW_ENTRY (-1) /* VirtualState(1.): ln 1 = 0   (AcousticModel.py:218,1039-1043) */
#define PCL_ROW_EXIT (-2)  /* VirtualState(0.): ln 0 = -inf (AcousticModel.py:219)          */

/* pcl_batch_get selectors */
typedef enum {
    PCL_GET_B = 0,       /* emission matrices, ragged, (N_u,T_u) row-major f64  == LHMM.B_p / embedded() B   */
    PCL_GET_ALPHA = 1,   /* forward  matrices of the final pass, same layout    == LHMM.__result_f           */
    PCL_GET_BETA = 2,    /* backward matrices of the final pass                 == LHMM.__result_b           */
    PCL_GET_LGAMMA = 3,  /* ln gamma_t(i) = alpha+beta - LSE_i(alpha+beta), (N_u,T_u)  (LHMM.py:486-500); ln 0 for a one-frame utterance (the reference raises on it) */
    PCL_GET_KSAI = 4,    /* un-normalised ln xi, ragged dense (N_u,N_u) f64     == LHMM.__ksai (quirk Q5)    */
    PCL_GET_GAMMA = 5,   /* un-normalised ln gamma, ragged (N_u,) f64           == LHMM.__gamma              */
    PCL_GET_PI = 6,      /* pi after the final pass, ragged (N_u,) f64, LINEAR  == LHMM.pi                   */
    PCL_GET_LOGP = 7,    /* LSE_i alpha_{T-1}(i) of the final pass, (U,) f64    == __expectation, LHMM.py:412 */
    PCL_GET_NPASS = 8,   /* Baum-Welch passes run, (U,) int32 (quirk Q6)                                     */
    PCL_GET_QTRACE = 9,  /* Q after each pass, (U, PCL_MAX_PASS) f64, unused = NaN                            */
    PCL_GET_PATH = 10,   /* Viterbi state indices, ragged (T_u,) int32          == LHMM.viterbi mark_state   */
    PCL_GET_POINT = 11,  /* Viterbi score, (U,) f64                             == LHMM.viterbi point        */
    PCL_GET_KSAI_NZ = 12 /* ln xi of the stored transitions only (ln A > -inf), row-major order per utterance, f64;
                            a sentence HMM has ~2N of them instead of N*N                                     */
} pcl_get_what;
#define PCL_MAX_PASS 16

/* ---------------------------------------------------------------- context */
int pcl_init(int device, pcl_ctx **out);
/* pcl_destroy may be called with work in flight: it drains every stream of the context first (so asynchronous result copies have
 * landed when it returns), then releases the communicator, the batches already handed to pcl_batch_destroy, the model and the
 * streams.  Batches the caller never destroyed are NOT walked: their device blocks stay in the process-wide pool's books (a
 * leak, not a fault) -- destroy batches first.  Page-locked host memory from pcl_host_alloc belongs to the caller: free it
 * with pcl_host_free BEFORE pcl_destroy (pcl_host_free itself waits for every stream of the context, because hipHostFree does
 * not wait for copies still using the block).  tools/lifecycle_stress.py exercises all of this.
 * Inside the library every device array and event belongs to one owning member of the context, the batch or the segment set, or to a
 * local of the call that made it: destroying the handle (or leaving the call, on any path) gives them back; pcl_pool_stats counts. */
int pcl_destroy(pcl_ctx *ctx);
/* The process-wide device memory pool's books (any argument may be NULL): blocks / bytes handed out and not yet given back (0 / 0 once
 * every handle of the process is destroyed), bytes cached for reuse, successful hipMalloc calls so far, and the device-wide waits
 * (hipDeviceSynchronize) its frees have made so far. */
int pcl_pool_stats(size_t *handed_out_blocks, size_t *handed_out_bytes, size_t *cached_bytes, uint64_t *device_allocs, uint64_t *device_waits);
const char *pcl_last_error(pcl_ctx *ctx); /* ctx may be NULL: error of a failed pcl_init */
int pcl_sync(pcl_ctx *ctx);
/* name (cap bytes), compute units, HBM bytes */
int pcl_device_info(pcl_ctx *ctx, char *name, int cap, int *cus, size_t *hbm_bytes);
/* GPU time of a kernel group since the last query, measured with HIP events recorded on the ctx
 * stream around every launch: which = "score" | "fb" | "viterbi" | "accumulate" | "allreduce" |
 * "mfcc" | "vad_dist" | "vad_osf" | "vad_select" | "vad_gather" | "moments" | "flat_fill" | "derive" (the derive pass of
 * pcl_model_upload / pcl_model_flat_start / pcl_model_mixup) | "mixup" (pcl_model_mixup's plan and fill) | "adapt" | "adapt_gk" | "adapt_solve" (pcl_mllr_estimate and its kin, below) | "fmllr" | "fmllr_frames" | "fmllr_gk" | "fmllr_solve" (pcl_fmllr_estimate and its kin, below) | "mllt" | "mllt_frames" | "mllt_gk" | "mllt_solve" (pcl_mllt_estimate and its kin, below) | "pcm_stage" | "pcm_h2d" (the front-end's transfer: see pcl_mfcc_pcm16) | "pitch_nccf" | "pitch_track" | "pitch_out" (pcl_pitch).
 * Returns the summed milliseconds and the number of launches, then resets the group. */
int pcl_kernel_time(pcl_ctx *ctx, const char *which, float *total_ms, int *launches);
/* The events behind pcl_kernel_time are recorded only while timing is on (default off, or env PCL_TIMERS=1): a
 * training run that never queries them pays nothing and keeps nothing.  Turning it off drops pending events. */
int pcl_timing_enable(pcl_ctx *ctx, int on);
/* HIP devices visible to this process (0 without a GPU); does not create a context. */
int pcl_device_count(int *n);

/* ------------------------------------------------------------------ model
 * Replaces Clustering.GMM parameter state (T2: mean (M,D), covariance (M,D,D) of which only the
 * diagonal is used -- util.py:23 --, alpha (M,)) for J GMM states at once.  `var` is the DIAGONAL.
 * Derived device layouts (f32 and f64) are built here, in float64, once. */
int pcl_model_upload(pcl_ctx *ctx, int J, int M, int D, const double *mean /* J*M*D */,
                     const double *var /* J*M*D */, const double *weight /* J*M */, int flags);

/* ----------------------------------------------------------------- frames
 * The (F,D) MFCC matrix of the whole batch/corpus shard, rows = frames (LHMM.add_data, the `data`
 * argument of cal_observation_pro).  dtype: PCL_F32 or PCL_F64 host element type. */
int pcl_frames_upload(pcl_ctx *ctx, int64_t F, int D, const void *frames, int dtype);

/* Streaming form for a corpus that is fed chunk by chunk (BASELINE config 5; the reference reads one utterance at a time
 * from disk inside its worker, AcousticModel.py:723-768).  Two device slots: pcl_frames_stage queues the H2D copy of the
 * NEXT chunk (float32, row-major (F,D)) on the library's copy stream, into the slot that is not current, behind the
 * last kernels that read that slot, and returns at once; pcl_frames_swap waits for that copy (after it returns the
 * caller's buffer is free again) and makes the staged chunk the current frame matrix for batches created afterwards.
 * Batches of the previous chunk stay valid for everything that does not read frames (decode, forward-backward, Viterbi,
 * downloads); scoring / accumulating them again fails the row check unless the new chunk is at least as long.
 * pcl_host_alloc returns page-locked host memory (the copy is then truly asynchronous); any host pointer works. */
int pcl_frames_stage(pcl_ctx *ctx, int64_t F, int D, const float *frames);
int pcl_frames_swap(pcl_ctx *ctx);
int pcl_host_alloc(pcl_ctx *ctx, size_t bytes, void **out);
int pcl_host_free(pcl_ctx *ctx, void *ptr);

/* ------------------------------------------------------------------ batch
 * A batch = U sentence-level HMMs (AcousticModel.embedded, AcousticModel.py:957-1014), utterance u
 * having N[u] states and T[u] frames starting at row frame_begin[u] of the uploaded frame matrix
 * (frame_begin may be NULL when emissions are supplied with pcl_batch_set_emissions).  At most 65535 utterances, 2^31 - 1 rows
 * (sum N) and frames (sum T) per batch: PCL_ERR_INVALID beyond that -- a corpus goes through in several batches. */
int pcl_batch_create(pcl_ctx *ctx, int U, const int32_t *N, const int32_t *T, const int64_t *frame_begin,
                     pcl_batch **out);
int pcl_batch_destroy(pcl_batch *b);

/* ln A (ragged dense (N_u,N_u) row-major, -inf where A == 0) and ln pi (ragged (N_u,)).
 * == the transmat / pi arguments of LHMM.__init__ (LHMM.py:19) and LHMM.viterbi (LHMM.py:547). */
int pcl_batch_set_transitions(pcl_batch *b, const double *logA, const double *logpi);

/* Row -> GMM state map, ragged (N_u,): state id in [0,J), or PCL_ROW_ENTRY / PCL_ROW_EXIT.
 * == the profunction list of each unit HMM laid out by embedded() (AcousticModel.py:990-1001). */
int pcl_batch_set_states(pcl_batch *b, const int32_t *row_state);

/* Emissions given by the caller (ragged (N_u,T_u) row-major f64) instead of scored here
 * == LHMM(probmat=[B]) (LHMM.py:75) and the `prob` argument of LHMM.viterbi (LHMM.py:547). */
int pcl_batch_set_emissions(pcl_batch *b, const double *B);

/* Posteriors given by the caller (ragged (N_u,T_u) row-major f64, ln gamma_t(i)) instead of computed by
 * pcl_batch_forward_backward == the l_value argument of Clustering.GMM.update_acc (Clustering.py:653). */
int pcl_batch_set_posteriors(pcl_batch *b, const double *lgamma);

/* A1+A4+A5+A6: fill every row of every emission matrix:  ln b_j(o_t) = LSE_m[ln w_m + N(o_t; mu_m, var_m)]
 * == LHMM.cal_observation_pro (LHMM.py:163-187) -> Clustering.GMM.point (Clustering.py:740-767)
 *    -> util.gaussian_function (util.py:20-31), batched state-major over the whole batch. */
int pcl_batch_score(pcl_batch *b, int precision);

/* A8..A11 (+ the per-frame posteriors of A12): the Baum-Welch pass loop of LHMM.baulm_welch
 * (LHMM.py:526-544) for an LHMM built with probmat: forward (:335-351), backward (:353-366),
 * xi/gamma/pi (:394-471), Q (:412-422); passes repeat while Q - Q_prev > threshold (0.64, :539).
 * fix_pi = bit0 of the reference's fix_code (LHMM.py:140-145).  Results stay on the device;
 * read them with pcl_batch_get. */
int pcl_batch_forward_backward(pcl_batch *b, int fix_pi, double threshold);

/* A14: LHMM.viterbi (LHMM.py:546-609), end_state_back = 0|1 (quirk Q9). Bit-exact in f64. */
int pcl_batch_viterbi(pcl_batch *b, int end_state_back);

/* Next row f2: what follows forced alignment in training scheme 1, per frame, on the device.  row_unit: ragged (N_u,)
 * int32, the unit each HMM row belongs to (the `states` dictionary of AcousticModel.embedded, AcousticModel.py:968-976,
 * as integers).  Outputs, ragged (T_u,) int32: frame_unit[t] = unit of the Viterbi path at t (the name sequence of
 * AcousticModel.viterbi, :1016-1027) and frame_k[t] = which of the unit's gmm_num GMM states the frame is given to when
 * every run of equal unit (AcousticModel.discriminate, :937-955) is cut into gmm_num slices the way __eq_segment mode 'g'
 * (:614-625) and __get_gmmdata (:629-644) do.  Needs pcl_batch_viterbi first.  Synchronous. */
int pcl_batch_regroup(pcl_batch *b, const int32_t *row_unit, int gmm_num, int32_t *frame_unit, int32_t *frame_k);

/* Row f8: realignment, the hop every round of training scheme 1 after the first goes through -- multi_process_data(init=False)
 * (AcousticModel.py:736-764): forced alignment, the drop rule (:751-757), then discriminate (:937-955) and __get_gmmdata's mode 'g'
 * (:614-644) -- from the Viterbi paths of a batch made by pcl_batch_create_labels to the owner map pcl_seg_create sorts by, on the
 * device.  The row -> unit map comes from the batch's own labels (row 0 -> label position 0, rows 1 .. gmm_num L -> position
 * (row - 1) / gmm_num, the exit row -> position L - 1; gmm_num = S - 2); runs and slices exactly as pcl_batch_regroup cuts them.  An
 * utterance whose path visits fewer distinct units than its label names is dropped (a label unit nobody visited).
 * frame_state_out (rows of the frame matrix,) int32 or NULL: unit * gmm_num + k for the frames of the kept utterances, -1 for the
 * dropped ones and for every row outside the batch -- pcl_seg_create's input.  dropped_out (U,) int32 or NULL: 1 = dropped.  out or
 * NULL: the pcl_seg of that map, built from it ON THE DEVICE by pcl_seg_create's counting sort and gather; the map travels to the host
 * only when frame_state_out is given.  At least one of frame_state_out and out must be given.  PCL_ERR_STATE: the batch was not made
 * from labels, or pcl_batch_viterbi has not run.  PCL_ERR_INVALID: the utterances overlap in the frame matrix (a frame has ONE owner),
 * the batch no longer fits the current frame matrix, the model's J is not n_units * (S - 2) or the inventory changed since the batch
 * was made, 2 T + 2 L of an utterance beyond 16384.  Integer arithmetic only.  Synchronous. */
int pcl_batch_align_segments(pcl_batch *b, int32_t *frame_state_out /* (rows of the frame matrix,) or NULL */,
                             int32_t *dropped_out /* (U,) or NULL */, pcl_seg **out /* or NULL */);

/* ----------------------------------------------------------------- unit inventory and label-built batches
 * The reference builds, PER UTTERANCE, one LHMM per label unit (AcousticModel.init_unit / init_parameter,
 * AcousticModel.py:164-240: transmat (S,S), S-2 GMM states between an entry and an exit VirtualState) and glues them
 * into a sentence HMM (AcousticModel.embedded, :957-1014).  Here the inventory is uploaded once:
 *   trans      [n_units][S][S]  unit transition matrices (LHMM.transmat), linear
 *   log_trans  the same through np.log on the caller's side (bit-exact Viterbi is defined on those values; NULL:
 *              this library's libm log is used)
 * Unit i owns the GMM states i*(S-2) .. i*(S-2)+S-3 of the uploaded model (pcl_model_upload with J = n_units*(S-2)). */
int pcl_units_upload(pcl_ctx *ctx, int n_units, int S, const double *trans, const double *log_trans);
int pcl_units_download(pcl_ctx *ctx, double *trans /* [n_units][S][S], after pcl_mstep_transitions */);

/* A7 for U utterances at once: labels = concatenated unit ids, label_len[u] of them per utterance.  Builds what
 * AcousticModel.embedded builds -- N_u = (S-2) L_u + 2 states, the banded transition structure (embedded_transmat
 * :979-989), the row -> GMM state map (embedded_prob :990-1001), uniform pi (embedded_pi :1003-1006; logpi[u] =
 * np.log(1/N_u) from the caller, NULL: libm) -- and keeps the label structure with the batch for pcl_batch_accumulate_hmm.
 * Equivalent to pcl_batch_create + pcl_batch_set_transitions + pcl_batch_set_states on host-built matrices. */
int pcl_batch_create_labels(pcl_ctx *ctx, int U, const int32_t *label_len, const int32_t *labels, const int32_t *T,
                            const int64_t *frame_begin, const double *logpi, pcl_batch **out);
/* Rebuild the batch's transitions from the CURRENT unit inventory (after pcl_mstep_transitions / pcl_em_exchange). */
int pcl_batch_refresh_transitions(pcl_batch *b);

/* A12, HMM half: LHMM.update_acc (LHMM.py:473-500) + LHMM.add_acc (:149-161) for every utterance x label position of
 * the batch: the (S-2,S) block of un-normalised ln xi and the (S-2,) slice of ln gamma (quirk Q5) of each position are
 * log-sum-exp'ed into context-resident per-unit accumulators ksai_acc [n_units][S-2][S], gamma_acc [n_units][S-2]
 * (log domain, initial -inf, LHMM.py:84-85).  pcl_stats_zero resets them too.  Needs pcl_batch_forward_backward. */
int pcl_batch_accumulate_hmm(pcl_batch *b);
int pcl_hmm_acc_zero(pcl_ctx *ctx);
int pcl_hmm_acc_download(pcl_ctx *ctx, double *ksai_acc, double *gamma_acc);
/* A15, transition half: LHMM.update_param (LHMM.py:519-520): transmat[1:-1,:] = exp(ksai_acc - gamma_acc[:,None]) for
 * every unit that occurred; a unit that never occurred keeps its matrix (the reference would write NaN). */
int pcl_mstep_transitions(pcl_ctx *ctx);

/* ----------------------------------------------------------------- decoder (next row f3: the decode half of config 5)
 * The pronunciation tree Lexicon.PronunciationLexicon builds (Lexicon/PronunciationLexicon.py:45-94), flattened: node i
 * spells node_nunits[i] (1 or 2) units node_units[2 i ..] of the uploaded inventory (a reading split at the comma:
 * initial + final, or a lone final: Token.__init__, Decoder.py:225), its children are child_idx[child_ptr[i] ..
 * child_ptr[i+1]) in the tree's insertion order, node_word[i] != 0 where words end, roots = the first-character nodes.
 * Needs pcl_units_upload first; a new pcl_units_upload drops the tree. */
int pcl_lexicon_upload(pcl_ctx *ctx, int n_nodes, const int32_t *node_units, const int32_t *node_nunits, const int32_t *child_ptr,
                       const int32_t *child_idx, const int32_t *node_word, int n_roots, const int32_t *roots);
/* A16: frame-synchronous token passing (Decoder.py:91-167, Token.viterbi :250-288) for every utterance of an ALL-STATE
 * batch (rows entry, GMM state 0 .. J-1, exit; emissions from pcl_batch_score).  beam 0.85 and min_distinct 8 are the
 * reference's pruning rule (:34,:159-167), candidate its `transfer` width (:175); max_tokens bounds the live tokens of one
 * utterance (hand-overs beyond it are dropped and flagged); logpi_* = np.log(1/N) for N = S+0 / 2(S-2)+2 states from the
 * caller.  The reference code is dead: the gaps D1-D5 filled here are listed in
 * oracle/decoder_oracle.py, the restatement this entry point is tested against bit for bit (recursion, pruning, frame loop and in-word
 * hand-over pinned by golden G14 from the reference's own Decoder.py; the completion rules D1-D5 unpinned).
 * Two kernels, the same bits: left-to-right 5-state units (every model the reference builds, AcousticModel.py:176-181) run one
 * lane per token (hmm_decode_lr.hip), any other unit matrices 8 lanes per token (hmm_decode.hip; env PCL_DEC_GENERAL=1 forces it). */
int pcl_batch_decode(pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, double logpi_one_unit,
                     double logpi_two_units);
/* Results (NULL pointers are skipped): n_final (U,) tokens returned per utterance; node / score / hist (U, candidate), best
 * first; the word history: hist_n (U,) entries, hist_prev / hist_node (U, Tmax): entry h = (previous entry or -1, node whose
 * word ended); n_tokens (U, Tmax): live tokens after every frame; overflow (U,): 1 if max_tokens was hit. */
int pcl_batch_decode_get(pcl_batch *b, int32_t *n_final, int32_t *node, double *score, int32_t *hist, int32_t *hist_n,
                         int32_t *hist_prev, int32_t *hist_node, int32_t *n_tokens, int32_t *overflow);
/* Rule D6: a bigram language model at word ends.  The reference's decoder imports `LanguageModel.Ngram` (Decoder.py:17), builds
 * `Ngram(n=i+1).init_gram()` (:200-204) and asks it for the followers of a finished word in `passing_between_word` (:146-156), a stub on a
 * module it never shipped; without a language model a finished word hands its raw score to every first-character node (D4).  Here:
 * words have ids 0 .. W-1, id 0 = the sentence start (no node spells it); a word-end node i has the homophones
 * node_word_ids[node_word_ptr[i] .. node_word_ptr[i+1]) in the tree's order.  lm(v, w) = val[k] where col[k] == w in row
 * [row_ptr[v], row_ptr[v+1]) of the CSR bigram (col strictly ascending in a row), else bow[v] + uni[w]: float64, finite, ARPA-shaped and
 * PRE-SCALED by the caller (val = scale ln P(w|v) + penalty, uni = scale ln P(w) + penalty, bow = scale ln bow(v)) -- the device only
 * adds.  A finished token at word-end node n with score s whose history entry chose word v (0 without one) offers the roots
 * s + max_w lm(v, w) over the node's homophones, the first w on ties = its chosen word; its offer to the node's own children stays s.
 * The frame's best offer (earliest donor on ties) seeds every root and makes the frame's one history entry (donor's entry, node, chosen
 * word).  Everything else is pcl_batch_decode's; with all tables zero so is every output, bit for bit.  Final scores hold the terms of
 * the words already ended, not of a word pending at the token's own node.  Single tree, no tree copies, no look-ahead.
 * Needs pcl_lexicon_upload first; whatever drops the tree (a new pcl_lexicon_upload, a pcl_units_upload of another shape) drops the
 * language model.  Rejected with PCL_ERR_INVALID and a pcl_last_error text: non-finite values, col unsorted or outside [0,W), ids in
 * node_word_ids outside [1,W), a word-end node without a word, a node with words whose node_word is 0. */
int pcl_lm_upload(pcl_ctx *ctx, int W, const double *uni, const double *bow, const int64_t *row_ptr, const int32_t *col, const double *val,
                  const int32_t *node_word_ptr, const int32_t *node_word_ids);
/* pcl_batch_decode with the resident language model (the kernels' LM = true instantiations); PCL_ERR_STATE if none is resident.
 * Results through pcl_batch_decode_get, and the chosen word of every history entry, hist_word (U, Tmax), through
 * pcl_batch_decode_get_words (PCL_ERR_STATE unless the batch's last decode was pcl_batch_decode_lm). */
int pcl_batch_decode_lm(pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, double logpi_one_unit,
                        double logpi_two_units);
int pcl_batch_decode_get_words(pcl_batch *b, int32_t *hist_word);
/* TIED STATES IN THE DECODER.  A model over the tied states of a decision tree (tying section below: pcl_tree_build(install) ->
 * pcl_tying_upload -> EM over pcl_batch_create_labels_tied batches) has J_t states reached through a tree walk, not n_units (S - 2) states
 * at unit (S - 2) + k.  pcl_lexicon_tie runs that walk (pcl_tying_lookup's) once for every (node, unit slot j, state position k) of the
 * resident lexicon, under the resident tying, and keeps the result beside the lexicon: node_state (n_nodes, 2 P) int32, P = S - 2.
 * node_ctx (n_nodes, 2, 3) int32 = (left, centre, right) of unit slot j of node i, in the tying section's conventions: unit ids
 * 0 .. n_units - 1, n_units = no or unknown neighbour.  Slot 1 of a one-unit node is ignored on input and its node_state entries are -1.
 * THE DEFAULT CONTEXT RULE (PronunciationLexicon.node_contexts on the host; a caller who knows better passes its own node_ctx):
 *   inside a node            the neighbour is the node's other unit
 *   left of the first unit   the LAST unit of the parent node (unique in a prefix tree); n_units for a first-character node
 *   right of the last unit   ALWAYS n_units: the children differ, the tree is not copied per right context, and the edge symbol is a
 *                            member of a question like any other unit
 * Consequence: a context across a syllable boundary to the right is answered as "edge", while training labels see the next syllable's
 * first unit there (labels[i + 1], pcl_batch_create_labels_tied: unchanged); cross-word contexts are unknown on both sides.
 * Snapshot, as for tied batches: a later pcl_tying_upload / pcl_tying_drop does not change the kept states; whatever drops the lexicon
 * (a new pcl_lexicon_upload, a pcl_units_upload of another shape) drops them; pcl_lexicon_untie removes them (no refusal when there are
 * none); they remember the J_t they were made under.  Checked before anything resident changes: PCL_ERR_STATE without a resident lexicon
 * or tying; PCL_ERR_INVALID, the text naming node and slot, for a centre that is not node_units[i][j], a neighbour outside [0, n_units],
 * or a tying whose P is not the inventory's S - 2.  pcl_lexicon_states: the kept node_state; PCL_ERR_STATE when the lexicon is not tied.
 * pcl_kernel_time group: "lexicon_tie".  Synchronous.
 * pcl_batch_decode_tied = pcl_batch_decode (lm = 0) or pcl_batch_decode_lm (lm != 0) with ONE difference: the emission row of state
 * position k of unit slot j of a token at node n is 1 + node_state[n][j P + k] of an all-state batch of J_t + 2 rows (entry, states
 * 0 .. J_t - 1, exit).  Transitions stay per centre unit; pi, D1 - D6, pruning, transfer and history are untouched; results through
 * pcl_batch_decode_get (and pcl_batch_decode_get_words after lm != 0).  The kernels' TIED = true instantiations; PCL_DEC_GENERAL=1 still
 * forces the general one.  PCL_ERR_STATE: the lexicon is not tied, the resident model's J is not the J_t it was tied under, lm != 0
 * without a language model; PCL_ERR_INVALID: the batch is not an all-state batch of J_t + 2 rows. */
int pcl_lexicon_tie(pcl_ctx *ctx, const int32_t *node_ctx /* n_nodes * 2 * 3 */);
int pcl_lexicon_untie(pcl_ctx *ctx);
int pcl_lexicon_states(pcl_ctx *ctx, int32_t *node_state /* n_nodes * 2 * P */);
int pcl_batch_decode_tied(pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, double logpi_one_unit,
                          double logpi_two_units, int lm);
/* WORD LATTICES (row f20).  The single tree with one history entry per frame is a time-conditioned search: every word that ends at
 * frame t joins the same continuation, the frame's entry.  So a lattice needs no second search -- its nodes are the history entries, its
 * arcs the word-end donors -- only a record of what the decode kernels see and drop.
 * pcl_batch_decode_lattice = pcl_batch_decode (lm = 0, tied = 0), _lm (lm != 0), _tied (tied != 0; with lm != 0 its lm form) through the
 * kernels' LAT = true instantiations (PCL_DEC_GENERAL=1 still forces the general one): EVERY output of pcl_batch_decode_get / _get_words is
 * what that call gives on the same batch, bit for bit, whatever max_arcs.  Beside them the kernels write, per utterance,
 *   one arc record per word-end donor -- a token that finished (D1) at frame t at a node where words end: frame t, tok = its index among
 *     the frame's tokens, node, hist = its history entry or -1, score = its raw score s (float64), and under lm what rule D6 gave it:
 *     term = max_w lm(v, w) and word = the chosen w (lm = 0: term 0.0, word 0);
 *   per history entry, beside hist_prev / hist_node / hist_word: hist_frame = the frame it was made at, hist_seed = the winning offer
 *     (s + term of the frame's best donor) that seeded the roots.
 * At most max_arcs records per utterance are kept: beyond them nothing is written, lat_overflow[u] = 1, and n_arcs_wanted[u] still counts
 * every donor (call again with a larger max_arcs).  The decode results of such an utterance are unaffected.
 * THE LATTICE of an utterance: nodes START (index 0: history -1, seed 0, frame -1), entry k at index k + 1 (the entries ascend in frame:
 * the index order is a topological order), END at index hist_n + 1.  A recorded arc goes from node hist + 1 to the entry made at its frame
 * (a frame with a word-end donor makes one) with ac = score - seed(start node) (-inf for a score of -inf) and lm = term.  The closing arcs
 * are the decoder's own ending, the n_final tokens pcl_batch_decode_get returns: from node hist + 1 to END, ac = score - seed(start), lm
 * 0, word -1, frame T - 1, tok = the rank in the transfer; they are pending words, as final scores hold no term of a word pending at the
 * token's node.  CANONICAL ORDER, built on the device behind the decode (pcl_kernel_time "lattice_build"): recorded arcs ascending in
 * (frame, tok), closing arcs behind them in transfer order; so the arcs are sorted by end node (a CSR), and a stable counting sort gives
 * the CSR by start node.  pcl_batch_lattice_get returns this order (NULLs are skipped): n_arcs (U,) = recorded + closing arcs held,
 * n_arcs_wanted (U,), lat_overflow (U,), the arc arrays (U, max_arcs + candidate) -- frame, tok, node, hist, score, term, word, start node,
 * end node -- and hist_frame / hist_seed (U, Tmax).
 * pcl_batch_lattice_posteriors(kappa), float64, no fused multiply-add, no floating-point atomics ("lattice_post"): arc weight w = kappa ac
 * + lm (the language-model tables are pre-scaled by the caller, as ever); forward over the nodes in index order, alpha(START) = 0,
 * alpha(n) = LSE over the arcs into n of alpha(start) + w; Viterbi the same with max, the earliest arc on ties; backward in descending
 * order, beta(END) = 0, beta(n) = LSE over the arcs out of n (ascending arc index) of w + beta(end); ln Z = alpha(END);
 * ln p(a) = ((alpha(start) + w) + beta(end)) - ln Z.  Every LSE is max, then the sum of exp(v - max), over the node's list: thread i of 256
 * takes list positions i, i + 256, ... in that order, the 64 lanes of a wave combine by a butterfly (partner lane ^ 32, 16, 8, 4, 2, 1),
 * the four waves in ascending order; a maximum of +-inf is returned as itself -- a node that cannot be reached, or cannot reach END, and
 * every arc at it hold -inf, never NaN.  The best path = the back-pointers from END, as arc indices in path order, its score the Viterbi
 * value of END.  Every word of it (arc a*, frames tau in (frame(start node), frame(a*)]) gets a confidence, Wessel's C_max: the maximum
 * over tau of P(tau) = the sum, in ascending arc order, of exp(ln p(a)) over the arcs a that cover tau the same way and share a*'s
 * identity -- the word id after lm != 0 for a recorded arc, the node otherwise and for the closing arc; an empty span (a closing arc out
 * of an entry made at the last frame) gives exp(ln p(a*)).  lat_status (U,): 0, or bits 1 = overflowed, 2 = n_final is 0, 4 = a record
 * out of range, 8 = ln Z is -inf; then ln Z, the posteriors and the score are NaN and best_n is 0.
 * pcl_batch_lattice_results (NULLs are skipped): lnZ (U,), arc_lnpost (U, max_arcs + candidate), best_n (U,), best_arc and best_conf
 * (U, Tmax + 3), best_score (U,), lat_status (U,).
 * Not here: exact bigram re-expansion over arc pairs (an arc carries the term the decoder gave it, under the one predecessor word its
 * node kept), N-best lists, lattice-based MMI / MPE statistics, pruning or compaction of the lattice.
 * PCL_ERR_STATE: what the underlying decode refuses (no lexicon, emissions, language model or tie the flags ask for); _get / _posteriors
 * without a preceding pcl_batch_decode_lattice, _results without _posteriors -- new emissions, transitions, states, scoring or any other
 * decode drop the lattice.  PCL_ERR_INVALID: max_arcs < 1; kappa not finite or not > 0.  All checked before anything is changed.  The
 * buffers are the batch's own, made on first use.  The decode is queued like pcl_batch_decode; the other three are on the main stream,
 * _get and _results synchronous. */
int pcl_batch_decode_lattice(pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, double logpi_one_unit,
                             double logpi_two_units, int lm, int tied, int max_arcs);
int pcl_batch_lattice_get(pcl_batch *b, int32_t *n_arcs, int32_t *n_arcs_wanted, int32_t *lat_overflow, int32_t *arc_frame, int32_t *arc_tok,
                          int32_t *arc_node, int32_t *arc_hist, double *arc_score, double *arc_term, int32_t *arc_word, int32_t *arc_start,
                          int32_t *arc_end, int32_t *hist_frame, double *hist_seed);
int pcl_batch_lattice_posteriors(pcl_batch *b, double kappa);
int pcl_batch_lattice_results(pcl_batch *b, double *lnZ, double *arc_lnpost, int32_t *best_n, int32_t *best_arc, double *best_score,
                              double *best_conf, int32_t *lat_status);
/* TEST ENTRY.  A record set of the caller's in place of a decode's, so that the lattice pass can be held at list lengths and node counts
 * no decode of a few seconds reaches: the arrays of pcl_batch_lattice_get ((U, max_arcs), as the kernels would have appended them: frames
 * ascending, any order inside a frame) and of pcl_batch_decode_get (hist_n (U,), n_final (U,), final_* (U, candidate)), hist_frame /
 * hist_seed (U, Tmax); n_arcs_wanted may exceed max_arcs.  The build runs on them as behind a decode; a record out of range sets
 * lat_status bit 4 and is never used as an index.  T_u of the closing arcs' frame is the batch's.  with_words: as after lm != 0. */
int pcl_batch_lattice_set_records(pcl_batch *b, int max_arcs, int candidate, int with_words, const int32_t *n_arcs_wanted,
                                  const int32_t *arc_frame, const int32_t *arc_tok, const int32_t *arc_node, const int32_t *arc_hist,
                                  const double *arc_score, const double *arc_term, const int32_t *arc_word, const int32_t *hist_n,
                                  const int32_t *hist_frame, const double *hist_seed, const int32_t *n_final, const int32_t *final_node,
                                  const double *final_score, const int32_t *final_hist);

/* Copy a result to a caller buffer (layouts in pcl_get_what). */
int pcl_batch_get(pcl_batch *b, int what, void *host);

/* Results on their way to the host WHILE the GPU goes on (the end-to-end protocol moves B / gamma / paths off the
 * device).  pcl_batch_fetch_async queues, behind everything this batch has queued so far (scoring, forward-backward on the second
 * stream, Viterbi), device-to-host copies of the selected results on the library's download stream and returns at once;
 * pcl_batch_fetch_wait blocks until they have landed.  A later compute call on the SAME batch waits for the copies on the device
 * (its buffers are being read), other batches run beside them.  Destinations should be page-locked (pcl_host_alloc): a copy
 * into pageable memory is staged by the runtime and is not asynchronous.  NULL pointers are skipped.  Layouts:
 *   logp   (U,) f64                                  == PCL_GET_LOGP
 *   lgamma ragged, per utterance TIME-MAJOR (T_u, N_u) f64: the transpose of PCL_GET_LGAMMA's (N_u, T_u) -- the device layout,
 *          so that nothing but the copy stands between the kernel and the host (the caller views it transposed);
 *          == l - sum_value of LHMM.update_acc (LHMM.py:486-500), what Clustering.GMM.update_acc is fed
 *   ksai_nz f64, ln xi of the stored transitions     == PCL_GET_KSAI_NZ (LHMM.__ksai, quirk Q5)
 *   path   ragged (T_u,) int32, point (U,) f64       == PCL_GET_PATH / PCL_GET_POINT (needs pcl_batch_viterbi) */
/* sizes of the ragged result arrays of a batch: sum N_u T_u, sum N_u, sum T_u, stored transitions (ln A > -inf).  NULLs are skipped. */
int pcl_batch_sizes(pcl_batch *b, int64_t *sum_nt, int64_t *sum_n, int64_t *sum_t, int64_t *nnz);
int pcl_batch_fetch_async(pcl_batch *b, double *logp, double *lgamma_tm, double *ksai_nz, int32_t *path, double *point);
int pcl_batch_fetch_wait(pcl_batch *b);

/* The clock the shader engines actually hold, measured on the device: one wavefront on the library's auxiliary stream reads the
 * shader-clock counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) `spin_us` microseconds apart, beside
 * whatever the other streams are running.  rocm-smi's sclk is the REQUESTED level; under the matrix-pipe kernels the chip holds
 * 1.6-1.8 GHz of its 2.4.  Synchronous (waits for the probe only). */
int pcl_clock_probe(pcl_ctx *ctx, int spin_us, double *shader_mhz);

/* ----------------------------------------------------------------- E-step statistics
 * A13: Clustering.GMM.update_acc (Clustering.py:653-680) for every (utterance, emitting row) of the
 * batch, summed into ctx-resident per-state statistics.  The reference keeps them in the log domain
 * per label position and merges files later (Clustering.py:314-367); here they are LINEAR sums
 *   acc[j,m]      = sum_t gamma_t(j,m)                      (exp of GMM.acc)
 *   alpha_acc[j]  = sum_t gamma_t(j)                        (exp of GMM.alpha_acc)
 *   mean_acc[j,m,d] = sum_t gamma_t(j,m) (o_td + bias)      (exp of GMM.mean_acc, bias = 100)
 *   cov_acc[j,m,d]  = sum_t gamma_t(j,m) (o_td - mu_jmd)^2  (exp of GMM.__covariance_acc)
 * which is what RCCL can sum.  Needs pcl_batch_forward_backward first. */
int pcl_stats_zero(pcl_ctx *ctx);
int pcl_batch_accumulate(pcl_batch *b, int precision);
/* J*M, J, J*M*D, J*M*D doubles */
/* Approximate mode of pcl_batch_accumulate (off by default): (frame, state) pairs with gamma_t(j) < 2^log2_threshold are
 * left out of the statistics.  The default leaves out only pairs whose every term is EXACTLY zero in the kernel's arithmetic
 * (2^-150 in f32, 2^-1076 in f64), which changes no bit; a threshold such as -40 drops contributions below 1e-12 of a frame
 * -- far inside the f32 path's own rounding -- and shortens the pass when the posteriors are flat.  The reference has no
 * such cut (it sums everything in the log domain, Clustering.py:653-680). */
int pcl_accumulate_prune(pcl_ctx *ctx, double log2_threshold);

int pcl_stats_download(pcl_ctx *ctx, double *acc, double *alpha_acc, double *mean_acc, double *cov_acc);

/* A15: Clustering.GMM.update_param (Clustering.py:682-693) for every state, on the device, from the resident
 * (all-reduced) statistics: w = acc/alpha_acc, mu = mean_acc/acc - bias, var = max(cov_acc/acc, c_covariance);
 * then every scoring layout is rebuilt, so the next E-step can start without leaving the GPU.
 * pcl_model_download returns the float64 master copy (J*M*D, J*M*D, J*M; NULL pointers are skipped). */
int pcl_mstep(pcl_ctx *ctx, double c_covariance);
int pcl_model_download(pcl_ctx *ctx, double *mean, double *var, double *weight);

/* ----------------------------------------------------------------- segmental GMM training (training scheme 1)
 * After forced alignment every frame belongs to ONE GMM state (pcl_batch_regroup), and the reference makes each state's GMM
 * from its own frames: AcousticModel.__cal_gmm (AcousticModel.py:532-561) runs ClusterInitialization.kmeans(algorithm=1)
 * (Clustering.py:838-1044) when the model is new or its mixture count changed, then the stand-alone Clustering.GMM.em
 * (Clustering.py:583-651, 695-719) -- one state at a time, in Python loops.  Here all J states go through each step at once.
 *
 * pcl_seg_create: frame_state[t] in [0,J) = the state that owns row t of the CURRENT frame matrix (n_frames_total = its rows), or
 * -1 = the frame is not used (dropped utterances).  Builds on the device the per-state frame lists (counting sort, stable in frame
 * order) and a copy of the frames in that order; the object does not refer to the context's frame matrix afterwards.  From the two
 * arrays pcl_batch_regroup writes: frame_state = frame_unit * gmm_num + frame_k.  At most 65535 states.  Synchronous. */
int pcl_seg_create(pcl_ctx *ctx, int64_t n_frames_total, int J, const int32_t *frame_state, pcl_seg **out);
int pcl_seg_destroy(pcl_seg *seg);
/* pcl_seg_get selectors */
#define PCL_SEG_COUNTS 0 /* (J,) int32: n_j                                                                                   */
#define PCL_SEG_ORDER 1  /* (sum n_j,) int32: the frame rows of state 0, then state 1, ...: each in ascending row order       */
#define PCL_SEG_ASSIGN 2 /* (sum n_j,) int32, same order: cluster of every frame after pcl_seg_kmeans (-1: state not trained) */
#define PCL_SEG_SEEDS 3  /* (J,K) int32: position inside its state's list of every k-means++ seed (-1: none drawn)            */
int pcl_seg_get(pcl_seg *seg, int what, void *host);
/* Replaces ClusterInitialization.kmeans as __cal_gmm uses it, NOT its arithmetic: the reference's routine measures distance on the
 * first coordinate only (cal_distance returns inside its loop, Clustering.py:797-801), moves one point per centre per sweep, keeps
 * the seed point twice and draws from Python's global `random`.  This is textbook k-means++ (D^2 sampling, full squared Euclidean
 * distance) + Lloyd, deterministic for a given seed:
 *   uniforms   u(j,k), k = 0..K-1, of state j:  x = seed * 0x9E3779B97F4A7C15 + (j << 32) + k + 1 (mod 2^64);  x ^= x >> 30;
 *              x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31;  u = (x >> 11) * 2^-53
 *   seeds      first:  position min(floor(u(j,0) n_j), n_j - 1) of the state's list.  k-th: with D2[i] = the squared distance of frame i
 *              to its nearest seed so far (float64), the first i whose running sum D2[0] + .. + D2[i] exceeds u(j,k) * total (a frame
 *              that is a seed has D2 = 0 and is never drawn again; rounding put the target at or beyond the total: the last frame with
 *              D2 > 0; total = 0, every frame sits on a seed: position min(floor(u n_j), n_j - 1))
 *   sweeps     every frame to its nearest centre (lowest index on a tie; float64 arithmetic under PCL_F64, float32 under PCL_F32);
 *              a state whose frames all kept their cluster is done, otherwise centre = mean of its cluster (float64 sums in a fixed
 *              order; an empty cluster keeps its centre) and the next sweep follows, max_sweeps (>= 1) at most
 * init_centres (J,K,D) float64 instead of seeding, or NULL.  sweeps_done (J,): assignment passes run, -1 for a state with fewer than K
 * frames, which is left untouched (AcousticModel.py:549-551).  Then the context's model becomes (J,K,D) as the reference leaves it after
 * clustering: mean = cluster mean, var = max(mean squared deviation from it, 1e-4) (cal_variance, Clustering.py:807-832, squared again
 * by cov_matrix=True), weight = n_jk / n_j (an empty cluster: its centre, 1e-4, 0), every scoring layout re-derived as pcl_mstep does.
 * A context holding a model of another shape (or none) first gets mean 0 / variance 1 / weight 1/K in every state.  1 <= K <= 8192.
 * Synchronous. */
int pcl_seg_kmeans(pcl_seg *seg, int K, uint64_t seed, int max_sweeps, int precision, const double *init_centres, int32_t *sweeps_done);
int pcl_seg_centres(pcl_seg *seg, double *centres /* (J,K,D) of the last pcl_seg_kmeans */);
/* Clustering.GMM.em (Clustering.py:695-719, smem=False) for all states at once, from the context's model (J states, M mixtures):
 * loop body = expectation (:583-599) -> maximization (:624-651) -> the new parameters stored -> q_function (:607-616), repeated while
 * Q - Q_prev > q_threshold (the reference: 1.28; Q_prev starts at -inf); the parameters of the step that fails the test are KEPT
 * (:704 assigns before :706 tests).  The variance is taken about the NEW mean and floored at c_covariance; weight = Gamma_m / n_j.  Q
 * uses this iteration's responsibilities with the new parameters, in closed form (csrc/gmm_segment.hip), with the constant the model
 * was uploaded with (quirk Q1 by default).  A mixture no frame reached keeps mean and variance, gets weight 0 and adds 0 to Q (the
 * reference: NaN).  Convergence is per state: a finished state is frozen and its frames are not scored again.  The E-step is the
 * scoring + accumulate pass of pcl_batch_score / pcl_batch_accumulate in `precision`.
 * iters (J,): loop bodies run (= M-steps), -1 for a state with fewer than M frames, which is left untouched (AcousticModel.py:549-551);
 * q (J,): the last accepted Q (NaN for a skipped state); q_trace (J, max_iters) or NULL: Q after every loop body, NaN beyond.
 * The context's E-step statistics are this call's work space: every loop body starts with pcl_stats_zero, so whatever
 * pcl_batch_accumulate had summed there before is gone, and afterwards the block holds the call's last E-step.  Synchronous. */
int pcl_seg_em(pcl_seg *seg, double c_covariance, double q_threshold, int max_iters, int precision, int32_t *iters, double *q,
               double *q_trace);

/* ----------------------------------------------------------------- starting from nothing (row f7: the step before either training scheme)
 * Both training schemes of the reference begin with a step that needs no model; csrc/bootstrap.hip runs them on the resident frames.
 *
 * pcl_frames_moments: what AcousticModel.__flat_start (AcousticModel.py:479-517) does with p_data.  The sample is data[::step] PER
 * UTTERANCE, concatenated, over the first n_utts utterances (n_utts = int(file_count * proportion), :492, taken by the caller): the rows
 * frame_begin[u] + step * i, i = 0 .. ceil(T[u] / step) - 1, of the current frame matrix; an utterance of length 0 adds nothing.
 * mean_out / var_out (D,) = what ClusterInitialization(p_data, 1, D).kmeans(algorithm=1, cov_matrix=True) returns for k = 1 (:499-501):
 * the arithmetic mean; the mean squared deviation ABOUT THAT MEAN divided by n (not n - 1), floored at 1e-4 (cal_variance,
 * Clustering.py:807-832), then sqrt and squared again, as cov_matrix=True does.  *n_rows_out = rows in the sample (may be NULL).
 * Float64 throughout, two passes (mean, then deviations); the float64 frame copy is read when the context holds one (float64 upload,
 * PCL_FRONTEND_KEEP_F64), otherwise the float32 rows are widened.  No floating-point atomics; the summation order is fixed: sample
 * row g belongs to workgroup g / 1024; inside a workgroup, row lane r (of 256 / 64 = 4) adds its rows r, r + 4, ... in ascending order
 * and the four lanes are added 0, 1, 2, 3; one workgroup then adds the workgroups' partial sums in ascending index order.  Two runs
 * give the same bits.  U is the length of T / frame_begin (frame_begin NULL: utterances back to back from row 0); n_utts < 1 or > U,
 * step < 1, an utterance outside the frame matrix, no frames loaded, or an empty sample (the reference indexes an empty list there):
 * PCL_ERR_INVALID.  Synchronous. */
int pcl_frames_moments(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, int n_utts, int step, double *mean_out /* D */,
                       double *var_out /* D */, int64_t *n_rows_out);
/* The flat-start model, made where it will live (AcousticModel.py:504-516): for every state j and mixture m
 *   mean[j,m,d] = mean[d] + coeff[m] * var[d]     (the coefficient multiplies the VARIANCE -- covariance_diagonal, :514 --, one rounded
 *                                                  product and one rounded sum, as NumPy evaluates it)
 *   var[j,m,d]  = var[d],   weight[j,m] = 1 / M   (the GMM constructor's default, Clustering.py:87-88)
 * written straight into the context's float64 master copy; then everything pcl_model_upload runs after its copy (derived layouts,
 * conditioning, split lists, a zeroed statistics block): pcl_model_download and every scoring path see the model an upload of the same
 * (J, M, D) arrays would give.  coeff (M,): the caller's draw, (np.random.random((M, 1)) - np.random.random((M, 1))) * coefficient --
 * drawn ONCE and shared by every unit and state (:508-516); NULL = differentiation=False (all zero).  flags: pcl_model_upload's.
 * A variance that is not positive and finite, a non-finite mean or coefficient, or D other than the dimension of the frame matrix the
 * context holds (none loaded: any D): PCL_ERR_INVALID, the model in place stays.  Synchronous. */
int pcl_model_flat_start(pcl_ctx *ctx, int J, int M, int D, const double *mean /* D */, const double *var /* D */,
                         const double *coeff /* M or NULL */, int flags);
/* The two calls above chained, the moments never visiting the host on their way into the model (D = the frame matrix's); mean_out /
 * var_out / n_rows_out (NULLs are skipped) report them.  Same results as pcl_frames_moments + pcl_model_flat_start, bit for bit. */
int pcl_flat_start(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, int n_utts, int step, int J, int M,
                   const double *coeff /* M or NULL */, int flags, double *mean_out, double *var_out, int64_t *n_rows_out);
/* Uniform segmentation: the first round of training scheme 1, multi_process_data(init=True) (AcousticModel.py:734-735) =
 * __eq_segment(data, label, mode='e') (:605-612), followed per unit by __get_gmmdata (:629-644, mode 'g' :613-625) in multi_training
 * (:834).  Label arguments as pcl_batch_create_labels (labels = concatenated unit ids, label_len[u] of them per utterance), but neither
 * a model nor an uploaded unit inventory is needed: J = number of GMM states, a multiple of gmm_num (= S - 2); unit i owns the states
 * i * gmm_num ...  For utterance u with L labels: chunk = T / L (integer); label position i owns the frames [i chunk, (i + 1) chunk); the
 * T - L chunk frames left over are NOT used (mode 'e' drops them).  Inside a chunk: c2 = chunk / gmm_num; state k < gmm_num - 1 takes
 * [k c2, (k + 1) c2), the last state the rest.  So T < L uses nothing, and chunk < gmm_num gives everything to the last state.
 * frame_state_out (rows of the frame matrix,) int32 or NULL: unit * gmm_num + k, -1 for unused frames and for rows outside the batch --
 * pcl_seg_create's input.  out or NULL: the pcl_seg of that map, built from it ON THE DEVICE by pcl_seg_create's counting sort and
 * gather (a unit named several times collects all of it, in row order).  At least one of the two must be given.  Not in the reference's
 * signature: the utterances must not overlap in the frame matrix (a frame has ONE owner; PCL_ERR_INVALID), and an utterance may have
 * T = 0 or no label (nothing is used).  A label id outside [0, J / gmm_num), J not a multiple of gmm_num, an utterance outside the frame
 * matrix, no frames loaded: PCL_ERR_INVALID.  Integer arithmetic only.  Synchronous. */
int pcl_uniform_segments(pcl_ctx *ctx, int U, const int32_t *label_len, const int32_t *labels, const int32_t *T, const int64_t *frame_begin,
                         int gmm_num, int J, int32_t *frame_state_out, pcl_seg **out);

/* ----------------------------------------------------------------- mix-up (row f9): growing a trained model by splitting mixtures
 * The context's (J, M, D) model becomes a (J, M_new, D) model, M < M_new <= 8192, without leaving the device (csrc/model_mixup.hip): the
 * way a GMM-HMM is grown 1 -> 2 -> 4 -> ... between rounds of EM instead of being started at its full size.  Not in the reference, which
 * clusters again when its mix_level changes.  THE RULE, per state j independently, in float64, one rounding per operation, cur = M:
 * while cur < M_new
 *   live = the mixtures i < cur with weight[i] > 0 (a NaN weight is not live);  n = min(M_new - cur, |live|)
 *   the n heaviest of live -- weight descending, equal weights by ascending index -- are split: the r-th of that order, i, gets child c = cur + r
 *     delta_d     = perturb * sqrt(var[i,d])        (one rounded product)
 *     mean[c,d]   = mean[i,d] + delta_d;   mean[i,d] = mean[i,d] - delta_d        (both from the parent's mean before this round)
 *     var[c,d]    = var[i,d];              weight[i] = weight[c] = 0.5 * weight[i]
 *   cur += n
 * A mixture may be split again in a later round.  perturb >= 0 and finite (HTK's MU uses 0.2).  The plan -- which slot descends from which
 * old mixture through which rounds -- is a function of the weights alone and is made by one workgroup per state (ranks by counting, no
 * atomics: two runs give the same bits); the new float64 master copy is then filled from the old one through that plan (padding as an
 * upload leaves it: mean 0, variance 1, weight 0) and everything pcl_model_upload runs after its copy follows: derived layouts,
 * conditioning, split lists, a zeroed statistics block of the new shape.  pcl_model_download and every scoring path see the model an
 * upload of the same (J, M_new, D) arrays would give; flags are the old model's.  The unit transitions, the frames and a live pcl_seg
 * are untouched (pcl_seg_em then runs from the grown model); a live batch is in whatever state a pcl_model_upload of another shape
 * leaves it in.  origin_out (J, M_new) int32 or NULL: the index in the OLD model that mixture m descends from, m itself for m < M -- the
 * only thing that travels to the host.
 * No model: PCL_ERR_STATE.  M_new <= M, M_new > 8192, a negative or non-finite perturb, or a state without a live mixture (it cannot
 * grow; the message names the state): PCL_ERR_INVALID, checked before anything is changed -- the model in place stays.  If the new
 * model's allocation fails the context is left WITHOUT a model, as a failed upload leaves it.  pcl_kernel_time group "mixup": the plan
 * and the fill ("derive": the pass behind them).  Synchronous. */
int pcl_model_mixup(pcl_ctx *ctx, int M_new, double perturb, int32_t *origin_out /* (J, M_new) or NULL */);

/* ----------------------------------------------------------------- speaker adaptation (row f10): MLLR mean transforms, MAP means
 * Both schemes read the resident statistics of pcl_batch_accumulate -- acc[j,m] = sum_t gamma_t(j,m) and mean_acc[j,m,d] = sum_t
 * gamma_t(j,m) (o_td + bias), bias = 100 -- and change the MEANS of the context's model in place, without the model or the statistics
 * leaving the device (csrc/model_adapt.hip).  Not in the reference.  Everything is float64.  With s[j,m,d] = mean_acc[j,m,d] - bias acc[j,m]:
 *
 * MLLR (Leggetter & Woodland), diagonal covariances: every state j has a regression class state_class[j] in [0, R), or -1 = "leave this
 * state alone" (silence); state_class = NULL puts every state in class 0.  A mixture (j, m), m < M, CONTRIBUTES when acc[j,m] is finite and
 * > 0; a mixture with acc == 0 (or a NaN / infinite / negative acc) contributes exactly nothing, and the padding mixtures of the device
 * layout are never visited.  For class r and feature dimension i, with xi = (1, mu_1 .. mu_D) of a mixture, over r's contributing mixtures:
 *     G[r,i] = sum (acc / var_i) xi xi^T        (D+1) x (D+1), symmetric          k[r,i] = sum (s_i / var_i) xi
 *     row i of W[r] = w with G[r,i] w = k[r,i], by Cholesky G = L L^T and two triangular solves
 * W[r] is D x (D+1): column 0 is the offset b_r, the rest the matrix A_r.  A class is REFUSED -- it gets the identity [0 | I] and a
 * non-zero status -- when, tested in this order,
 *     PCL_MLLR_LOW_OCCUPANCY          its occupancy, the sum of acc over its contributing mixtures, is below min_occ
 *     PCL_MLLR_FEW_MIXTURES           fewer than D+1 of its mixtures contribute (G cannot have full rank)
 *     PCL_MLLR_NOT_POSITIVE_DEFINITE  a pivot of any of its D factorisations is not finite or not > 0
 * (a class without states has occupancy 0 and no mixture).  G and k are a GEMM with K = the class's mixtures: the states are grouped by
 * class on the host (J ints travel), a class's mixtures are cut into chunks of PCL_MLLR_CHUNK mixtures (env, read on every call; default
 * 65536), one workgroup per (chunk, i) forms the chunk's partial on the float64 matrix pipe (env PCL_MLLR_VALU=1: on the VALU), a second
 * kernel sums a class's partials in chunk order.  No floating-point atomics: two calls on the same statistics give the same bits.
 * pcl_mllr_estimate changes nothing of the model.  It keeps W resident with the model it was estimated for (any call that makes a new
 * model -- an upload, a flat start, a mix-up -- drops it), so that estimate followed by pcl_model_transform_means(W = NULL) moves nothing
 * to the host but the R statuses.  W_out (R, D, D+1), occ_out (R,), status_out (R,): NULLs are skipped.  D <= 48.
 *
 * pcl_model_transform_means: mean[j,m,:] <- A_r mean[j,m,:] + b_r (the offset first, then the products in ascending feature order, one
 * rounding each) for every mixture m < M of every state with class r >= 0.  A class whose W[r] is exactly [0 | I] -- every refused class --
 * is skipped: its means keep their bits, as do those of the states of class -1.  Variances, weights and padding are untouched.  W: host
 * (R, D, D+1), or NULL = the resident estimate, which must be of the same R.  Then the pass pcl_mstep runs after its kernel: derived
 * layouts, conditioning, split lists, so that every scoring path sees the model an upload of the downloaded arrays would give.
 *
 * pcl_mstep_map (Gauvain & Lee, means only): mean <- (tau mean + s) / (tau + acc) for every mixture with a finite acc > 0, the others keep
 * their mean; tau = 0 is pcl_mstep's ML mean.  Variances and weights are untouched.  The same derive pass follows.  There is no solve
 * behind it and no limit on D beyond the model's own (D <= 64).
 *
 * The statistics block is treated as pcl_mstep treats it: read, neither cleared nor marked -- it describes the model BEFORE the call until
 * the caller's next pcl_stats_zero.  With more than one rank the caller runs pcl_stats_allreduce first: all three calls read the block as
 * it is on this rank, and the ranks then make the same model.
 * No model (and so no statistics): PCL_ERR_STATE.  R < 1, a class outside [-1, R), a negative or non-finite min_occ / tau, D > 48, W = NULL
 * without a resident estimate of R classes for this model: PCL_ERR_INVALID.  All checked before anything is changed.  Synchronous.
 * pcl_kernel_time group "adapt": the kernels of each call ("adapt_gk": the GEMM and its reduction, "adapt_solve": the factorisations;
 * "derive": the pass behind the two calls that change the model). */
#define PCL_MLLR_OK 0
#define PCL_MLLR_LOW_OCCUPANCY 1
#define PCL_MLLR_FEW_MIXTURES 2
#define PCL_MLLR_NOT_POSITIVE_DEFINITE 3
int pcl_mllr_estimate(pcl_ctx *ctx, int R, const int32_t *state_class /* J, or NULL = all 0 */, double min_occ,
                      double *W_out /* R*D*(D+1) or NULL */, double *occ_out /* R or NULL */, int32_t *status_out /* R or NULL */);
int pcl_model_transform_means(pcl_ctx *ctx, int R, const int32_t *state_class /* J, or NULL = all 0 */,
                              const double *W /* host R*D*(D+1), or NULL = the resident last estimate */);
int pcl_mstep_map(pcl_ctx *ctx, double tau);

/* ----------------------------------------------------------------- discriminative training (row f18): MMI by extended Baum-Welch
 * The last training stage: means, variances and weights from TWO statistics sets of pcl_batch_accumulate, both accumulated under the
 * current model -- the numerator (the label batches) and the denominator (a competing graph: any general batch) -- without the model or
 * either set leaving the device (csrc/model_ebw.hip).  Not in the reference.  Everything is float64.  The objective is the caller's:
 * sum logp of the numerator batches - sum logp of the denominator batches.
 *
 * pcl_ebw_hold copies the live statistics block into a second resident block of the same layout, the NUMERATOR set; the live block keeps
 * its bits and is then the caller's to clear and fill with the denominator.  The held set belongs to the model it was accumulated under
 * (cov_acc is centred on that model's means): any call that makes a new model (an upload, a flat start, a mix-up, the segmental trainers)
 * or changes the resident one (pcl_mstep, pcl_em_exchange, pcl_batch_accumulate_exchange, pcl_mstep_map, pcl_model_transform_means,
 * pcl_mstep_ebw itself) drops it, as the resident MLLR estimate is dropped with its model.  pcl_ebw_drop drops it by hand (no held set:
 * nothing happens).  pcl_ebw_stats_download is pcl_stats_download of the held set; NULLs are skipped.  With more than one rank the caller
 * runs pcl_stats_allreduce before pcl_ebw_hold and again before pcl_mstep_ebw, the rule pcl_mstep_map documents.
 *
 * pcl_mstep_ebw: numerator = the held set (suffix n), denominator = the live block (suffix d).  In coordinates centred on the current mean
 * mu, so that the bias of mean_acc never cancels against a large term: per mixture (j, m), m < M, feature dimension d, and set,
 *     g = acc      x = mean_acc - (bias + mu) acc      c = cov_acc                                     (bias = 100)
 * I-smoothing, numerator only, when gn is finite and > 0:   xn += tau xn / gn,  cn += tau cn / gn,  gn += tau.   Then
 *     g = gn - gd,  x = xn - xd,  c = cn - cd
 *     Dmin = max over d of the larger real root of  v D^2 + (c + g v) D + (c g - x^2) = 0  (0 where the roots are complex or not positive)
 *     D = max(E gd, 2 Dmin)
 *     delta = x / (g + D)      mu' = mu + delta      v' = max((c + D v) / (g + D) - delta^2, c_covariance)
 * A mixture KEEPS mu and v bit for bit when its gn, gd, any x or any c is not finite, when gn (unsmoothed) and gd are both 0, or when
 * g + D is not finite or not > 0.
 * Weights (Povey's iteration), per state, on the UNSMOOTHED gn: k_m = gd_m / w_m over the mixtures with w_m > 0, kmax = max k_m, c^0 = w,
 * weight_iters times  c_m <- (gn_m + (kmax - k_m) c_m) / sum_m' (gn_m' + (kmax - k_m') c_m');  a mixture with w_m = 0 stays 0.  A state
 * whose gn and gd are all 0, or one of whose sums is not finite or not > 0, keeps its weights.  The ORDER of that sum is part of the rule
 * (in any other order the weights of a state of a thousand mixtures drift past rounding over 100 iterations): mixture m belongs to thread
 * m mod 256 of the state's workgroup; a thread adds its mixtures in ascending order starting from 0; the 64 lanes of a wave are summed by a
 * butterfly with partner lane ^ 32, 16, 8, 4, 2, 1; the four waves' sums are added in ascending order.
 * Then the derive pass pcl_mstep runs: every scoring path sees the model an upload of the downloaded arrays would give.
 * D_out (J, M) = the constant used, 0 for a kept mixture.  counts_out (4,) = mixtures updated, mixtures kept, variance elements floored,
 * states whose weights were kept.  Padding mixtures and padding dimensions of the device layout are never read into a result and never
 * change.  No floating-point atomics and every sum in a fixed order: two calls on the same inputs give the same bits.
 * Transitions stay maximum-likelihood (pcl_mstep_transitions); there is no acoustic scale on the denominator (kappa = 1).
 * No model, or no held set for this model: PCL_ERR_STATE.  E, tau or c_covariance negative or not finite, E == 0, weight_iters < 0:
 * PCL_ERR_INVALID.  All checked before anything is changed.  Synchronous.  pcl_kernel_time group "ebw": the update's kernel ("derive":
 * the pass behind it). */
int pcl_ebw_hold(pcl_ctx *ctx);
int pcl_ebw_drop(pcl_ctx *ctx);
int pcl_ebw_stats_download(pcl_ctx *ctx, double *acc, double *alpha_acc, double *mean_acc, double *cov_acc);
int pcl_mstep_ebw(pcl_ctx *ctx, double E, double tau, double c_covariance, int weight_iters, double *D_out /* J*M or NULL */,
                  int64_t *counts_out /* 4 or NULL */);

/* ----------------------------------------------------------------- minimum Bayes risk (row f19): sMBR / MPFE and an acoustic scale
 * One forward-backward of a batch under an acoustic scale kappa that carries the expected frame accuracy against a reference alignment
 * beside alpha and beta (csrc/hmm_mbr.hip).  Not in the reference.  Float64 throughout.  For discriminative use it REPLACES
 * pcl_batch_forward_backward (whose pass loop and pi re-estimation a discriminative pass must not run, and which has no scale): it runs ONE
 * pass with the batch's ln pi as set; and it REPLACES scaling the emissions by hand, which is wrong because the accumulate pass reads Bt as
 * ln b_j to form the mixture responsibilities.  What follows it stays: pcl_batch_mbr_posteriors puts a ln gamma into the batch where
 * pcl_batch_accumulate (and _fmllr, _mllt) read it, pcl_ebw_hold / pcl_mstep_ebw turn a positive and a negative set into a model.  With
 * this path the denominator of MMI has an acoustic scale: the "kappa = 1" of pcl_mstep_ebw's text describes pcl_batch_forward_backward only.
 *
 * The rule, per utterance of N rows and T >= 1 frames; ln a, ln pi, B as the batch holds them; bs_j(t) = kappa B[j,t]:
 *     alpha_0(j) = ln pi_j + bs_j(0)          alpha_t(j) = LSE_i[alpha_{t-1}(i) + ln a_ij] + bs_j(t)
 *     beta_{T-1} = 0                          beta_t(i)  = LSE_j[ln a_ij + (bs_j(t+1) + beta_{t+1}(j))]
 *     ln P = LSE_j alpha_{T-1}(j)             ln gamma_t(j) = alpha_t(j) + beta_t(j) - LSE_i(alpha_t(i) + beta_t(i))
 * (oracle.forward / oracle.backward's conventions: every row may end, quirk Q8; LSE returns a maximum of +-inf as itself, quirk Q4;
 * ln gamma is normalised per frame as PCL_GET_LGAMMA is).
 * Accuracy: A_t(j) = 1 when row_state[j] >= 0, frame_ref[t] >= 0 and row_state[j] / group == frame_ref[t] / group (integer division), else
 * 0.  group = 1 compares states (sMBR); group = S - 2 compares units (phone-frame accuracy, MPFE).  Entry and exit rows and frames with
 * frame_ref = -1 score 0.
 * Expected accuracy.  Each LSE above is evaluated as  m = max_k v_k;  e_k = exp(v_k - m);  s = sum_k e_k;  result m + ln s  (m = +-inf:
 * m itself).  The SAME e_k weigh the accuracies:  sp = sum_k e_k y_k,  mean = sp / s  (0 when m = +-inf), with
 *     alpha'_0(j) = A_0(j)        alpha'_t(j) = mean over predecessors i of y = alpha'_{t-1}(i), + A_t(j);   0 where alpha_t(j) = -inf
 *     beta'_{T-1}(i) = 0          beta'_t(i)  = mean over successors j of y = beta'_{t+1}(j) + A_{t+1}(j);    0 where beta_t(i) = -inf
 *     c_avg = sum_j gamma_0(j) (alpha'_0(j) + beta'_0(j))                 (gamma = exp(ln gamma); terms with gamma = 0 are left out)
 *     g_t(j) = kappa gamma_t(j) ((alpha'_t(j) + beta'_t(j)) - c_avg)      signed; 0 where gamma_t(j) = 0
 * sum_j gamma_t(j) (alpha'_t(j) + beta'_t(j)) is the same number at every t -- the expected accuracy of the utterance; the pass takes it at
 * frame 0, where it is known before the forward recursion starts.  g is d c_avg / d B[j,t], and sum_j g_t(j) = 0.  T = 1 is legal:
 * c_avg = sum_j gamma_0(j) A_0(j).
 * Order of the sums, part of the rule (tests/_mbr_twin.py repeats it): over predecessors in ascending source row (the CSC arrays), over
 * successors in ascending target row (the CSR arrays), both from 0; across the rows of a frame (the normaliser, c_avg, ln P) row i belongs
 * to lane i mod 64 of wave i / 64, the 64 lanes of a wave are summed by a butterfly with partner lane ^ 32, 16, 8, 4, 2, 1 (lanes past N
 * hold 0, or -inf under a maximum), the waves' sums are added in ascending order.  No contraction, no floating-point atomics: two calls on
 * the same inputs give the same bits.
 *
 * pcl_batch_mbr needs transitions, a row -> state map and emissions (pcl_batch_score or pcl_batch_set_emissions), not
 * pcl_batch_forward_backward.  At most 1024 rows per utterance, any transition structure.  It keeps its results in buffers of its own and
 * changes no bit of what pcl_batch_get returns (B, ALPHA .. QTRACE, PATH).  pcl_batch_mbr_get: ln P (U,), c_avg (U,), ln gamma and g
 * ragged (N_u, T_u) row-major like PCL_GET_LGAMMA; NULLs are skipped.  pcl_batch_mbr_posteriors writes the batch's posteriors, in the
 * layout pcl_batch_set_posteriors leaves: which = 0: ln gamma under kappa (the scaled MMI denominator; on a label batch the numerator);
 * which = +1: ln max(g, 0); which = -1: ln max(-g, 0) -- the positive and the negative set of an sMBR / MPFE iteration, whose
 * difference is g.  It marks the posteriors as set (as pcl_batch_set_posteriors does) and leaves the forward-backward results alone;
 * PCL_GET_LGAMMA then reads what it wrote.
 * PCL_ERR_STATE: pcl_batch_mbr without transitions, states or emissions; _get / _posteriors before pcl_batch_mbr, or after a call that
 * invalidates the pass (pcl_batch_set_transitions, pcl_batch_refresh_transitions, pcl_batch_set_states, pcl_batch_set_emissions,
 * pcl_batch_score).  PCL_ERR_INVALID: kappa not finite or <= 0, group < 1, a frame_ref outside [-1, J), more than 1024 rows, which outside
 * {-1, 0, 1}.  All checked before anything is changed.  pcl_batch_mbr is queued on the main stream; _get is synchronous.
 * pcl_kernel_time group "mbr": the pass ("mbr_post": the posteriors kernel). */
int pcl_batch_mbr(pcl_batch *b, const int32_t *frame_ref /* ragged (T_u,), host: state id in [0,J) or -1 */, double kappa, int group);
int pcl_batch_mbr_get(pcl_batch *b, double *logp /* U */, double *c_avg /* U */, double *lgamma /* ragged (N_u,T_u) */,
                      double *g /* ragged (N_u,T_u), signed */);
int pcl_batch_mbr_posteriors(pcl_batch *b, int which);

/* ----------------------------------------------------------------- fMLLR (row f11): per-speaker transforms of the FEATURES, y = b + A x
 * Constrained MLLR (Gales 1998, section 3.2 and appendix B) on the resident frames (csrc/frame_adapt.hip).  The model stays untouched; every
 * speaker of a batch gets a transform of its own; the transformed frames stay where scoring, forward-backward, decode and the segmental
 * trainers read them.  Not in the reference.  Everything is float64.  zeta_t = (1, x_t) (length D+1), W = [b | A] (D x (D+1), column 0 the
 * offset, as pcl_mllr_estimate lays W out), s = the speaker of the utterance, gamma_t(j,m) = the mixture posterior of frame t,
 *     gamma_t(j,m) = exp(ln gamma_t(row) + ln w_jm + ln N(x_t; mu_jm, var_jm) - ln b_j(x_t))        summed over the utterance's rows of state j
 * from the batch's resident ln gamma (pcl_batch_forward_backward / pcl_batch_set_posteriors) and ln b (pcl_batch_score), in the direct
 * float64 form of pcl_batch_accumulate(PCL_F64), on the float64 frame copy when the context holds one, else on the float32 rows widened.
 * A mixture with weight 0 or a weight that is not finite, and the padding mixtures, contribute exactly nothing; so does a (frame, row)
 * whose ln gamma or ln b is -inf.
 *
 * STATISTICS.  Per frame:   p_i(t) = sum_{j,m} gamma_t(j,m) / var_jm,i      q_i(t) = sum_{j,m} gamma_t(j,m) mu_jm,i / var_jm,i      beta(t) = sum_{j,m} gamma_t(j,m)
 * (1 / var and mu / var are recovered from the float64 scoring row s = sqrt(log2 e / (2 var)), c = -mu s as 2 ln2 s^2 and -2 ln2 c s: the
 * sums of gamma s^2 and gamma c s are formed and scaled once).  Order: one workgroup of four waves per (utterance, tile of 64 frames), lane
 * l owns frame l of the tile; wave w adds, over the utterance's rows in ascending order, the row's mixtures w, w + 4, w + 8, ... in ascending
 * order; the four waves' sums are then added through LDS as ((w0 + w1) + w2) + w3.
 * Per speaker:  G[s,i] = sum_t p_i(t) zeta_t zeta_t^T   ((D+1) x (D+1), symmetric)      k[s,i] = sum_t q_i(t) zeta_t      beta[s] = sum_t beta(t)
 * over the frames of the speaker's utterances: the split-K float64 GEMM pcl_mllr_estimate uses (csrc/adapt_common.h; K = the speaker's
 * frames in batch order, cut into chunks of PCL_MLLR_CHUNK frames; column D+1 of the second operand carries q_i(t), so k comes out of the
 * same chain; upper-triangular tiles only; on v_mfma_f64_16x16x4_f64, or on the VALU under PCL_MLLR_VALU=1); a call's chunks are added to
 * the resident sums in chunk order, then the lower triangle mirrors the upper.  beta[s]: thread t of 256 adds the speaker's frames t,
 * t + 256, ... in ascending order, then a fixed binary tree.  No floating-point atomics: two runs give the same bits.
 * pcl_fmllr_zero makes (or clears) the context's statistics for S speakers -- 8 D (D+1)(D+2) bytes per speaker, at most 2^32 bytes in all and
 * S <= 65535 -- and drops the resident estimate.  The statistics are additive over calls of pcl_batch_accumulate_fmllr (several batches of one
 * speaker) and are dropped by any call that makes a new model (an upload, a flat start, a mix-up, k-means) or a frame matrix of another D.
 * pcl_batch_accumulate_fmllr: utt_speaker (U,) int32 in [0, S), or -1 = the utterance is skipped.  Needs what pcl_batch_accumulate needs
 * (emissions, posteriors, the row map, frames of the model's dimension).  Synchronous.
 * pcl_fmllr_stats_download: G (S, D, D+1, D+1), k (S, D, D+1), beta (S,); NULLs are skipped.
 *
 * ESTIMATE, per speaker, from W = [0 | I], A^-1 = I; n_iter sweeps; a sweep visits the rows i = 0 .. D-1 in order:
 *   1. p = (0, column i of A^-1): the cofactor row up to scale (the update does not depend on the scale of p, so no determinant is formed)
 *   2. v = G_i^-1 p^T through the Cholesky factor G_i = L L^T (L y = p, L^T v = y), g = G_i^-1 k_i^T likewise (once per (s, i), as is the
 *      factor);  a = sum_q p_q v_q,  c = sum_q p_q g_q  (ascending q)
 *   3. disc = c c + 4 a beta;  alpha+- = (-c +- sqrt(disc)) / (2 a);  f(alpha) = beta ln|alpha a + c| - 0.5 a alpha alpha;  alpha = alpha+
 *      when f(alpha+) >= f(alpha-), else alpha-
 *   4. w_i = alpha v + g
 *   5. A^-1 by a rank-one update: u = column i of A^-1 (before), denom = sum_q w_i[1+q] u_q, z = ((w_i - w_i_old)[1..] A^-1) / denom,
 *      A^-1 <- A^-1 - u z.  Every sweep ENDS with a full re-inversion of A (in-place Gauss-Jordan with row pivoting: the first row of
 *      largest |element| in column k at or below the diagonal is swapped up; ln|det A| = sum ln|pivot|; the swaps are undone on the columns
 *      of the inverse in reverse order), which also gives the ln|det A| of
 *         Q = beta ln|det A| - 1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T)          q_trace[s, sweep]
 * A speaker is REFUSED -- it gets [0 | I], ln|det A| = 0, NaN in q_trace and a non-zero status -- when, tested in this order,
 *     PCL_FMLLR_LOW_OCCUPANCY          beta[s] < min_occ
 *     PCL_FMLLR_NOT_POSITIVE_DEFINITE  a Cholesky pivot of any G[s,i] is not finite or not > 0
 *     PCL_FMLLR_SINGULAR               a is not finite or not > 0, disc is negative or not finite, alpha is not finite, denom or a
 *                                      Gauss-Jordan pivot is 0 or not finite
 * Statuses are decided before anything is written.  One wave per (s, i) factors; one wave per speaker sweeps, W and A^-1 in LDS, the factor
 * of the row at hand staged into LDS, G read through L2 for Q.  W stays resident (until the next pcl_fmllr_zero or new model) for
 * pcl_frames_transform(W = NULL).  W_out (S, D, D+1), logdet_out (S,), q_trace_out (S, n_iter), status_out (S,) int32: NULLs are skipped.
 * 1 <= n_iter <= 1000; min_occ finite and >= 0; D <= 48.  Synchronous.
 *
 * APPLY.  pcl_frames_transform: y = b + A x in place on the CURRENT frame matrix for the rows [frame_begin[u], + T[u]) of every utterance
 * with utt_speaker[u] >= 0: the offset first, then the products in ascending feature order, one rounding per operation.  x is read from
 * the float64 copy when the context holds one (which then receives y), else from the float32 rows widened; the float32 rows receive y
 * rounded to nearest; the padding columns stay as pcl_frames_upload left them.  A speaker whose W is exactly [0 | I] -- every refused
 * speaker -- and the utterances of speaker -1 keep their bits; rows outside every utterance are untouched.  W: host (S, D, D+1), or NULL =
 * the resident estimate, which must be of the same S.  The utterances must not overlap in the frame matrix (PCL_ERR_INVALID, as
 * pcl_batch_align_segments checks): a frame is transformed once.  A live pcl_seg has its own copy of the frames and is untouched; live
 * batches keep the emissions they scored from the old rows until they are scored again -- the state pcl_frames_swap leaves them in.
 *
 * No model / no statistics (never made, or dropped): PCL_ERR_STATE.  A speaker outside [-1, S), S out of range, W = NULL without a resident
 * estimate of S speakers, frames of another dimension than the model: PCL_ERR_INVALID.  All checked before anything is changed.
 * pcl_kernel_time groups: "fmllr" (every kernel of each call), "fmllr_frames" (the per-frame reduction), "fmllr_gk" (the GEMM and its
 * reduction), "fmllr_solve" (factorisations and sweeps). */
#define PCL_FMLLR_OK 0
#define PCL_FMLLR_LOW_OCCUPANCY 1
#define PCL_FMLLR_NOT_POSITIVE_DEFINITE 2
#define PCL_FMLLR_SINGULAR 3
int pcl_fmllr_zero(pcl_ctx *ctx, int S);
int pcl_batch_accumulate_fmllr(pcl_batch *b, const int32_t *utt_speaker /* U, -1 = skip */);
int pcl_fmllr_stats_download(pcl_ctx *ctx, double *G /* S*D*(D+1)*(D+1) or NULL */, double *k /* S*D*(D+1) or NULL */, double *beta /* S or NULL */);
int pcl_fmllr_estimate(pcl_ctx *ctx, int n_iter, double min_occ, double *W_out /* S*D*(D+1) or NULL */, double *logdet_out /* S or NULL */,
                       double *q_trace_out /* S*n_iter or NULL */, int32_t *status_out /* S or NULL */);
int pcl_frames_transform(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *utt_speaker, int S,
                         const double *W /* host S*D*(D+1), or NULL = the resident last estimate */);

/* ----------------------------------------------------------------- MLLT (row f13): one square transform of the features for the whole corpus
 * The maximum-likelihood linear transform of semi-tied covariances (Gales 1999; Kaldi's est-mllt) on the resident frames and statistics
 * (csrc/frame_mllt.hip): the step between LDA (f12) and fMLLR (f11).  An LDA projection does not decorrelate the classes it separates and
 * every Gaussian here is diagonal; ONE matrix A, estimated under the current alignment and applied to the frames AND the means, makes the
 * diagonal model fit better.  Not in the reference; tests/_mllt_twin.py is the rule's NumPy twin.  Everything is float64, built with
 * -ffp-contract=off; no floating-point atomics: two runs give the same bits.
 *
 * THE RULE.  With gamma_t(j,m) the mixture posterior as fMLLR defines it above, over the KEPT states (state_keep[j] != 0; NULL = all), for
 * feature dimension i:
 *     G_i = sum_t sum_jm gamma_t(j,m) / var_jm,i (x_t - mu_jm)(x_t - mu_jm)^T        (D x D, symmetric)          beta = sum_t sum_jm gamma_t(j,m)
 *     Q(A) = beta ln|det A| - 1/2 sum_i a_i G_i a_i^T                                (a_i = row i of A)
 * The centred product per (frame, mixture) pair costs D^2 per pair.  It is expanded instead: with n_jm = acc[j,m] and s_jm = mean_acc[j,m,:]
 * - bias acc[j,m] of the resident statistics block (bias = 100, the accumulate pass's),
 *     G_i = F_i - C_i
 *     F_i = sum_t p_i(t) x_t x_t^T,   p_i(t) = sum_jm gamma_t(j,m) / var_jm,i                             the frame side, per batch
 *     C_i = sum_jm (s_jm mu_jm^T + mu_jm s_jm^T - n_jm mu_jm mu_jm^T) / var_jm,i                          the mixture side, at estimate time
 * which is exact when both sides saw the same posteriors: the caller runs pcl_batch_accumulate AND pcl_batch_accumulate_mllt on the same
 * batches (and the same utterances of them), with pcl_stats_zero and pcl_mllt_zero in front.  pcl_batch_accumulate(PCL_F32) carries its
 * 1e-4 error into C_i; PCL_F64 does not.  The estimate returns both occupancies -- beta from the frames, the sum of acc over the kept
 * contributing mixtures -- so that a caller can tell when the two sides do not belong together.
 * Which mixtures contribute to C_i follows pcl_mllr_estimate: m < M with acc finite and > 0, padding is never visited.  Which (frame, row)
 * pairs contribute to F_i follows fMLLR: ln gamma or ln b = -inf, a weight of 0 or a weight that is not finite contribute exactly nothing.
 * A state with state_keep[j] == 0 -- silence, say -- is left out of both sides.
 *
 * STATISTICS.  pcl_mllt_zero makes (or clears) F (D, D, D) and beta for the current model and stores state_keep (J,) with them.  They
 * are additive over calls of pcl_batch_accumulate_mllt and are dropped by any call that makes a new model (an upload, a flat start, a
 * mix-up, k-means) or a frame matrix of another D, as fMLLR's are.
 * pcl_batch_accumulate_mllt: utt_keep (U,) int32, 0 = the utterance is skipped, NULL = all.  Needs what pcl_batch_accumulate needs.  p_i(t)
 * and beta(t): fMLLR's reduction without q, in its order, all D + 1 sums of a frame in one workgroup.  F_i += the split-K float64 GEMM of
 * csrc/adapt_common.h with K = the call's kept frames in batch order -- ONE group -- cut into chunks of PCL_MLLT_CHUNK frames (env, read on
 * every call; default 4096 for this side); operands a = x_t[p], b = p_i(t) x_t[p]; upper-triangular 16 x 16 tiles on
 * v_mfma_f64_16x16x4_f64 (wave w of four takes the 4-frame k-steps w, w + 4, ..; the waves' sums are added ((w0 + w1) + w2) + w3), or on the
 * VALU under PCL_MLLR_VALU=1; the chunks' partials are added from 0 in chunk order, that sum is added to the resident element, and the
 * lower triangle takes the upper one's values.  beta += the frames' beta(t): thread t of 256 adds the frames t, t + 256, .. in ascending
 * order, then a fixed binary tree.
 * pcl_mllt_stats_download: F (D, D, D), beta (1,); NULLs are skipped.
 *
 * ESTIMATE.  C_i is the same GEMM with K = the kept states' mixtures -- states ascending, the M real mixtures of each ascending -- in the
 * TWO-PRODUCT form: every mixture is two consecutive K-elements,
 *     a = s[p], b = mu[p] / var_i              then              a = mu[p], b = (s[p] - n mu[p]) / var_i
 * whose sum over K is C_i; a 4-element k-step holds two mixtures; chunks of PCL_MLLT_CHUNK K-elements (default 65536 for this side),
 * waves and chunks added as above.  Then G_i = F_i - C_i, once per element of the full matrix, the lower triangle from the upper one's
 * partials.  The occupancy of the mixtures: up to 1024 blocks each add a contiguous range (thread t its mixtures t, t + 256, .., a fixed
 * tree), the blocks' sums are added likewise.
 * From A = I, A^-1 = I, n_iter sweeps over the rows i = 0 .. D-1 -- fMLLR's sweep above with k = 0 and no offset column, the same kernel:
 *   1. c = column i of A^-1: the cofactor row up to scale
 *   2. v = G_i^-1 c through the Cholesky factor G_i = L L^T (factored once per i: one wave each);  a = sum_q c_q v_q  (ascending q)
 *   3. alpha = sqrt(4 a beta) / (2 a)  (= sqrt(beta / (c . v)): with k = 0 fMLLR's two roots are +- this and the + root is taken)
 *   4. a_i = alpha v
 *   5. A^-1 by fMLLR's rank-one update; every sweep ENDS with the full re-inversion of A with row pivoting, which gives ln|det A|
 * q_trace has n_iter + 1 entries: entry 0 is Q(I) = -1/2 sum_i G_i[i,i], entry s is Q after sweep s.
 * The estimate is REFUSED -- A = I, ln|det A| = 0, NaN in q_trace and a non-zero status -- when, tested in this order,
 *     PCL_MLLT_LOW_OCCUPANCY          beta < min_occ
 *     PCL_MLLT_NOT_POSITIVE_DEFINITE  a Cholesky pivot of any G_i is not finite or not > 0
 *     PCL_MLLT_SINGULAR               PCL_FMLLR_SINGULAR's conditions
 * The status is decided before anything is written.  G_out (D, D, D) and occ_out (2,) = (beta, sum of acc) are given either way.
 * A_out (D, D), logdet_out (1,), q_trace_out (n_iter + 1,), status_out (1,) int32: NULLs are skipped.  1 <= n_iter <= 1000; min_occ finite
 * and >= 0; D <= 48.  Neither the model nor the statistics are changed.
 *
 * APPLY.  No call of its own: pcl_frames_transform with one speaker and pcl_model_transform_means with one class take W = [0 | A], and
 * ln P(O) of the transformed frames is comparable after adding (frames) x ln|det A|.  The VARIANCES ARE NOT TRANSFORMED: diag(A Sigma A^T)
 * would need a full covariance per mixture.  The next M-step on the transformed frames re-estimates them (as Kaldi's recipes do after
 * est-mllt); until then the model's variances are those of the old space.
 *
 * No model / no statistics (never made, or dropped): PCL_ERR_STATE.  D > 48, n_iter or min_occ out of range: PCL_ERR_INVALID.  All checked
 * before anything is changed.  Synchronous.  pcl_kernel_time groups: "mllt" (every kernel of each call), "mllt_frames" (the per-frame
 * reduction), "mllt_gk" (both GEMMs and their reductions), "mllt_solve" (factorisations and sweeps). */
#define PCL_MLLT_OK 0
#define PCL_MLLT_LOW_OCCUPANCY 1
#define PCL_MLLT_NOT_POSITIVE_DEFINITE 2
#define PCL_MLLT_SINGULAR 3
int pcl_mllt_zero(pcl_ctx *ctx, const int32_t *state_keep /* J or NULL */);
int pcl_batch_accumulate_mllt(pcl_batch *b, const int32_t *utt_keep /* U or NULL; 0 = skip */);
int pcl_mllt_stats_download(pcl_ctx *ctx, double *F /* D*D*D or NULL */, double *beta /* 1 or NULL */);
int pcl_mllt_estimate(pcl_ctx *ctx, int n_iter, double min_occ, double *A_out /* D*D */, double *logdet_out, double *q_trace_out /* n_iter+1 */,
                      double *G_out /* D*D*D or NULL */, double *occ_out /* 2: beta, sum acc */, int32_t *status_out);

/* ----------------------------------------------------------------- LDA (row f12): class statistics of spliced frames, projection to a new width
 * Linear discriminant analysis of the resident frames (csrc/frame_lda.hip): the step between the front-end's static cepstra and fMLLR in a
 * GMM-HMM recipe -- splice +-4 frames, project 117 dimensions to 39 or 40.  Not in the reference; tests/_lda_twin.py is the rule's NumPy twin.
 *
 * SPLICE.  Utterance u occupies the rows [begin_u, begin_u + T_u) of the resident (F, D) matrix.  With context (left, right) the spliced
 * vector of row g is the concatenation, for k = -left .. right, of row clamp(g + k, begin_u, begin_u + T_u - 1): edge replication, the
 * rule the front-end's deltas use; nothing is read across an utterance boundary.  Ds = (left + right + 1) D; the calls refuse Ds + 1 > 128.
 *
 * STATISTICS.  frame_class[g] in [0, R), or -1 = the row is skipped; rows outside every utterance of the call are skipped.  Per class
 *     n_r = the rows     s_r = sum x     S_r = sum x x^T                    (x the spliced vector, float64)
 * formed as ONE product of the augmented vector [x | 1] with itself, of order Ds + 1, read from the float64 frame copy when the context
 * holds one, else from the float32 rows widened.  Order: the kept rows are counting-sorted by class (stable: a class's rows ascend); a
 * class's rows are cut into chunks of PCL_LDA_CHUNK rows (env, read on every call; default 1024) that never straddle a class; a chunk's
 * upper-triangular 16 x 16 tiles are formed on v_mfma_f64_16x16x4_f64 -- 32 rows are staged per step, wave w of four takes the 4-row
 * k-steps w and w + 4 of every step, the waves' sums are added ((w0 + w1) + w2) + w3 -- or, under PCL_LDA_VALU=1, on the VALU with the
 * chunk's rows in ascending order; the chunks' partials are then added onto the running statistics in chunk order.  No floating-point
 * atomics: two runs give the same bits.  n_r is exact (a sum of ones).
 * pcl_lda_zero makes (and clears) the context's statistics for R classes and the context (left, right) at the dimension of the CURRENT
 * frame matrix: 8 R (Ds + 1)^2 bytes from the context's pool, at most 2^32, R <= 65535; freed by pcl_destroy and by the next pcl_lda_zero.
 * The statistics are additive over calls of pcl_lda_accumulate / pcl_batch_accumulate_lda.
 * pcl_lda_accumulate: T / frame_begin (U,) as pcl_frames_transform takes them (disjoint: a row is spliced inside ONE utterance),
 * frame_class (F,) int32 on the host, one entry per row of the frame matrix.
 * pcl_batch_accumulate_lda: the classes come from the batch's Viterbi paths -- everything pcl_batch_align_segments needs and checks (a
 * label-built batch, pcl_batch_viterbi run, its drop rule); the owner map stays on the device.  state_class (J,) int32 in [-1, R) maps the
 * owner state to its class (-1: skipped), as pcl_mllr_estimate takes it; NULL = every state its own class (needs J <= R).
 * pcl_lda_stats_download: n (R,), s (R, Ds), S (R, Ds, Ds) float64, S as full symmetric matrices mirrored from the upper triangle; NULLs
 * are skipped.
 *
 * ESTIMATE: on the host, in float64 (poccala_amd.Engine.lda_estimate; at most 127 x 127, once per training stage).  N = sum n_r, m = sum s_r / N,
 * m_r = s_r / n_r over the classes with n_r > 0:
 *   1. W = sum_r (S_r - s_r s_r^T / n_r) / N          2. B = sum_r n_r (m_r - m)(m_r - m)^T / N
 *   3. W += eps trace(W) / Ds on the diagonal         4. W = L L^T          5. eigh(L^-1 B L^-T)
 *   6. V = the D_out leading eigenvectors, eigenvalues descending          7. A = V^T L^-1, b = -A m  (the projected data: zero mean, unit
 *   within-class covariance)                          8. every row's sign is fixed so that its largest-magnitude entry is positive
 *
 * PROJECT.  pcl_frames_splice_project: y = b + A x over the spliced vector x of every row of the listed utterances, float64, b first, then
 * the products in ascending index order, one rounding per operation; the float32 row is float32(y).  One pass, the splice at load, into
 * NEW buffers which then replace the resident ones: the frame matrix becomes (F, D_out) with the row stride and bookkeeping
 * pcl_frames_upload would leave for that width (padding columns zero), the float64 copy kept when one was held.  Rows that belong to no
 * listed utterance become zero.  A (D_out, Ds) row-major, b (D_out,), finite; 1 <= D_out <= min(Ds, 64).  A resident model stays: a model
 * of another dimension is the caller's business, as after pcl_frames_upload (fMLLR statistics of another dimension are dropped, as there).
 * Live batches: pcl_frames_upload lets a batch outlive it and re-checks the batch's ROWS against the new matrix at its next use.  That
 * check cannot see this call -- the rows stay, the width changes -- so it refuses (PCL_ERR_STATE) while any batch or pcl_seg made on the
 * old matrix is alive: destroy them first.
 * pcl_frames_download: the resident frames as held, unpadded (F, D): f64 from the float64 copy (PCL_ERR_STATE when the context holds
 * none), f32 from the float32 rows; NULLs are skipped.
 *
 * No frames / no statistics: PCL_ERR_STATE; so is an accumulate after the frame matrix changed its dimension since pcl_lda_zero (the
 * context (left, right) no longer gives the statistics' order).  Ds + 1 > 128, D_out outside 1 .. Ds, a class outside [-1, R), R out of
 * range, an utterance outside the frame matrix or overlapping another: PCL_ERR_INVALID.  All checked before anything is changed.
 * pcl_kernel_time groups: "lda_sort" (keys and counting sort), "lda_stats" (the product and its reduction), "lda_project".  Synchronous. */
int pcl_lda_zero(pcl_ctx *ctx, int R, int left, int right);
int pcl_lda_accumulate(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *frame_class /* host, F */);
int pcl_batch_accumulate_lda(pcl_batch *b, const int32_t *state_class /* J, or NULL = identity */);
int pcl_lda_stats_download(pcl_ctx *ctx, double *n /* R or NULL */, double *s /* R*Ds or NULL */, double *S /* R*Ds*Ds or NULL */);
int pcl_frames_splice_project(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, int left, int right, int D_out,
                              const double *A /* D_out*Ds */, const double *b /* D_out */);
int pcl_frames_download(pcl_ctx *ctx, double *f64 /* F*D or NULL */, float *f32 /* F*D or NULL */);

/* ----------------------------------------------------------------- CMVN (row f14): cepstral mean and variance normalisation of the resident frames
 * The step every recipe puts in front of splice + LDA (f12), MLLT (f13) and fMLLR (f11): per speaker (or per utterance) from resident
 * statistics, or over a sliding window, in place on the resident frame matrix (csrc/frame_cmvn.hip).  Not in the reference;
 * tests/_cmvn_twin.py is the rule's NumPy twin.  Everything is float64: x is read from the float64 copy when the context holds one (which
 * then receives y), else from the float32 rows widened; the float32 rows always receive y rounded to nearest.  Padding columns, rows
 * outside every listed utterance and the utterances that are skipped or refused keep their bits.  No floating-point atomics: two runs give
 * the same bits.  Utterance u occupies the rows [frame_begin[u], + T[u]) of the (F, D) matrix, as pcl_frames_transform takes them; the
 * utterances of a call must not overlap.
 *
 * STATISTICS.  Per speaker  n = the rows (an exact integer)    s_d = sum x_d    q_d = sum x_d x_d   (x_d x_d rounded, then added)
 * at the dimension D of the CURRENT frame matrix.  Order: an utterance's rows are cut into chunks of 1024; in a chunk, row lane r of four
 * adds the chunk's rows r, r + 4, r + 8, ... in ascending order from 0, and the four lanes' sums are added ((l0 + l1) + l2) + l3; the
 * utterance's sum is its chunks' sums added in chunk order from 0; the sums of a speaker's utterances with T > 0 are added onto the
 * speaker's resident sums in ascending utterance index.  One workgroup per (utterance, chunk), then one per speaker walking its utterances.
 * pcl_cmvn_zero makes (and clears) the statistics for S <= 65535 speakers; needs a frame matrix.  They are additive over calls of
 * pcl_cmvn_accumulate (a speaker may span several calls and several frame matrices of the same D) and are dropped by the next
 * pcl_cmvn_zero, by pcl_destroy, and by a frame matrix of another D: every call that uses them is then PCL_ERR_STATE until the next
 * pcl_cmvn_zero.  utt_speaker (U,) int32 in [0, S), or -1 = the utterance is skipped.
 * pcl_cmvn_stats_download: n (S,) int64, s (S, D), q (S, D) float64; NULLs are skipped.
 *
 * APPLY.  pcl_frames_cmvn, from the resident statistics, which must be of the same S.  Per speaker and column, one rounding per operation,
 * in this order:
 *     m = s / n        t = q / n - m m        v = t when t > var_floor, else var_floor        y = (x - m) / sqrt(v)   (norm_vars != 0)
 *                                                                                             y = x - m                (norm_vars == 0)
 * A speaker is REFUSED -- its utterances keep their bits, its status is non-zero -- when, tested in this order,
 *     PCL_CMVN_LOW_COUNT    n < min_count  (so is every speaker without a row: min_count >= 1)
 *     PCL_CMVN_NOT_FINITE   any s_d or q_d is not finite
 * Statuses are decided before anything is written (one wave per speaker, which also forms m and sqrt(v)); status_out (S,) int32 or NULL.
 * Per-utterance CMVN is utt_speaker = 0 .. U-1 with S = U.  The apply is elementwise over an utterance's contiguous run of rows, in aligned
 * 16-byte groups.
 *
 * SLIDING WINDOW.  pcl_frames_cmvn_sliding: no resident statistics.  For frame t of an utterance of T rows the window [lo, hi) is
 *     center != 0:  lo = t - window / 2 (integer division), hi = lo + window;  if lo < 0: hi -= lo, lo = 0;
 *                   if hi > T: lo = max(0, lo - (hi - T)), hi = T
 *     center == 0:  lo = max(0, t - window + 1), hi = t + 1;  if hi - lo < min_window: hi = min(T, lo + min_window)
 * n = hi - lo, s = P[hi] - P[lo], q = Pq[hi] - Pq[lo], then m, t, v, y as above, from the sums of the ORIGINAL rows: the prefix arrays of
 * x and of x x are built into a block of the context's pool before any row is written.  Order of a prefix: the utterance is cut into
 * blocks of 64 rows; local[r] = the inclusive sum of the block's rows up to r in ascending order from 0; offset[0] = 0, offset[b + 1] =
 * offset[b] + (the total of block b), in ascending block order; P[0] = 0 and P[r + 1] = offset[block of r] + local[r].  One wave per
 * (utterance, block) with a lane per feature, one workgroup per utterance for the offsets.  Nothing is read across an utterance
 * boundary; T = 0 is a no-op.  1 <= min_window <= window <= 2^20.  The block holds 16 D bytes per row: the utterances are processed in
 * groups of consecutive utterances of at most PCL_CMVN_GROUP_ROWS rows (env, read on every call; default 2^28 / D; a single longer
 * utterance is a group of its own), on which the result does not depend.
 *
 * No frames, no statistics (never made, or dropped): PCL_ERR_STATE.  Overlapping utterances, an utterance outside the matrix, a speaker
 * outside [-1, S), S out of range or not the statistics', var_floor not finite or not > 0 under norm_vars, min_count < 1, the window limits:
 * PCL_ERR_INVALID.  All checked before anything is changed.  A live pcl_seg has its own copy of the frames and is untouched; live batches
 * keep the emissions they scored from the old rows until they are scored again, as after pcl_frames_transform.  The statistics of the
 * fMLLR, MLLT and LDA rows are not touched.  pcl_kernel_time groups: "cmvn_stats", "cmvn_apply", "cmvn_sliding".  Synchronous. */
#define PCL_CMVN_OK 0
#define PCL_CMVN_LOW_COUNT 1
#define PCL_CMVN_NOT_FINITE 2
int pcl_cmvn_zero(pcl_ctx *ctx, int S);
int pcl_cmvn_accumulate(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *utt_speaker /* U, -1 = skip */);
int pcl_cmvn_stats_download(pcl_ctx *ctx, int64_t *n /* S or NULL */, double *s /* S*D or NULL */, double *q /* S*D or NULL */);
int pcl_frames_cmvn(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *utt_speaker, int S, int norm_vars,
                    double var_floor, int64_t min_count, int32_t *status_out /* S or NULL */);
int pcl_frames_cmvn_sliding(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, int window, int min_window, int center,
                            int norm_vars, double var_floor);

/* ----------------------------------------------------------------- phonetic decision tree (row f16): context statistics, tied states
 * The first half of monophone -> context-dependent (csrc/tree_cluster.hip): per-context single-Gaussian statistics from an alignment, trees
 * grown top-down over phonetic questions, the tied-state map, and a one-Gaussian-per-leaf seed model that pcl_model_mixup and the E-step
 * then grow.  Not in the reference; tests/_tree_twin.py is the rule's NumPy twin.  Everything is float64, one rounding per operation; no
 * floating-point atomics: two runs give the same bits.
 *
 * ROWS.  The caller lists the E distinct contexts it saw: event_ctx (E, 3) int32 = (left, centre, right), unit ids 0 .. n_units - 1, the
 * value n_units = no neighbour (utterance edge); the centre is a unit.  P = S - 2 state positions; statistics row r = e P + k, R = E P.
 * Per row   n = its frames (int64)    s_d = sum x_d    q_d = sum x_d x_d   (x_d x_d rounded, then added)
 * pcl_tree_zero makes (and clears) them for R rows at the dimension D of the CURRENT frame matrix: ONE block of 8 R (2 D + 1) bytes from
 * the context's pool, at most 2^32; freed by pcl_destroy and by the next pcl_tree_zero.  They are additive over calls.
 *
 * ACCUMULATE.  pcl_tree_accumulate: frame_row (F,) int32, the statistics row of every row of the frame matrix, or -1; utterance u occupies
 * the rows [frame_begin[u], + T[u]), the utterances must not overlap, rows outside every utterance are not counted.
 * pcl_batch_accumulate_tree: a label-built batch after pcl_batch_viterbi -- everything pcl_batch_align_segments needs and checks, its drop
 * rule and its slices; label_event (sum of the label lengths,) int32 = the event of every label position, or -1 = the position's frames
 * are skipped.  A frame whose path row belongs to label position i (entry row -> 0, rows 1 .. P L -> (row - 1) / P, exit row -> L - 1)
 * and whose slice in pcl_batch_align_segments' owner map is k goes to row label_event[i] P + k.  The owner map stays on the device.
 * x is read from the float64 copy when the context holds one, else the float32 rows are widened, as in pcl_frames_moments.
 * Order: the kept frame rows are counting-sorted by statistics row, stably; a statistics row's frames, in ascending frame row, are cut into
 * chunks of PCL_TREE_CHUNK (env, read on every call; default 256); a chunk's frames are added in ascending order from 0; the chunks'
 * sums are added onto the resident sum in chunk order.  One group of lanes per chunk, one 16-byte load per frame and lane.
 *
 * LIKELIHOOD of a pooled set (n, s, q), n > 0, d ascending:
 *     m_d = s_d / n      v_d = max(q_d / n - m_d m_d, var_floor)      L = -0.5 n (D c + sum_d ln v_d),  c = 1 + ln 2 pi = 2.8378770664093453
 * L = 0 for n = 0.
 *
 * QUESTIONS.  q_member (Q, n_units + 1) uint8: unit sets, the edge symbol a member like any other.  Candidate c = pos Q + qi, pos 0 left,
 * 1 centre, 2 right; an event answers yes iff q_member[qi][event_ctx[e][pos]].  ROOTS.  root_of (n_units P,) int32 in [0, R0) maps
 * (centre, k) to its root; row (e, k) starts in root root_of[centre(e) P + k]; nodes 0 .. R0 - 1 are the roots.
 *
 * GROWTH.  For a leaf and a candidate, the yes-set is the leaf's rows whose event answers yes, the no-set the rest; either side's (n, s, q)
 * is the sum of its rows in ascending row order from +0.0, the same for every candidate.  gain = (L_yes + L_no) - L_leaf, L_leaf from the
 * sum of all the leaf's rows in ascending order.  A candidate is valid iff n_yes >= min_count, n_no >= min_count and gain >= min_gain.
 * Each step splits the (leaf, candidate) of largest gain among all current leaves; ties go to the lowest node id, then the lowest c.
 * Split number t (from 0) creates the nodes R0 + 2 t (no) and R0 + 2 t + 1 (yes).  Growth stops when no candidate is valid or the leaves
 * number max_leaves (>= R0).  Tied-state ids are the leaves in ascending node id, 0 .. J_t - 1.  Rows with n = 0 follow their answers.
 * One workgroup per (leaf, 8 candidates) walks the leaf's rows once; the gains and the arg-max of a leaf run on the device, the choice
 * among the leaves and the stable partition of the chosen leaf's row list on the host.
 *
 * OUTPUTS (NULLs are skipped; capacity N <= R0 + 2 (max_leaves - R0)): node_cand (N,) c or -1 at leaves; node_child (N, 2) (no, yes) or
 * -1; node_state (N,) tied id or -1; node_n (N,) int64; split_gain ((N - R0) / 2,) in split order; row_state (R,); the leaves' sums
 * leaf_n (J_t,) int64, leaf_s, leaf_q (J_t, D).  *n_nodes_out = N, *n_states_out = J_t.
 * INSTALL (install != 0).  The resident model becomes (J_t, 1, D): mean = s / n, var = v as above, weight 1, written into the float64
 * master copy, then everything pcl_model_upload runs after its copy (pcl_model_flat_start's path and flags).  A leaf with n = 0:
 * PCL_ERR_INVALID naming the node, before anything is written; the model in place stays.  Unit transitions, frames and the tree
 * statistics are untouched.
 * pcl_tree_stats_upload REPLACES the resident statistics (externally merged sums; tests drive the build with exact values).
 * pcl_tree_stats_shape: *R and *D of the resident statistics, the sizes a download needs; 0 and 0 when there are none (no refusal).
 *
 * PCL_ERR_STATE: no frames or no statistics; the frame matrix changed its width since pcl_tree_zero; the batch conditions of
 * pcl_batch_align_segments.  PCL_ERR_INVALID: R < 1 or 8 R (2 D + 1) > 2^32; a row or event id outside [-1, R) / [-1, E); E P != R; a
 * context id outside [0, n_units] or a centre = n_units; root_of outside [0, R0) or a root nobody maps to; Q < 1 or 3 Q > 4096;
 * max_leaves < R0; min_gain negative or not finite; var_floor <= 0; min_count < 1; uploaded statistics not finite or n < 0; overlapping
 * utterances.  All checked before anything is changed.  pcl_kernel_time groups: "tree_sort", "tree_stats", "tree_build".  Synchronous. */
int pcl_tree_zero(pcl_ctx *ctx, int R);
int pcl_tree_accumulate(pcl_ctx *ctx, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *frame_row /* F, -1 = skip */);
int pcl_batch_accumulate_tree(pcl_batch *b, const int32_t *label_event /* sum L_u, -1 = skip */);
int pcl_tree_stats_shape(pcl_ctx *ctx, int32_t *R, int32_t *D);
int pcl_tree_stats_download(pcl_ctx *ctx, int64_t *n /* R or NULL */, double *s /* R*D or NULL */, double *q /* R*D or NULL */);
int pcl_tree_stats_upload(pcl_ctx *ctx, const int64_t *n /* R */, const double *s /* R*D */, const double *q /* R*D */);
int pcl_tree_build(pcl_ctx *ctx, int E, int P, const int32_t *event_ctx /* E*3 */, int n_units, int Q, const uint8_t *q_member /* Q*(n_units+1) */,
                   int R0, const int32_t *root_of /* n_units*P */, int64_t min_count, double min_gain, int max_leaves, double var_floor, int install,
                   int flags, int32_t *node_cand, int32_t *node_child, int32_t *node_state, int64_t *node_n, double *split_gain,
                   int32_t *row_state, int64_t *leaf_n, double *leaf_s, double *leaf_q, int32_t *n_nodes_out, int32_t *n_states_out);

/* ----------------------------------------------------------------- resident tying, label-built batches over tied states (row f17)
 * The second half of monophone -> context-dependent (csrc/tying.hip): the trees of a build stay on the device, one kernel maps every label
 * position of a corpus to its tied states, and the batch made from them is a label-built batch for every entry point that asks for one.
 * Not in the reference; tests/_tied_twin.py is the NumPy twin.  Integer work only: equal inputs give equal bytes.
 *
 * TYING.  pcl_tying_upload takes the arrays a build returned, with the meaning of the tree section above: q_member (Q, n_units + 1) uint8,
 * candidate c = pos Q + qi, n_units = the utterance-edge symbol; node_cand (N,), node_child (N, 2) = (no, yes), node_state (N,); the nodes
 * 0 .. R0 - 1 are the roots, root_of (n_units P,) maps (centre, k) to its root; J_t tied states.  Checked, in this order, before anything
 * resident changes (PCL_ERR_INVALID unless stated): a unit inventory is resident (PCL_ERR_STATE); P = S - 2 of the inventory; n_units is the
 * inventory's; 1 <= Q, 3 Q <= 4096; 1 <= R0 <= N; 1 <= J_t <= N; per node in ascending id -- a leaf (cand = -1) has children (-1, -1) and a
 * state in [0, J_t) no earlier leaf names; an inner node has 0 <= cand < 3 Q, both children in (node, N) and state -1 -- the leaves number J_t;
 * root_of in [0, R0).  pcl_tree_build creates children after their parent, so a built tree passes, and a walk, which only ever moves to a
 * larger node id, ends.  The upload REPLACES a resident tying as a whole; pcl_tying_drop removes it (no refusal when there is none);
 * pcl_destroy and a pcl_units_upload of another (n_units, S) free it too.  On the device: one 16-byte record (cand, no, yes, state) per node
 * in global memory -- a step of a walk is one load -- and q_member as a bit table of ceil((n_units + 1) / 32) words per question, staged in
 * LDS by every workgroup when it is at most 16 KiB.
 *
 * WALK of (left, centre, right) at state position k: node = root_of[centre P + k]; while node_cand[node] = c >= 0: pos = c / Q, qi = c mod Q,
 * node = node_child[node][q_member[qi][context[pos]]]; the result is node_state[node].  ContextTree.Tree.lookup is the same walk.
 * pcl_tying_lookup: ctx3 (n, 3) int32 contexts, seen in training or not -> state_out (n, P) int32.  PCL_ERR_STATE without a resident
 * tying; PCL_ERR_INVALID for n < 1, a centre outside [0, n_units) or a neighbour outside [0, n_units], before anything runs.
 *
 * BATCH.  pcl_batch_create_labels_tied: the arguments, the N_u = P L_u + 2 rows, the banded transitions of the centre units, the uniform
 * pi and the unit -> occurrence lists of pcl_batch_create_labels, and its refusals under its own name; PCL_ERR_STATE without a resident
 * tying, for a tying of another inventory shape, or when the model's J is not the tying's J_t.  Label position i of utterance u has the context
 * (labels[i - 1], labels[i], labels[i + 1]) with n_units in place of a neighbour beyond either end (ContextTree.triphone_events); one
 * workgroup per utterance, its lanes striding the (i, k) pairs, walks once per pair and writes pos_state (sum L, P) and the row -> state
 * map: entry row, row 1 + i P + k -> pos_state[i][k], exit row.  pos_state stays with the batch: a later pcl_tying_upload or
 * pcl_tying_drop does not change a batch that exists.  The map comes back to the host once (sum N int32) for the scoring work lists.
 *
 * LABEL-BASED CALLS on a tied batch.  Where pcl_batch_align_segments and the calls that share its checks demand J = n_units (S - 2) of a
 * monophone batch, they demand J = the batch's J_t of a tied one (PCL_ERR_INVALID); every other check is unchanged.
 * pcl_batch_align_segments: the owner of a kept frame t is pos_state[i(t)][k(t)], i(t) = the label position of the frame's path row by the
 * rule of pcl_batch_accumulate_tree above, k(t) = the slice the monophone owner map gives the same labels and path (runs of equal units,
 * adjacent equal units merged); the drop rule is unchanged; the pcl_seg holds J_t lists.  pcl_batch_accumulate_lda: the class of a frame is
 * that owner, or state_class[owner] (J_t entries).  pcl_batch_accumulate_tree: rows label_event[i(t)] P + k(t), as for a monophone batch.
 * pcl_batch_accumulate_hmm, pcl_mstep_transitions, pcl_batch_refresh_transitions: transitions are per centre unit, the calls do on a tied
 * batch what they do on a monophone one; the refresh refuses (PCL_ERR_STATE) when J is no longer the batch's J_t or the inventory no
 * longer fits the batch's labels and rows.
 * pcl_batch_get_states: the device copies of a batch's row -> state map (row_state, sum N int32; any batch that has one) and of a tied
 * batch's pos_state (sum L * P int32; PCL_ERR_STATE for any other batch); NULLs are skipped.
 * pcl_kernel_time groups: "tying" (the batch's walks), "tying_lookup", "tying_owner".  Synchronous. */
int pcl_tying_upload(pcl_ctx *ctx, int n_units, int P, int Q, const uint8_t *q_member /* Q*(n_units+1) */, int N, const int32_t *node_cand /* N */,
                     const int32_t *node_child /* N*2 */, const int32_t *node_state /* N */, int R0, const int32_t *root_of /* n_units*P */, int J_t);
int pcl_tying_drop(pcl_ctx *ctx);
int pcl_tying_lookup(pcl_ctx *ctx, int n, const int32_t *ctx3 /* n*3 */, int32_t *state_out /* n*P */);
int pcl_batch_get_states(pcl_batch *b, int32_t *row_state /* sum N or NULL */, int32_t *pos_state /* sum L * P or NULL */);
int pcl_batch_create_labels_tied(pcl_ctx *ctx, int U, const int32_t *label_len, const int32_t *labels, const int32_t *T,
                                 const int64_t *frame_begin, const double *logpi, pcl_batch **out);

/* Numerical guard of the f32 matrix-core path.  The MFMA kernels evaluate the Gaussian exponent in a form expanded
 * around a per-state centre c_j; its f32 rounding error grows with cond[j] = max_m log2(e) * sum_d (mu_jmd - c_jd)^2 /
 * (2 var_jmd) (about 5e-7 * cond nats).  States with cond[j] > *cond_max (default 96, env PCL_MFMA_COND_MAX) are scored
 * and accumulated by the direct-form (x-mu)^2 kernels instead, so util.py:78-88's result keeps its 1e-4 tolerance on
 * any model.  cond: J floats (may be NULL); cond_max: 1 float (may be NULL).  Recomputed by upload and by pcl_mstep. */
int pcl_model_conditioning(pcl_ctx *ctx, float *cond, float *cond_max);

/* Split states (round 4).  The limit above is a property of single mixtures: one tight mixture far from the state's centre
 * used to send its whole state (2048 mixtures) to the direct-form kernels, and after an M-step nearly every state has a few.
 * A mixture whose own term cond_jm exceeds cond_max is now taken out of the matrix-core layouts instead (it looks like a
 * zero-weight mixture there and does not enter the state's feature scales or cond[j]); the direct-form kernels evaluate the
 * state's list of such mixtures and the two parts are merged -- ln(e^a + e^b) of the two partial log-sum-exps in scoring,
 * += into the same statistics in the accumulate pass -- so the result is the reference's sum over all mixtures
 * (Clustering.py:740-767, :653-680) whichever kernel evaluated a term.  A state leaves the matrix cores as a whole only when
 * more than *limit of its mixtures are out.  Round 6: in SCORING the list is no longer evaluated in direct form but by the coarse pass
 * (csrc/gmm_score_coarse.hip: a bound of each off-pipe mixture computed on the matrix pipe rules out almost every (frame, mixture) pair,
 * the pairs it cannot rule out are evaluated in direct form), and *limit is 0.99 M there (env PCL_COARSE_SPLIT_MAX; PCL_COARSE=0:
 * direct form, limit 0.5 M).  The accumulate pass keeps direct form and 0.5 M.  env PCL_SPLIT_MAX = share of M sets both limits;
 * 0 = whole states, as before round 4.  *limit reports the scoring limit.
 * n_off: J ints, off-pipe mixtures per state (may be NULL); limit: 1 int (may be NULL). */
int pcl_model_split_info(pcl_ctx *ctx, int *n_off, int *limit);
/* Diagnostics of the coarse pass over the off-pipe mixtures (csrc/gmm_score_coarse.hip; counted only under env PCL_COARSE_STATS=1):
 * *pairs = (frame, mixture) pairs evaluated in direct form since the last reset -- the pairs the bound on the matrix pipe could not rule
 * out; every other pair of an off-pipe mixture was proven to lie 2^-36 below its frame's likelihood, or its tile was flagged and rescored in
 * direct form (below).  reset != 0 clears the count. */
int pcl_coarse_counter(pcl_ctx *ctx, unsigned long long *pairs, int reset);
/* ... and *tiles_given_up (may be NULL) = tiles of 256 frames x one state on which the pass gave up -- a wave had evaluated more than
 * max(4096, 2 x the state's off-pipe mixtures) pairs: the state's on-pipe part is no reference for those frames; in the state's last
 * stage of mixture tiles, with a tile of the stage left untested -- and which the direct-form subset kernel rescored in the same call (as
 * it does tiles with a feature out of the f16 range).  Same results either way.  The pass also flags (without counting it here) a tile
 * with a frame whose threshold the f16 slot's clamp to +-5e4 log2 units from the state's K0 raised above what its reference asked for
 * (what the pipe wrote more than ~3.5e4 nats below K0, or -inf: no on-pipe mixture) and which ruled out a pair whose bound is not below
 * what the frame's reference at the end (the pipe's value or the largest exact value) asks for: such a pair is not proven negligible. */
int pcl_coarse_counters(pcl_ctx *ctx, unsigned long long *pairs, unsigned long long *tiles_given_up, int reset);

/* How much of a CU the matrix-core scoring kernel takes.  0 (default): three workgroups per CU, the fastest for the kernel alone.
 * 2: two -- a third of the registers stays free for kernels of OTHER streams, which is what lets the token passing of chunk k-1
 * (pcl_batch_decode, second stream) run beside the scoring of chunk k in a streamed decode (Decoder.py has no such loop: the
 * reference decodes utterance by utterance, Decoder.py:146-187).  Same kernel, same results; applies to the launches that follow. */
int pcl_score_occupancy(pcl_ctx *ctx, int workgroups_per_cu);

/* ----------------------------------------------------------------- MFCC front-end (next row f4: the step before the path)
 * AudioProcessing.MFCC.mfcc (StatisticalModel/AudioProcessing.py:416-448) for U signals at once, float64:
 * pre-emphasis 0.98 (:184), framing sampletime/overlap (:201), per-FRAME window factor (:228, as the reference
 * computes it), |rFFT_nfft| (:250), mel filter bank + frame energy (:279), ln + DCT (:347), c0 <- ln(energy)
 * (flags bit0), deltas / delta-deltas over +-2 frames (flags bit1 / bit2, :401).  signal = concatenated samples,
 * sig_off[U+1]; twiddle_cos/sin[nfft], mel_response[filterbanks][nfft/2+1] and dct_matrix[rank][filterbanks] are
 * built by the caller (poccala_amd/StatisticalModel/AudioProcessing.py) so the reference's filter and DCT
 * conventions are defined in one place.  out: out_rows x (rank * {1,2,3}) row-major, out_rows = total frames. */
int pcl_mfcc(pcl_ctx *ctx, int U, const double *signal, const int64_t *sig_off, int framerate, double sampletime,
             double overlap, int nfft, int filterbanks, int rank, int flags, const double *twiddle_cos,
             const double *twiddle_sin, const double *mel_response, const double *dct_matrix, double *out,
             int64_t out_rows);
/* pcl_mfcc on int16 PCM, the samples as a wav file holds them (AudioProcessing.py:128-176 reads np.short): a quarter of the bytes of
 * the float64 form on the wire.  The arguments are pcl_mfcc's with int16_t samples (sig_off still counts SAMPLES); a sample becomes a
 * double at the kernel's load and every operation after it is pcl_mfcc's, so the result is bit-identical to pcl_mfcc on
 * (double)sample.  Checks, error codes and texts (prefixed pcl_mfcc_pcm16) are pcl_mfcc's.
 * The samples travel through two page-locked staging buffers owned by the context: the library copies chunk k+1 into one while the
 * asynchronous H2D copy of chunk k runs from the other on a stream of its own; the kernels start behind the last chunk.  Samples per
 * chunk: env PCL_PCM_CHUNK, read on EVERY call (default 2097152 = 4 MiB per buffer: the per-chunk queueing cost stays below 5 % of the
 * chunk's host memcpy, which is the longer of the two overlapping legs, and the context pins 8 MiB); the buffers grow when a call asks
 * for a larger chunk.  Device buffers come from the library's pool, and the four tables stay on the device with the context: they are
 * uploaded again only when their geometry or their BYTES differ from the last call's (both for pcl_mfcc / pcl_frontend too).
 * pcl_kernel_time groups, while timing is on: "pcm_stage" = host milliseconds spent copying into the staging buffers, "pcm_h2d" = the
 * chunks' copies on the staging stream (for the float64 entry points: the host time of their one blocking copy).  Synchronous. */
int pcl_mfcc_pcm16(pcl_ctx *ctx, int U, const int16_t *signal, const int64_t *sig_off, int framerate, double sampletime,
                   double overlap, int nfft, int filterbanks, int rank, int flags, const double *twiddle_cos,
                   const double *twiddle_sin, const double *mel_response, const double *dct_matrix, double *out,
                   int64_t out_rows);

/* ----------------------------------------------------------------- voice-activity detector (row f6: the second half of the front-end)
 * AudioProcessing.VAD.mfcc (StatisticalModel/AudioProcessing.py:538-543) = mel_distance (:462-478) -> osf (:480-507) -> detect (:509-536)
 * for U utterances at once, float64, on the device (csrc/vad.hip).  It is what AcousticModel.__load_audio (AcousticModel.py:463-477) and
 * Decoder (Decoder.py:55-60) put between MFCC.mfcc and the hot path.  The reference's conventions, kept exactly (golden G19):
 *   V1 (:467-472)  noise = (1/s) * (sum of the first s = simple_size rows), then for i = 0..s-1: noise = alpha*noise + (1-alpha)*x_i
 *   V2 (:475-477)  dist_t = sqrt(sum_d (noise_d - x_td)^2) over all D columns (deltas included), summed over d in ascending order
 *   V3 (:500-507)  for s <= i < T - s: the window is d[i-s : i+s] -- 2s values, not the 2s+1 the comment speaks of --, sorted ascending
 *                  (NaN last), h = int(beta*(2s+1)), osf_i = (1-beta)*w[h] + beta*w[h+1]; every other frame keeps its distance
 *   V4 (:516-536)  thr = osf[int(s/2)] * (max - min) / max over the utterance (the sorted sample of :516-517 is never used: no median);
 *                  frame t is kept iff osf_t - thr > 0, IEEE semantics: a non-finite distance makes thr NaN and nothing is kept
 *   V5             T_u < s: the reference raises IndexError (:472) -> PCL_ERR_INVALID naming the utterance; s <= T_u <= 2s: no frame is filtered
 * Every step is one correctly rounded float64 operation at a time (nothing contracted into an fma), the selection is exact, nothing is
 * summed with atomics: from equal distances, osf / thr / the kept set are those of a NumPy restatement bit for bit (tests/_vad_twin.py).
 * mfcc: (row_off[U], D) row-major features, utterance u = rows [row_off[u], row_off[u+1]), row_off[0] = 0; D <= 64 as pcl_frames_upload.
 * Outputs (NULL pointers are skipped; a stage none of whose results is asked for does not run): dist / dist_osf (rows,), thr (U,),
 * kept_len (U,), kept_idx (rows,) int32: utterance u's kept rows, counted from ITS first row, ascending, at kept_idx[row_off[u] ..
 * row_off[u] + kept_len[u]), -1 behind them.  flags: PCL_VAD_DIST_IN = `dist` is the caller's (V1-V2 skipped, mfcc may be NULL),
 * PCL_VAD_OSF_IN = `dist_osf` is the caller's (V1-V3 skipped): the reference's three methods one at a time.
 * h + 1 >= 2s is PCL_ERR_INVALID when V3 runs and some utterance has T > 2s (the reference indexes out of range as soon as a frame is
 * filtered; with every T <= 2s it never looks at h, and neither does this).  1 <= s <= 1024, U <= 65535.
 * Synchronous. */
#define PCL_VAD_DIST_IN 1
#define PCL_VAD_OSF_IN 2
int pcl_vad(pcl_ctx *ctx, int U, const double *mfcc, const int64_t *row_off, int D, int simple_size, double alpha, double beta, int flags,
            int32_t *kept_len, int32_t *kept_idx, double *dist, double *dist_osf, double *thr);
/* PCM -> resident frames: pcl_mfcc's kernels, then V1-V5 above on their device result, then the survivors gathered into the context's
 * frame matrix -- what AcousticModel.__load_audio (AcousticModel.py:463-477) does per file, for U signals, without the features leaving the
 * device.  signal .. dct_matrix are pcl_mfcc's arguments (mfcc_flags = its flags).  On return the survivors ARE the current frame matrix,
 * exactly as pcl_frames_upload would have left them: float32, rows padded with zeros to the device dimension, rounded to nearest; with
 * PCL_FRONTEND_KEEP_F64 the float64 copy parity mode (PCL_F64) reads is kept too (otherwise it is derived from the float32 rows on first use,
 * as after a float32 upload).  T_out (U,) int32 / frame_begin_out (U,) int64 are what pcl_batch_create(_labels) takes: batches follow with
 * no feature upload.  An utterance that keeps no frame has T_out = 0 (leave it out of the batch).  PCL_FRONTEND_NO_VAD: every MFCC row is
 * kept (MFCC straight to resident frames).  out_host: NULL, or out_rows x D float64 (out_rows = total MFCC frames, as pcl_mfcc) whose
 * first sum(T_out) rows receive the survivors.  Every check -- V5 from the signal lengths, the order statistics, D > 64 -- runs before
 * the first launch: a failed call leaves the previous frame matrix in place.  When no frame of ANY utterance survives the call succeeds
 * like any other: every T_out is 0 and the current frame matrix is empty (0 rows: no batch can be created on it).  Synchronous. */
#define PCL_FRONTEND_NO_VAD 1
#define PCL_FRONTEND_KEEP_F64 2
int pcl_frontend(pcl_ctx *ctx, int U, const double *signal, const int64_t *sig_off, int framerate, double sampletime, double overlap, int nfft,
                 int filterbanks, int rank, int mfcc_flags, const double *twiddle_cos, const double *twiddle_sin, const double *mel_response,
                 const double *dct_matrix, int simple_size, double alpha, double beta, int flags, int32_t *T_out, int64_t *frame_begin_out,
                 double *out_host, int64_t out_rows);
/* pcl_frontend on int16 PCM: its arguments with int16_t samples, pcl_mfcc_pcm16's transfer (staging, PCL_PCM_CHUNK, pooled buffers,
 * cached tables) in front of the same kernels.  T_out, frame_begin_out, the resident float32 (and float64) frames and out_host are
 * bit-identical to pcl_frontend on (double)sample; every check runs before the first copy or launch, and a failed call leaves the
 * previous frame matrix in place (error texts prefixed pcl_frontend_pcm16).  Synchronous. */
int pcl_frontend_pcm16(pcl_ctx *ctx, int U, const int16_t *signal, const int64_t *sig_off, int framerate, double sampletime, double overlap,
                       int nfft, int filterbanks, int rank, int mfcc_flags, const double *twiddle_cos, const double *twiddle_sin,
                       const double *mel_response, const double *dct_matrix, int simple_size, double alpha, double beta, int flags,
                       int32_t *T_out, int64_t *frame_begin_out, double *out_host, int64_t out_rows);

/* ----------------------------------------------------------------- pitch and voicing features (csrc/pitch.hip)
 * The unit inventory is toned (XIF_tone.csv): two finals that differ only in tone are different units, and the mel filters of the MFCC
 * smooth away the harmonics that carry tone.  pcl_pitch gives three float64 columns per frame -- voicing, ln f0, delta ln f0 -- on the
 * MFCC's frame grid, for U signals at once.  The reference has no pitch code; the rule is this project's (tests/_pitch_twin.py is its
 * NumPy definition):
 *   geometry  size = int(rate * sampletime), step = int(size * overlap), T = max(1, 1 + ceil((n - size) / step)), frame t starts at sample
 *             t * step, samples beyond the signal are zero: the rows of pcl_mfcc (which refuses n < size; here that is one frame).
 *             Lags are the integers Lmin = ceil(rate / f_max) .. Lmax = floor(rate / f_min), L = Lmax - Lmin + 1 of them.
 *   P1  w = x[t*step : t*step + size + Lmax] minus the mean of its first `size` samples (the zero padding included in the subtraction);
 *       the mean's sum is 64 partial sums, partial j = 0 + w[j] + w[j + 64] + ..., then 0 + partial 0 + partial 1 + ..., then / size
 *   P2  a = w[0 : size], b_l = w[l : l + size]; p = a.b_l, e0 = a.a, el = b_l.b_l, each summed over the sample index in ascending order
 *       from 0, one rounded multiplication and one rounded addition at a time (el directly for every lag, not from e_{l-1});
 *       nccf_raw = p / sqrt(e0 * el), 0 where e0 * el == 0; nccf_bal = p / sqrt(e0 * el + ballast), 0 where that sum is 0 (ballast in
 *       squared sample units, 7000 for int16 speech: it pulls quiet frames towards 0)
 *   P3  c(t, l) = 1 - nccf_bal(t, l) * (1 - soft_min_f0 * l / rate)
 *   P4  best(0, l) = c(0, l); best(t, l) = c(t, l) + min over l' of [best(t-1, l') + pf * (g[l] - g[l'])^2], ties to the smallest l';
 *       the last frame takes the smallest l of its minimum and the back-pointers are followed.  g[n_lags] = ln(lag) is the CALLER's float64
 *       table (as the mel and DCT tables are): the device only subtracts, multiplies and adds
 *   P5  v = nccf_raw(t, l*); ln f0 = ln(rate / (l* + shift)), shift = 0.5 (y- - y+) / ((y- - 2 y0) + y+) from nccf_raw at l* - 1, l*, l* + 1,
 *       clamped to +-0.5; no shift at the ends of the lag grid or where that denominator is >= 0; delta ln f0 = ((x[t+1] - x[t-1]) +
 *       2 (x[t+2] - x[t-2])) / 10 with the frame indices clamped to the utterance's rows (the MFCC's +-2-frame rule, written as differences so
 *       that a constant column gives exactly 0)
 * Every step is one correctly rounded float64 operation in the order written (nothing contracted into an fma), nothing is summed with
 * atomics: nccf_bal, nccf_raw, the lags and v are the twin's bits, ln f0 differs by the device's log alone.  Mean normalisation of ln f0
 * is NOT part of the rule: pcl_frames_cmvn / pcl_frames_cmvn_sliding do it on resident columns.
 * signal / sig_off as pcl_mfcc (sig_off[0] = 0).  Outputs (NULL pointers are skipped): out (out_rows, 3) = [v, ln f0, delta], lag
 * (out_rows,) int32 in samples, nccf_bal / nccf_raw (out_rows, L); out_rows = total frames.  flags: PCL_PITCH_NCCF_IN = nccf_bal and
 * nccf_raw are the CALLER's (P1-P2 skipped, signal may be NULL; sig_off still gives the rows).
 * PCL_ERR_INVALID with a pcl_last_error text, before any launch: f_max > rate / 2, L > 1024, L < 2, Lmin < 1, n_lags != L, a negative or
 * non-finite parameter, a window of more than 64 KiB (size + Lmax + 64 doubles), U outside 1 .. 65535, out_rows != the geometry's.
 * pcl_kernel_time groups: "pitch_nccf" (P1-P2), "pitch_track" (P3-P4), "pitch_out" (P5).  Device buffers come from the pool and go back
 * on every path.  Synchronous. */
#define PCL_PITCH_NCCF_IN 1
int pcl_pitch(pcl_ctx *ctx, int U, const double *signal, const int64_t *sig_off, int framerate, double sampletime, double overlap, double f_min,
              double f_max, double ballast, double soft_min_f0, double pf, const double *g, int n_lags, int flags, double *out, int32_t *lag,
              double *nccf_bal, double *nccf_raw, int64_t out_rows);
/* pcl_pitch on int16 PCM through pcl_mfcc_pcm16's staging: a sample becomes a double at the kernel's load, every output is bit-identical
 * to pcl_pitch on (double)sample. */
int pcl_pitch_pcm16(pcl_ctx *ctx, int U, const int16_t *signal, const int64_t *sig_off, int framerate, double sampletime, double overlap,
                    double f_min, double f_max, double ballast, double soft_min_f0, double pf, const double *g, int n_lags, int flags, double *out,
                    int32_t *lag, double *nccf_bal, double *nccf_raw, int64_t out_rows);
/* pcl_frontend with the three pitch columns behind the MFCC's: its arguments, then pcl_pitch's parameters.  The MFCC is computed, the
 * detector runs on the MFCC columns ALONE (V2's distance does not see the pitch columns: T_out, frame_begin_out and the first
 * rank * {1,2,3} columns are pcl_frontend's bit for bit), P1-P5 run on the same samples, and the survivors are gathered as resident rows
 * of width rank * {1,2,3} + 3 (float32, padded to the device dimension; float64 too with PCL_FRONTEND_KEEP_F64): the pitch columns are those
 * of the rows the detector kept (the delta was taken over ALL of the utterance's rows, before the detector).  out_host: NULL or out_rows x
 * (rank * {1,2,3} + 3).  Every check -- pcl_frontend's, pcl_pitch's, width + 3 > 64 -- runs before the first launch: a failed call leaves the
 * previous frame matrix in place.  Synchronous. */
int pcl_frontend_pitch(pcl_ctx *ctx, int U, const double *signal, const int64_t *sig_off, int framerate, double sampletime, double overlap,
                       int nfft, int filterbanks, int rank, int mfcc_flags, const double *twiddle_cos, const double *twiddle_sin,
                       const double *mel_response, const double *dct_matrix, int simple_size, double alpha, double beta, int flags, double f_min,
                       double f_max, double ballast, double soft_min_f0, double pf, const double *g, int n_lags, int32_t *T_out,
                       int64_t *frame_begin_out, double *out_host, int64_t out_rows);
int pcl_frontend_pitch_pcm16(pcl_ctx *ctx, int U, const int16_t *signal, const int64_t *sig_off, int framerate, double sampletime, double overlap,
                             int nfft, int filterbanks, int rank, int mfcc_flags, const double *twiddle_cos, const double *twiddle_sin,
                             const double *mel_response, const double *dct_matrix, int simple_size, double alpha, double beta, int flags,
                             double f_min, double f_max, double ballast, double soft_min_f0, double pf, const double *g, int n_lags,
                             int32_t *T_out, int64_t *frame_begin_out, double *out_host, int64_t out_rows);

/* ----------------------------------------------------------------- multi-GPU (RCCL over xGMI)
 * Replaces the reference's file-based accumulator merge (LHMM.py:256-290, Clustering.py:314-367).
 * id_bytes is a 128-byte ncclUniqueId made by rank 0 and distributed by the caller. */
int pcl_comm_unique_id(void *id_bytes128);
int pcl_comm_init(pcl_ctx *ctx, int rank, int nranks, const void *id_bytes128);
/* Rehearsal transport for several ranks on ONE device (RCCL refuses that: "Duplicate GPU detected"): every collective
 * becomes an all-gather of host bytes through `fn` (returns 0 on success; recv_all = nranks * bytes, in rank order).
 * Same orchestration code as the RCCL path; refuses exchanges beyond 256 MiB.  Not a production path. */
typedef int (*pcl_allgather_fn)(void *user, const void *send, size_t bytes, void *recv_all);
int pcl_comm_init_host(pcl_ctx *ctx, int rank, int nranks, pcl_allgather_fn fn, void *user);
/* transport: 0 none, 1 RCCL, 2 host rehearsal; rccl_nranks = ncclCommCount (0 unless transport 1).  NULLs are skipped. */
int pcl_comm_info(pcl_ctx *ctx, int *rank, int *nranks, int *transport, int *rccl_nranks);
/* Sum all-reduce of all GMM statistics (f64) + log-sum-exp merge of the per-unit HMM accumulators: afterwards every
 * rank holds the global statistics (then pcl_mstep on every rank).  Kept for parity checks; the E-step uses: */
int pcl_stats_allreduce(pcl_ctx *ctx);
/* The E-step exchange + M-step: reduce-scatter of the GMM statistics by state range -> GMM.update_param
 * (Clustering.py:682-693) on the owned J/nranks states -> all-gather of (mean, var, weight) -> every layout re-derived;
 * the per-unit HMM accumulators are merged by max + sum all-reduces and, if update_transitions, LHMM.update_param's
 * transition update (LHMM.py:519-520) follows.  payload: PCL_F64, or PCL_F32 = half the bytes on the wire (sums and
 * parameters rounded to f32 in flight; every rank continues from the same rounded model).  With one rank and no
 * communicator this is pcl_mstep (+ pcl_mstep_transitions).  Synchronous at return. */
int pcl_em_exchange(pcl_ctx *ctx, double c_covariance, int payload, int update_transitions);
/* The LAST accumulate pass of an E-step and the exchange as one call, pipelined: the states are cut into n_chunks equal
 * chunks, and as soon as the accumulate pass (which walks the states in ascending order, a group at a time) is done with a
 * chunk, the chunk goes through reduce-scatter (inside a chunk rank r owns the r-th slice) -> GMM.update_param -> all-gather ->
 * its layouts re-derived, on a stream of its own, beside the accumulation of the later states.  Replaces, like pcl_em_exchange,
 * the reference's file merge + per-unit M-step (LHMM.py:256-290, Clustering.py:314-367,682-693; AcousticModel.py:918-935);
 * same sums and M-step arithmetic, so the gathered model equals pcl_batch_accumulate + pcl_em_exchange (bit for bit on
 * the rehearsal transport; RCCL's ring order may differ in the last bit).  Default (env PCL_PIPE_MODE=1): only a chunk's
 * reduce-scatter leaves early, M-steps / all-gathers / derive run at the end; PCL_PIPE_MODE=0: the whole chain per chunk (on one
 * rank: M-step + derive of finished chunks beside the rest of the pass).  Synchronous at return. */
int pcl_batch_accumulate_exchange(pcl_batch *b, int precision, double c_covariance, int payload, int update_transitions, int n_chunks);
/* The same exchange for a rank that has NO batch for this last pass (fewer batches on this rank than on the others: every rank must run
 * the same sequence of collectives): the rank's statistics -- zero, or whatever its earlier batches accumulated -- go through the
 * n_chunks chunk exchanges of pcl_batch_accumulate_exchange without an accumulate pass in front.  Same arguments, same result. */
int pcl_accumulate_exchange_idle(pcl_ctx *ctx, double c_covariance, int payload, int update_transitions, int n_chunks);
/* Of the last pcl_batch_accumulate_exchange: its number of chunks and how many of them left for the exchange WHILE the accumulate pass was
 * still running (0: the pass released none -- states out of ascending order or on the direct-form kernel -- and the call was the plain
 * accumulate + exchange).  NULLs are skipped. */
int pcl_pipe_info(pcl_ctx *ctx, int *chunks, int *released_early);
int pcl_comm_destroy(pcl_ctx *ctx);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* POCCALA_HIP_H */
