// Internal structures shared by the C-ABI host code and the HIP kernels of libpoccala_hip.so.
// Target: gfx950 (MI355X) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>

#include <map>
#include <string>
#include <vector>

#include "../../include/poccala_hip.h"
#include "pcl_own.h"
#include "pcl_desc.h"
#include "batch_plan.h"
#include "frontend_host.h"

// ---------------------------------------------------------------- device-side descriptors
// (ScoreSeg, DupRow, ScoreTile, UttDesc: batch_plan.h, with the host code that fills them)
// One surviving (frame, state) pair of the accumulate pass.
struct ActiveFrame {
    long long frame;  // row of the frame matrix
    double coef;      // ln gamma_t(j) - ln b_j(o_t)
    double lg;        // gamma_t(j) = exp(ln gamma_t(j)), taken once when the list is built (alpha_acc sums it)
};

// ---------------------------------------------------------------- host-side objects
struct KernelTimer {
    std::vector<TimedEventPair> ev;
    double host_ms = 0.0;   // groups measured on the host clock ("pcm_stage", the float64 route's blocking "pcm_h2d"): added to the events' sum
    int host_n = 0;
};

// The int16 PCM route of the front-end (mfcc.hip): two page-locked staging buffers of one chunk each and the stream their H2D copies run
// on, beside the host's memcpy of the next chunk.  Made on the first int16 call, kept with the context, gone with it after pcl_destroy
// has drained `stream` (declared first: destroyed after the buffers and events that were used on it).  ev[s] = the last copy that read pin[s] is done.
struct PcmStage {
    Stream stream;                           // StreamKind::NonBlocking
    PinBuf<int16_t> pin[2];                  // one chunk of samples each
    LazyEvent ev[2];
};
// The four host-built MFCC tables (twiddle cos | sin | mel response | DCT basis) in ONE device block, kept with the context: `host` is the
// copy the next call's tables are compared with byte for byte (the caller builds them: equal geometry does not mean equal contents).
struct MfccTables {
    DevBuf<double> d;
    int nfft = 0, nfilt = 0, rank = 0;       // nfft = 0: nothing valid on the device
    std::vector<double> host;
};

// Scratch of the accumulate pass (gmm_accumulate.hip, gmm_accumulate_f16.hip): everything here is rebuilt by every pass and dead when the
// pass's last kernel has run, and the passes of a context are serialised on its main stream (the auxiliary stream's producers are
// joined by the consumers) -- so it belongs to the CONTEXT, not to the batch: rounds 2-4 gave every batch its own (4 GB of tile images +
// up to 442 MB of active-frame lists: 35 GB for the 8 resident batches of config 4, and a corpus sweep that makes a batch per step
// allocated them per step).  Every array has its own capacity: a pass reserves what it needs, pcl_accumulate_release gives all of it back.
struct AccScratch {
    // work lists: per-segment counts / offsets, per-state active-frame lists, the accumulate order of the states
    DevBuf<int> cnt; DevBuf<long long> off; DevBuf<ActiveFrame> list;
    DevBuf<int> work_states, seg_lo, seg_hi, split_flag;   // (split_flag: 1 = a split state, in accumulate order)
    // producer / consumer: tile images in LDS order, per-state tile offsets, outlier masks; two sets: the producer of state group g + 1
    // runs on the auxiliary stream beside the consumer of group g
    DevBuf<unsigned char> images[2];
    DevBuf<int> tile_off[2], state_flag[2];
    DevBuf<unsigned int> tile_mask[2];                     // one word per tile: its capacity is the sets' capacity in tiles
    LazyEvent ev_prod[2], ev_cons[2], ev_start;
};

// What a context owns on the device, in the groups that live and die together: pcl_ctx inherits them, so a member reads ctx->pm32 as before,
// and a group is dropped by assigning it an empty one (every DevBuf releases its block).
// The model: float64 master copy and the layouts derived from it (model_derive.hip).
struct ModelDev {
    DevBuf<float> params32;      // J * Mpad * row : [s_0 c_0 s_1 c_1 ... const2]  (log2 domain)
    DevBuf<double> params64;     // same layout, float64
    DevBuf<float> pm32;          // MFMA scoring layout: [J][Mpad32/32][KS4][64 lanes][4], see gmm_score_mfma.hip
    DevBuf<float> centers32;     // J * D per-state expansion centres c_j
    DevBuf<unsigned short> pm16f;     // split-f16 layout with the constants folded into the spare K slot: [J][Mpad32/32][2][KS8f][64 lanes][8], see gmm_score_split.hip
    DevBuf<double> kzero;             // [J] K0_j = max_m k'_m of that layout
    DevBuf<float> fscale;             // [J][2][KS8f*8] power-of-two feature scales of that layout
    DevBuf<float> d_cond;             // [J] conditioning of the centred expansion (pcl_ctx::cond is the host copy)
    DevBuf<unsigned char> d_bad;      // [J][Mpad] 1 = the mixture is off the matrix pipe
    DevBuf<int> d_bad_idx;            // [J][Mpad] the state's off-pipe mixtures in ascending order (first nbad[j] entries)
    DevBuf<int> d_nbad;               // [J]
    DevBuf<int> d_non;                // [J] mixtures on the pipe (M - nbad)
    DevBuf<int> d_good_idx;           // [J][Mpad] the state's ON-pipe mixtures in ascending order (first M - nbad[j] entries): row r of a split state's matrix-pipe layout is mixture good_idx[r]
    DevBuf<int> d_npt;                // [J] 32-mixture tiles of the matrix-pipe layout in use: ceil((M - nbad) / 32)
    DevBuf<float> mean32;        // J * Mpad * D raw means (accumulate kernel)
    DevBuf<double> mean64;       // float64 master copy of the model: mean, var (J*Mpad*D), weight (J*Mpad)
    DevBuf<double> var64, w64;
    DevBuf<double> stats;        // E-step statistics (float64, linear domain), one allocation: [acc J*Mpad | alpha J | mean J*Mpad*D | cov J*Mpad*D]
    DevBuf<double> fmllr_Gk;     // fMLLR statistics (frame_adapt.hip): [fmllr_S][Dhost][Dhost + 1][Dhost + 2], row p of a pair = (G[p][0 .. D], k[p]); gone with the model
    DevBuf<double> fmllr_beta;   // [fmllr_S] occupancies
    DevBuf<double> fmllr_W;      // the last pcl_fmllr_estimate's transforms [fmllr_S][Dhost][Dhost + 1]; pcl_fmllr_zero drops it
    DevBuf<double> mllr_W;       // the last pcl_mllr_estimate's transforms [mllr_R][Dhost][Dhost + 1] (model_adapt.hip): gone with the model they were estimated for
    DevBuf<double> ebw_num;      // pcl_ebw_hold's copy of `stats`, same layout (model_ebw.hip): the numerator set of pcl_mstep_ebw; gone with the model it was accumulated under
    DevBuf<double> mllt_F;       // MLLT statistics (frame_mllt.hip): the frame side F[Dhost][Dhost][Dhost], full symmetric matrices; gone with the model
    DevBuf<double> mllt_beta;    // [1] their occupancy
    DevBuf<int> mllt_keep;       // [J] pcl_mllt_zero's state_keep on the device (empty: every state is kept) ...
    std::vector<int32_t> mllt_keep_host;   // ... and on the host, for the estimate's walk over the kept states' mixtures
};
// Coarse layout of the off-pipe mixtures (gmm_score_coarse.hip): their bound v_up on the matrix pipe, exact evaluation of what it
// cannot rule out.  Derived on first use after the model changed (coarse_gen != model_gen).
struct CoarseDev {
    DevBuf<unsigned short> pmc;       // [J][Mpad32/32][2][KS8f][64 lanes][8]: the state's bad_idx list, 32 per tile
    DevBuf<float> fscale_c;           // [J][2][KS8f*8]
    DevBuf<double> kzero_c;           // [J]
    DevBuf<float> rows_c;             // [J][Mpad][D][2]: the tight mixtures' direct-form rows (s_d, c_d) in bad_idx order, for the pairs the coarse pass cannot rule out
    DevBuf<float> kgap_c;             // [J]: (the state's largest tight k2) - K0, rounded up (the one-product pass: see EPS1 in gmm_score_coarse.hip)
    DevBuf<double> k2c;               // [J][Mpad] exact log2-domain constant of the idx-th off-pipe mixture
    DevBuf<int> d_nct;                // [J] coarse tiles in use
    DevBuf<unsigned long long> d_coarse_counter;   // PCL_COARSE_STATS=1: pairs evaluated exactly
};
// Unit inventory (hmm_units.hip)
struct UnitsDev {
    DevBuf<double> d_unit_trans;                  // device copy of unit_trans (the transition M-step writes it)
    DevBuf<double> hmm_ksai;                      // per-unit accumulators, LOG domain: [n_units][S-2][S] and, behind them (hmm_gamma), [n_units][S-2]
};
// Pronunciation tree for the decoder (hmm_decode.hip)
struct LexiconDev {
    DevBuf<int> lex_units, lex_nunits, lex_child_ptr, lex_child_idx, lex_word, lex_roots;
    DevBuf<int4> lex_info;                        // per node (first child, children, words end here, unit pair)
    DevBuf<double> d_unit_logtrans;
    // the bigram language model over the tree's words (pcl_lm_upload; DecLm, hmm_decode_common.h): gone with the tree
    DevBuf<double> lm_uni, lm_bow, lm_val;
    DevBuf<long long> lm_row_ptr;
    DevBuf<int> lm_col, lm_node_word_ptr, lm_node_word_ids;
    // the nodes' tied states (pcl_lexicon_tie, tying.hip; DecTie, hmm_decode_common.h): a snapshot of the walks under the tying that was
    // resident then, gone with the tree or with pcl_lexicon_untie
    DevBuf<int> lex_tie_gen;                      // [lex_nodes][2 P] int32, -1 in slot 1 of a one-unit node: node_state as pcl_lexicon_states returns it
    DevBuf<int4> lex_tie_lr;                      // [lex_nodes] the same ids, 16 bits each, for the left-to-right kernel
};

// Resident tying (tying.hip): a decision tree's node arrays in the layouts the walk reads.  Replaced as a whole by pcl_tying_upload, gone with
// pcl_tying_drop, with an inventory of another shape, and with the context.
struct TyingDev {
    DevBuf<int4> ty_nodes;                        // [ty_N] (cand, no, yes, state): one 16-byte load per step of a walk
    DevBuf<unsigned int> ty_qbits;                // [ty_Q][ty_W] bit u of row qi = q_member[qi][u]
    DevBuf<int> ty_root;                          // [n_units * P] root_of
};

// The three resident statistics sets of the frame rows.  Each is made and cleared by its pcl_*_zero (frames loaded: the set takes its width
// D from the frame matrix then) and goes with the next pcl_*_zero that SUCCEEDS and with pcl_destroy, with nothing else: a zero that is
// refused or fails leaves the set in place as it was.  Release is `ctx->lda = {}`.  An entry point asks a set one of two questions, in one
// form (below pcl_ctx): have, was it made, and fits, was it made and at the frame matrix's CURRENT width.  An entry's checks in order:
//   pcl_lda_accumulate          have, frame_class NULL, frames loaded, labels in [-1, R) | the LDA launcher's
//   pcl_batch_accumulate_lda    have, the batch (align_precheck), state_class NULL with J > R | the LDA launcher's
//   the LDA launcher            fits, U / NULL lists, frames loaded, F < 2^31, the spans, state_class in [-1, R)
//   pcl_tree_accumulate         have, frames loaded, fits, F < 2^31 (pcl_tree_accumulate_ready), frame_row NULL, labels in [-1, R) | the spans
//   pcl_batch_accumulate_tree   pcl_tree_accumulate_ready, the batch, R % P, label_event | the spans
//   pcl_cmvn_accumulate         frames loaded, the spans, fits, the speakers (pcl_frames_cmvn: fits, S, the speakers, the rest); the downloads: have (CMVN's: fits)
struct LdaStats {                                 // frame_lda.hip: [R][n][n], the upper triangle of sum [x | 1][x | 1]^T over the class's spliced rows
    static constexpr const char *rule = "lda";
    DevBuf<double> stats;
    int R = 0, left = 0, right = 0, D = 0;
    bool have() const { return stats && R > 0; }
    int Ds() const { return (left + right + 1) * D; }
    int n() const { return Ds() + 1; }
};
struct CmvnStats {                                // frame_cmvn.hip: n [S] rows, sq [S][2][D] = (sum x | sum x^2)
    static constexpr const char *rule = "cmvn";
    DevBuf<long long> n;
    DevBuf<double> sq;
    int S = 0, D = 0;
    bool have() const { return sq && S > 0; }
};
struct TreeStats {                                // tree_cluster.hip: ONE block [n (R) int64 | s (R, D) | q (R, D)]
    static constexpr const char *rule = "tree";
    DevBuf<double> stats;
    int R = 0, D = 0;
    bool have() const { return stats && R > 0; }
    long long *n() const { return reinterpret_cast<long long *>(stats.p); }
    double *s() const { return stats.p + R; }
    double *q() const { return stats.p + (size_t)R * (1 + D); }
};

// The context's own streams (the int16 front-end's staging stream lives with its buffers, PcmStage::stream; pcl_ctx::streams() lists all seven).
struct CtxStreams {
    Stream stream_main;          // the owner of the main stream; launchers read the VIEW pcl_ctx::stream, which pcl_stream_scope redirects
    Stream stream_dp;            // HighPriority: forward-backward runs here, beside the next batch's scoring on the main stream
    Stream stream_aux;           // the accumulate pass's tile-image producer runs here, beside its consumer on the main stream
    Stream stream_desc;          // NonBlocking: descriptor uploads of batches that have nothing in flight (pcl_h2d_fresh)
    Stream stream_d2h;           // NonBlocking: pcl_batch_fetch_async, results travel to the host beside the next step's kernels
    Stream stream_comm;          // NonBlocking, made by the first pcl_pipe_begin: the pipelined exchange (pcl_comm.hip)
};

// TEARDOWN ORDER.  `delete ctx` (ctx_teardown, pcl_api.hip) destroys the members below in reverse order of declaration and then the base
// structs in reverse order, and every one of them gives back what it owns.  One thing in that order is relied upon: CtxStreams is the FIRST
// base, so the streams outlive every buffer, event, timer and staging area of the context (PcmStage keeps the same order for its own
// stream).  Nothing else depends on the order: pcl_destroy has drained every stream before, and the steps whose order IS a decision
// (communicator, buried batches, zero_pending) are spelled out in ctx_teardown.
struct pcl_ctx : CtxStreams, ModelDev, CoarseDev, UnitsDev, LexiconDev, TyingDev {
    int device = 0;
    AccScratch acc;
    hipStream_t stream = nullptr;      // VIEW of stream_main, or of the stream an open pcl_stream_scope has put in its place
    std::string err;
    int cus = 0;
    // model (device)
    int J = 0, M = 0, Mpad = 0, D = 0, Dhost = 0, row = 0;  // D = device (padded) feature dimension
    int model_flags = 0;
    int mllr_R = 0;              // classes of mllr_W
    int fmllr_S = 0;             // speakers of fmllr_Gk / fmllr_beta / fmllr_W
    int Mpad32 = 0;              // M rounded up to a multiple of 32
    int layouts_valid = 0;             // PCL_LAYOUT_* derived for the current model (the f64 rows are derived on first use)
    bool dp_async = true;              // env PCL_DP_STREAM=0: everything on one stream
    int score_wgs_per_cu = 0;    // pcl_score_occupancy: 2 = the matrix-pipe scoring kernel leaves a third of each CU to kernels beside it
    int score_variant = 0;       // 7 = two-piece f16 split on the matrix pipe (default), 3 = f32-input MFMA (strict f32), 1 = direct form on the VALU
    // conditioning of the centred expansion the MFMA kernels use: cond[j] = max_m log2e sum_d (mu - c_j)^2 / (2 var),
    // the magnitude of the terms that cancel in it.  States above cond_max are scored / accumulated by the
    // direct-form VALU kernels instead (f32 error of the expansion ~ 5e-7 * cond nats).
    std::vector<float> cond;             // (host copy of d_cond)
    float cond_max = 96.f;
    // Split states.  The limit is a property of single MIXTURES (one tight mixture far from the state's centre), and after an M-step most states
    // have a few of them (tools/cond_probe.py: 7 % of the mixtures, every state).  A mixture with cond_m > cond_max is therefore taken OUT of
    // the matrix-pipe layouts (written like a zero-weight mixture, left out of the state's feature scales, K0 and cond) and evaluated by the
    // direct-form kernels over the state's compacted list of such mixtures, merged by a log-add (scoring) / added to the statistics
    // (accumulate).  A state goes to the direct-form kernels as a whole only when more than split_max of its mixtures are out.
    bool compact_main = true;          // env PCL_COMPACT_MAIN=0 (read when the context is made): every state keeps derive_kernel's tiles in mixture order, all of them walked (A/B)
    std::vector<int> nbad;
    float split_frac = 0.5f;           // env PCL_SPLIT_MAX: the share of a state's mixtures that may be off the pipe (0 = no splitting)
    bool split_frac_set = false;       // PCL_SPLIT_MAX was given (otherwise: 1.0 for scoring when the coarse pass is available, 0.5 for the accumulate pass)
    int split_max = 0;                 // = split_frac * M: mixtures per state that may be off the pipe (0: no splitting -- whole states, as before round 4)
    int model_gen = 0;           // bumped whenever the layouts (and cond) are re-derived
    // the coarse layout (CoarseDev)
    int coarse_np = 1;                 // env PCL_COARSE_PASSES (read when the context is made): 1 = one f16 product per term, 3 = the two-piece operands' three
    int coarse_gen = -1;
    float coarse_split_frac = 0.99f;   // env PCL_COARSE_SPLIT_MAX: the share of a state's mixtures that may be off the pipe with the coarse pass (see pcl_model_upload)
    bool coarse_stats = false;         // env PCL_COARSE_STATS=1 (read when the context is made): count the pairs evaluated exactly (pcl_coarse_counter)
    bool coarse_on = true;             // env PCL_COARSE=0 (read when the context is made): the direct-form subset launch of rounds 4-5 instead (A/B)
    // the accumulate pass keeps the round 4-5 rule (whole states in direct form above acc_split_max off-pipe mixtures): its subset launch has
    // no coarse pass, and at a high share of off-pipe mixtures the whole-state kernel is the cheaper of its two routes
    int acc_split_max = 0;
    // frames (device)
    int64_t F = 0;
    int FD = 0, FDhost = 0;
    float *frames32 = nullptr;            // VIEW: the current f32 frame matrix -- frames_up (a plain upload, frames_front < 0) or frames_slot[frames_front]
    DevBuf<float> frames_up;
    DevBuf<double> frames64;
    // What was made ON the current frame matrix and is alive for the caller (pcl_batch_create .. pcl_batch_destroy, pcl_seg_create ..
    // pcl_seg_destroy): pcl_frames_splice_project changes the matrix's width under an unchanged row count and refuses while any is left
    int live_batches = 0, live_segs = 0;
    LdaStats lda;                      // the statistics sets of the frame rows (above): each goes with its next pcl_*_zero and with pcl_destroy
    CmvnStats cmvn;
    TreeStats tree;
    // streaming: two frame slots (grow only); pcl_frames_stage copies the next chunk into the slot that is not current on stream_aux,
    // pcl_frames_swap makes it current
    DevBuf<float> frames_slot[2];
    int frames_front = -1, staged_slot = -1, staged_D = 0;
    int64_t staged_F = 0;
    LazyEvent ev_stage, ev_slot_free;
    bool have_slot_free = false;
    // E-step statistics (ModelDev::stats)
    size_t stats_len = 0;
    double *st_acc = nullptr, *st_alpha = nullptr, *st_mean = nullptr, *st_cov = nullptr;   // VIEWS into stats
    DevBuf<double> d_softplus;  // table of log1p(exp(-d)) for the forward-backward recursion (hmm_dp.hip)
    bool stats_fresh = false;
    // pcl_stats_zero clears the block on the auxiliary stream (3.9 GB: 0.58 ms on the main stream in front of every E-step's scoring,
    // which does not touch it); whoever touches the statistics next on the main stream waits for it first (pcl_stats_join)
    LazyEvent ev_zero, ev_zero_src;
    bool zero_pending = false;
    double acc_prune_log2 = -1e300;   // pcl_accumulate_prune: frames with gamma_t(j) below 2^this are left out (default: only exact zeros)    // all zero since pcl_stats_zero: the first accumulate pass may store instead of read-modify-write
    // unit inventory (hmm_units.hip): n_units HMMs of S states, unit i owns GMM states i*(S-2) .. i*(S-2)+S-3
    int n_units = 0, S = 0;
    std::vector<double> unit_trans, unit_logtrans;   // host copies [n_units][S][S]: transmat and np.log(transmat)
    double *hmm_gamma = nullptr;                     // VIEW into hmm_ksai (UnitsDev): [n_units][S-2]
    // pronunciation tree for the decoder (LexiconDev)
    int lex_nodes = 0, lex_nroots = 0;
    std::vector<int> lex_word_host;                  // node_word as uploaded: pcl_lm_upload checks its node -> word lists against it
    std::vector<int> lex_units_host, lex_nunits_host;   // node_units (n, 2) / node_nunits as uploaded: pcl_lexicon_tie checks the centres against them
    int lex_tie_Jt = 0, lex_tie_P = 0;               // J_t and P of the tying the lexicon was tied under (0: not tied)
    int lm_W = 0;                                    // words of the resident language model (0: none)
    // resident tying (TyingDev): ty_N = 0 means none
    int ty_N = 0, ty_Q = 0, ty_W = 0, ty_R0 = 0, ty_Jt = 0, ty_P = 0, ty_units = 0;
    // multi-GPU (pcl_comm.hip): RCCL communicator, or the host-callback rehearsal transport
    void *comm = nullptr;
    int rank = 0, nranks = 1;
    int transport = 0;                               // 0 none, 1 RCCL, 2 host callback (several ranks on ONE device)
    pcl_allgather_fn host_allgather = nullptr;
    void *host_user = nullptr;
    DevBuf<float> payload32;                         // f32 staging of the statistics / parameters (payload = PCL_F32)
    // pipelined exchange (pcl_comm.hip): state chunks go through reduce-scatter -> M-step -> all-gather -> derive on stream_comm
    // as soon as the accumulate pass has queued the last kernel that touches them
    std::vector<LazyEvent> pipe_ev;
    LazyEvent pipe_done;
    bool pipe_active = false;
    int pipe_early = 0;                                            // chunks of the last pipelined call that left while the pass was still running
    int pipe_K = 0, pipe_next = 0, pipe_payload = 0, pipe_mode = 1;   // mode 1: only the reduce-scatter leaves early; 0: the whole chain
    double pipe_c_cov = 0.0;
    std::map<std::string, KernelTimer> timers;
    bool timing = false;         // pcl_timing_enable / env PCL_TIMERS: record HIP events around every launch
    // Batches the caller has destroyed while the GPU was still working on them (a corpus sweep drops the batch of step k - 2 while
    // step k runs): pcl_batch_destroy returns at once; the memory goes back to the pool when the batch's OWN last work on every
    // stream has completed (its events: ev_mark / ev_dp / ev_fetch; pcl_batch_reap on the next create / destroy, pcl_sync, pcl_destroy).
    std::vector<struct pcl_batch *> graves;
    DescStager<> desc;           // descriptor uploads of a batch under construction (pcl_desc_group; pcl_desc.h)
    PcmStage pcm;
    MfccTables mfcc_tab;
    // Every stream of the context, made or not (null): the ONE list behind pcl_destroy's drain.
    std::array<hipStream_t, 7> streams() const { return {stream_main, stream_dp, stream_aux, stream_d2h, stream_desc, stream_comm, pcm.stream}; }
};

// Decoder state of a batch (hmm_decode.hip): token buffers, node -> token map, scratch, results; re-made as a group when a call needs more room
struct BatchDecodeDev {
    DevBuf<double> dec_f64;
    DevBuf<int> dec_slot, dec_work, dec_int;
    DevBuf<double> dec_score;
    int dec_cap = 0, dec_cand = 0, dec_nodes = 0;    // what the buffers were sized for
    DevBuf<int> dec_word;                            // pcl_batch_decode_lm only: [U][Tmax] the chosen word of every history entry
    bool dec_has_words = false;                      // the last decode was pcl_batch_decode_lm
};

// The minimum-Bayes-risk pass of a batch (hmm_mbr.hip; pcl_batch_mbr): its own buffers, made on first use -- nothing pcl_batch_get returns
struct BatchMbrDev {
    DevBuf<double> mbr_beta, mbr_betap;              // beta and beta' under kappa, time-major like `beta`: stored by the backward pass, read by the forward pass
    DevBuf<double> mbr_lgam, mbr_g;                  // ln gamma under kappa and the signed g, time-major: what pcl_batch_mbr_posteriors turns into `lgam`
    DevBuf<double> mbr_logp, mbr_cavg;               // [U]
    DevBuf<int32_t> mbr_ref;                         // [sum T] frame_ref / group (-1 stays -1), uploaded by every pcl_batch_mbr
    bool have_mbr = false;                           // the buffers hold a pass over the batch's CURRENT transitions, states and emissions
};

// The word lattice of a batch's last pcl_batch_decode_lattice (the records: the decode kernels' LAT instantiations; everything else:
// lattice.hip): its own buffers, made on first use and re-made as a group when a call needs more room.  A = max_arcs + candidate arcs and
// NN = Tmax + 3 node slots per utterance.
struct BatchLatDev {
    DevBuf<int> lat_raw_i;                           // [5][U][max_arcs] frame | tok | node | hist | word as the kernels appended them
    DevBuf<double> lat_raw_f;                        // [2][U][max_arcs] score | term
    DevBuf<int> lat_arc_i;                           // [7][U][A] canonical order: frame | tok | node | hist | word | start node | end node
    DevBuf<double> lat_arc_f;                        // [4][U][A] score | term | arc weight under kappa | ln posterior
    DevBuf<int> lat_out_idx;                         // [U][A] the arcs by start node (the counting sort)
    DevBuf<int> lat_node_i;                          // [4][U][NN] in_ptr | out_ptr | Viterbi back-pointer | best path
    DevBuf<double> lat_node_f;                       // [4][U][NN] seed | alpha | beta | Viterbi score
    DevBuf<int> lat_hist_frame;                      // [U][Tmax]
    DevBuf<double> lat_hist_seed;                    // [U][Tmax]
    DevBuf<int> lat_utt_i;                           // [7][U] n_wanted | n_rec | n_arcs | n_nodes (entries) | overflow | status | best_n
    DevBuf<double> lat_utt_f;                        // [2][U] ln Z | best score
    DevBuf<double> lat_conf;                         // [U][NN] the confidence of every word of the best path
    int lat_max_arcs = 0, lat_cand = 0;              // what the buffers were sized for
    bool lat_lm = false;                             // the decode ran with the language model: a word's identity is its word id
    bool have_lat = false;                           // the buffers hold the lattice of the batch's last decode
    bool have_lat_post = false;                      // ... and pcl_batch_lattice_posteriors' results for it
};

// Every device array and event below is the batch's own: `delete b` gives them back (batch_free_now, pcl_batch.hip).
struct pcl_batch : BatchDecodeDev, BatchMbrDev, BatchLatDev {
    pcl_ctx *ctx = nullptr;
    int U = 0;
    // What the host planned for the kernels (batch_plan.h), each the host copy of what the device holds: replaced as a whole by the call
    // that plans it again, and only once the plan has been accepted
    BatchShape shape;              // pcl_batch_create: the utterances' offsets (d_utt)
    TransShape trans;              // pcl_batch_set_transitions / the sentence HMMs of the labels: what the CSR / CSC arrays below look like
    ScorePlan plan;                // pcl_batch_set_states: the row -> state map and the scoring work lists (d_row_state, d_segs, d_dups, d_seg_of_row)
    LabelPlan lab;                 // label-built batches: the labels and per unit the list of its occurrences (occ_ptr / occ_utt / occ_row0)
    int model_J = 0;               // J of the model the state lists were built for
    bool have_trans = false, have_states = false, have_B = false, have_fb = false, have_vit = false, have_post = false;
    bool launched = false;           // a kernel that reads this batch's descriptors may be in flight: their re-upload goes through the main stream
    bool virt_rows_filled = false;   // the constant entry / exit rows of Bt are in place for the current row map
    // device
    DevBuf<UttDesc> d_utt;
    DevBuf<double> Bt, alpha, beta, lgam;
    DevBuf<double> logpi, pi_out, gamma_out, ksai;
    DevBuf<double> logp, qtrace, point;
    DevBuf<int32_t> npass, path;
    DevBuf<int> row_ptr, col_idx;   // CSR (successors)
    DevBuf<double> csr_val;
    DevBuf<int> col_ptr, row_idx;   // CSC (predecessors, ascending source index)
    DevBuf<double> csc_val;
    DevBuf<double> xi_m, xi_s;      // per CSR entry online-LSE state
    // scaled linear-domain forward-backward (hmm_fb_linear.inc): packed exp(B), the int32 exponents of alpha / beta (their
    // mantissas live in `alpha` / `beta`), per utterance the exponent maxima of the range test
    DevBuf<unsigned long long> Bp;
    DevBuf<int> alpha_e, beta_e, fb_kmax;
    DevBuf<double> fb_dump;
    DevBuf<double> fb_part_m;                  // per utterance, sum and wave: the posterior kernel's partial sums (mantissa, exponent)
    DevBuf<int> fb_part_e;
    bool fb_linear = false;                       // the last forward-backward left (mantissa, exponent) pairs in alpha / beta
    DevBuf<unsigned short> bp;                 // Viterbi back-pointers, time-major (t, n)
    DevBuf<int32_t> d_row_state;
    // scoring work lists
    DevBuf<ScoreSeg> d_segs;
    DevBuf<DupRow> d_dups;
    DevBuf<ScoreTile> d_tiles;            // tiles for the precision last scored with (MFMA kernel in MFMA mode)
    std::vector<int> acc_ws, acc_lo, acc_hi, acc_split; // accumulate's state order (well-conditioned first)
    LazyEvent ev_main, ev_dp;   // main stream -> stream_dp hand-over, and back
    bool mark_is_score = false;              // ev_mark sits right behind this batch's last scoring: the second stream may wait for IT instead of a new record on the main stream
    LazyEvent ev_mark;            // the main stream behind the last work this batch queued there (pcl_batch_mark): what pcl_batch_destroy waits for -- not the work later batches queued behind it
    bool dp_pending = false;                 // forward-backward queued on stream_dp and not yet joined
    LazyEvent ev_fetch, ev_fetch_src;   // pcl_batch_fetch_async: copies done / the main stream at the time of the call
    bool fetch_pending = false;              // result copies queued on stream_d2h: the next compute call on this batch waits for them
    DevBuf<int> d_tile_flags;             // split-f16 scoring: per tile, 1 = a scaled feature left the f16 range (rescored)
    DevBuf<ScoreTile> d_tiles_v;          // MFMA mode only: tiles of ill-conditioned states for the VALU kernel
    DevBuf<ScoreTile> d_tiles_s;          // MFMA mode only: tiles of the split states for the subset launch (their off-pipe mixtures)
    DevBuf<ScoreTile> d_tiles_c;          // ... and for the coarse pass (gmm_score_coarse.hip): the same states at the matrix-pipe tile size
    DevBuf<int> d_tile_flags_c;           // coarse pass: per tile, 1 = a scaled feature left the f16 range (the direct-form subset kernel rescored it)
    int n_tiles_c = 0;
    int n_tiles = 0, n_tiles_v = 0, n_tiles_s = 0, tile_frames = 0, tile_gen = -1;
    DevBuf<double> tmp;                   // sumNT staging buffer for layout conversion
    DevBuf<double> nz_tmp;                // nnz staging buffer for the sparse xi download
    DevBuf<int> d_seg_of_row;                 // ScorePlan::seg_of_row (sumN ints)
    bool counted = false;                     // in ctx->live_batches (a batch pcl_batch_create gave out)
    // (the accumulate pass's device work lists and tile images are the CONTEXT's scratch, pcl_ctx::acc; the host staging of its state order is acc_ws ... above)
    // decoder state: BatchDecodeDev
    bool have_dec = false;
    // label-built batches (pcl_batch_create_labels): `lab`, and
    bool from_labels = false;
    std::vector<double> logpi_u;             // ln pi of every state of utterance u (uniform 1/N, AcousticModel.py:1003-1006)
    DevBuf<int> occ_ptr, occ_utt, occ_row0;   // unit -> [occ_ptr[u], occ_ptr[u+1]) -> (utterance, first emitting row)
    DevBuf<int32_t> d_labels;             // the labels on the device and the U + 1 offsets into them: uploaded by the first
    DevBuf<int> d_label_off;              // pcl_batch_align_segments of the batch, kept for the next
    // ... over tied states (pcl_batch_create_labels_tied): the tied state of every (label position, state position), written by the walk
    // when the batch was made and the batch's own from then on -- a later pcl_tying_upload / pcl_tying_drop does not reach it
    bool tied = false;
    int tied_J = 0;                          // J_t of the tying the batch was made with
    DevBuf<int32_t> pos_state;               // [sum L][P]
};

// ---------------------------------------------------------------- the Baum-Welch pass loop's stopping rule and trace
// LHMM.baulm_welch (LHMM.py:539) with quirk Q6, for the four forward-backward kernels of hmm_dp.hip (log domain) and
// hmm_fb_linear*.inc (scaled): one pass = judge(Q of the pass) -> record() -> [finish() and leave | next pass].
struct FbPassRule {
    struct Verdict { bool final_pass, q6; };
    const bool fix_pi;
    const double threshold;
    double q = -INFINITY;                 // Q of the pass before
    int npass = 0;                        // passes the reference would have run so far
    __device__ __forceinline__ FbPassRule(int fix_pi_, double threshold_) : fix_pi(fix_pi_ != 0), threshold(threshold_) {}
    // is the pass that gave qnew the last one?
    __device__ __forceinline__ Verdict judge(double qnew) const {
        const bool natural = !(qnew - q > threshold) || (npass + 1 >= PCL_MAX_PASS);   // LHMM.py:539
        // quirk Q6: with pi locked nothing changes between passes, so the next pass would reproduce this one bit for bit and
        // then stop (Q - Q = 0 <= threshold): this pass's statistics are taken, the pass the reference would have run is reported
        const bool q6 = fix_pi && !natural && threshold >= 0.0 && npass + 1 < PCL_MAX_PASS;
        return {natural || q6, q6};
    }
    // Q of the pass into the utterance's trace (`writer`: the one thread of the workgroup that stores), two slots under Q6
    __device__ __forceinline__ void record(Verdict v, double qnew, double *__restrict__ trace, bool writer) {
        if (writer) trace[npass] = qnew;
        ++npass;
        if (v.q6) {
            if (writer) trace[npass] = qnew;
            ++npass;
        }
        q = qnew;
    }
    // the loop's results behind the final pass (the writer thread alone calls this); unused trace slots are NaN
    __device__ __forceinline__ void finish(double qnew, double *__restrict__ logp_u, int32_t *__restrict__ npass_u, double *__restrict__ trace) const {
        *logp_u = qnew;
        *npass_u = npass;
        for (int k = npass; k < PCL_MAX_PASS; ++k) trace[k] = NAN;
    }
    // The scaled kernels write alpha to HBM only in a pass that can be the last one -- the first with a locked pi (Q6), the third
    // with a free one -- and repeat a pass that ended the loop without its stores (same inputs, same bits).
    __device__ __forceinline__ bool may_be_last() const { return fix_pi || npass >= 2; }
    static __device__ __forceinline__ bool replay(Verdict v, bool stored) { return v.final_pass && !stored; }
};

// ---------------------------------------------------------------- scaled linear-domain forward-backward (hmm_fb_linear.inc)
// value = m 2^e, e an int32 per lane.  Zero lives in the exponent: below LE_PZ a value IS zero; a zero factor (ln 0) adds
// LE_ZADD; sums are floored at LE_FLOOR so that nothing wraps; real exponents stay inside (-LE_LIMIT, LE_LIMIT).
constexpr int LE_ZADD = -(1 << 29);
constexpr int LE_FLOOR = -(1 << 30);
constexpr int LE_PZ = -(1 << 28);
constexpr int LE_LIMIT = 1 << 26;
// does utterance u (T frames) fit the int32 exponents and the packed emission word?  kmax = per utterance a record of
// PCL_FB_KREC ints written by hmm_emis_pack_kernel: max |k| (k = power of two of exp(.)) of the emissions, one per packing
// workgroup [0..7], of ln A [8], of the caller's ln pi [9]; nullptr = the scaled kernels are not in use
constexpr int PCL_FB_KREC = 10;
__device__ __forceinline__ bool pcl_fb_linear_ok(const int *kmax, int u, int T) {
    if (!kmax) return false;
    const int *r = kmax + (size_t)PCL_FB_KREC * u;
    int kb = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) kb = max(kb, r[k]);
    const long long ka = r[8], kp = r[9];
    return kb < 32760 && ((long long)kb + ka + 4) * (long long)(T + 2) + kp < (long long)LE_LIMIT;
}

// ---------------------------------------------------------------- helpers (the error macros, dev_alloc / dev_free and the owning types: pcl_own.h)
inline int pcl_ctx_device(const pcl_ctx *ctx) { return ctx->device; }
// The launchers and their timers read the stream from the context: work for another stream is launched inside one of these.
struct pcl_stream_scope {
    pcl_ctx *ctx;
    hipStream_t keep;
    pcl_stream_scope(pcl_ctx *c, hipStream_t s) : ctx(c), keep(c->stream) { c->stream = s; }
    ~pcl_stream_scope() { ctx->stream = keep; }
    pcl_stream_scope(const pcl_stream_scope &) = delete;
    pcl_stream_scope &operator=(const pcl_stream_scope &) = delete;
};
// Host -> device copy on the context's main stream, complete on return: unlike hipMemcpy (legacy null stream) it does not
// wait for the work of the other streams (a decoder running on the second stream while the next chunk's batch is built).
static inline hipError_t pcl_h2d(pcl_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!bytes) return hipSuccess;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}
// Device -> host copy QUEUED on the main stream: the caller waits for the stream before it reads dst.
static inline hipError_t pcl_d2h_queue(pcl_ctx *ctx, void *dst, const void *src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
}
// Descriptors into a buffer NO queued kernel can be reading (freshly allocated, or any buffer of a batch that has not launched
// anything yet): a stream of their own, so that creating a batch in the middle of a stream of chunks does not wait for the
// scoring kernel that happens to run on the main stream (28 ms per new batch in the C5 pipeline).  Complete at return.
// Inside a pcl_desc_group the array is staged (pcl_desc.h) and copied with the group's other arrays by ONE launch at its end.
hipError_t pcl_desc_launch(pcl_ctx *ctx, const DescCopyArgs &a, const char *pin);   // pcl_api.hip: copy the entries on stream_desc and wait for them
static inline auto pcl_desc_flusher(pcl_ctx *ctx) {
    return [ctx](const DescCopyArgs &a, const char *pin) { return pcl_desc_launch(ctx, a, pin); };
}
static inline hipError_t pcl_h2d_fresh(pcl_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!bytes) return hipSuccess;
    if (!ctx->stream_desc) return pcl_h2d(ctx, dst, src, bytes);
    if (ctx->desc.group > 0) return ctx->desc.stage(dst, src, bytes, pcl_desc_flusher(ctx));
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream_desc);
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream_desc);
}
// Scope of a batch's descriptor uploads: every pcl_h2d_fresh inside is staged; `finish` copies and waits once for all of them
// (the destructor does too, for the error paths).  Groups nest: the outermost one copies.
struct pcl_desc_group {
    pcl_ctx *ctx;
    bool open;
    explicit pcl_desc_group(pcl_ctx *c) : ctx(c), open(true) { ctx->desc.enter(); }
    hipError_t finish() {
        if (!open) return hipSuccess;
        open = false;
        return ctx->desc.leave(pcl_desc_flusher(ctx));
    }
    ~pcl_desc_group() { (void)finish(); }
};

// the main stream behind an asynchronous pcl_stats_zero: called by every entry point that reads or writes the statistics block
static inline hipError_t pcl_stats_join(pcl_ctx *ctx) {
    if (!ctx->zero_pending) return hipSuccess;
    ctx->zero_pending = false;
    return hipStreamWaitEvent(ctx->stream, ctx->ev_zero, 0);
}

// Called at the end of every entry point that queues main-stream work reading or writing the batch's buffers (the auxiliary
// stream's producers are always joined by a main-stream consumer queued behind them).
static inline hipError_t pcl_batch_mark(pcl_batch *b) {
    hipError_t e = b->ev_mark.make();
    if (e != hipSuccess) return e;
    return hipEventRecord(b->ev_mark, b->ctx->stream);
}

// Fewer packets between two scoring launches on the main queue (tools/trace_gaps.py: every event record is a marker the command
// processor handles between the kernels): the recursion on the second stream waits for the event pcl_batch_score left (ev_mark), and
// pcl_batch_fetch_async for the recursion's event, instead of each recording one more on the main stream.  PCL_FEWER_MARKERS=0: as rounds 1-4.
static inline bool pcl_fewer_markers() {
    static const bool on = !(getenv("PCL_FEWER_MARKERS") && atoi(getenv("PCL_FEWER_MARKERS")) == 0);
    return on;
}
// stream_dp behind this batch's main-stream work.  `after_fetch`: result copies of an earlier recursion (pcl_batch_fetch_async) were
// still pending when the caller was entered -- the caller put the MAIN stream behind them, but under the shortcut below stream_dp does
// not follow the main stream's head, so it waits for the copies itself (score -> FB -> fetch_async -> FB again would
// otherwise overwrite lgam / ksai / logp / path under the D2H copies).  The shortcut is good for ONE recursion per scoring: whatever
// the main stream queues on this batch afterwards (the accumulate pass reads lgam) has to be ahead of the next recursion, so the flag
// is consumed here and the next caller records a fresh event on the main stream.
static inline hipError_t pcl_dp_follows_main(pcl_batch *b, bool after_fetch = false) {
    pcl_ctx *ctx = b->ctx;
    hipError_t e;
    if (after_fetch && b->ev_fetch && (e = hipStreamWaitEvent(ctx->stream_dp, b->ev_fetch, 0)) != hipSuccess) return e;
    const bool shortcut = pcl_fewer_markers() && b->mark_is_score && b->ev_mark;
    b->mark_is_score = false;
    if (shortcut) return hipStreamWaitEvent(ctx->stream_dp, b->ev_mark, 0);
    if ((e = b->ev_main.make()) != hipSuccess) return e;
    if ((e = hipEventRecord(b->ev_main, ctx->stream)) != hipSuccess) return e;
    return hipStreamWaitEvent(ctx->stream_dp, b->ev_main, 0);
}

// A recursion of batch `b` (forward-backward, Viterbi, decode) on the second stream: stream_dp goes behind the batch's main-stream work,
// `launch` runs with ctx->stream redirected to it, and ev_dp is left for whoever touches the batch next (batch_join, pcl_batch_fetch_async).
template <typename Launch>
static inline int pcl_run_on_dp_stream(pcl_batch *b, bool after_fetch, Launch launch) {
    pcl_ctx *ctx = b->ctx;
    HIPCHK(ctx, b->ev_dp.make());
    HIPCHK(ctx, pcl_dp_follows_main(b, after_fetch));
    {
        pcl_stream_scope on_dp(ctx, ctx->stream_dp);
        TRY(launch());
    }
    HIPCHK(ctx, hipEventRecord(b->ev_dp, ctx->stream_dp));
    b->dp_pending = true;
    return PCL_OK;
}

// shared by pcl_batch.hip and hmm_units.hip, and below by pcl_batch.hip, pcl_api.hip and hmm_decode.hip (C linkage, internal)
extern "C" {
int pcl_batch_upload_sparse(pcl_batch *b, const SparseTrans &t, const double *logpi);
int pcl_batch_set_states_impl(pcl_batch *b, const int32_t *row_state);
int pcl_batch_reap(pcl_ctx *ctx, bool wait);   // pcl_batch.hip: frees the destroyed batches the GPU is done with (wait: all of them); returns how many are left
int batch_join(pcl_batch *b);                  // pcl_batch.hip: the main stream behind the batch's pending recursion and result copies
int ensure_frames64(pcl_ctx *ctx);             // pcl_api.hip: the float64 copy of the frame matrix, derived on first use
// pcl_api.hip: what pcl_batch_accumulate_exchange and pcl_accumulate_exchange_idle (`who`) need of the context; joins a pending pcl_stats_zero
int exchange_precheck(pcl_ctx *ctx, const char *who, int payload, int n_chunks, int update_transitions);
}

// The one entry into a recursion of batch `b` (forward-backward, Viterbi, decode): on the second stream (pcl_run_on_dp_stream), or with
// PCL_DP_STREAM=0 on the main stream with the batch's mark behind it.  What the three callers do differently is said here.  The last two
// are kept as each caller had them and change nothing today: dp_pending is set, and mark_is_score read, on the second stream's route alone.
enum : unsigned {
    PCL_REC_AFTER_FETCH = 1,     // the recursion rewrites buffers pcl_batch_fetch_async copies from: the main stream, and stream_dp (after_fetch), go behind pending copies
    PCL_REC_JOIN_ON_MAIN = 2,    // main-stream route: batch_join first (Viterbi)
    PCL_REC_RETIRES_MARK = 4     // main-stream route: ev_mark is no longer the scoring's event, mark_is_score goes (forward-backward, Viterbi)
};
template <typename Launch>
static inline int pcl_run_recursion(pcl_batch *b, unsigned how, Launch launch) {
    pcl_ctx *ctx = b->ctx;
    const bool after_fetch = (how & PCL_REC_AFTER_FETCH) && b->fetch_pending;
    if (after_fetch) {
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, b->ev_fetch, 0));
        b->fetch_pending = false;
    }
    if (ctx->dp_async) return pcl_run_on_dp_stream(b, after_fetch, launch);
    if (how & PCL_REC_JOIN_ON_MAIN) TRY(batch_join(b));
    TRY(launch());
    HIPCHK(ctx, pcl_batch_mark(b));
    if (how & PCL_REC_RETIRES_MARK) b->mark_is_score = false;
    return PCL_OK;
}
void pcl_timer_begin(pcl_ctx *ctx, const char *which);
void pcl_timer_end(pcl_ctx *ctx, const char *which);

// ---------------------------------------------------------------- kernel launchers (one per .hip file)
int pcl_launch_score(pcl_ctx *ctx, pcl_batch *b, int precision, const ScoreTile *tiles, int n_tiles);
int pcl_launch_fill_virtual_rows(pcl_ctx *ctx, pcl_batch *b);
int pcl_launch_forward_backward(pcl_ctx *ctx, pcl_batch *b, int fix_pi, double threshold);
int pcl_launch_viterbi(pcl_ctx *ctx, pcl_batch *b, int end_state_back);
// hmm_mbr.hip: the pass's buffers (grow only), the scaled forward-backward with the expected accuracy, and lgam <- ln gamma / ln max(+-g, 0)
int pcl_mbr_reserve(pcl_ctx *ctx, pcl_batch *b);
int pcl_mbr_max_rows();
int pcl_launch_mbr(pcl_ctx *ctx, pcl_batch *b, double kappa, int group);
int pcl_launch_mbr_posteriors(pcl_ctx *ctx, pcl_batch *b, int which);
bool pcl_fb_linear_enabled();                                              // env PCL_FB_LINEAR=0: the log-domain kernels only
int pcl_launch_fb_linear(pcl_ctx *ctx, pcl_batch *b, int fix_pi, double threshold);
int pcl_launch_fb_linear_post(pcl_ctx *ctx, pcl_batch *b);
int pcl_launch_fb_to_log(pcl_ctx *ctx, pcl_batch *b, const double *m, const int *e, double *out);
int pcl_launch_regroup(pcl_ctx *ctx, pcl_batch *b, const int32_t *d_row_unit, int gmm_num, int32_t *d_frame_unit, int32_t *d_frame_k);
int pcl_launch_align_segments(pcl_ctx *ctx, pcl_batch *b, int Lmax, int gmm_num, int32_t *d_frame_state, int32_t *d_dropped);
int pcl_launch_ksai_gather(pcl_ctx *ctx, pcl_batch *b, double *dst);
int pcl_launch_clock_probe(pcl_ctx *ctx, int spin_us, unsigned long long *d_out);
int pcl_launch_accumulate(pcl_ctx *ctx, pcl_batch *b, int precision);
int pcl_launch_fmllr_accumulate(pcl_ctx *ctx, pcl_batch *b, const int32_t *utt_speaker);   // frame_adapt.hip, behind pcl_batch_accumulate_fmllr's checks
void pcl_fmllr_release(pcl_ctx *ctx);                // the fMLLR statistics and estimate (a frame matrix of another dimension)
int pcl_launch_mllt_accumulate(pcl_ctx *ctx, pcl_batch *b, const int32_t *utt_keep);        // frame_mllt.hip, behind pcl_batch_accumulate_mllt's checks
void pcl_mllt_release(pcl_ctx *ctx);                 // the MLLT statistics (a frame matrix of another dimension)
void pcl_accumulate_release(pcl_ctx *ctx);           // the context's accumulate scratch (pcl_model_upload)
// frame_lda.hip, behind the checks of pcl_lda_accumulate / pcl_batch_accumulate_lda: d_src (rows of the frame matrix, on the device) = the
// class of every row, or with state_class (host, J entries) its owner state; -1 = not kept
int pcl_launch_lda_accumulate(pcl_ctx *ctx, const char *who, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *d_src,
                              const int32_t *state_class, int J);
// Readiness of a statistics set (LdaStats, CmvnStats, TreeStats), one form for all three: PCL_OK, or `who` fails with the message
template <typename Set>
static inline int stats_have(pcl_ctx *ctx, const char *who, const Set &set) {
    if (!set.have()) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no statistics: pcl_%s_zero first", who, Set::rule);
    return PCL_OK;
}
template <typename Set>
static inline int stats_fits(pcl_ctx *ctx, const char *who, const Set &set) {
    TRY(stats_have(ctx, who, set));
    if (ctx->FDhost != set.D)
        PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the statistics were made for %d-dimensional frames; the frame matrix now has %d dimensions: pcl_%s_zero again", who, set.D,
                 ctx->FDhost, Set::rule);
    return PCL_OK;
}
static inline int stats_fits(pcl_ctx *ctx, const char *who, const LdaStats &set) {   // (a set that has a context to name as well)
    TRY(stats_have(ctx, who, set));
    if (ctx->FDhost != set.D)
        PCL_FAIL(ctx, PCL_ERR_STATE, "%s: the statistics were made for context (%d, %d) of %d-dimensional frames (order %d); the frame matrix now has %d dimensions: pcl_lda_zero again",
                 who, set.left, set.right, set.D, set.n(), ctx->FDhost);
    return PCL_OK;
}
// tree_cluster.hip, for pcl_batch_accumulate_tree (pcl_batch.hip).  pcl_tree_accumulate_ready: its row of the table at LdaStats.
// pcl_launch_tree_label_rows: the batch's owner map (d_frame_state, unit * P + slice) and the caller's label position -> event list
// (d_label_event, on the device) -> the statistics row of every frame (d_frame_row, set to -1 before); queued on ctx->stream.
// pcl_launch_tree_accumulate: behind the checks of both entries; d_src (F entries on the device) = per frame row a statistics row in [-1, R).
int pcl_tree_accumulate_ready(pcl_ctx *ctx, const char *who);
int pcl_launch_tree_label_rows(pcl_ctx *ctx, pcl_batch *b, const int32_t *d_label_event, int P, const int32_t *d_frame_state, int32_t *d_frame_row);
int pcl_launch_tree_accumulate(pcl_ctx *ctx, const char *who, int U, const int32_t *T, const int64_t *frame_begin, const int32_t *d_src);
// tying.hip.  pcl_launch_tied_label_states, for pcl_batch_create_labels_tied (hmm_units.hip): the batch's labels and their offsets go to the
// device (d_labels / d_label_off), one walk per (label position, k) of the resident tying fills b->pos_state and the row -> state map, which
// comes back to the host (row_state, sum N entries) for pcl_batch_set_states_impl's bookkeeping.  Complete on return.
// pcl_launch_tied_owner, for the label-based entry points (pcl_batch.hip): d_frame_state holds pcl_launch_align_segments' owner map of the
// batch (unit * P + slice, -1 = not kept); every kept frame's entry becomes pos_state[i * P + slice], i = the label position of its path row.
// Queued on ctx->stream.
int pcl_launch_tied_label_states(pcl_ctx *ctx, pcl_batch *b, int32_t *row_state);
int pcl_launch_tied_owner(pcl_ctx *ctx, pcl_batch *b, int P, int32_t *d_frame_state);
void pcl_tying_release(pcl_ctx *ctx);                // the resident tying
void pcl_lexicon_untie_release(pcl_ctx *ctx);        // the lexicon's tied states (tying.hip)
int pcl_launch_transpose(pcl_ctx *ctx, pcl_batch *b, const double *src, double *dst, int to_time_major);
int pcl_score_tile_frames(int D, int precision);
int pcl_launch_score_mfma(pcl_ctx *ctx, pcl_batch *b, const ScoreTile *tiles, int n_tiles);
int pcl_launch_acc16_produce(pcl_ctx *ctx, int first, int ns, int max_tiles, int buf, hipStream_t stream);
int pcl_launch_acc16_consume(pcl_ctx *ctx, int first, int ns, int buf, bool fresh, hipStream_t stream);
size_t pcl_acc16_image_bytes(int D);
int pcl_launch_score_split16(pcl_ctx *ctx, pcl_batch *b, const ScoreTile *tiles, int n_tiles);
int pcl_score_split16_tile_frames();
int pcl_launch_score_fixup(pcl_ctx *ctx, pcl_batch *b, const ScoreTile *tiles, int n_tiles, const int *flags);
int pcl_launch_score_subset(pcl_ctx *ctx, pcl_batch *b, const ScoreTile *tiles, int n_tiles);
int pcl_score_subset_tile_frames(int D);
int pcl_score_mfma_tile_frames();
// The (padded) feature dimensions the matrix-pipe kernels have an instance for: the ONE list behind pcl_score_mfma_supported and every
// per-D switch of those kernels' launchers (largest first, the order those switches always had: it is the order of the kernels in the code objects).
#define PCL_MFMA_DIMS(X) X(47) X(39) X(26) X(13)
inline bool pcl_score_mfma_supported(int D) {
#define PCL_IS_DIM(DD) || D == DD
    return false PCL_MFMA_DIMS(PCL_IS_DIM);
#undef PCL_IS_DIM
}
// Which kernel family scores / accumulates at this precision for a model of (padded) dimension D, numbered like score_variant: the direct
// form on the VALU (also: every f64 pass, every dimension without a matrix-pipe instance), the f32-input MFMA kernels, the split-f16 ones.
enum { PCL_ROUTE_DIRECT = 1, PCL_ROUTE_MFMA32 = 3, PCL_ROUTE_SPLIT16 = 7 };
inline int pcl_route(const pcl_ctx *ctx, int precision, int D) {
    if (precision != PCL_F32 || ctx->score_variant < 3 || !pcl_score_mfma_supported(D)) return PCL_ROUTE_DIRECT;
    return ctx->score_variant == 7 ? PCL_ROUTE_SPLIT16 : PCL_ROUTE_MFMA32;
}
int pcl_launch_dup_rows(pcl_ctx *ctx, pcl_batch *b);
int pcl_launch_derive(pcl_ctx *ctx);
int pcl_launch_derive_range(pcl_ctx *ctx, int j_lo, int j_hi);   // no wait, no generation bump: pcl_derive_finish closes
int pcl_derive_finish(pcl_ctx *ctx);
int pcl_pipe_begin(pcl_ctx *ctx, double c_covariance, int payload, int n_chunks);
int pcl_pipe_progress(pcl_ctx *ctx, int final_below);
int pcl_pipe_finish(pcl_ctx *ctx, int update_transitions);
void pcl_pipe_release(pcl_ctx *ctx);
int pcl_ensure_layouts(pcl_ctx *ctx, int need);
enum { PCL_LAYOUT_P32 = 1, PCL_LAYOUT_P64 = 2, PCL_LAYOUT_PM32 = 4, PCL_LAYOUT_COND = 32, PCL_LAYOUT_PM16F = 128 };
inline bool pcl_state_uses_valu(const pcl_ctx *ctx, int j) {
    if (ctx->cond.empty()) return false;
    if (ctx->split_max > 0 && !ctx->nbad.empty())              // split states: only too many off-pipe mixtures (or constants out of f16 range)
        return ctx->nbad[j] > ctx->split_max || ctx->cond[j] >= 1.0e30f;
    return ctx->cond[j] > ctx->cond_max;
}
inline bool pcl_state_is_split(const pcl_ctx *ctx, int j) { return !ctx->nbad.empty() && ctx->nbad[j] > 0 && !pcl_state_uses_valu(ctx, j); }
// ... and for the accumulate pass (its own limit: see acc_split_max)
inline bool pcl_state_acc_uses_valu(const pcl_ctx *ctx, int j) {
    if (ctx->cond.empty()) return false;
    if (ctx->split_max > 0 && !ctx->nbad.empty()) return ctx->nbad[j] > ctx->acc_split_max || ctx->cond[j] >= 1.0e30f;
    return ctx->cond[j] > ctx->cond_max;
}
inline bool pcl_state_acc_is_split(const pcl_ctx *ctx, int j) { return !ctx->nbad.empty() && ctx->nbad[j] > 0 && !pcl_state_acc_uses_valu(ctx, j); }
bool pcl_coarse_enabled(const pcl_ctx *ctx);
bool pcl_coarse_enabled_for(const pcl_ctx *ctx, int D);   // ... for a model of (padded) dimension D about to be uploaded
int pcl_coarse_tile_frames();
void pcl_coarse_release(pcl_ctx *ctx);
int pcl_ensure_coarse(pcl_ctx *ctx);
int pcl_launch_score_coarse(pcl_ctx *ctx, pcl_batch *b);
int pcl_launch_compact_main(pcl_ctx *ctx, int j_lo, int j_hi);
int pcl_launch_score_subset_flagged(pcl_ctx *ctx, pcl_batch *b, const ScoreTile *tiles, int n_tiles, const int *flags);
inline float pcl_split_threshold(const pcl_ctx *ctx) { return ctx->split_max > 0 ? ctx->cond_max : 3.0e38f; }   // cond_m above this: off the pipe
int pcl_launch_cast(pcl_ctx *ctx, const double *src64, float *f32, double *dst64, size_t n);
int pcl_launch_mstep(pcl_ctx *ctx, double floor_var);
// the held numerator statistics (model_ebw.hip) describe the model they were accumulated under: every pass that makes a new model generation drops them
inline void pcl_ebw_release(pcl_ctx *ctx) { ctx->ebw_num.release(); }
// pcl_stats_download of `block`, a statistics block in the live block's layout (pcl_api.hip); waits for the main stream
int pcl_stats_block_download(pcl_ctx *ctx, const double *block, double *acc, double *alpha_acc, double *mean_acc, double *cov_acc);
int pcl_launch_mstep_range(pcl_ctx *ctx, double floor_var, int j_lo, int j_hi);
int pcl_launch_hmm_acc_merge_prepare(pcl_ctx *ctx, double *top);          // top[i] = acc[i] (copy for the max all-reduce)
int pcl_launch_hmm_acc_merge_scale(pcl_ctx *ctx, const double *top);      // acc[i] = exp(acc[i] - top[i]) (0 where top = -inf)
int pcl_launch_hmm_acc_merge_finish(pcl_ctx *ctx, const double *top);     // acc[i] = top[i] + ln(acc[i])
int pcl_launch_trans_mstep(pcl_ctx *ctx);
void pcl_units_release(pcl_ctx *ctx);
void pcl_comm_release(pcl_ctx *ctx);
void pcl_lexicon_release(pcl_ctx *ctx);
int pcl_launch_pack(pcl_ctx *ctx, const double *src, bool per_dim, double *dst);
extern "C" {   // defined inside pcl_api.hip's extern "C" block; hidden like every symbol the public header does not declare
int pcl_device_dim(int D);                                   // the padded feature dimension the kernels have an instance for (-1: D > 64)
void pcl_frames_adopt(pcl_ctx *ctx, DevBuf<float> &&f32, DevBuf<double> &&f64, int64_t F, int D);   // device-built (F, pcl_device_dim(D)) matrices become the current frames
// pcl_model_upload in two halves, for a model that is MADE on the device (bootstrap.hip): pcl_model_alloc drops the old model, allocates the
// float64 master copy (mean64 / var64 / w64, padded device layout, contents undefined) and every derived buffer, and sets the shape fields;
// the caller fills the master copy on ctx->stream; pcl_model_finish derives the layouts, conditioning and split lists and makes the
// statistics block -- exactly what pcl_model_upload runs after its copy.
int pcl_model_alloc(pcl_ctx *ctx, int J, int M, int D, int flags, const char *who);
int pcl_model_finish(pcl_ctx *ctx);
}
// pcl_seg_create from an owner array that is already on the device (F = ctx->F entries, every one -1 or in [0, J): the CALLER guarantees it,
// nothing is validated here); the array is only read and stays the caller's.  gmm_segment.hip.
int pcl_seg_create_device(pcl_ctx *ctx, int64_t n_frames_total, int J, const int32_t *d_frame_state, pcl_seg **out);
// pcl_seg_create's counting sort alone (gmm_segment.hip): d_key[f] in [0, J) or anything else = not kept -> counts (J, host) and the kept
// rows key by key, each key in ascending row order (*d_order, sum counts entries).  Complete on return.
int pcl_count_sort_device(pcl_ctx *ctx, long long F, int J, const int *d_key, std::vector<int> *counts, DevBuf<int> *d_order);
// The front-end's internal halves (the structs and the one frame geometry: frontend_host.h).  `who` prefixes the error messages.
// mfcc.hip.  pcl_mfcc_check: the arguments, nfft and the frame kernel's LDS need against the device's grant, before anything is allocated.
// pcl_mfcc_device: the (rows, dim) float64 feature matrix of rows `fr` (frame_rows, whole frames), left on the device in *d_out (the
// caller's from then on), complete on return.  int16 samples travel through the context's page-locked staging, double ones are copied from
// the caller's memory as they are; with d_sig the samples stay on the device too (pcl_frontend_pitch reads them again).
int pcl_mfcc_check(pcl_ctx *ctx, const char *who, const SignalView &sig, const MfccSpec &m);
int pcl_mfcc_device(pcl_ctx *ctx, const char *who, const SignalView &sig, const MfccSpec &m, const FrameRows &fr, DevBuf<double> *d_out,
                    DevBuf<unsigned char> *d_sig = nullptr);
// The samples into d_sig, as pcl_mfcc_device sends them.  Returns with the main stream behind the last copy; on a failure the caller drains
// ctx->pcm.stream before it lets d_sig go.
int pcl_signal_upload(pcl_ctx *ctx, const char *who, void *d_sig, const SignalView &sig);
// pitch.hip: the device buffers of one call, and what the caller wants of it
struct PitchWork {
    DevBuf<long long> row_off, sig_off;
    DevBuf<int> frame_utt, lagidx, lag;      // lagidx: the track's lag index (0 = Lmin) per row; lag: in samples, when asked for
    DevBuf<double> g, bal, raw, out;         // bal / raw (rows, L); out (rows, 3) = [v, ln f0, delta ln f0]
    DevBuf<short> bp;                        // (rows, L) back-pointers
    bool nccf_in = false;                    // bal / raw hold the caller's correlations (PCL_PITCH_NCCF_IN): d_sig is not read
    bool want_lag = false;
};
int pcl_pitch_device(pcl_ctx *ctx, const char *who, const PitchGeom &gm, const PitchArgs &a, const SignalView &sig, const FrameRows &fr,
                     const void *d_sig, PitchWork *w);
void pcl_timer_host(pcl_ctx *ctx, const char *which, double ms);   // a host-clock entry of a timer group (only while timing is on)
