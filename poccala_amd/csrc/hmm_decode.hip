// hmm_decode.hip -- frame-synchronous token passing over the pronunciation tree, batched one workgroup per utterance
// (gfx950).  SURVEY.md section 8(a) row A16 and 8(f) rank 3: the decode half of BASELINE config 5.
//
// What is restated from the reference (all of it dead code there: Decoder.py cannot be imported):
//   Token.viterbi        Decoder.py:250-288   first step p = ln pi + B[:,t]; later p_j = max_i(p_i + ln A_ij) + B_j;
//                                              score += max_j p_j; mark = first argmax
//   Token.__init__       Decoder.py:222-236   the token's HMM = AcousticModel.embedded of the node's units
//                                              (AcousticModel.py:957-1014): uniform pi, entry row 0, exit row -inf
//   token_passing        Decoder.py:91-111    one step of every token per frame, finished tokens hand over and go
//   passing_in_word      Decoder.py:114-143   children of the tree node get the finished token's score; a child that
//                                              already has a token takes the score if strictly better and keeps its p
//   pruning              Decoder.py:159-167   nothing below 8 distinct scores; else the int(width (1 - beam)) lowest go
//   transfer             Decoder.py:175-187   the `candidate` best tokens at the end
// and the gaps D1..D5 that had to be filled because the source cannot run (finished <=> best state is the last emitting
// one; tokens keyed by tree node; all first-character nodes start; a finished word re-seeds every first-character node
// with a uniform language model and one history entry per frame; frame semantics "all step, then all hand over") are
// spelled out next to the CPU restatement the parity tests hold this kernel to, bit for bit (include/poccala_hip.h names it).
// The restatement's recursion, pruning, frame loop and in-word hand-over are pinned by golden G14 (those pieces of Decoder.py run
// with a stand-in for its missing import); D1..D5 are the builder's completion of what the source cannot do.
//
// Mapping.  The emissions are the all-state matrix of a scoring batch (rows entry, 0..J-1, exit: pcl_batch_score), time
// major, so a frame's J values are contiguous; the frame's row and the unit matrices (183 x 25 doubles) are staged in
// LDS.  A token is 8 lanes in its step (N = two units x three emitting states + 2 <= 8: lane j holds p_j, two tokens per
// lane group in flight) and one lane in the bookkeeping phases; its state lives in separate arrays (score, p[8], node,
// history, unit pair), so every pass is coalesced.  All float64: scores reach -1e5.  Per frame the workgroup runs
//   step -> donors (finished tokens), the best word-end donor, and the donors' children as ONE flattened list of
//   (donor, target) pairs -> merge / create, a pair per thread (a node with hundreds of children is spread over the
//   workgroup) -> first step of the new tokens -> prune (one pass for the width, the key range and a hashed occupancy map
//   that settles the "8 distinct scores" rule; radix select below the keys' common prefix; ties by token order) ->
//   stable compaction of the small fields into the other set of arrays (the 64 bytes of p stay where the step wrote them:
//   the next step reads them through a source map and writes the other p buffer in the new order),
// with workgroup barriers between phases; ordered prefix sums are a ballot per 64 tokens plus one exchange of 16 wave
// totals.  A tree node has at most one live token and one parent, so no hand-over needs an atomic and the result does not
// depend on timing.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hmm_decode_common.h"

namespace {

#include "hmm_decode_dims.inc"      // DW: threads per workgroup; HB: the radix digit of the pruning select
constexpr int NWV = DW / 64;        // wavefronts per workgroup
constexpr int NS = 8;               // lanes per token = states of its HMM at most
constexpr int TG = DW / NS;         // tokens stepped per pass of the workgroup
constexpr int SEG_LDS = 4096;       // donor segments whose offsets are searched in LDS (more: searched in HBM)

// What a lane (state j = sub of its token) needs of ln A of the embedded HMM (AcousticModel.py:979-989), fixed per thread:
// predecessor i reaches j through entry rc[i] of its unit's (S,S) matrix, or not at all.
struct LaneCtx {
    int e, SS, mypos, myk;
    int rc[NS];                     // entry r S + c of the unit matrix, + 256 when the predecessor sits in the second unit; -1: none
    double lpi1, lpi2;
};

// One step of one token by its 8 lanes (they sit in one wave and run in lockstep).  FIRST: p = ln pi + B[:,t]
// (Decoder.py:270); else the max recursion (:278-283).  best = max_j p_j and fin (D1) come back on every lane.
// TIED: the lane's emission row is 1 + sid, its entry of the node's tied states (DecTie::gen), instead of 1 + unit e + k.
template <bool FIRST, bool TIED>
__device__ __forceinline__ void token_step(const LaneCtx &c, const double *lt, const double *Bs, int up, [[maybe_unused]] int sid, double pold, int sub,
                                           double &pj, double &best, int &fin) {
    const int u0 = up & 0xffff, u1 = (int)((unsigned int)up >> 16);
    const int nu = (u1 == 0xffff) ? 1 : 2, N = c.e * nu + 2;
    double bj = -INFINITY;
    if (sub == 0) bj = 0.0;                                        // entry VirtualState: ln 1 (AcousticModel.py:218)
    else if (sub < N - 1) {                                        // (exit VirtualState: ln 0, :219)
        if constexpr (TIED) bj = Bs[1 + sid];
        else bj = Bs[1 + (c.mypos ? u1 : u0) * c.e + c.myk];
    }
    pj = -INFINITY;
    if (FIRST) {
        if (sub < N) pj = (nu == 1 ? c.lpi1 : c.lpi2) + bj;
    } else {
        double m = -INFINITY;
#pragma unroll
        for (int i = 0; i < NS; ++i) {                             // every lane's old value travels by shuffle
            const double pi = __shfl(pold, i, NS);
            if (i < N - 1 && c.rc[i] >= 0 && sub < N) m = fmax(m, pi + lt[((c.rc[i] & 256) ? u1 : u0) * c.SS + (c.rc[i] & 255)]);
        }
        if (sub < N) pj = m + bj;
    }
    best = pj;
    int arg = (sub < N) ? sub : NS;
#pragma unroll
    for (int o = 1; o < NS; o <<= 1) {                             // max and FIRST argmax over the token's lanes (:263-268)
        const double ob = __shfl_xor(best, o, NS);
        const int oa = __shfl_xor(arg, o, NS);
        if (ob > best || (ob == best && oa < arg)) {
            best = ob;
            arg = oa;
        }
    }
    fin = arg >= N - 2;
}

// tokens [lo, hi) take a step, two per 8-lane group and pass, software-pipelined over the passes: while pass k computes,
// the old p of pass k+1 and the indices of pass k+2 are on their way (the old p of token i sits at src[i] of the other p
// buffer: the compaction at the end of a frame only writes that map).
struct StepTied {
    int nd[2], st[2];               // TIED: the token's node (with the indices) and the lane's tied state (with the old p)
};
struct StepUntied {};
template <bool TIED>
struct StepIn : std::conditional_t<TIED, StepTied, StepUntied> {
    int up[2], at[2];
    double sc[2];
};
template <bool FIRST, bool TIED>
__device__ __forceinline__ void step_range(const LaneCtx &c, const double *lt, const double *Bs, int lo, int hi, const int *up, const double *pin,
                                           const int *src, double *p, double *sc, int *flag, int tk8, int sub, [[maybe_unused]] const int *nd,
                                           [[maybe_unused]] const int *tie) {
    using StepIn = StepIn<TIED>;
    auto fetch = [&](int i0, StepIn &in) {                         // indices, unit pairs, scores of the pass that starts at i0
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const int i = i0 + tk8 + x * TG;
            const bool ok = i < hi;
            in.up[x] = ok ? up[i] : (int)0xffff0000;
            in.at[x] = (!FIRST && ok) ? src[i] : 0;
            in.sc[x] = (ok && sub == 0) ? sc[i] : 0.0;
            if constexpr (TIED) in.nd[x] = ok ? nd[i] : 0;
        }
    };
    auto fetch_p = [&](int i0, StepIn &in, double (&po)[2]) {
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            po[x] = (!FIRST && i0 + tk8 + x * TG < hi) ? pin[(size_t)in.at[x] * NS + sub] : 0.0;
            // (lanes 1 .. 2 e of a token; -1 in the second slot of a one-unit node, which token_step does not use; a pass without a token: node 0)
            if constexpr (TIED) in.st[x] = (sub >= 1 && sub <= 2 * c.e) ? tie[(size_t)in.nd[x] * (2 * c.e) + sub - 1] : 0;
        }
    };
    if (lo >= hi) return;
    StepIn in0, in1, in2;
    double po0[2], po1[2];
    fetch(lo, in0);
    fetch(lo + 2 * TG, in1);
    fetch_p(lo, in0, po0);
    for (int i0 = lo; i0 < hi; i0 += 2 * TG) {
        fetch(i0 + 4 * TG, in2);
        fetch_p(i0 + 2 * TG, in1, po1);
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const int i = i0 + tk8 + x * TG;
            double pj, best;
            int fin;
            int sid = 0;
            if constexpr (TIED) sid = in0.st[x];
            token_step<FIRST, TIED>(c, lt, Bs, in0.up[x], sid, po0[x], sub, pj, best, fin);
            if (i < hi) {
                p[(size_t)i * NS + sub] = pj;
                if (sub == 0) {
                    sc[i] = in0.sc[x] + best;                      // score += max_j p_j (Decoder.py:285)
                    flag[i] = fin;
                }
            }
        }
        in0 = in1;
        in1 = in2;
        po0[0] = po1[0];
        po0[1] = po1[1];
    }
}

// TLDS: the unit matrices and the frame's emission row are staged in LDS (dynamic: (n_units S S + N) doubles).
// Light phases use a wave-blocked ownership of the tokens: wave w owns [w C, (w+1) C), lane l its tokens w C + 64 k + l --
// coalesced, and an ORDERED prefix over the tokens is a ballot per 64 tokens plus one exchange of 16 wave totals.
// KMAX: a lane owns at most KMAX old tokens (cap <= DW KMAX): their sort keys stay in registers through the pruning phase.
#ifdef PCL_DEC_WAVES
#define PCL_DEC_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(PCL_DEC_WAVES, PCL_DEC_WAVES)))
#else
#define PCL_DEC_WAVES_ATTR
#endif
// LM (compile time): rule D6, the bigram language model at word ends (pcl_batch_decode_lm; hmm_decode_common.h) -- a word-end donor's
// offer to the roots is its score plus pcl_lm_word_term, the chosen word goes into the history beside the node.  LM = false is
// pcl_batch_decode's kernel and does not read `lm`.  As for the left-to-right kernel, the LM = true instantiations are compiled in a
// translation unit of their own (hmm_decode_lm.hip defines PCL_DEC_LM and includes this file), so the LM = false ones come out as they
// did before there was a switch.
// TIED (compile time): a lane's emission row comes from its node's tied states (pcl_batch_decode_tied; DecTie, hmm_decode_common.h),
// gathered in the step by the token's node id; TIED = false reads nothing of `tie`.  The TIED = true instantiations (with and without LM)
// have a translation unit of their own too: hmm_decode_tied.hip defines PCL_DEC_TIED and includes this file.
// LAT (compile time): the word lattice's records (pcl_batch_decode_lattice; DecLat, hmm_decode_common.h, states the rule): the donor phase
// sees every word-end donor, and thread 0 the frame's entry.  LAT = false reads nothing of `lat`; all four (LM, TIED) combinations of
// LAT = true are in hmm_decode_lat.hip, which defines PCL_DEC_LAT and includes this file.
template <bool TLDS, int KMAX, bool LM, bool TIED, bool LAT>
__global__ __launch_bounds__(DW) PCL_DEC_WAVES_ATTR void hmm_decode_kernel(DecArgs a, DecLmArg<LM> lm, DecTieArg<TIED> tie, DecLatArg<LAT> lat) {
    extern __shared__ double dyn[];
    __shared__ int seg_l[SEG_LDS + 1];
    __shared__ unsigned int hist256[256];                          // pruning: the occupancy map, then the radix histogram
    __shared__ int wsum[2][NWV];
    __shared__ double red_d[NWV];
    __shared__ unsigned long long red_u[2][NWV];
    __shared__ int red_i[2][NWV];
    __shared__ unsigned long long s_sel;                           // pruning select: the chosen bin (pcl_select_kth's s_key)
    __shared__ int s_i[4];                                         // [0..2] the donor phase's winner; [3] the select's rank
    __shared__ double s_d[1];
    [[maybe_unused]] __shared__ int lat_cnt;                       // LAT: the utterance's word-end donors so far
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const UttDesc d = a.utts[u];
    const int T = d.T, Nb = d.N, cap = a.cap;
    const double *B = a.Bt + d.b_off;
    double *scb[2] = {a.score + (size_t)u * 2 * cap, a.score + ((size_t)u * 2 + 1) * cap};
    double *pb[2] = {a.p + (size_t)u * 2 * cap * NS, a.p + ((size_t)u * 2 + 1) * cap * NS};
    int *ndb[2] = {a.node + (size_t)u * 2 * cap, a.node + ((size_t)u * 2 + 1) * cap};
    int *hsb[2] = {a.hist + (size_t)u * 2 * cap, a.hist + ((size_t)u * 2 + 1) * cap};
    int *upb[2] = {a.upair + (size_t)u * 2 * cap, a.upair + ((size_t)u * 2 + 1) * cap};
    int *flag = a.flag + (size_t)u * cap, *src = a.dst + (size_t)u * cap;
    int *seg_ofs = a.seg_ofs + (size_t)u * (cap + 2), *seg_cptr = a.seg_cptr + (size_t)u * (cap + 2), *seg_hist = a.seg_hist + (size_t)u * (cap + 2);
    double *seg_score = a.seg_score + (size_t)u * (cap + 2);
    int *slot = a.slot + (size_t)u * a.n_nodes;
    int *hprev = a.hist_prev + (size_t)u * a.Tmax, *hnode = a.hist_node + (size_t)u * a.Tmax;
    // LM: the chosen word of every history entry (thread 0 writes it in the donor phase; donors of later frames read it, behind the
    // barriers in between).  The waves' winning words borrow red_u[1]'s slots: the pruning phase's, idle in the donor phase.
    [[maybe_unused]] int *hword = nullptr, *w_word = (int *)red_u[1];
    if constexpr (LM) hword = lm.hist_word + (size_t)u * a.Tmax;
    const int tk8 = tid >> 3, sub = tid & 7;                       // token group of 8 lanes

    LaneCtx c;
    c.e = a.S - 2;
    c.SS = a.S * a.S;
    c.mypos = (sub == 0) ? 0 : (sub - 1) / c.e;
    c.myk = (sub == 0) ? 0 : (sub - 1) % c.e;
    c.lpi1 = a.lpi1;
    c.lpi2 = a.lpi2;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int pos = (i == 0) ? 0 : (i - 1) / c.e, r = (i == 0) ? 0 : 1 + (i - 1) % c.e, col = sub - pos * c.e;
        c.rc[i] = (col >= 0 && col < a.S) ? (r * a.S + col) | (pos ? 256 : 0) : -1;
    }
    const double *lt;
    double *Bs_l = nullptr;
    if (TLDS) {
        for (int k = tid; k < a.n_units * c.SS; k += DW) dyn[k] = a.unit_logtrans[k];
        lt = dyn;
        Bs_l = dyn + a.n_units * c.SS;
    } else {
        lt = a.unit_logtrans;
    }
    auto pack_units = [&](int node) -> int {
        const int u0 = a.node_units[2 * node];
        const int u1 = (a.node_nunits[node] == 2) ? a.node_units[2 * node + 1] : 0xffff;
        return u0 | (u1 << 16);
    };
    [[maybe_unused]] const int *tie_gen = nullptr;
    if constexpr (TIED) tie_gen = tie.gen;
    STAMP_BEGIN

    // ---- frame 0: every first-character node starts (D3)
    if (tid < 256) hist256[tid] = 0u;                              // (the pruning steps take it zero and leave it zero)
    if constexpr (LAT) {
        if (tid == 0) lat_cnt = 0;                                 // (the barriers of frame 0 come before the first append)
    }
    int cur = 0, n = min(a.n_roots, cap), ovf = a.n_roots > cap, nh = 0;
    for (int i = tid; i < n; i += DW) {
        const int node = a.roots[i];
        ndb[0][i] = node;
        hsb[0][i] = -1;
        scb[0][i] = 0.0;
        upb[0][i] = pack_units(node);
        slot[node] = i;
    }
    if (TLDS)
        for (int k = tid; k < Nb; k += DW) Bs_l[k] = B[k];
    __syncthreads();
    step_range<true, TIED>(c, lt, TLDS ? Bs_l : B, 0, n, upb[0], nullptr, nullptr, pb[0], scb[0], flag, tk8, sub, ndb[0], tie_gen);
    for (int i = tid; i < n; i += DW) src[i] = i;
    __syncthreads();
    if (tid == 0) a.trace[(size_t)u * a.Tmax] = n;
    int pcur = 0;                                                  // the p buffer the tokens' values are in (at src[])

    for (int t = 1; t < T; ++t) {
        double *sc = scb[cur], *p = pb[pcur ^ 1];
        const double *pin = pb[pcur];
        int *nd = ndb[cur], *hs = hsb[cur], *up = upb[cur];
        const double *Bf = B + (size_t)t * Nb;
        if (TLDS) {
            for (int k = tid; k < Nb; k += DW) Bs_l[k] = Bf[k];
            __syncthreads();
        }
        const double *Bs = TLDS ? Bs_l : Bf;
        const int C = ((n + DW - 1) / DW) * 64, w0 = wave * C;     // this frame's ownership of the old tokens
        // ---- (1) every live token takes its step
        step_range<false, TIED>(c, lt, Bs, 0, n, up, pin, src, p, sc, flag, tk8, sub, nd, tie_gen);
        __syncthreads();
        STAMP(0)
        // ---- (2) donors = finished tokens.  The best finished word-end token (earliest on ties) re-seeds the first
        //      characters (D4); first_w = the first finished word-end token: the roots are created right after its children
        int nd_cnt = 0, ch_cnt = 0, bw_i = NONE, fw = NONE;
        [[maybe_unused]] int bw_word = 0;
        double bw = -INFINITY;
        for (int k = 0; k < C; k += 64) {
            const int i = w0 + k + lane;
            [[maybe_unused]] bool rec = false;                     // LAT: this lane's token is a word-end donor, and its record
            [[maybe_unused]] int r_node = 0, r_hist = 0, r_word = 0;
            [[maybe_unused]] double r_score = 0.0, r_term = 0.0;
            if (i < n && (flag[i] & 1)) {
                const int node = nd[i];
                ++nd_cnt;
                ch_cnt += a.child_ptr[node + 1] - a.child_ptr[node];
                if (a.node_word[node]) {
                    fw = min(fw, i);
                    double s = sc[i];
                    [[maybe_unused]] int wsel = 0;
                    if constexpr (LAT) {
                        rec = true;
                        r_node = node;
                        r_hist = hs[i];
                        r_score = s;
                    }
                    if constexpr (LM) {                            // D6: the offer to the roots
                        const double term = pcl_lm_word_term(lm, hword, hs[i], node, wsel);
                        if constexpr (LAT) {
                            r_term = term;
                            r_word = wsel;
                        }
                        s += term;
                    }
                    if (bw_i == NONE || s > bw) {                  // (a thread's tokens come in ascending order)
                        bw = s;
                        bw_i = i;
                        if constexpr (LM) bw_word = wsel;
                    }
                }
            }
            if constexpr (LAT) {                                   // (C is the workgroup's: every lane of the wave is here)
                const unsigned long long rmask = __ballot(rec);
                if (rmask != 0ull) pcl_lat_record(lat, u, pcl_lat_place(&lat_cnt, rmask, rec), t, i, r_node, r_hist, r_score, r_term, r_word);
            }
        }
        nd_cnt = pcl_wave_sum(nd_cnt);
        ch_cnt = pcl_wave_sum(ch_cnt);
        if constexpr (LM) pcl_wave_best(bw, bw_i, bw_word);
        else pcl_wave_best(bw, bw_i);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) fw = min(fw, __shfl_xor(fw, o, 64));
        if (lane == 0) {
            wsum[0][wave] = nd_cnt;
            wsum[1][wave] = ch_cnt;
            red_d[wave] = bw;
            red_i[0][wave] = bw_i;
            red_i[1][wave] = fw;
            if constexpr (LM) w_word[wave] = bw_word;
        }
        __syncthreads();
        if (tid == 0) {
            double b;
            int bi, f = NONE;
            pcl_best_of_waves<NWV>(red_d, red_i[0], b, bi);
            for (int w = 0; w < NWV; ++w) f = min(f, red_i[1][w]);
            s_d[0] = b;
            s_i[0] = bi;
            s_i[1] = f;
            s_i[2] = -1;
            if (bi != NONE) {                                      // one history entry per frame: the winning donor's word
                if (nh < a.Tmax) {
                    hprev[nh] = hs[bi];
                    hnode[nh] = nd[bi];
                    if constexpr (LM) {
                        for (int w = 0; w < NWV; ++w)
                            if (red_i[0][w] == bi) hword[nh] = w_word[w];   // (the wave the winner came from: token indices are unique)
                    }
                    if constexpr (LAT) pcl_lat_entry(lat, u, a.Tmax, nh, t, b);
                }
                s_i[2] = nh;
            }
        }
        int nd_tot, ch_tot;
        const int dbase = pcl_waves_before<NWV>(wsum[0], wave, &nd_tot), cbase = pcl_waves_before<NWV>(wsum[1], wave, &ch_tot);
        __syncthreads();
        const double w_score = s_d[0];
        const int w_i = s_i[0], first_w = s_i[1], w_hist = s_i[2];
        const bool has_w = w_i != NONE;
        if (has_w) ++nh;
        // the frame's hand-overs as ONE flattened list of (donor, target) pairs in the order the restated rules create
        // tokens: donors in token order, each donor's children in child order, the first characters as the children of a
        // pseudo-donor right behind the first word-end donor.  seg_ofs = where each donor's pairs start.
        const int nseg = nd_tot + (has_w ? 1 : 0), Q = ch_tot + (has_w ? a.n_roots : 0);
        const bool use_l = nseg <= SEG_LDS;
        {
            int drun = dbase, crun = cbase;
            for (int k = 0; k < C; k += 64) {
                const int i = w0 + k + lane;
                const bool fin = i < n && (flag[i] & 1);
                int cptr = 0, cnt = 0;
                if (fin) {
                    const int node = nd[i];
                    cptr = a.child_ptr[node];
                    cnt = a.child_ptr[node + 1] - cptr;
                }
                const unsigned long long mask = __ballot(fin);
                const int r = drun + __popcll(mask & lt_mask);
                const int inc = pcl_wave_scan(cnt, lane);
                if (fin) {
                    const int after = (has_w && i > first_w) ? 1 : 0, seg = r + after;
                    const int ofs = crun + inc - cnt + (after ? a.n_roots : 0);
                    seg_ofs[seg] = ofs;
                    if (use_l) seg_l[seg] = ofs;
                    seg_cptr[seg] = cptr;
                    seg_hist[seg] = hs[i];
                    seg_score[seg] = sc[i];
                    if (has_w && i == first_w) {
                        seg_ofs[seg + 1] = ofs + cnt;
                        if (use_l) seg_l[seg + 1] = ofs + cnt;
                        seg_cptr[seg + 1] = -1;
                        seg_hist[seg + 1] = w_hist;
                        seg_score[seg + 1] = w_score;
                    }
                }
                drun += __popcll(mask);
                crun += __shfl(inc, 63, 64);
            }
        }
        __syncthreads();
        STAMP(1)
        // ---- (3) merges and creations, one pair per thread (passing_in_word, Decoder.py:114-143).  A target is "live"
        //      when its node has a token that did not finish in this frame: it keeps its recursion and takes the score if
        //      strictly better (:126-134); otherwise a new token is made behind the old ones, in pair order.
        int created = 0;
        for (int q0 = 0; q0 < Q; q0 += DW) {
            const int q = q0 + tid;
            bool isnew = false;
            int child = 0, dh = 0;
            double ds = 0.0;
            if (q < Q) {
                int lo = 0, hi = nseg;                             // the last segment that starts at or before q
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const int v = use_l ? seg_l[mid] : seg_ofs[mid];
                    if (v <= q) lo = mid + 1;
                    else hi = mid;
                }
                const int seg = lo - 1, o = use_l ? seg_l[seg] : seg_ofs[seg], cptr = seg_cptr[seg];
                ds = seg_score[seg];
                dh = seg_hist[seg];
                child = (cptr < 0) ? a.roots[q - o] : a.child_idx[cptr + q - o];
                const int s = slot[child];
                if (s >= 0 && !(flag[s] & 1)) {
                    if (ds > sc[s]) {
                        sc[s] = ds;
                        hs[s] = dh;
                    }
                } else {
                    isnew = true;
                }
            }
            const unsigned long long mask = __ballot(isnew);
            if (lane == 0) wsum[0][wave] = __popcll(mask);
            __syncthreads();
            int tot;
            const int base = pcl_waves_before<NWV>(wsum[0], wave, &tot);
            if (isnew) {
                const int pos = n + created + base + __popcll(mask & lt_mask);
                if (pos < cap) {                                   // (slots n .. cap-1 of the current buffer)
                    nd[pos] = child;
                    hs[pos] = dh;
                    sc[pos] = ds;
                    up[pos] = pack_units(child);
                }
            }
            created += tot;
            __syncthreads();
        }
        const int n_new = min(created, cap - n);
        if (created > cap - n) ovf = 1;
        STAMP(2)
        // the new tokens take their first step at once (Decoder.py:138-139)
        step_range<true, TIED>(c, lt, Bs, n, n + n_new, up, nullptr, nullptr, p, sc, flag, tk8, sub, nd, tie_gen);
        STAMP(3)
        // ---- (4) pruning over the tokens that were alive before the frame and did not finish (Decoder.py:159-167): the four steps
        //      of hmm_decode_common.h; the radix histogram is the occupancy map's 256 words
        unsigned long long keys[KMAX];
#pragma unroll
        for (int kk = 0; kk < KMAX; ++kk) {
            const int i = w0 + kk * 64 + lane;
            keys[kk] = (kk * 64 < C && i < n && !(flag[i] & 1)) ? pcl_okey(sc[i]) : NOKEY;
        }
        int n_old, bins;
        unsigned long long kmin, kmax;
        pcl_prune_stats<DW, KMAX>(keys, hist256, wsum[0], red_u[0], red_u[1], n_old, kmin, kmax, bins);
        const int m = (int)((double)n_old * (1.0 - a.beam));                   // int(width * (1 - beam))
        bool prune = m > 0 && n_old >= a.min_distinct;
        if (prune && bins < a.min_distinct) prune = pcl_prune_distinct<DW, KMAX>(keys, a.min_distinct, red_u[0], red_i[0]);
        if (prune) {
            unsigned long long sel;
            int rank;
            pcl_select_kth<DW, KMAX, HB, 0>(keys, kmin, kmax, m, hist256, nullptr, red_i[1], &s_sel, &s_i[3], sel, rank);
            const unsigned int gone = pcl_prune_mark<DW, KMAX>(keys, sel, rank, wsum[1]);
#pragma unroll
            for (int kk = 0; kk < KMAX; ++kk)
                if ((gone >> kk) & 1u) flag[w0 + kk * 64 + lane] |= 2;
        }
        __syncthreads();
        STAMP(4)
        // ---- (5) stable compaction: the survivors of the old tokens, then the new ones; the node -> token map follows
        double *scn = scb[cur ^ 1];
        int *ndn = ndb[cur ^ 1], *hsn = hsb[cur ^ 1], *upn = upb[cur ^ 1];
        int keep_cnt = 0;
        for (int k = 0; k < C; k += 64) {
            const int i = w0 + k + lane;
            if (i < n) {
                if (flag[i] & 3) {
                    const int node = nd[i];
                    if (slot[node] == i) slot[node] = -1;
                } else {
                    ++keep_cnt;
                }
            }
        }
        keep_cnt = pcl_wave_sum(keep_cnt);
        if (lane == 0) wsum[1][wave] = keep_cnt;
        __syncthreads();
        int n_keep;
        int krun = pcl_waves_before<NWV>(wsum[1], wave, &n_keep);
        for (int k = 0; k < C; k += 64) {
            const int i = w0 + k + lane;
            const bool keep = i < n && !(flag[i] & 3);
            const unsigned long long mask = __ballot(keep);
            {
                if (keep) {
                    const int to = krun + __popcll(mask & lt_mask);
                    const int node = nd[i];
                    scn[to] = sc[i];
                    ndn[to] = node;
                    hsn[to] = hs[i];
                    upn[to] = up[i];
                    src[to] = i;                                   // where the token's p sits in this frame's p buffer
                    slot[node] = to;
                }
            }
            krun += __popcll(mask);
        }
        for (int j = tid; j < n_new; j += DW) {
            const int i = n + j, to = n_keep + j, node = nd[i];
            scn[to] = sc[i];
            ndn[to] = node;
            hsn[to] = hs[i];
            upn[to] = up[i];
            src[to] = i;
            slot[node] = to;
        }
        __syncthreads();
        STAMP(5)
        n = n_keep + n_new;
        cur ^= 1;
        pcur ^= 1;
        if (tid == 0) a.trace[(size_t)u * a.Tmax + t] = n;
    }
    // ---- transfer (Decoder.py:175-187): the tokens sit where their index says; the flags are free now
    const size_t o_out = (size_t)u * a.candidate;
    const int n_out = pcl_transfer<DW>(n, a.candidate, scb[cur], ndb[cur], hsb[cur], [](int i) { return i; }, flag, red_d, red_i[0],
                                       a.out_node + o_out, a.out_score + o_out, a.out_hist + o_out);
    if (tid == 0) {
        a.out_n[u] = n_out;
        a.hist_n[u] = min(nh, a.Tmax);
        a.overflow[u] = ovf;
        if constexpr (LAT) lat.n_wanted[u] = lat_cnt;              // (behind the transfer's barriers: every append is in)
    }
    STAMP_END(a.stamps)
}

// The launch of one (LM, TIED) pair of instantiations, for the three translation units that hold them.
template <bool LM, bool TIED, bool LAT = false>
int dec_launch_kernel(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLmArg<LM> &lma, const DecTieArg<TIED> &tie, const DecLatArg<LAT> &lat = {}) {
    // the unit matrices and one emission row in LDS when they fit beside the kernel's static 18 KB
    const size_t table_bytes = ((size_t)ctx->n_units * ctx->S * ctx->S + (size_t)n_rows) * sizeof(double);
    const bool tlds = table_bytes <= 44u * 1024u;
    const int cap = a.cap;
#define PCL_DEC_LAUNCH(K)                                                                                                                  \
    do {                                                                                                                                   \
        if (tlds) hipLaunchKernelGGL((hmm_decode_kernel<true, K, LM, TIED, LAT>), dim3(U), dim3(DW), table_bytes, ctx->stream, a, lma, tie, lat);   \
        else hipLaunchKernelGGL((hmm_decode_kernel<false, K, LM, TIED, LAT>), dim3(U), dim3(DW), 0, ctx->stream, a, lma, tie, lat);                  \
    } while (0)
    if (cap <= DW) PCL_DEC_LAUNCH(1);
    else if (cap <= 2 * DW) PCL_DEC_LAUNCH(2);
    else if (cap <= 4 * DW) PCL_DEC_LAUNCH(4);
    else if (cap <= 8 * DW) PCL_DEC_LAUNCH(8);
    else PCL_DEC_LAUNCH(16);
#undef PCL_DEC_LAUNCH
    static_assert(PCL_DEC_MAX_KEYS_PER_LANE == 16, "the largest KMAX instantiated above");
    return PCL_OK;
}

#if defined(PCL_DEC_LAT)
}  // namespace
int pcl_decode_general_launch_lat(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm *lm, const DecTie *tie, const DecLat &lat) {
    if (tie) return lm ? dec_launch_kernel<true, true, true>(ctx, a, U, n_rows, *lm, *tie, lat) : dec_launch_kernel<false, true, true>(ctx, a, U, n_rows, DecNoLm{}, *tie, lat);
    return lm ? dec_launch_kernel<true, false, true>(ctx, a, U, n_rows, *lm, DecNoTie{}, lat)
              : dec_launch_kernel<false, false, true>(ctx, a, U, n_rows, DecNoLm{}, DecNoTie{}, lat);
}
#elif defined(PCL_DEC_TIED)
}  // namespace
int pcl_decode_general_launch_tied(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm *lm, const DecTie &tie) {
    return lm ? dec_launch_kernel<true, true>(ctx, a, U, n_rows, *lm, tie) : dec_launch_kernel<false, true>(ctx, a, U, n_rows, DecNoLm{}, tie);
}
#elif defined(PCL_DEC_LM)
}  // namespace
int pcl_decode_general_launch_lm(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm &lma) {
    return dec_launch_kernel<true, false>(ctx, a, U, n_rows, lma, DecNoTie{});
}
#else
// ---- host side of pcl_batch_decode

// The decoder's workspace, described ONCE: the element counts of the batch's allocations and the offset of every array in them.
// The same DecLayout sizes the allocations, fills DecArgs and tells pcl_batch_decode_get where the results are; the per-utterance
// extents below ([2][cap], [cap + 2], ...) are the kernels' own indexing (DecArgs, hmm_decode_common.h).  The counts do not depend
// on the kernel: of the 8 cap ints per utterance behind upair the general kernel makes flag [cap] | dst [cap], the left-to-right
// kernel src [2][cap] (DecArgs::dst) and no flags -- so a batch may change kernels between two calls.
struct DecLayout {
    static constexpr size_t ABSENT = ~(size_t)0;
    size_t n_f64, n_work, n_int;                                               // doubles in dec_f64, ints in dec_work, ints in dec_int
    size_t score, p, seg_score;                                                // dec_f64
    size_t node, hist, upair, flag, dst, seg_ofs, seg_cptr, seg_hist;          // dec_work
    size_t out_n, out_node, out_hist, hist_n, hist_prev, hist_node, trace, overflow;   // dec_int, in the order they are downloaded
};

DecLayout dec_layout(int U, int cap, int candidate, int Tmax, bool use_lr) {
    const size_t u = (size_t)U, tok = u * cap, seg = u * ((size_t)cap + 2), out = u * candidate, frm = u * Tmax;
    DecLayout l;
    size_t end = 0;
    auto take = [&end](size_t n) {
        const size_t at = end;
        end += n;
        return at;
    };
    l.score = take(2 * tok);
    l.p = take(2 * tok * NS);                                                  // (the left-to-right kernel: 6 of the 8 cap per buffer)
    l.seg_score = take(seg);
    l.n_f64 = end;
    end = 0;
    l.node = take(2 * tok);
    l.hist = take(2 * tok);
    l.upair = take(2 * tok);
    l.flag = use_lr ? DecLayout::ABSENT : take(tok);
    l.dst = take(use_lr ? 2 * tok : tok);
    l.seg_ofs = take(seg);
    l.seg_cptr = take(seg);
    l.seg_hist = take(seg);
    l.n_work = end;
    end = 0;
    l.out_n = take(u);
    l.out_node = take(out);
    l.out_hist = take(out);
    l.hist_n = take(u);
    l.hist_prev = take(frm);
    l.hist_node = take(frm);
    l.trace = take(frm);
    l.overflow = take(u);
    l.n_int = end;
    return l;
}

// tied: pcl_batch_decode_tied -- the rows are those of the J_t tied states the lexicon was tied under, and so must the resident model's be
int dec_validate(const pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, bool tied) {
    pcl_ctx *ctx = b->ctx;
    if (!ctx->lex_nodes) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_decode: pcl_lexicon_upload first");
    if (tied && !ctx->lex_tie_Jt) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_decode_tied: the lexicon is not tied (pcl_lexicon_tie first)");
    if (tied && ctx->J != ctx->lex_tie_Jt)
        PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_decode_tied: the resident model has %d states, the lexicon was tied under J_t = %d", ctx->J, ctx->lex_tie_Jt);
    if (!b->have_B) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_decode: no emissions (pcl_batch_score first)");
    if (!(beam > 0.0 && beam <= 1.0) || min_distinct < 1 || candidate < 1 || max_tokens < 1)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_decode: beam %g, min_distinct %d, candidate %d, max_tokens %d", beam, min_distinct, candidate, max_tokens);
    // the general kernel's limit: it takes every unit inventory, so what it cannot hold nothing can (the left-to-right kernel's smaller
    // workgroup holds half as many: pcl_decode_lr_applicable)
    if (max_tokens > PCL_DEC_MAX_KEYS_PER_LANE * DW)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_decode: max_tokens %d > %d (a lane keeps the sort keys of its tokens in registers)", max_tokens, PCL_DEC_MAX_KEYS_PER_LANE * DW);
    // the emission rows must be [entry, state 0 .. J-1, exit]: the all-state matrix
    const int J = tied ? ctx->lex_tie_Jt : ctx->n_units * (ctx->S - 2);
    for (int u = 0; u < b->U; ++u) {
        const UttDesc &d = b->shape.utt[u];
        bool ok = d.N == J + 2 && (int)b->plan.row_state.size() >= d.vec_off + d.N;
        for (int n = 0; ok && n < d.N; ++n) ok = b->plan.row_state[d.vec_off + n] == (n == 0 ? PCL_ROW_ENTRY : n == d.N - 1 ? PCL_ROW_EXIT : n - 1);
        if (!ok && tied)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_decode_tied: utterance %d is not an all-state batch of J_t + 2 = %d rows (entry, 0..%d, exit)", u, J + 2, J - 1);
        if (!ok) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_decode: utterance %d is not an all-state batch (rows entry, 0..%d, exit)", u, J - 1);
    }
    return PCL_OK;
}

// the batch's buffers, sized for (cap, candidate, tree); the node -> token map and the results start clean for every call
int dec_ensure_workspace(pcl_batch *b, const DecLayout &l, int cap, int candidate) {
    pcl_ctx *ctx = b->ctx;
    const size_t n_slot = (size_t)b->U * ctx->lex_nodes;
    if (b->dec_cap != cap || b->dec_cand != candidate || b->dec_nodes != ctx->lex_nodes) {
        static_cast<BatchDecodeDev &>(*b) = {};
        TRY(b->dec_f64.alloc(ctx, l.n_f64));
        TRY(b->dec_work.alloc(ctx, l.n_work));
        TRY(b->dec_slot.alloc(ctx, n_slot));
        TRY(b->dec_int.alloc(ctx, l.n_int));
        TRY(b->dec_score.alloc(ctx, (size_t)b->U * candidate));
        b->dec_cap = cap;
        b->dec_cand = candidate;
        b->dec_nodes = ctx->lex_nodes;
    }
    HIPCHK(ctx, hipMemsetAsync(b->dec_slot, 0xff, n_slot * sizeof(int), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(b->dec_int, 0, l.n_int * sizeof(int), ctx->stream));
    return PCL_OK;
}

DecArgs dec_fill_args(const pcl_batch *b, const DecLayout &l, double beam, int min_distinct, int candidate, int cap, double lpi1, double lpi2) {
    const pcl_ctx *ctx = b->ctx;
    DecArgs a;
    a.utts = b->d_utt;
    a.Bt = b->Bt;
    a.unit_logtrans = ctx->d_unit_logtrans;
    a.node_units = ctx->lex_units;
    a.node_nunits = ctx->lex_nunits;
    a.child_ptr = ctx->lex_child_ptr;
    a.child_idx = ctx->lex_child_idx;
    a.node_word = ctx->lex_word;
    a.roots = ctx->lex_roots;
    a.node_info = ctx->lex_info;
    a.n_nodes = ctx->lex_nodes;
    a.n_roots = ctx->lex_nroots;
    a.n_units = ctx->n_units;
    a.S = ctx->S;
    a.cap = cap;
    a.candidate = candidate;
    a.min_distinct = min_distinct;
    a.Tmax = b->shape.Tmax;
    a.beam = beam;
    a.lpi1 = lpi1;
    a.lpi2 = lpi2;
    double *f = b->dec_f64;
    a.score = f + l.score;
    a.p = f + l.p;
    a.seg_score = f + l.seg_score;
    int *w = b->dec_work;
    a.node = w + l.node;
    a.hist = w + l.hist;
    a.upair = w + l.upair;
    a.flag = l.flag == DecLayout::ABSENT ? nullptr : w + l.flag;
    a.dst = w + l.dst;
    a.seg_ofs = w + l.seg_ofs;
    a.seg_cptr = w + l.seg_cptr;
    a.seg_hist = w + l.seg_hist;
    a.slot = b->dec_slot;
    int *r = b->dec_int;
    a.out_n = r + l.out_n;
    a.out_node = r + l.out_node;
    a.out_hist = r + l.out_hist;
    a.hist_n = r + l.hist_n;
    a.hist_prev = r + l.hist_prev;
    a.hist_node = r + l.hist_node;
    a.trace = r + l.trace;
    a.overflow = r + l.overflow;
    a.out_score = b->dec_score;
    a.stamps = nullptr;
    return a;
}

int dec_launch_general(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm *lm) {
    if (lm) return pcl_decode_general_launch_lm(ctx, a, U, n_rows, *lm);     // (hmm_decode_lm.hip)
    return dec_launch_kernel<false, false>(ctx, a, U, n_rows, DecNoLm{}, DecNoTie{});
}

#ifdef PCL_DEC_STAMPS
int dec_print_stamps(pcl_ctx *ctx, DevBuf<long long> &d_stamps) {
    long long h[PCL_DEC_N_STAMP];
    HIPCHK(ctx, hipMemcpyAsync(h, d_stamps, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    fprintf(stderr, "decode stamps (utterance 0, 100 MHz ticks): step %lld donors %lld pairs %lld first|keys %lld prune %lld compact %lld select %lld\n", h[0], h[1], h[2], h[3], h[4], h[5], h[6]);
    d_stamps.release();
    return PCL_OK;
}
#endif

}  // namespace

void pcl_lexicon_release(pcl_ctx *ctx) {
    static_cast<LexiconDev &>(*ctx) = {};                // (the language model's tables with it)
    ctx->lex_nodes = ctx->lex_nroots = 0;
    ctx->lex_word_host.clear();
    ctx->lex_units_host.clear();
    ctx->lex_nunits_host.clear();
    ctx->lex_tie_Jt = ctx->lex_tie_P = 0;                // (the tied states went with LexiconDev)
    ctx->lm_W = 0;
}

extern "C" {

int pcl_lexicon_upload(pcl_ctx *ctx, int n_nodes, const int32_t *node_units, const int32_t *node_nunits, const int32_t *child_ptr,
                       const int32_t *child_idx, const int32_t *node_word, int n_roots, const int32_t *roots) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ctx->n_units) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_lexicon_upload: pcl_units_upload first");
    if (n_nodes <= 0 || n_roots <= 0 || !node_units || !node_nunits || !child_ptr || !node_word || !roots)
        PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: bad arguments (n_nodes=%d, n_roots=%d)", n_nodes, n_roots);
    const int e = ctx->S - 2;
    if (child_ptr[0] != 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: child_ptr[0] = %d, must be 0", child_ptr[0]);
    for (int i = 0; i < n_nodes; ++i) {
        const int nu = node_nunits[i];
        if (ctx->n_units >= 0xffff) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: %d units (the decoder packs unit ids into 16 bits)", ctx->n_units);
        if (nu < 1 || nu > 2 || e * nu + 2 > NS) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: node %d has %d units (1 or 2; %d-state units need %d <= %d HMM states)", i, nu, ctx->S, e * nu + 2, NS);
        for (int k = 0; k < nu; ++k)
            if (node_units[2 * i + k] < 0 || node_units[2 * i + k] >= ctx->n_units) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: node %d unit %d outside [0,%d)", i, node_units[2 * i + k], ctx->n_units);
        if (child_ptr[i + 1] < child_ptr[i]) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: child_ptr is not monotone at node %d", i);
    }
    const int nc = child_ptr[n_nodes];
    if (nc > 0 && !child_idx) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: child_idx is NULL");
    std::vector<char> has_parent(n_nodes, 0);
    for (int k = 0; k < nc; ++k) {
        if (child_idx[k] < 0 || child_idx[k] >= n_nodes) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: child index %d outside [0,%d)", child_idx[k], n_nodes);
        if (has_parent[child_idx[k]]) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: node %d has two parents (not a tree)", child_idx[k]);
        has_parent[child_idx[k]] = 1;
    }
    for (int r = 0; r < n_roots; ++r) {
        if (roots[r] < 0 || roots[r] >= n_nodes || has_parent[roots[r]] == 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: root %d is not a parentless node", roots[r]);
        if (has_parent[roots[r]] == 2) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lexicon_upload: root %d is listed twice", roots[r]);
        has_parent[roots[r]] = 2;                    // (seen as a root)
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pcl_lexicon_release(ctx);
    TRY(ctx->lex_units.alloc(ctx, (size_t)2 * n_nodes));
    TRY(ctx->lex_nunits.alloc(ctx, (size_t)n_nodes));
    TRY(ctx->lex_child_ptr.alloc(ctx, (size_t)n_nodes + 1));
    TRY(ctx->lex_child_idx.alloc(ctx, (size_t)std::max(nc, 1)));
    TRY(ctx->lex_word.alloc(ctx, (size_t)n_nodes));
    TRY(ctx->lex_roots.alloc(ctx, (size_t)n_roots));
    TRY(ctx->lex_info.alloc(ctx, (size_t)n_nodes));
    {   // (first child, children, words end here, unit pair) of a node in one 16-byte record
        std::vector<int4> info(n_nodes);
        for (int i = 0; i < n_nodes; ++i) {
            const int u0 = node_units[2 * i], u1 = node_nunits[i] == 2 ? node_units[2 * i + 1] : 0xffff;
            info[i] = make_int4(child_ptr[i], child_ptr[i + 1] - child_ptr[i], node_word[i] ? 1 : 0, u0 | (u1 << 16));
        }
        HIPCHK(ctx, hipMemcpy(ctx->lex_info, info.data(), (size_t)n_nodes * sizeof(int4), hipMemcpyHostToDevice));
    }
    TRY(ctx->d_unit_logtrans.alloc(ctx, ctx->unit_logtrans.size()));
    HIPCHK(ctx, hipMemcpy(ctx->lex_units, node_units, (size_t)2 * n_nodes * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->lex_nunits, node_nunits, (size_t)n_nodes * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->lex_child_ptr, child_ptr, ((size_t)n_nodes + 1) * 4, hipMemcpyHostToDevice));
    if (nc) HIPCHK(ctx, hipMemcpy(ctx->lex_child_idx, child_idx, (size_t)nc * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->lex_word, node_word, (size_t)n_nodes * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->lex_roots, roots, (size_t)n_roots * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->d_unit_logtrans, ctx->unit_logtrans.data(), ctx->unit_logtrans.size() * 8, hipMemcpyHostToDevice));
    ctx->lex_nodes = n_nodes;
    ctx->lex_nroots = n_roots;
    ctx->lex_word_host.assign(node_word, node_word + n_nodes);
    ctx->lex_units_host.assign(node_units, node_units + 2 * (size_t)n_nodes);
    ctx->lex_nunits_host.assign(node_nunits, node_nunits + n_nodes);
    return PCL_OK;
}

int pcl_lm_upload(pcl_ctx *ctx, int W, const double *uni, const double *bow, const int64_t *row_ptr, const int32_t *col, const double *val,
                  const int32_t *node_word_ptr, const int32_t *node_word_ids) {
    if (!ctx) return PCL_ERR_INVALID;
    if (!ctx->lex_nodes) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_lm_upload: pcl_lexicon_upload first");
    if (W < 2 || !uni || !bow || !row_ptr || !node_word_ptr) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: bad arguments (W=%d)", W);
    const int n_nodes = ctx->lex_nodes;
    if (row_ptr[0] != 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: row_ptr[0] = %lld, must be 0", (long long)row_ptr[0]);
    for (int v = 0; v < W; ++v) {
        if (!std::isfinite(uni[v]) || !std::isfinite(bow[v])) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: uni / bow of word %d is not finite", v);
        if (row_ptr[v + 1] < row_ptr[v]) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: row_ptr is not monotone at word %d", v);
    }
    const int64_t nnz = row_ptr[W];
    if (nnz > 0 && (!col || !val)) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: col / val is NULL");
    for (int v = 0; v < W; ++v)
        for (int64_t k = row_ptr[v]; k < row_ptr[v + 1]; ++k) {
            if (col[k] < 0 || col[k] >= W) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: successor %d of word %d outside [0,%d)", col[k], v, W);
            if (k > row_ptr[v] && col[k] <= col[k - 1]) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: the successors of word %d are not strictly ascending", v);
            if (!std::isfinite(val[k])) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: bigram (%d, %d) is not finite", v, col[k]);
        }
    if (node_word_ptr[0] != 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: node_word_ptr[0] = %d, must be 0", node_word_ptr[0]);
    for (int i = 0; i < n_nodes; ++i) {
        const int cnt = node_word_ptr[i + 1] - node_word_ptr[i];
        if (cnt < 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: node_word_ptr is not monotone at node %d", i);
        if (ctx->lex_word_host[i] && cnt == 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: words end at node %d and it has no word", i);
        if (!ctx->lex_word_host[i] && cnt != 0) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: node %d has %d words and no word ends there (node_word is 0)", i, cnt);
    }
    const int n_ids = node_word_ptr[n_nodes];
    if (n_ids > 0 && !node_word_ids) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: node_word_ids is NULL");
    for (int k = 0; k < n_ids; ++k)
        if (node_word_ids[k] < 1 || node_word_ids[k] >= W) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_lm_upload: word id %d outside [1,%d) (0 is the sentence start)", node_word_ids[k], W);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream_dp));             // (a decoder may still be reading the old tables on the second stream)
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->lm_W = 0;
    TRY(ctx->lm_uni.alloc(ctx, (size_t)W));
    TRY(ctx->lm_bow.alloc(ctx, (size_t)W));
    TRY(ctx->lm_row_ptr.alloc(ctx, (size_t)W + 1));
    TRY(ctx->lm_col.alloc(ctx, (size_t)std::max<int64_t>(nnz, 1)));
    TRY(ctx->lm_val.alloc(ctx, (size_t)std::max<int64_t>(nnz, 1)));
    TRY(ctx->lm_node_word_ptr.alloc(ctx, (size_t)n_nodes + 1));
    TRY(ctx->lm_node_word_ids.alloc(ctx, (size_t)std::max(n_ids, 1)));
    static_assert(sizeof(long long) == sizeof(int64_t), "row_ptr travels as it is");
    HIPCHK(ctx, hipMemcpy(ctx->lm_uni, uni, (size_t)W * 8, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->lm_bow, bow, (size_t)W * 8, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->lm_row_ptr, row_ptr, ((size_t)W + 1) * 8, hipMemcpyHostToDevice));
    if (nnz) {
        HIPCHK(ctx, hipMemcpy(ctx->lm_col, col, (size_t)nnz * 4, hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(ctx->lm_val, val, (size_t)nnz * 8, hipMemcpyHostToDevice));
    }
    HIPCHK(ctx, hipMemcpy(ctx->lm_node_word_ptr, node_word_ptr, ((size_t)n_nodes + 1) * 4, hipMemcpyHostToDevice));
    if (n_ids) HIPCHK(ctx, hipMemcpy(ctx->lm_node_word_ids, node_word_ids, (size_t)n_ids * 4, hipMemcpyHostToDevice));
    ctx->lm_W = W;
    return PCL_OK;
}

// pcl_batch_decode (with_lm = false: the LM = false kernels, nothing of the language model is touched), pcl_batch_decode_lm, and
// pcl_batch_decode_tied (tied: the TIED = true kernels of either); max_arcs > 0: pcl_batch_decode_lattice -- the LAT = true kernels of
// whichever it is, and the lattice's build behind them
static int dec_run(pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, double logpi_one_unit, double logpi_two_units, bool with_lm,
                   bool tied = false, int max_arcs = 0) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    const bool lattice = max_arcs > 0;
    TRY(dec_validate(b, beam, min_distinct, candidate, max_tokens, tied));
    if (with_lm && !ctx->lm_W)
        PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no language model (pcl_lm_upload after pcl_lexicon_upload)",
                 lattice ? "pcl_batch_decode_lattice" : tied ? "pcl_batch_decode_tied" : "pcl_batch_decode_lm");
    b->have_lat = b->have_lat_post = false;                                    // (any decode drops the lattice of the one before)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (b->dp_pending) {
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, b->ev_dp, 0));
        b->dp_pending = false;
    }
    // Like the forward-backward recursion, the decoder does no matrix work and is latency / bandwidth bound: it runs on
    // the second stream, beside the scoring of the next chunk on the main one (every later call on this batch joins it).
    auto launch = [&]() -> int {                                               // (on ctx->stream: the second stream when dp_async)
        const int cap = max_tokens, U = b->U, n_rows = (tied ? ctx->lex_tie_Jt : ctx->n_units * (ctx->S - 2)) + 2;
        // left-to-right units (every model the reference builds): one lane per token, hmm_decode_lr.hip; PCL_DEC_GENERAL=1 keeps
        // the general kernel (the parity tests run both against the restatement)
        const char *force_general = getenv("PCL_DEC_GENERAL");
        const bool use_lr = !(force_general && atoi(force_general)) && pcl_decode_lr_applicable(ctx, n_rows, cap, b->shape.Tmax, tied);
        const DecLayout l = dec_layout(U, cap, candidate, b->shape.Tmax, use_lr);
        TRY(dec_ensure_workspace(b, l, cap, candidate));
        DecArgs a = dec_fill_args(b, l, beam, min_distinct, candidate, cap, logpi_one_unit, logpi_two_units);
        DecLm lm = {};
        if (with_lm) {
            const size_t n_word = (size_t)U * b->shape.Tmax;
            if (!b->dec_word || b->dec_word.cap < n_word) TRY(b->dec_word.alloc(ctx, n_word));
            HIPCHK(ctx, hipMemsetAsync(b->dec_word, 0, n_word * sizeof(int), ctx->stream));
            lm = DecLm{ctx->lm_uni, ctx->lm_bow, ctx->lm_row_ptr, ctx->lm_col, ctx->lm_val, ctx->lm_node_word_ptr, ctx->lm_node_word_ids, b->dec_word};
        }
#ifdef PCL_DEC_STAMPS
        DevBuf<long long> d_stamps;
        TRY(d_stamps.alloc(ctx, (size_t)PCL_DEC_N_STAMP));
        HIPCHK(ctx, hipMemsetAsync(d_stamps, 0, PCL_DEC_N_STAMP * sizeof(long long), ctx->stream));
        a.stamps = d_stamps;
#endif
        DecLat lat = {};
        if (lattice) {
            TRY(pcl_lattice_reserve(ctx, b, max_arcs, candidate));
            lat = pcl_lattice_dec_args(b);
        }
        pcl_timer_begin(ctx, "decode");
        const DecLm *lmp = with_lm ? &lm : nullptr;
        const DecTie tie{ctx->lex_tie_lr, ctx->lex_tie_gen};
        const int rc = lattice ? (use_lr ? pcl_decode_lr_launch_lat(ctx, a, U, n_rows, lmp, tied ? &tie : nullptr, lat)
                                         : pcl_decode_general_launch_lat(ctx, a, U, n_rows, lmp, tied ? &tie : nullptr, lat))
                       : tied  ? (use_lr ? pcl_decode_lr_launch_tied(ctx, a, U, n_rows, lmp, tie) : pcl_decode_general_launch_tied(ctx, a, U, n_rows, lmp, tie))
                               : (use_lr ? pcl_decode_lr_launch(ctx, a, U, n_rows, lmp) : dec_launch_general(ctx, a, U, n_rows, lmp));
        pcl_timer_end(ctx, "decode");
        TRY(rc);
        HIPCHK(ctx, hipGetLastError());
        if (lattice) TRY(pcl_lattice_build(ctx, b, PclLatDecEnd{a.out_n, a.out_node, a.out_hist, a.hist_n, a.out_score, candidate}, with_lm));
#ifdef PCL_DEC_STAMPS
        TRY(dec_print_stamps(ctx, d_stamps));
#endif
        return PCL_OK;
    };
    // no flag of pcl_run_recursion: the decoder writes its own workspace only -- nothing pcl_batch_fetch_async copies, nothing another
    // recursion reads behind the scoring -- and the main stream was put behind a pending recursion above
    TRY(pcl_run_recursion(b, 0, launch));
    b->have_dec = true;
    b->dec_has_words = with_lm;
    b->have_lat = lattice;
    return PCL_OK;
}

int pcl_batch_decode(pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, double logpi_one_unit, double logpi_two_units) {
    return dec_run(b, beam, min_distinct, candidate, max_tokens, logpi_one_unit, logpi_two_units, false);
}

int pcl_batch_decode_lm(pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, double logpi_one_unit, double logpi_two_units) {
    return dec_run(b, beam, min_distinct, candidate, max_tokens, logpi_one_unit, logpi_two_units, true);
}

int pcl_batch_decode_tied(pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, double logpi_one_unit, double logpi_two_units, int lm) {
    return dec_run(b, beam, min_distinct, candidate, max_tokens, logpi_one_unit, logpi_two_units, lm != 0, true);
}

int pcl_batch_decode_lattice(pcl_batch *b, double beam, int min_distinct, int candidate, int max_tokens, double logpi_one_unit, double logpi_two_units, int lm, int tied,
                             int max_arcs) {
    if (!b) return PCL_ERR_INVALID;
    if (max_arcs < 1) PCL_FAIL(b->ctx, PCL_ERR_INVALID, "pcl_batch_decode_lattice: max_arcs = %d", max_arcs);
    return dec_run(b, beam, min_distinct, candidate, max_tokens, logpi_one_unit, logpi_two_units, lm != 0, tied != 0, max_arcs);
}

// the chosen words of the history entries, on the stream the decoder ran on (before or after pcl_batch_decode_get)
int pcl_batch_decode_get_words(pcl_batch *b, int32_t *hist_word) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_dec || !b->dec_has_words) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_decode_get_words: run pcl_batch_decode_lm (or pcl_batch_decode_tied with lm) first");
    if (!hist_word) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_decode_get_words: hist_word is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = b->dp_pending ? ctx->stream_dp : ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(hist_word, b->dec_word, (size_t)b->U * b->shape.Tmax * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return PCL_OK;
}

int pcl_batch_decode_get(pcl_batch *b, int32_t *n_final, int32_t *node, double *score, int32_t *hist, int32_t *hist_n, int32_t *hist_prev,
                         int32_t *hist_node, int32_t *n_tokens, int32_t *overflow) {
    if (!b) return PCL_ERR_INVALID;
    pcl_ctx *ctx = b->ctx;
    if (!b->have_dec) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_decode_get: run pcl_batch_decode first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t U = (size_t)b->U, c = (size_t)b->dec_cand, Tm = (size_t)b->shape.Tmax;
    const DecLayout l = dec_layout(b->U, b->dec_cap, b->dec_cand, b->shape.Tmax, false);   // (the results sit alike for both kernels)
    const int *r = b->dec_int;
    // the results come down on the stream the decoder ran on, and only that stream is waited for: the scoring of the next
    // chunk, queued on the main stream meanwhile, keeps running
    hipStream_t st = b->dp_pending ? ctx->stream_dp : ctx->stream;
    auto get = [&](void *dst, const void *src, size_t bytes) -> int {
        if (dst) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        return PCL_OK;
    };
    TRY(get(n_final, r + l.out_n, U * 4));
    TRY(get(node, r + l.out_node, U * c * 4));
    TRY(get(hist, r + l.out_hist, U * c * 4));
    TRY(get(hist_n, r + l.hist_n, U * 4));
    TRY(get(hist_prev, r + l.hist_prev, U * Tm * 4));
    TRY(get(hist_node, r + l.hist_node, U * Tm * 4));
    TRY(get(n_tokens, r + l.trace, U * Tm * 4));
    TRY(get(overflow, r + l.overflow, U * 4));
    TRY(get(score, b->dec_score, U * c * 8));
    HIPCHK(ctx, hipStreamSynchronize(st));
    b->dp_pending = false;                                                     // (complete: nothing left to join)
    return PCL_OK;
}

}  // extern "C"
#endif  // the kernel-only translation units (PCL_DEC_LM, PCL_DEC_TIED)
