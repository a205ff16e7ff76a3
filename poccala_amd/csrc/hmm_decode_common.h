// hmm_decode_common.h -- what the two token-passing kernels (hmm_decode.hip: any unit matrices, 8 lanes per token;
// hmm_decode_lr.hip: left-to-right units, the shape every model of the reference has, one lane per token) share: the launch
// arguments, the small wave idioms, and the two parts of the rules that do not depend on how a token steps -- pruning
// (Decoder.py:159-167) and the final transfer (Decoder.py:175-187).  Both kernels are held bit for bit to the same CPU
// restatement, so a rule lives here once.
//
// The helpers are workgroup-collective: every thread of the NT-thread workgroup calls them, with uniform arguments.  Their LDS
// scratch is the caller's and comes in as pointers ([NT / 64] per-wave slots unless said otherwise), so each kernel keeps its
// own LDS plan; a helper says which barrier protects its slots.
#pragma once
#include <type_traits>

#include "pcl_internal.h"

// Token state is kept as separate arrays (coalesced passes), two buffers of each.  upair = the node's units, u0 | u1 << 16
// (u1 = 0xffff: a one-unit node).  Where the arrays sit in the batch's allocations: DecLayout (hmm_decode.hip).
struct DecArgs {
    const UttDesc *utts;
    const double *Bt;
    const double *unit_logtrans;    // [n_units][S][S]
    const int *node_units, *node_nunits, *child_ptr, *child_idx, *node_word, *roots;
    const int4 *node_info;          // [n_nodes] (first child, children, words end here, upair): one gather instead of four
    int n_nodes, n_roots, n_units, S, cap, candidate, min_distinct, Tmax;
    double beam, lpi1, lpi2;        // ln(1/N) for one- and two-unit nodes, from the caller's np.log
    double *score, *p;              // [U][2][cap], [U][2][cap][8] (general kernel: 8 per token; left-to-right kernel: [6][cap] of the 8 cap)
    int *node, *hist, *upair;       // [U][2][cap]
    int *flag;                      // general kernel only, [U][cap]: bit 0 finished, bit 1 pruned (this frame); 4 = taken by the transfer
    int *dst;                       // general kernel: [U][cap], where a token's p sits in the other p buffer;  left-to-right kernel:
                                    // [U][2][cap], where token i's state sits in the other buffers, | fresh << 31
    int *seg_ofs, *seg_cptr, *seg_hist;   // [U][cap + 2]: the frame's donors as segments of the flattened (donor, child) list
    double *seg_score;              //              (left-to-right kernel: what a wave's donor list does not hold in LDS)
    int *slot;                      // [U][n_nodes]: live token of a node, or -1
    int *out_n, *out_node, *out_hist, *hist_n, *hist_prev, *hist_node, *trace, *overflow;
    double *out_score;
    long long *stamps;              // PCL_DEC_STAMPS: clock ticks per phase, utterance 0
};

// The resident bigram language model (pcl_lm_upload) and the batch's chosen words, for the LM = true instantiations of the two kernels
// (pcl_batch_decode_lm).  A kernel argument of its own, so DecArgs and with it the LM = false kernels stay what they were.
// Tables are pre-scaled float64, ARPA-shaped: the kernels only add.
struct DecLm {
    const double *uni, *bow;        // [W]: scale ln P(w) + penalty, scale ln bow(v)
    const long long *row_ptr;       // [W + 1] CSR over predecessors ...
    const int *col;                 // ... successors, strictly ascending inside a row
    const double *val;              // ... scale ln P(w|v) + penalty
    const int *node_word_ptr, *node_word_ids;   // [n_nodes + 1], ids of a word-end node's homophones (1 .. W-1) in the tree's order
    int *hist_word;                 // [U][Tmax]: the chosen word of every history entry, beside hist_prev / hist_node
};
struct DecNoLm {};                  // what the LM = false kernels take in its place: nothing
template <bool LM>
using DecLmArg = std::conditional_t<LM, DecLm, DecNoLm>;

// The lexicon's tied states (pcl_lexicon_tie; tying.hip) for the TIED = true instantiations of the two kernels (pcl_batch_decode_tied): the
// emission row of state position k of unit slot j of a token at node n is 1 + node_state[n][j P + k] instead of 1 + unit (S - 2) + k.  Like
// DecLm a kernel argument of its own: DecArgs and the TIED = false kernels stay what they were.  Both forms are indexed by the node id the
// step has at hand anyway (one gather per token and step; DESIGN.md says what carrying the ids in the token arrays would cost instead).
struct DecTie {
    const int4 *lr;                 // [n_nodes] six 16-bit ids (s0 | s1 << 16, s2 | s3 << 16, s4 | s5 << 16, 0); a one-unit node repeats slot 0 in slot 1
    const int *gen;                 // [n_nodes][2 P] int32, -1 in slot 1 of a one-unit node: lane `sub` of a token reads entry sub - 1
};
struct DecNoTie {};
template <bool TIED>
using DecTieArg = std::conditional_t<TIED, DecTie, DecNoTie>;

// The word lattice's records (pcl_batch_decode_lattice; the lattice pass: lattice.hip) for the LAT = true instantiations of the two kernels.
// Like DecLm and DecTie a kernel argument of its own: DecArgs and the LAT = false kernels stay what they were.  The rule, once:
//   every word-end donor of frame t (a finished token at a node where words end: exactly the tokens that take part in the frame's choice
//   of a history entry) leaves ONE arc record (t, its token index in the frame, node, its history entry or -1, its raw score s, and under
//   LM what pcl_lm_word_term returned for it: term and word; without LM 0.0 and 0), appended to the utterance's list at the next free
//   place -- frames ascend in the list, the order inside a frame is whatever the waves' appends give (lattice.hip sorts it).  A record
//   whose place is >= max_arcs is not written; the counter still counts it (n_wanted), so overflow = n_wanted > max_arcs.
//   Every history entry gets the frame it was made at and the winning offer w_score that seeded the roots (hist_frame, hist_seed).
// Nothing the decoder itself reads is written: its results are those of the LAT = false kernel, bit for bit, overflow or not.
struct DecLat {
    int max_arcs;
    int *arc_frame, *arc_tok, *arc_node, *arc_hist, *arc_word;     // [U][max_arcs]
    double *arc_score, *arc_term;                                  // [U][max_arcs]
    int *n_wanted;                                                 // [U]: every word-end donor, written or not
    int *hist_frame;                                               // [U][Tmax], beside hist_prev / hist_node / hist_word
    double *hist_seed;                                             // [U][Tmax]
};
struct DecNoLat {};
template <bool LAT>
using DecLatArg = std::conditional_t<LAT, DecLat, DecNoLat>;

constexpr int PCL_DEC_N_STAMP = 8;
// A lane keeps the sort keys of the old tokens it owns in registers through the pruning phase, at most this many: a kernel of NT
// threads takes cap <= 16 NT tokens per utterance.  The general kernel's 16 x 1024 is what pcl_batch_decode accepts; the
// left-to-right kernel's 16 x 512 is part of pcl_decode_lr_applicable (above it the general kernel runs).
constexpr int PCL_DEC_MAX_KEYS_PER_LANE = 16;
constexpr int NONE = 0x7fffffff;                  // no token index
constexpr unsigned long long NOKEY = ~0ull;       // not an old unfinished token (no score has this key: it would be a NaN)

// Clock ticks per phase of utterance 0 (-DPCL_DEC_STAMPS); `u` and `tid` are the kernel's own names.
#ifdef PCL_DEC_STAMPS
#define STAMP_BEGIN long long st_acc[PCL_DEC_N_STAMP] = {0, 0, 0, 0, 0, 0, 0, 0}, st_t = wall_clock64();
#define STAMP(k)                                  \
    if (u == 0 && tid == 0) {                     \
        const long long now_ = wall_clock64();    \
        st_acc[k] += now_ - st_t;                 \
        st_t = now_;                              \
    }
#define STAMP_END(out)                            \
    if (u == 0 && tid == 0 && (out))              \
        for (int k_ = 0; k_ < PCL_DEC_N_STAMP; ++k_) (out)[k_] = st_acc[k_];
#else
#define STAMP_BEGIN
#define STAMP(k)
#define STAMP_END(out)
#endif

__device__ __forceinline__ unsigned long long pcl_okey(double s) {       // order-preserving bits of a float64
    const unsigned long long b = (unsigned long long)__double_as_longlong(s);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ int pcl_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int pcl_wave_scan(int v, int lane) {          // inclusive prefix sum over the wave
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(inc, o, 64);
        if (lane >= o) inc += x;
    }
    return inc;
}

// Rule D6, the language model at a word end (the reference's stub: passing_between_word, Decoder.py:146-156, on the n-gram model it
// imports at :17 and builds at :200-204).  A finished token at word-end node `node` whose history entry is `hist` offers the roots its
// score plus the value returned here: max over the node's homophones w of lm(v, w), where v = the chosen word of the token's history
// entry (0, the sentence start, without one) and lm(v, w) = the explicit bigram val[k] (col[k] == w in row v, binary search), else
// bow[v] + uni[w].  `word` = the first w that reaches the maximum.  hword = the utterance's row of DecLm::hist_word: entry `hist` was
// written by one thread in an earlier frame, behind that frame's barriers.  Additions only (no product: nothing to contract), so the
// host restatement gets the same bits; compiles for the host as well.
__host__ __device__ __forceinline__ double pcl_lm_word_term(const DecLm &lm, const int *hword, int hist, int node, int &word) {
    const int v = hist < 0 ? 0 : hword[hist];
    const long long r0 = lm.row_ptr[v], r1 = lm.row_ptr[v + 1];
    const double bv = lm.bow[v];
    const int k0 = lm.node_word_ptr[node], k1 = lm.node_word_ptr[node + 1];
    double best = 0.0;
    word = 0;
    for (int k = k0; k < k1; ++k) {
        const int w = lm.node_word_ids[k];
        long long lo = r0, hi = r1;                                // the first entry of the row with col >= w
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (lm.col[mid] < w) lo = mid + 1;
            else hi = mid;
        }
        const double x = (lo < r1 && lm.col[lo] == w) ? lm.val[lo] : bv + lm.uni[w];
        if (k == k0 || x > best) {                                 // strictly greater: the first homophone on ties
            best = x;
            word = w;
        }
    }
    return best;
}

// LAT: the wave's word-end donors of one ballot (`mask`, wave-uniform and not zero; `mine`: this lane is one) take their places in the
// utterance's record list: one integer add on the workgroup's counter in LDS by lane 0, the lanes' places in lane order behind it.
__device__ __forceinline__ int pcl_lat_place(int *counter, unsigned long long mask, bool mine) {
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(counter, __popcll(mask));
    base = __shfl(base, 0, 64);
    return mine ? base + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
}
__device__ __forceinline__ void pcl_lat_record(const DecLat &lat, int u, int place, int frame, int tok, int node, int hist, double score, double term, int word) {
    if (place < 0 || place >= lat.max_arcs) return;
    const size_t x = (size_t)u * lat.max_arcs + place;
    lat.arc_frame[x] = frame;
    lat.arc_tok[x] = tok;
    lat.arc_node[x] = node;
    lat.arc_hist[x] = hist;
    lat.arc_word[x] = word;
    lat.arc_score[x] = score;
    lat.arc_term[x] = term;
}
__device__ __forceinline__ void pcl_lat_entry(const DecLat &lat, int u, int Tmax, int entry, int frame, double seed) {
    lat.hist_frame[(size_t)u * Tmax + entry] = frame;
    lat.hist_seed[(size_t)u * Tmax + entry] = seed;
}

// (ob, oi) replaces (b, bi) as the best (score, index): greater, or equal and earlier; NONE = nothing yet
__device__ __forceinline__ bool pcl_beats(double ob, int oi, double b, int bi) {
    return oi != NONE && (bi == NONE || ob > b || (ob == b && oi < bi));
}

// the wave's best (score, index), earliest index on ties, on every lane; `with` = ints that travel with the winner
template <class... Ints>
__device__ __forceinline__ void pcl_wave_best(double &b, int &bi, Ints &...with) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(b, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        const bool take = pcl_beats(ob, oi, b, bi);
        auto carry = [&](int &v) {
            const int ov = __shfl_xor(v, o, 64);
            if (take) v = ov;
        };
        (carry(with), ...);
        if (take) {
            b = ob;
            bi = oi;
        }
    }
}

// the same over the waves' results in LDS (one thread's job)
template <int NW>
__device__ __forceinline__ void pcl_best_of_waves(const double *w_best, const int *w_idx, double &g, int &gi) {
    g = -INFINITY;
    gi = NONE;
    for (int w = 0; w < NW; ++w)
        if (pcl_beats(w_best[w], w_idx[w], g, gi)) {
            g = w_best[w];
            gi = w_idx[w];
        }
}

// A loop over the waves' LDS slots, unrolled, has all its loads in flight at once: fine for 8 waves, but with 16 (the general
// kernel, which has no register to spare) it is where the register allocator starts to spill -- those loops stay rolled.
constexpr int pcl_wave_loop_unroll(int nw) { return nw <= 8 ? nw : 1; }

// sum of the wave totals before mine (the base of an ordered prefix over the workgroup), and of all of them
template <int NW>
__device__ __forceinline__ int pcl_waves_before(const int *totals, int wave, int *total = nullptr) {
    constexpr int UNR = pcl_wave_loop_unroll(NW);
    int base = 0, tot = 0;
#pragma unroll UNR
    for (int w = 0; w < NW; ++w) {
        const int x = totals[w];
        if (w < wave) base += x;
        tot += x;
    }
    if (total) *total = tot;
    return base;
}

// ---- pruning (Decoder.py:159-167) over the tokens that were alive before the frame and did not finish: nothing below min_distinct
// different scores, else the m = int(width (1 - beam)) lowest go (stable ascending order: ties by token order).  A lane's keys
// (pcl_okey of the score, NOKEY for a slot that takes no part) stay in its registers: keys[k] belongs to token w0 + 64 k + lane of
// the wave's range, so (wave, k, lane) ascending IS token order.  Four steps, glued by the caller:
//   stats -> n_old, key range, occupied hash bins;  m = int(n_old (1 - beam)), prune = m > 0 && n_old >= min_distinct;
//   bins < min_distinct (different bins => different scores, not the reverse) -> distinct settles it exactly;
//   select_kth -> the m-th smallest key and its rank among its equals;  mark -> the bitmask over k of the lane's tokens that go.

// Step 1.  occ: [256] hashed occupancy map, zero on entry and zero again on return (behind a barrier: the caller may hand the same
// words to select_kth as its histogram).  The slots are free again once the next barrier has passed.
template <int NT, int KMAX>
__device__ __forceinline__ void pcl_prune_stats(const unsigned long long (&keys)[KMAX], unsigned int *occ, int *w_cnt, unsigned long long *w_min,
                                                unsigned long long *w_max, int &n_old, unsigned long long &kmin, unsigned long long &kmax, int &bins) {
    static_assert(NT >= 256 && NT % 64 == 0, "a thread per bin of the occupancy map");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cnt = 0;
    unsigned long long kmn = ~0ull, kmx = 0ull;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const unsigned long long key = keys[k];
        if (key != NOKEY) {
            ++cnt;
            kmn = min(kmn, key);
            kmx = max(kmx, key);
            atomicOr(&occ[(unsigned int)((key * 0x9E3779B97F4A7C15ull) >> 56)], 1u);
        }
    }
    cnt = pcl_wave_sum(cnt);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kmn = min(kmn, (unsigned long long)__shfl_xor((long long)kmn, o, 64));
        kmx = max(kmx, (unsigned long long)__shfl_xor((long long)kmx, o, 64));
    }
    if (lane == 0) {
        w_cnt[wave] = cnt;
        w_min[wave] = kmn;
        w_max[wave] = kmx;
    }
    __syncthreads();
    const bool occupied = tid < 256 && occ[tid] != 0u;
    if (tid < 256) occ[tid] = 0u;
    bins = __syncthreads_count(occupied);
    constexpr int UNR = pcl_wave_loop_unroll(NT / 64);
    n_old = 0;
    kmin = ~0ull;
    kmax = 0ull;
#pragma unroll UNR
    for (int w = 0; w < NT / 64; ++w) {
        n_old += w_cnt[w];
        kmin = min(kmin, w_min[w]);
        kmax = max(kmax, w_max[w]);
    }
}

// Step 2.  Are there at least min_distinct different keys?  The next larger key, min_distinct times at most.  Every round begins
// with a barrier (w_key may be step 1's w_min) and the last one ends with one.
template <int NT, int KMAX>
__device__ __forceinline__ bool pcl_prune_distinct(const unsigned long long (&keys)[KMAX], int min_distinct, unsigned long long *w_key, int *w_any) {
    constexpr int UNR = pcl_wave_loop_unroll(NT / 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long prev = 0ull;
    bool have_prev = false;
    int distinct = 0;
#pragma nounroll
    for (int round = 0; round < min_distinct; ++round) {
        unsigned long long mn = ~0ull;
        bool any = false;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const unsigned long long key = keys[k];
            if (key != NOKEY && (!have_prev || key > prev) && (!any || key < mn)) {
                mn = key;
                any = true;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long om = (unsigned long long)__shfl_xor((long long)mn, o, 64);
            const int oa = __shfl_xor((int)any, o, 64);
            if (oa && (!any || om < mn)) {
                mn = om;
                any = true;
            }
        }
        __syncthreads();
        if (lane == 0) {
            w_key[wave] = mn;
            w_any[wave] = any;
        }
        __syncthreads();
        unsigned long long g = ~0ull;
        bool gany = false;
#pragma unroll UNR
        for (int w = 0; w < NT / 64; ++w)
            if (w_any[w] && (!gany || w_key[w] < g)) {
                g = w_key[w];
                gany = true;
            }
        if (!gany) break;                                          // (uniform)
        prev = g;
        have_prev = true;
        ++distinct;
    }
    __syncthreads();
    return distinct >= min_distinct;
}

// Step 3.  sel = the m-th smallest key (m >= 1), rank = its 0-based position among the keys equal to it in ascending order: a radix
// select, HB bits a round, from the highest bit in which kmin and kmax differ down to bit 0.  A round histograms the digit of the
// keys still in play, every thread scans its share of the bins, and the bin that holds the rank narrows the keys.  CAND > 0: as soon
// as that bin holds at most CAND keys they are ranked directly, each against all; CAND = 0: never, the rounds go on to bit 0.
// The value is determined by the keys alone, whatever HB and CAND.
//   hist [1 << HB]: zero on entry, zero again on return;  cand [CAND] (unused at 0);  w_scan: per-wave slots;
//   s_key: one word, the chosen bin and then the directly ranked key;  s_int: [0] the rank inside the bin, and for CAND > 0
//   [1] the bin's count, [2] the candidates gathered so far (zero between calls).
template <int NT, int KMAX, int HB, int CAND>
__device__ __forceinline__ void pcl_select_kth(const unsigned long long (&keys)[KMAX], unsigned long long kmin, unsigned long long kmax, int m,
                                               unsigned int *hist, unsigned long long *cand, int *w_scan, unsigned long long *s_key, int *s_int,
                                               unsigned long long &sel, int &rank) {
    constexpr int HBINS = 1 << HB, BPT = HBINS >= NT ? HBINS / NT : 1;         // bins per scanning thread
    static_assert(HBINS % NT == 0 || NT % HBINS == 0, "the bins divide among the threads");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    sel = kmin;
    rank = m - 1;
    const unsigned long long diff = kmin ^ kmax;
    if (diff == 0ull) return;                                                   // one score: it is the m-th smallest, rank m - 1
    const int hb = 63 - __clzll((long long)diff);                              // the highest bit in which the keys differ
    const unsigned long long lowmask = (2ull << hb) - 1ull;                    // (hb = 63: all ones)
    int shift = max(hb - (HB - 1), 0);
    unsigned long long pmask = 0ull, pval = 0ull;                               // keys still in play: (key & pmask) == pval
    for (;;) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const unsigned long long key = keys[k];
            if (key != NOKEY && (key & pmask) == pval) atomicAdd(&hist[(unsigned int)(key >> shift) & (HBINS - 1)], 1u);
        }
        __syncthreads();
        const bool scans = HBINS >= NT || tid < HBINS;
        int h[BPT], s4 = 0;                                                     // the thread's bins: does one of them hold rank?
#pragma unroll
        for (int j = 0; j < BPT; ++j) {
            h[j] = scans ? (int)hist[BPT * tid + j] : 0;
            s4 += h[j];
            if (scans) hist[BPT * tid + j] = 0u;
        }
        const int inc = pcl_wave_scan(s4, lane);
        if (lane == 63) w_scan[wave] = inc;
        __syncthreads();
        const int lo = pcl_waves_before<NT / 64>(w_scan, wave) + inc - s4;
        if (rank >= lo && rank < lo + s4) {
            int acc = lo, j = 0;
            for (; j < BPT - 1; ++j) {
                if (acc + h[j] > rank) break;
                acc += h[j];
            }
            *s_key = (unsigned long long)(BPT * tid + j);
            s_int[0] = rank - acc;
            if (CAND > 0) s_int[1] = h[j];
        }
        __syncthreads();
        const unsigned long long digits = (unsigned long long)(HBINS - 1) << shift;
        pmask |= digits;
        pval = (pval & ~digits) | (*s_key << shift);
        rank = s_int[0];
        if (shift == 0) {
            sel = (kmin & ~lowmask) | (pval & lowmask);
            return;
        }
        if constexpr (CAND > 0) {
            const int c = s_int[1];
            if (c <= CAND) {                                                    // the bin's keys, ranked directly
#pragma unroll
                for (int k = 0; k < KMAX; ++k) {
                    const unsigned long long key = keys[k];
                    if (key != NOKEY && (key & pmask) == pval) cand[atomicAdd(&s_int[2], 1)] = key;
                }
                __syncthreads();
                for (int x = tid; x < c; x += NT) {
                    const unsigned long long kx = cand[x];
                    int less = 0, eq = 0;
                    for (int y = 0; y < c; ++y) {
                        const unsigned long long ky = cand[y];
                        less += ky < kx;
                        eq += ky == kx;
                    }
                    if (less <= rank && rank < less + eq) {                     // (equal keys write the same two values)
                        *s_key = kx;
                        s_int[0] = rank - less;
                    }
                }
                __syncthreads();
                sel = *s_key;
                rank = s_int[0];
                if (tid == 0) s_int[2] = 0;
                return;
            }
        }
        shift = max(shift - HB, 0);
    }
}

// Step 4.  Everything below sel goes, and of the tokens equal to it the first rank + 1 in token order.  Returns the lane's
// tokens that go as a bitmask over k.  One barrier, behind the write of w_eq.
template <int NT, int KMAX>
__device__ __forceinline__ unsigned int pcl_prune_mark(const unsigned long long (&keys)[KMAX], unsigned long long sel, int rank, int *w_eq) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    int eq = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) eq += keys[k] == sel;
    eq = pcl_wave_sum(eq);
    if (lane == 0) w_eq[wave] = eq;
    __syncthreads();
    int run = pcl_waves_before<NT / 64>(w_eq, wave);
    unsigned int gone = 0u;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const unsigned long long key = keys[k];
        const bool is_eq = key == sel;                                         // (sel is a real key, never NOKEY)
        const unsigned long long mask = __ballot(is_eq);
        if (key != NOKEY && (key < sel || (is_eq && run + __popcll(mask & lt_mask) <= rank))) gone |= 1u << k;
        run += __popcll(mask);
    }
    return gone;
}

// ---- transfer (Decoder.py:175-187): the `candidate` best of the n tokens, ties in token order.  Token i's state sits at index at(i)
// of sc / nd / hs; taken: [n] ints of the caller's that nothing else needs any more (4 = taken); the outputs are the utterance's
// own [candidate] rows.  Returns how many came out.
template <int NT, class At>
__device__ __forceinline__ int pcl_transfer(int n, int candidate, const double *sc, const int *nd, const int *hs, At at, int *taken, double *w_best,
                                            int *w_idx, int *out_node, double *out_score, int *out_hist) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < n; i += NT) taken[i] = 0;
    __syncthreads();
    int n_out = 0;
    for (int cc = 0; cc < candidate && cc < n; ++cc) {
        double b = -INFINITY;
        int bi = NONE;
        for (int i = tid; i < n; i += NT) {
            const double v = sc[at(i)];
            if (taken[i] != 4 && (bi == NONE || v > b)) {          // (strictly greater keeps the earliest on ties)
                b = v;
                bi = i;
            }
        }
        pcl_wave_best(b, bi);
        if (lane == 0) {
            w_best[wave] = b;
            w_idx[wave] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            double g;
            int gi;
            pcl_best_of_waves<NT / 64>(w_best, w_idx, g, gi);
            const int x = at(gi);
            out_node[cc] = nd[x];
            out_score[cc] = sc[x];
            out_hist[cc] = hs[x];
            taken[gi] = 4;
        }
        ++n_out;
        __syncthreads();
    }
    return n_out;
}

// hmm_decode_lr.hip: true when every unit matrix is left-to-right (row 0 reaches state 1 only, an emitting state itself and
// its successor only) and S = 5 -- then the fast kernel gives the general kernel's bits and pcl_decode_lr_launch runs it.
// tied: n_rows = J_t + 2 (the two staged emission rows), and the state ids must fit DecTie::lr's 16 bits.
bool pcl_decode_lr_applicable(const pcl_ctx *ctx, int n_rows, int cap, int t_max, bool tied = false);
int pcl_decode_lr_launch(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm *lm = nullptr);   // lm: the LM = true instantiation ...
int pcl_decode_lr_launch_lm(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm &lm);           // ... which hmm_decode_lr_lm.hip holds
int pcl_decode_general_launch_lm(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm &lm);      // the general kernel's, hmm_decode_lm.hip
// the TIED = true instantiations, with (lm) and without (nullptr) the language model: hmm_decode_lr_tied.hip, hmm_decode_tied.hip
int pcl_decode_lr_launch_tied(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm *lm, const DecTie &tie);
int pcl_decode_general_launch_tied(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm *lm, const DecTie &tie);
// the LAT = true instantiations, all four (lm, tie) combinations (nullptr = without): hmm_decode_lr_lat.hip, hmm_decode_lat.hip
int pcl_decode_lr_launch_lat(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm *lm, const DecTie *tie, const DecLat &lat);
int pcl_decode_general_launch_lat(pcl_ctx *ctx, const DecArgs &a, int U, int n_rows, const DecLm *lm, const DecTie *tie, const DecLat &lat);
// lattice.hip: the batch's lattice buffers for (max_arcs, candidate), the kernels' view of them, and the build behind the decode kernel (on
// ctx->stream) from the decoder's own ending -- what the transfer returned and how many history entries were made
struct PclLatDecEnd {
    const int *out_n, *out_node, *out_hist, *hist_n;               // [U], [U][candidate], [U][candidate], [U]
    const double *out_score;                                       // [U][candidate]
    int candidate;
};
int pcl_lattice_reserve(pcl_ctx *ctx, pcl_batch *b, int max_arcs, int candidate);
DecLat pcl_lattice_dec_args(const pcl_batch *b);
int pcl_lattice_build(pcl_ctx *ctx, pcl_batch *b, const PclLatDecEnd &end, bool with_lm);
