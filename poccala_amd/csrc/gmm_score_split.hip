// gmm_score_split.hip -- GMM scoring as an f32-class contraction on the f16 matrix pipe (gfx950): the default f32 path.
//
// Reference rows (as gmm_score.hip): A1/A4/A6 -- util.gaussian_function (util.py:20-31), Clustering.GMM.point
// (Clustering.py:740-767), LHMM.cal_observation_pro (LHMM.py:163-187).  Expanded around a per-state centre c_j the
// exponent of mixture m for frame f is a contraction over K = 2D + 2:
//     v[f,m] = k'_m + sum_d ( a_md x'_fd^2 + b_md x'_fd ) - ref_f,      x' = x - c_j
// (centring keeps the cancellation of the expanded form at the direct form's level; states whose expansion is still ill
// conditioned go to the direct-form kernel, pcl_model_conditioning).
//
// Which pipe.  v_mfma_f32_32x32x2_f32 runs at the VALU's rate AND blocks the VALU while it runs (gmm_score_mfma.hip,
// PCL_SCORE_VARIANT=3: 0.65 of its 157 TFLOP/s peak, the strict-f32 number kept in the bench line).  The f16 / bf16 pipe is
// 16x faster and separate.  f16 has 11 significand bits, so x = h1 + h2 carries 22 and
//     a x = a1 x1 + a1 x2 + a2 x1 + O(2^-22 |a x|)
// three v_mfma_f32_32x32x16_f16 per K-step with f32 accumulation.  f16's narrow exponent range is handled by exact
// power-of-two scaling per (state, feature): A'' = coef 2^-e with max_m |A''| in [1, 2), B'' = feature 2^e (model_derive.hip
// writes 2^e next to the layout); subnormal second pieces are honoured by the f16 MFMA (tools/ubench_f16denorm.hip), so small
// features keep an ABSOLUTE error of 2^-25.  The spare K slot d = D of each side carries the constants:
//     a1: [k1 | 0]   a2: [k2 | 1]   x1: [1 | -ref']   x2: [0 | 0]   ->  a2 x1 + a1 x2 + a1 x1 = k1 + k2 - ref'
// with k1 + k2 = k'_m - K0_j (K0_j = max_m k'_m, added back in f64 at the end, so the 22 bits go to a small number) and
// ref' the f16-rounded log-sum-exp reference (any nearby value serves).  Log zero is -6e4.  A frame whose scaled feature
// exceeds 6e4 (|x - c| beyond ~300 sigma of the tightest mixture) or whose reference leaves the f16 range raises its tile's
// flag: the direct-form kernel then rescored flagged tiles in the same call (pcl_launch_score_fixup), so no input sees an
// overflowed result.  Measured max |d ln b| against float64 at |ln b| ~ 85: 1.5e-5 (the exact f32 chain: 1.0e-5).
//
// Mapping (v_mfma_f32_32x32x16_f16: D[32 mixtures x 32 frames] += A[32 x 16] B[16 x 32]).  K-step s, lane l (r = l&31,
// h = l>>5), element j <-> feature d = 8s + j of the side h selects:
//   B (frames):     h = 0: x'_d^2 2^e,  h = 1: x'_d 2^e     -- two f16 pieces, resident in VGPRs (a wave owns NT = 2 tiles)
//   A (parameters): h = 0: a_md 2^-e,   h = 1: b_md 2^-e    -- layout [m-tile][piece 2][KS8][64 lanes][8 f16] = 10 KB per 32
//                   mixtures, staged in LDS by LDS-DMA one stage of two m-tiles ahead (a ring, PCL_SPLIT16_RING) and shared by the 4 waves.
// Pass order a2x1, a1x2, a1x1 (small terms first).  In the accumulator a lane owns 16 mixture values of ONE frame, so the
// log-sum-exp is per lane: s += exp2(v - ref) (one v_exp_f32 + one add per Gaussian); ref is a true earlier maximum,
// raised on a wave-uniform slow path (first tile, or when a sum overflows f32).  ln2 (ref + K0 + log2 s) is finished in f64.
//
// History (profiles/r01_split_variants.txt, r01_score_variants.txt; the superseded kernels were removed in round 2): VALU
// kernel 64 TFLOP/s -> f32-input MFMA 102 -> three-piece bf16 split (six products) 186 -> two-piece f16 split with a separate
// constant MFMA 274 -> constants folded into the spare slot 300; the same scheme on 16x16x32 MFMAs measured 16.7 ms against
// 15.1 (more B-operand registers, more LDS fragment traffic: this kernel reads each of the 2 KS8 fragments of an m-tile once,
// 10 ds_read_b128 at D = 39, not once per pass) -> the m-tile loop scheduled by hand (process(), profiles/r19_score_schedule.txt):
// 14.8 -> 14.2 ms per step, results bit for bit -> the double buffer made a ring, two m-tiles per stage and barrier
// (profiles/r22_score_ring.txt): 14.03 -> 13.73 ms per step on one device, 13.63 -> 13.20 on another, results bit for bit -> one
// frame tile's chain at a time, the last tile's log-sum-exp carried under the next m-tile's first chain (process_carry(),
// PCL_SPLIT16_CARRY; profiles/r28_score_carry.txt), results bit for bit.
#include <stdlib.h>

#include "pcl_internal.h"

namespace {

#ifndef PCL_SPLIT_WG
#define PCL_SPLIT_WG 256    // threads per workgroup = 64 x (waves sharing one LDS copy of the A tile)
#endif
constexpr int WG = PCL_SPLIT_WG;
typedef float f16v __attribute__((ext_vector_type(16)));

#ifndef PCL_SPLIT16_NT
#define PCL_SPLIT16_NT 2
#endif
#ifndef PCL_SPLIT16_MINW
#define PCL_SPLIT16_MINW 3    // waves per SIMD (f16 x2 kernel: fits 168 VGPRs)
#endif
// The parameter ring of the m-tile loop: PCL_SPLIT16_RING stages of PCL_SPLIT16_MTS m-tiles each, one workgroup barrier per stage, a stage
// refilled RING - 1 stages ahead of its use.  RING x MTS <= 5 keeps three workgroups of the D = 39 kernel on a CU (10 KB per m-tile).
// Measured (profiles/r22_score_ring.txt; 2 x 1 is the double buffer of rounds 1-19): 2 x 2 is 2-3 % faster per step -- half the barriers,
// and a DMA has two m-tile periods to land; 3 x 1, 4 x 1 and 5 x 1 (a barrier per m-tile, counted waits) are no faster than 2 x 1.
#ifndef PCL_SPLIT16_RING
#define PCL_SPLIT16_RING 2
#endif
#ifndef PCL_SPLIT16_MTS
#define PCL_SPLIT16_MTS 2     // m-tiles staged per workgroup barrier
#endif
// The order of one m-tile in the KS8 <= 5 kernels (NT = 2): 1 = one frame tile's MFMA chain at a time, the other tile's log-sum-exp in
// its gaps, the last tile's carried under the first chain of the next m-tile (process_carry()); 0 = the order of rounds 19-22 (process()).
#ifndef PCL_SPLIT16_CARRY
#define PCL_SPLIT16_CARRY 1
#endif
typedef _Float16 h8v __attribute__((ext_vector_type(8)));

// The ring of the D-dimensional kernel.  D = 47 (KS8 = 6: 12 KB per m-tile, the rolled DMA loop) keeps the double buffer.
template <int D>
struct Ring {
    static constexpr int KS8 = (D + 7) / 8;
    static constexpr int R = KS8 > 5 ? 2 : PCL_SPLIT16_RING;
    static constexpr int MTS = KS8 > 5 ? 1 : PCL_SPLIT16_MTS;
    static constexpr int STAGE_CH = MTS * 2 * KS8;                              // 1-KiB chunks per stage
#ifdef PCL_DIAG_NOLSE
    static constexpr bool CARRY = false;
#else
    static constexpr bool CARRY = PCL_SPLIT16_CARRY && KS8 <= 5 && PCL_SPLIT16_NT == 2;
#endif
    // (the carried order parks each lane's output indices in LDS over the m-tile loop: the registers go to the held fragments)
    static constexpr size_t STASH = CARRY ? (size_t)WG * PCL_SPLIT16_NT * sizeof(long long) : 0;
    static constexpr size_t LDS = (size_t)R * STAGE_CH * 64 * 16 + 16 + STASH;  // static LDS per workgroup: the ring, s_ovf, the parked indices
    static_assert(R >= 2 && MTS >= 1, "a ring has at least two stages");
    static_assert(3 * LDS <= (160u << 10), "three workgroups per CU: the ring does not fit a third of the 160 KB of LDS");
    static_assert(LDS <= (56u << 10), "pcl_score_occupancy(ctx, 2) pads a workgroup to 56 KB");
};

// (a counted wait takes its count as an immediate)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int D, int NT>
__global__ __launch_bounds__(WG, PCL_SPLIT16_MINW * 256 / WG > 0 ? PCL_SPLIT16_MINW * 256 / WG : 1) void gmm_score_split16_kernel(
    const float *__restrict__ frames, const uint4 *__restrict__ pm, const float *__restrict__ fscale, const float *__restrict__ centers,
    int nmt_max, const ScoreTile *__restrict__ tiles, const ScoreSeg *__restrict__ segs, double *__restrict__ out,
    int *__restrict__ flags, const double *__restrict__ kzero, const int *__restrict__ n_on_pipe, const int *__restrict__ npt) {
    static_assert(D % 8 != 0, "the folded constants need a spare slot");
    constexpr int KS8 = (D + 7) / 8;       // K-steps of 16 over the 2D features (8 per half-wave)
    constexpr int CH = 2 * KS8;            // 1-KiB chunks per m-tile: two f16 pieces
    constexpr int SC = D / 8, JC = D % 8;  // the spare slot
    constexpr float FMAXH = 6.0e4f;
    const ScoreTile tile = tiles[blockIdx.x];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int half = lane >> 5;
    const int col = lane & 31;
    if (tile.seg_lo >= tile.seg_hi) {       // padding tile of the XCD-aware order
        if (threadIdx.x == 0) flags[blockIdx.x] = 0;
        return;
    }
    // tiles of the state's layout in use: all of them, or -- a split state, whose on-pipe mixtures are compacted to the front (round 6) --
    // ceil(on-pipe / 32)
    const int n_mtiles = npt[tile.state];
    __shared__ int s_ovf;
    if (threadIdx.x == 0) s_ovf = 0;
    __syncthreads();
    const int vend = segs[tile.seg_hi - 1].vstart + segs[tile.seg_hi - 1].len;
    const bool wave_active = tile.vstart + wave * NT * 32 < vend;
    const int wave_u = Ring<D>::CARRY ? __builtin_amdgcn_readfirstlane(wave) : 0;      // (on the scalar unit ahead of the branch, for the same reason as below)
    if (n_mtiles == 0) {                    // not one mixture of the state on the pipe: ln 0 for every frame (the coarse pass adds the rest), no flag
        if (wave_active) {
            for (int c = 0; c < NT; ++c) {
                int v = tile.vstart + (wave * NT + c) * 32 + col;
                // (the carried order: this path's frame index from a lane counted afresh, or the compiler keeps its pieces over the m-tile loop)
                if constexpr (Ring<D>::CARRY)
                    v = tile.vstart + (wave_u * NT + c) * 32 + ((int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 31);
                if (v < vend && half == 0) {
                    int lo = tile.seg0;
                    const int hi = tile.seg_hi - 1;
                    while (lo < hi && segs[lo + 1].vstart <= v) ++lo;
                    const ScoreSeg sg = segs[lo];
                    out[sg.out0 + (long long)(v - sg.vstart) * sg.out_stride] = -INFINITY;
                }
            }
        }
        if (threadIdx.x == 0) flags[blockIdx.x] = 0;
        return;
    }

    // ---- B operand: scaled features of this lane's frames in two f16 pieces (spare slot: x1 = [1 | -ref'])
    h8v xb[NT][2][KS8];
    long long oidx[NT];
    bool valid[NT];
    const float *cen = centers + (size_t)tile.state * D;
    const float *fs = fscale + ((size_t)tile.state * 2 + half) * (KS8 * 8);
    bool ovf = false;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        int v = tile.vstart + (wave * NT + c) * 32 + col;
        valid[c] = v < vend;
        if (!valid[c]) v = tile.vstart;
        // last segment with vstart <= v: almost always seg0 or its successor (two dependent loads instead of the
        // ~log2(#segments) of a full search, at the start of every tile), the search only for what is left
        int lo = tile.seg0, hi = tile.seg_hi - 1;
        if (lo < hi && segs[lo + 1].vstart <= v) {
            ++lo;
            if (lo < hi && segs[lo + 1].vstart <= v) {
                ++lo;
                while (lo < hi) {
                    int mid = (lo + hi + 1) >> 1;
                    if (segs[mid].vstart <= v) lo = mid; else hi = mid - 1;
                }
            }
        }
        const ScoreSeg sg = segs[lo];
        const long long t = v - sg.vstart;
        const float *fp = frames + (sg.frame0 + t) * D;
#pragma unroll
        for (int s = 0; s < KS8; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = 8 * s + j;
                float val = 0.f;
                if (d < D) {
                    const float xc = fp[d] - cen[d];
                    val = (half ? xc : xc * xc) * fs[d];
                    ovf |= __builtin_fabsf(val) > FMAXH;
                    val = __builtin_fminf(__builtin_fmaxf(val, -FMAXH), FMAXH);
                }
                if (d == D) val = half ? 0.f : 1.f;              // x1: [1 | -ref' (0 so far)]
                const _Float16 h1 = (_Float16)val;
                xb[c][0][s][j] = h1;
                xb[c][1][s][j] = (_Float16)(val - (float)h1);
            }
        oidx[c] = sg.out0 + t * (long long)sg.out_stride;
    }
    if (__any(ovf) && lane == 0) s_ovf = 1;

    float sm[NT], ref[NT];
    bool inited[NT];                          // the lane's frame has a log-sum-exp reference (a real value was seen)
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        sm[c] = 0.f;
        ref[c] = 0.f;
        inited[c] = false;
    }
    bool ref_ovf = false;

    // a ring of R stages of MTS m-tiles each: one workgroup barrier per MTS x 32 mixtures
    constexpr int R = Ring<D>::R, MTS = Ring<D>::MTS;
    constexpr bool CARRY = Ring<D>::CARRY && NT == PCL_SPLIT16_NT;
    __shared__ __attribute__((aligned(16))) uint4 abuf[R][MTS * CH * 64];
    const uint4 *pstate = pm + (size_t)tile.state * nmt_max * (CH * 64);
    // every wave issues its share of the stage's 1-KiB chunks: the chunk index is wave-uniform, so it is kept on the scalar unit
    // (readfirstlane) and the 2-3 trips are unrolled -- as a loop over threadIdx.x >> 6 each trip cost ~5 VALU instructions
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    // (the carried order holds ten fragments, two accumulators and the sums over the whole m-tile: the output indices, needed again only
    //  behind the loop, wait in LDS, each lane's own slots and -1 for a frame past the end, addressed by what the loop keeps anyway, so
    //  that the D = 39 kernel keeps 168 registers without scratch)
    __shared__ long long s_oidx[Ring<D>::CARRY ? NT : 1][Ring<D>::CARRY ? WG : 1];
    if constexpr (Ring<D>::CARRY) {
#pragma unroll
        for (int c = 0; c < NT; ++c) s_oidx[c][wave_s * 64 + lane] = valid[c] ? oidx[c] : -1;
    }
    auto dma = [&](int buf, int stage) {
        const uint4 *src = pstate + (size_t)stage * (MTS * CH * 64);
        const int nch = min(MTS, n_mtiles - stage * MTS) * CH;
        if constexpr (KS8 > 5) {                   // D = 47 keeps the loop: unrolled it measured 3 % slower there (one more spill in the m-tile loop)
            for (int p = wave; p < nch; p += WG / 64)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + p * 64 + lane),
                                                 (__attribute__((address_space(3))) void *)&abuf[buf][p * 64], 16, 0, 0);
            return;
        }
#pragma unroll
        for (int i = 0; i < (MTS * CH + WG / 64 - 1) / (WG / 64); ++i) {
            const int p = wave_s + i * (WG / 64);
            if (p >= nch) continue;
            if constexpr (R == 2) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + p * 64 + lane),
                                                 (__attribute__((address_space(3))) void *)&abuf[buf][p * 64], 16, 0, 0);
            } else {
                // The same instruction written out (m0 = the chunk's LDS address, as the builtin sets it).  The compiler counts the
                // builtin's DMAs itself, and with one of them in flight across the loop's back edge it puts vmcnt(0) in front of the first
                // LDS read of every m-tile, whichever buffer that reads: the ring would drain once per m-tile.  The waits of these are the
                // counted ones of the stage loop below and nothing else.  (m0 is reserved: the compiler keeps nothing in it from one
                // statement to the next and sets it in front of every instruction that reads it, so it is not on the clobber list.)
                const unsigned lds = (unsigned)(size_t)(__attribute__((address_space(3))) char *)&abuf[buf][p * 64];
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
                             :: "s"(lds), "v"(src + p * 64 + lane) : "memory");
            }
        }
    };

#ifdef PCL_SPLIT_STAMPS
    unsigned long long st_acc[4] = {0, 0, 0, 0}, st_t = 0;
#define SSTAMP(k) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[k] += t_ - st_t; st_t = t_; }
#else
#define SSTAMP(k)
#endif
    // The carried order's log-sum-exp of one frame tile's accumulator: the 32 operations of process()'s lse_op and the same pairwise
    // tree -- P(r) = e[r] + e[r + 8], Q(r) = P(r) + P(r + 4), R(r) = Q(r) + Q(r + 2), S = R(0) + R(1), sm + S -- walked depth first, so
    // that five partial sums are live instead of nine: every add has the operands it has there, so every sum is that one bit for bit.
    // (Those four registers are what keeps all 2 KS8 fragments, both accumulators and the sums of the D = 39 kernel within 168.)
    // LSE_WALK[k] = {kind, dst, src}: kind 0: t[dst] = exp2(a[src]), 1: t[dst] += t[src], 2: sn = sm[c] + t[0].
    auto lse_step = [&](const f16v &a, float (&t)[5], float &sn, int c, int k) {
        constexpr signed char LSE_WALK[32][3] = {
            {0, 0, 0}, {0, 1, 8},  {1, 0, 1}, {0, 1, 4}, {0, 2, 12}, {1, 1, 2}, {1, 0, 1},                   // Q(0)
            {0, 1, 2}, {0, 2, 10}, {1, 1, 2}, {0, 2, 6}, {0, 3, 14}, {1, 2, 3}, {1, 1, 2}, {1, 0, 1},        // Q(2), R(0)
            {0, 1, 1}, {0, 2, 9},  {1, 1, 2}, {0, 2, 5}, {0, 3, 13}, {1, 2, 3}, {1, 1, 2},                   // Q(1)
            {0, 2, 3}, {0, 3, 11}, {1, 2, 3}, {0, 3, 7}, {0, 4, 15}, {1, 3, 4}, {1, 2, 3}, {1, 1, 2},        // Q(3), R(1)
            {1, 0, 1}, {2, 0, 0}};                                                                           // S, sm + S
        const int kind = LSE_WALK[k][0], dst = LSE_WALK[k][1], src = LSE_WALK[k][2];
        if (kind == 0) t[dst] = __builtin_amdgcn_exp2f(a[src]);
        else if (kind == 1) t[dst] += t[src];
        else sn = sm[c] + t[0];
    };
    // frame tile c's accumulator a of one m-tile and the sum sn = sm[c] + (its 16 exponentials) go into sm[c]; on the wave-uniform slow
    // path the reference moves first, and with it the spare slot of xb[c] that every later MFMA chain of tile c subtracts
    // (the statements are those at the end of process(), where the comments are; that copy stays as it is so that PCL_SPLIT16_CARRY=0 and
    //  the D = 47 kernel compile to the code they had)
    auto settle = [&](f16v &a, int c, float sn) {
        if (__any(!inited[c]) | __any(!(sn < 3.0e38f))) {
            float gm = a[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) gm = __builtin_fmaxf(gm, a[r]);
            const float gp = __builtin_fmaxf(gm, __shfl_xor(gm, 32, 64));
            float s = sm[c];
            const bool first = !inited[c];
            if ((first || gp > 0.f) && gp > -5.0e4f) {
                const _Float16 r1 = (_Float16)__builtin_fminf(__builtin_fmaxf(-(ref[c] + gp), -FMAXH), FMAXH);
                const float nref = -(float)r1, dl = nref - ref[c];
                ref_ovf |= __builtin_fabsf(nref) > 5.0e4f;
#ifdef PCL_LSE_FLUSH_REPRO                                    // mutation build (tests are expected to FAIL on it)
                s = first ? 0.f : s * __builtin_amdgcn_exp2f(-dl);
#else
                const float hs = __builtin_amdgcn_exp2f(-0.5f * dl);
                s = first ? 0.f : (s * hs) * hs;
#endif
                inited[c] = true;
#pragma unroll
                for (int r = 0; r < 16; ++r) a[r] -= dl;
                ref[c] = nref;
                if (half) xb[c][0][SC][JC] = r1;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s += __builtin_amdgcn_exp2f(a[r]);
            sm[c] = s;
        } else {
            sm[c] = sn;
        }
    };
    auto process = [&](int mt) {
        const uint4 *ab = &abuf[(unsigned)(mt / MTS) % R][(mt % MTS) * (CH * 64)];
        f16v acc[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
        // Schedule (the results are those of the plain three-pass loop bit for bit: every accumulator still sees a2x1 s0.., a1x2 s0..,
        // a1x1 s0.. in that order).  All 2 KS8 fragments of the m-tile are read once, ahead of use: two before the first MFMA, the
        // rest under the first MFMAs, so that the waits of the later steps find them landed -- left to itself the compiler issues
        // every batch of reads right before a full lgkmcnt(0), three exposed LDS round trips per m-tile.  The a1 passes then run one frame
        // tile at a time, so that the log-sum-exp of frame tile c - 1 issues in the gaps of tile c's MFMAs (two exponentials and an
        // add per 32-cycle gap) and only the last tile's runs with no MFMA of this wave in flight.  sched_barrier pins that order.
        auto frag = [&](int pa, int s) { return *reinterpret_cast<const h8v *>(&ab[(pa * KS8 + s) * 64 + lane]); };
        auto mfma = [&](const h8v &a, int c, int pb, int s) { acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, xb[c][pb][s], acc[c], 0, 0, 0); };
        // the log-sum-exp of frame tile c as 32 single operations in a fixed order (the sums are those of the pairwise tree
        // es[r] += es[r + w], w = 8, 4, 2, 1, whichever way the operations are spread over the MFMA gaps).  Plain v_add_f32: under
        // -O3 the compiler SLP-packs such adds into v_pk_add_f32, which costs far more than its issue slot beside MFMAs (in-kernel
        // stamps: log-sum-exp phase 1830 -> 1230 cycles per m-tile), so this file is built with -fno-slp-vectorize (Makefile).
        // (Pinning the adds with inline asm instead returned wrong sums: the hazard recogniser does not cover a transcendental
        // result consumed inside an asm block.)
        float es[8], eh, snew[NT];
        auto lse_op = [&](int c, int k) {
            if (k < 24) {
                const int r = k / 3;
                if (k % 3 == 0) es[r] = __builtin_amdgcn_exp2f(acc[c][r]);
                else if (k % 3 == 1) eh = __builtin_amdgcn_exp2f(acc[c][r + 8]);
                else es[r] += eh;
            } else if (k < 28) es[k - 24] += es[k - 24 + 4];
            else if (k < 30) es[k - 28] += es[k - 28 + 2];
            else if (k == 30) es[0] += es[1];
            else snew[c] = sm[c] + es[0];
        };
        // (KS8 > 5, D = 47: the fragments held ahead do not fit the 168 registers of three waves per SIMD beside the wider frame
        //  operand -- that kernel keeps the plain three-pass loop and the compiler's own order)
        if constexpr (KS8 <= 5) {
            // fragment f of the m-tile in the order of first use: the a2 set, then the a1 set
            h8v af[2 * KS8];
            auto rd = [&](int f) { af[f] = frag(f < KS8 ? 1 : 0, f % KS8); };
            constexpr int LATE = KS8 > 2 ? 2 : 0;          // read into the registers the first two a2 fragments leave
            rd(0);
            rd(1);
            __builtin_amdgcn_sched_barrier(0);
#ifdef PCL_SPLIT_PRIO
            __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
            for (int s = 0; s < KS8; ++s) {
#pragma unroll
                for (int c = 0; c < NT; ++c) {
                    mfma(af[s], c, 0, s);
                    if (s == 0 && c == 0) {                // behind the first MFMA: its wait is the one exposed round trip
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int f = 2; f < 2 * KS8 - LATE; ++f) rd(f);
                    }
                }
                if (s == 2) {
#pragma unroll
                    for (int f = 2 * KS8 - LATE; f < 2 * KS8; ++f) rd(f);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                // beside tile c's MFMAs: three operations of tile c - 1's log-sum-exp per gap
                int k = 0;
#pragma unroll
                for (int g = 0; g < 2 * KS8; ++g) {
                    mfma(af[KS8 + g % KS8], c, g < KS8 ? 1 : 0, g % KS8);
                    if (c == 0) __builtin_amdgcn_sched_barrier(0);
#ifndef PCL_DIAG_NOLSE
                    if (c > 0) {
#pragma unroll
                        for (int q = 0; q < 3 && k < 32; ++q, ++k) lse_op(c - 1, k);
                        __builtin_amdgcn_sched_barrier(0);
                    }
#endif
                }
#ifndef PCL_DIAG_NOLSE
                if (c > 0) {
#pragma unroll
                    for (; k < 32; ++k) lse_op(c - 1, k);
                }
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            auto pass = [&](int pa, int pb) {
#pragma unroll
                for (int s = 0; s < KS8; ++s) {
                    const h8v a = frag(pa, s);
#pragma unroll
                    for (int c = 0; c < NT; ++c) mfma(a, c, pb, s);
                }
            };
            pass(1, 0);
            pass(0, 1);
            pass(0, 0);
#ifndef PCL_DIAG_NOLSE
#pragma unroll
            for (int c = 0; c + 1 < NT; ++c)
#pragma unroll
                for (int k = 0; k < 32; ++k) lse_op(c, k);
#endif
        }
#ifndef PCL_DIAG_NOLSE
#pragma unroll
        for (int k = 0; k < 32; ++k) lse_op(NT - 1, k);
#endif
        SSTAMP(1)
#ifdef PCL_SPLIT_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
#ifdef PCL_DIAG_NOLSE
#pragma unroll
        for (int c = 0; c < NT; ++c) sm[c] += acc[c][0] + acc[c][15];
        return;
#endif
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            // (round 6: the reference is taken at the first tile that HAS a real value, not at tile 0 -- with most of a state's mixtures off
            //  the pipe its first 32 are often all log zero, which used to flag every tile of the state for the direct-form fix-up: 34 ms
            //  per EM iteration at 91 % off-pipe mixtures; a frame that never sees a value above the f16 constants' reach is flagged at the end)
            // (both votes always evaluated: the sum above stays in the block of the MFMAs it is scheduled beside)
            if (__any(!inited[c]) | __any(!(snew[c] < 3.0e38f))) {
                float gm = acc[c][0];
#pragma unroll
                for (int r = 1; r < 16; ++r) gm = __builtin_fmaxf(gm, acc[c][r]);
                const float gp = __builtin_fmaxf(gm, __shfl_xor(gm, 32, 64));
                float s = sm[c];
                const bool first = !inited[c];
                if ((first || gp > 0.f) && gp > -5.0e4f) {
                    // the reference the pipe subtracts is the f16-rounded one: shift by what it actually moves
                    const _Float16 r1 = (_Float16)__builtin_fminf(__builtin_fmaxf(-(ref[c] + gp), -FMAXH), FMAXH);
                    const float nref = -(float)r1, dl = nref - ref[c];
                    ref_ovf |= __builtin_fabsf(nref) > 5.0e4f;
                    // (in two half-steps: this path is entered when a sum overflows, i.e. with dl ~ 128, and exp2(-128) is a denormal that
                    //  v_exp_f32 flushes to 0 -- which dropped everything summed so far, up to a third of the frame's mass, rounds 1-5)
#ifdef PCL_LSE_FLUSH_REPRO                                    // mutation build (tests are expected to FAIL on it): rounds 1-5
                    s = first ? 0.f : s * __builtin_amdgcn_exp2f(-dl);
#else
                    const float hs = __builtin_amdgcn_exp2f(-0.5f * dl);
                    s = first ? 0.f : (s * hs) * hs;
#endif
                    inited[c] = true;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[c][r] -= dl;
                    ref[c] = nref;
                    if (half) xb[c][0][SC][JC] = r1;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) s += __builtin_amdgcn_exp2f(acc[c][r]);
                sm[c] = s;
            } else {
                sm[c] = snew[c];
            }
        }
        SSTAMP(2)
    };
    // The carried order (PCL_SPLIT16_CARRY, KS8 <= 5, NT = 2).  One frame tile's whole chain at a time -- a2x1 s0.., a1x2 s0.., a1x1 s0.. on
    // one accumulator, the first MFMA on C = 0 -- with the OTHER tile's 32 log-sum-exp operations in its gaps:
    //   chain(0) of m-tile k      beside it the log-sum-exp of tile 1 of m-tile k - 1, read from cacc[1], which nothing has overwritten yet;
    //                             behind it settle(1) of m-tile k - 1, so xb[1] is final before chain(1) reads it
    //   chain(1) of m-tile k      its first MFMA (C = 0) frees the old cacc[1]; beside it the log-sum-exp of tile 0 of m-tile k;
    //                             behind it settle(0) of m-tile k, before chain(0) of m-tile k + 1
    // sm, ref, inited and xb[c] move at the same points relative to the MFMAs that read xb[c] as in process(), and every sum keeps its
    // order: the results are process()'s bit for bit.  The first m-tile has nothing to carry: cacc[1] starts as a tile of log zeros, which
    // settles to what is there already (sm = 0 + 16 exp2(-6e4) = 0, no reference taken) -- under a test of mt the compiler sinks the whole
    // log-sum-exp out of chain(0)'s gaps into the branch.  The last m-tile leaves tile 1 to carry_tail() behind the stage loop, the one tail
    // per workgroup.  cacc[1] lives across the stage loop's wait and barrier -- registers only.  All 2 KS8 fragments are read under
    // chain(0) and held for chain(1).
    f16v cacc[2];
    if constexpr (CARRY) {
#pragma unroll
        for (int r = 0; r < 16; ++r) cacc[1][r] = -FMAXH;
    }
    auto process_carry = [&](int mt) {
        const uint4 *ab = &abuf[(unsigned)(mt / MTS) % R][(mt % MTS) * (CH * 64)];
        auto frag = [&](int pa, int s) { return *reinterpret_cast<const h8v *>(&ab[(pa * KS8 + s) * 64 + lane]); };
        h8v af[2 * KS8];                               // in the order of first use: the a2 set, then the a1 set
        auto rd = [&](int f) { af[f] = frag(f < KS8 ? 1 : 0, f % KS8); };
        float t[5], snew;
        rd(0);
        rd(1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            int k = 0;
#pragma unroll
            for (int g = 0; g < 3 * KS8; ++g) {
                const int s = g % KS8;
                const h8v &a = af[g < KS8 ? s : KS8 + s];
                const h8v &x = xb[c][g >= KS8 && g < 2 * KS8 ? 1 : 0][s];
                if (g == 0) {
                    f16v zero;
#pragma unroll
                    for (int r = 0; r < 16; ++r) zero[r] = 0.f;
                    cacc[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, x, zero, 0, 0, 0);
                } else {
                    cacc[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, x, cacc[c], 0, 0, 0);
                }
                if (g == 0) {
                    // the chain starts before anything waits for the other chain's last MFMA; behind chain(0)'s first MFMA the rest of
                    // the reads: the wait of the first two is the one exposed round trip
                    __builtin_amdgcn_sched_barrier(0);
                    if (c == 0) {
#pragma unroll
                        for (int f = 2; f < 2 * KS8; ++f) rd(f);
                    }
                }
                // three operations of the other tile's log-sum-exp per gap (the gap of the fragment reads takes none)
                if (c == 1 || g > 0) {
#pragma unroll
                    for (int q = 0; q < 3 && k < 32; ++q, ++k) lse_step(cacc[1 - c], t, snew, 1 - c, k);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (; k < 32; ++k) lse_step(cacc[1 - c], t, snew, 1 - c, k);       // (KS8 = 2: six gaps hold 18 of the 32)
            __builtin_amdgcn_sched_barrier(0);
            if (c == 0) {
                settle(cacc[1], 1, snew);
            } else {
                SSTAMP(1)
                settle(cacc[0], 0, snew);
                SSTAMP(2)
            }
        }
    };
    auto carry_tail = [&]() {                          // tile 1 of the last m-tile
        float t[5], snew;
#pragma unroll
        for (int k = 0; k < 32; ++k) lse_step(cacc[1], t, snew, 1, k);
        settle(cacc[1], 1, snew);
    };
    // The ring.  Stage st + R - 1 is issued right behind the barrier of stage st, which proves all four waves done with stage st - 1, whose
    // buffer it takes: R - 1 stages ahead of its use, so its DMA has (R - 1) x MTS m-tile periods to land.  With R = 2 (the default) nothing
    // younger is in flight at the wait: vmcnt(0) and the plain barrier.  With R > 2 a wave waits for ITS pieces of the oldest stage only:
    // LDS-DMA returns in order, so vmcnt(n) with n = the wave's DMA instructions of the R - 2 younger stages (a constant per wave while those
    // stages are full; anything else the wave has in flight only makes the wait stricter); the tail, where a younger stage is short or
    // absent, waits for everything; and the barrier is the bare instruction behind a wait for the wave's LDS operations, since the fence of
    // __syncthreads() (any fence, an LDS-only one included) drains the DMAs in flight with vmcnt(0).
    const int n_stages = (n_mtiles + MTS - 1) / MTS;
    dma(0, 0);
#pragma unroll
    for (int s = 1; s < R - 1; ++s)
        if (s < n_stages) dma(s, s);
#ifdef PCL_SPLIT_STAMPS
    st_t = __builtin_amdgcn_s_memtime();
#endif
    constexpr int NW = WG / 64, YLO = (R - 2) * ((MTS * CH) / NW), YHI = (R - 2) * ((MTS * CH) / NW + 1);
    for (int st = 0; st < n_stages; ++st) {
        // this wave's pieces of stage st have landed
        if (R > 2 && (st + R - 1) * MTS <= n_mtiles) {
            if (wave_s < (MTS * CH) % NW) wait_vmcnt<YHI>(); else wait_vmcnt<YLO>();
        } else {
            wait_vmcnt<0>();
        }
        SSTAMP(3)
        if constexpr (R == 2) {                             // nothing in flight here: the plain barrier, as ever
            __syncthreads();
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }                                                   // everyone's have landed; the buffer of stage st - 1 is free
        SSTAMP(0)
        if (st == 0 && threadIdx.x == 0) flags[blockIdx.x] = s_ovf;
        if (st + R - 1 < n_stages) dma((unsigned)(st + R - 1) % R, st + R - 1);
        if (wave_active) {
            const int mend = min(n_mtiles, (st + 1) * MTS);
            for (int mt = st * MTS; mt < mend; ++mt) {
                if constexpr (CARRY) process_carry(mt); else process(mt);
            }
        }
    }
    if constexpr (CARRY) {
        if (wave_active) carry_tail();
    }
#ifdef PCL_SPLIT_STAMPS
    if (blockIdx.x == 800 && lane == 0)
        printf("wave %d: per m-tile: dma-wait %llu  barrier %llu  dma-issue+lds+mfma %llu  lse %llu (memtime ticks)\n", wave,
               st_acc[3] / n_mtiles, st_acc[0] / n_mtiles, st_acc[1] / n_mtiles, st_acc[2] / n_mtiles);
#endif
    constexpr double LN2 = 0.693147180559945309417232121458;
    const double k0 = kzero[tile.state];
    // a frame no tile gave a reference: every on-pipe mixture log zero for it -- right (-inf) when the state HAS no on-pipe mixture, otherwise
    // out of the f16 constants' reach: the direct-form fix-up rescored the tile
    if (wave_active && n_on_pipe[tile.state] > 0) {
#pragma unroll
        for (int c = 0; c < NT; ++c) ref_ovf |= !inited[c];
    }
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        const double S = (double)sm[c] + (double)__shfl_xor(sm[c], 32, 64);
        if constexpr (Ring<D>::CARRY) {
            // (the lane counted afresh: an address the compiler shares with the store's is one more register held over the loop)
            oidx[c] = s_oidx[c][wave_s * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u))];
            valid[c] = oidx[c] >= 0;
        }
        if (valid[c] && half == 0) out[oidx[c]] = (S > 0) ? LN2 * ((double)ref[c] + k0 + ::log2(S)) : -INFINITY;
    }
    if (__any(ref_ovf) && lane == 0) s_ovf = 1;
    __syncthreads();
    if (threadIdx.x == 0 && s_ovf) flags[blockIdx.x] = 1;         // (the flag of the features was stored after the first barrier)
}

template <int D>
void launch16_t(pcl_ctx *ctx, pcl_batch *b, const ScoreTile *tiles, int n_tiles) {
    // pcl_score_occupancy(ctx, 2): dynamic LDS nobody reads, so that two instead of three scoring workgroups fit a CU and another kernel's
    // waves -- the token passing of a streamed decode -- find registers beside them (config 5 streamed: 0.79 -> 0.87 M frames/s; the
    // scoring kernel alone loses ~9 %, so the streamed decoder asks for it and nobody else does).  Per workgroup: 56 KB > 160 / 3.
    constexpr size_t static_lds = Ring<D>::LDS;
    const size_t pad = (ctx->score_wgs_per_cu == 2 && static_lds < (56u << 10)) ? (56u << 10) - static_lds : 0;
    hipLaunchKernelGGL((gmm_score_split16_kernel<D, PCL_SPLIT16_NT>), dim3(n_tiles), dim3(WG), pad, ctx->stream, ctx->frames32,
                       reinterpret_cast<const uint4 *>(ctx->pm16f.p), ctx->fscale, ctx->centers32, ctx->Mpad32 / 32, tiles, b->d_segs,
                       b->Bt, b->d_tile_flags, ctx->kzero, ctx->d_non, ctx->d_npt);
}

}  // namespace

int pcl_score_split16_tile_frames() { return WG / 64 * PCL_SPLIT16_NT * 32; }

int pcl_launch_score_split16(pcl_ctx *ctx, pcl_batch *b, const ScoreTile *tiles, int n_tiles) {
    if (n_tiles == 0) return PCL_OK;
    pcl_timer_begin(ctx, "score");
    switch (ctx->D) {
#define CASE(DD) case DD: launch16_t<DD>(ctx, b, tiles, n_tiles); break;
        PCL_MFMA_DIMS(CASE)
#undef CASE
        default: PCL_FAIL(ctx, PCL_ERR_INVALID, "internal: no split-f16 scoring kernel for D=%d", ctx->D);
    }
    pcl_timer_end(ctx, "score");
    HIPCHK(ctx, hipGetLastError());
    return PCL_OK;
}
