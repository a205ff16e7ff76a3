// hmm_fb_linear.inc -- (included by hmm_dp.hip inside its anonymous namespace, behind the log-domain kernel bodies)
// Baum-Welch forward / backward for left-to-right sentence HMMs in a SCALED LINEAR domain (gfx950).
//
// Replaces the same reference code as hmm_dp.hip's hmm_fb2_kernel + hmm_post_kernel (SURVEY.md section 8a rows A8..A12):
//   LHMM.__forward_algorithm   StatisticalModel/LHMM.py:335-351
//   LHMM.__backward_algorithm  StatisticalModel/LHMM.py:353-366
//   LHMM.__maximization        StatisticalModel/LHMM.py:426-471   (xi / gamma / pi)
//   LHMM.__expectation         StatisticalModel/LHMM.py:412-422   (Q)
//   LHMM.baulm_welch           StatisticalModel/LHMM.py:526-544   (pass loop, quirk Q6)
//   LHMM.update_acc            StatisticalModel/LHMM.py:486-500   (per-frame posteriors l - sum_value)
//
// Why.  The reference walks the lattice in the log domain: every step of the T-long dependent chain is a two-term
// log-sum-exp, ~35 dependent float64 instructions + a table read even after round 3's work (~680 cycles per step; it was the
// floor of BASELINE config 2 and the kernel furthest from any roof).  The same numbers are products and sums of
//   alpha_t(j) = (alpha_{t-1}(j) a_jj + alpha_{t-1}(j-1) a_{j-1,j}) b_j(o_t)
// so here every quantity is carried as  value = m * 2^e  with m a float64 and e an int32 kept PER LANE (per state): the
// step of the chain is two v_ldexp_f64 (aligning the two terms to the larger exponent), one add and one multiply, the
// exponents run on the integer pipe ahead of the mantissas, and nothing is ever exponentiated or logged inside the chain:
//   - exp(B_t(j)) is split OFF the chain, for all t in parallel, by hmm_emis_pack_kernel into one 64-bit word per (t, j):
//     a 16-bit power of two (k + 32768; 0 = outside the packed range, 65535 = ln 0) and the 48 leading mantissa bits of
//     2^frac in [1, 2) (rounded to nearest: 2^-49 relative per frame, ~3e-14 after 300 frames);
//   - per-lane exponents cannot underflow, so a state 5000 nats below the best one keeps its exact value, as in the reference's
//     log domain (a per-frame common scale would flush it to zero and turn a finite ln alpha into -inf);
//   - zero (ln 0 = -inf: the exit state's emission row, the entry state after t = 0, absent transitions) lives in the
//     EXPONENT: anything below LE_PZ is zero whatever its mantissa, zero factors add LE_ZADD, sums are floored at LE_FLOOR,
//     so no test of a mantissa sits on the chain;
//   - beta does not depend on pi, the only thing that changes between the passes of baulm_welch for an embedded HMM
//     (quirk Q6): the backward chain is walked ONCE per call (the reference recomputes identical numbers every pass), beside
//     the first forward pass; alpha is written to HBM only in the pass that can be the last one (the third with a free pi,
//     the first with a locked one; a call that ends on another pass repeats that forward pass with the stores on -- same
//     inputs, same bits);
//   - ln alpha / ln beta are what PCL_GET_ALPHA / PCL_GET_BETA return: they are produced on demand by
//     pcl_launch_fb_to_log (nothing on the device reads them in the log domain);
//   - xi, gamma and the per-frame posteriors (hmm_postl_kernel, eight waves per utterance, parallel over t) accumulate
//     m * 2^e pairs per lane and take ONE logarithm per (t, j) -- ln gamma_t(j), which the accumulate kernels and
//     PCL_GET_LGAMMA need in the log domain -- instead of three exponentials.
// Rounding: products and sums of float64 mantissas, ~4 roundings per step: |d ln alpha| ~ 1e-13 after 300 frames, below the
// reference's own log-domain rounding (an ulp of |ln alpha| ~ 2e4 is 3.6e-12 per step); golden G6 holds at 1e-10.
//
// Range.  int32 exponents hold as long as  (max|k_B| + max|k_A| + 4) (T + 2) + max|k_pi| < 2^26  and max|k_B| fits the
// packed word (|ln b| < 22000 nats).  hmm_emis_pack_kernel measures the three maxima per utterance; an utterance outside
// the range (frames 1e6 sigma away, a caller-supplied ln A of -1e9) runs the log-domain bodies of hmm_dp.hip (hmm_fb2_body /
// hmm_post_body) inside the same launches -- a block-uniform branch at the top of the two kernels.  PCL_FB_LINEAR=0 launches
// the log-domain kernels for everything (A/B).
constexpr double LOG2E = 1.4426950408889634074;
constexpr double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// ln(m 2^e); zero (e in the pseudo-zero region) -> -inf
__device__ __forceinline__ double le_log(double m, int e) {
    if (e < LE_PZ || !(m > 0.0)) return -INFINITY;
    return fma((double)e, LN2_HI, fma((double)e, LN2_LO, log(m)));
}
// x = ln v  ->  v = m 2^e with m in [1, 2).  x = -inf -> a zero factor.  |x| log2e < 2^27 is the caller's business.
__device__ __forceinline__ void exp_split(double x, double &m, int &e) {
    if (!(x > -INFINITY)) {
        m = 1.0;
        e = LE_ZADD;
        return;
    }
    const double k = rint(x * LOG2E);
    double r = fma(-k, LN2_HI, x);                // one rounding: the product is exact inside the fma
    r = fma(-k, LN2_LO, r);
    double p = 1.0 / 479001600.0;                 // degree-12 Taylor polynomial on |r| <= ln 2 / 2: 1.7e-16 relative
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);                           // in [0.707, 1.415]
    int ki = (int)k;
    if (p < 1.0) {
        p *= 2.0;
        ki -= 1;
    }
    m = p;
    e = ki;
}
// the packed emission word: [63:52] = field >> 4, [51:4] = 48 leading fraction bits of m in [1, 2), [3:0] = field & 15
__device__ __forceinline__ unsigned long long emis_pack(double m, int k) {
    unsigned long long bits = (unsigned long long)__double_as_longlong(m);
    unsigned long long frac = (bits & 0xfffffffffffffULL) + 8ULL;      // round the 4 dropped bits to nearest
    if (frac >> 52) {                                                   // 1.111..1 rounds up to 2.0 = 1.0 * 2^(k+1)
        frac = 0;
        k += 1;
    }
    const unsigned long long field = (unsigned long long)(k + 32768);
    return ((field >> 4) << 52) | (frac & 0xffffffffffff0ULL) | (field & 15ULL);
}
__device__ __forceinline__ void emis_unpack(unsigned long long w, double &m, int &k) {
    const unsigned int hi = (unsigned int)(w >> 32), lo = (unsigned int)w;
    const int field = (int)(((hi >> 20) << 4) | (lo & 15u));
    m = __hiloint2double((int)((hi & 0x000fffffu) | 0x3ff00000u), (int)(lo & 0xfffffff0u));
    k = (field == 65535) ? LE_ZADD : field - 32768;
}
constexpr unsigned long long EMIS_ZERO = (0xfffULL << 52) | 15ULL;     // field 65535: ln 0
constexpr double EMIS_MAX_ABS = 22000.0;                               // |ln b| the 16-bit power of two holds

// DPP wave shifts with an explicit value for the lane that has no source (lane 0 of wave_shr, lane 63 of wave_shl)
__device__ __forceinline__ int shr_i(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int shl_i(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x130, 0xf, 0xf, false); }
// mantissas: 0 for the lane without a source (bound_ctrl: no move to preset the destination).  The chains run with every lane
// switched on (round 6): the state after the last one is a lane that carries a zero, not a lane that is missing
__device__ __forceinline__ double shr_d(double v) {
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, true),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ double shl_d(double v) {
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, true),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, true));
}
// exponent arithmetic saturates (v_add_i32 / v_sub_i32 clamp: one instruction): a zero that keeps collecting zero factors -- the exit
// state, whose emission is ln 0 in every frame -- stops at INT_MIN instead of wrapping, and INT_MIN minus a real exponent stays there
__device__ __forceinline__ int floor_add(int a, int b) { return __builtin_elementwise_add_sat(a, b); }
__device__ __forceinline__ int le_sub(int a, int b) { return __builtin_elementwise_sub_sat(a, b); }

// ------------------------------------------------------------------------------------------------
// exp(B) off the chain: Bt (time-major ln b) -> packed words, and the per-utterance exponent maxima the range test needs:
// per utterance a record of PCL_FB_KREC ints: the emission maxima of the PACK_BLOCKS workgroups, then transitions, then the
// caller's ln pi (grid (PACK_BLOCKS, U); block 0 also looks at the utterance's ln A and ln pi).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int kabs(double x) {          // |rint(x log2e)| saturated; -inf (a zero) does not count
    if (x == -INFINITY) return 0;
    const double a = fabs(x) * LOG2E;
    return (a < 1073741824.0) ? (int)a + 1 : (1 << 30);  // (NaN and +inf saturate too)
}
constexpr int PACK_BLOCKS = 8;                 // workgroups per utterance (256 threads, 36 VGPRs: one fits beside three scoring waves of a SIMD at once)
__global__ __launch_bounds__(256) void hmm_emis_pack_kernel(const UttDesc *__restrict__ utts, const double *__restrict__ Bt,
                                                           unsigned long long *__restrict__ Bp, int *__restrict__ kmax,
                                                           const int *__restrict__ row_ptr, const double *__restrict__ csr_val,
                                                           const double *__restrict__ logpi) {
    __shared__ int red[4];
    const UttDesc d = utts[blockIdx.y];
    const long long n = (long long)d.N * d.T;
    int km = 0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += PACK_BLOCKS * 256) {
        const double x = Bt[d.b_off + e];
        unsigned long long w;
        if (x == -INFINITY) w = EMIS_ZERO;
        else if (!(fabs(x) < EMIS_MAX_ABS)) {
            w = 0;                                                    // outside the packed range: the utterance takes the log-domain bodies
            km = 1 << 30;
        } else {
            double m;
            int k;
            exp_split(x, m, k);
            w = emis_pack(m, k);
            km = max(km, abs(k) + 1);
        }
        Bp[d.b_off + e] = w;
    }
    km = wave_max_i(km);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = km;
    __syncthreads();
    // every workgroup owns its slot of the utterance's record: plain stores, no atomics, nothing to reset between calls
    int *rec = kmax + (size_t)PCL_FB_KREC * blockIdx.y;
    if (threadIdx.x == 0) rec[blockIdx.x] = max(max(red[0], red[1]), max(red[2], red[3]));
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        int ka = 0, kp = 0;
        const int nz = row_ptr[d.ptr_off + d.N];
        for (int k = threadIdx.x; k < nz; k += 64) ka = max(ka, kabs(csr_val[d.nnz_off + k]));
        for (int k = threadIdx.x; k < d.N; k += 64) kp = max(kp, kabs(logpi[d.vec_off + k]));
        ka = wave_max_i(ka);
        kp = wave_max_i(kp);
        if (threadIdx.x == 0) {
            rec[PACK_BLOCKS] = ka;
            rec[PACK_BLOCKS + 1] = kp;
        }
    }
}
static_assert(PACK_BLOCKS + 2 <= PCL_FB_KREC, "the per-utterance record holds the partial maxima of every packing workgroup + two");

constexpr int FBL_BLK = 4;      // frames of packed emissions in flight ahead of the recursion = steps between renormalisations

// ------------------------------------------------------------------------------------------------
// What the single-wave kernels here and the multi-wave kernels of hmm_fb_linear_mw.inc share: straight-line pieces only.  What
// decides a schedule -- where the neighbour's value comes from, the stores, the barrier, the double-buffered block / tail loop --
// stays written out in the two walks (le_chain here, le_chain_mw there).
// ------------------------------------------------------------------------------------------------
// m 2^e brought to the exponent E >= e of a sum (far below it: an exact 0.0)
__device__ __forceinline__ double le_align(double m, int e, int E) { return ldexp(m, max(le_sub(e, E), -4000)); }
// one more term into a lane's running sum  S = sm 2^se
__device__ __forceinline__ void le_accumulate(double g, int ge, double &sm, int &se) {
    const int e1 = max(se, ge);
    sm = le_align(sm, se, e1) + le_align(g, ge, e1);
    se = e1;
}
// state i's two stored transitions: to itself (s) and to the next state (o); absent, or a lane beyond N = a zero factor
struct LeTrans {
    double as_m = 1.0, ao_m = 1.0;
    int as_e = LE_ZADD, ao_e = LE_ZADD;
};
__device__ __forceinline__ LeTrans le_transitions(const UttDesc &d, int i, bool act, const int *__restrict__ row_ptr, const int *__restrict__ col_idx,
                                                  const double *__restrict__ csr_val) {
    LeTrans a;
    if (act) {
        const int sr0 = row_ptr[d.ptr_off + i] + d.nnz_off, sr1 = row_ptr[d.ptr_off + i + 1] + d.nnz_off;
        for (int k = sr0; k < sr1; ++k) {
            const int j = col_idx[k];
            if (j == i) exp_split(csr_val[k], a.as_m, a.as_e);
            else if (j == i + 1) exp_split(csr_val[k], a.ao_m, a.ao_e);
        }
    }
    return a;
}
// One step of a chain for one lane.  The loop-carried chain is  mul -> (DPP) -> ldexp -> add.  Three pieces, because the walks put
// their own work between them and the order in the source is the order the scheduler starts from (one function that took the
// neighbour's value and did the rest moved the publish in front of the stores: the same instructions in another order, measured 0.5-2 % slower):
//   LeStep st(...)  the step's unpacked emission (cb, kb) folded into the two transitions the lane publishes along: off the chain
//   [the walk selects the neighbour's published value (pn, epn)]
//   st.sum()        the step's sum s 2^e0 (alpha_t = s b_t, beta_t = s)
//   [the walk stores]
//   st.publish()    the lane's two published values move on
struct LeStep {
    double cz, cp;
    int kz, kp;
    __device__ __forceinline__ LeStep(double cb, int kb, double as_m, int as_e, double ap_m, int ap_e)
        : cz(cb * as_m), cp(cb * ap_m), kz(floor_add(kb, as_e)), kp(floor_add(kb, ap_e)) {}
    __device__ __forceinline__ void sum(double z, int ez, double pn, int epn, double &s, int &e0) const {
        e0 = max(ez, epn);
        s = ldexp(z, le_sub(ez, e0)) + ldexp(pn, le_sub(epn, e0));
    }
    __device__ __forceinline__ void publish(double s, int e0, double &z, int &ez, double &p, int &ep) const {
        z = s * cz;
        p = s * cp;
        ez = floor_add(e0, kz);
        ep = floor_add(e0, kp);
    }
};
// one common power of two for the lane's two published values
__device__ __forceinline__ void le_renorm(double &z, int &ez, double &p, int &ep) {
    const int x = __builtin_amdgcn_frexp_exp(z + p);
    z = ldexp(z, -x);
    p = ldexp(p, -x);
    ez = floor_add(ez, x);
    ep = floor_add(ep, x);
}
// alpha_0(i) = pi_i b_i(o_0) (LHMM.py:335-351) as a mantissa in [0.5, 1) and its exponent, kept in a pass that stores; the lane's first
// published values
__device__ __forceinline__ void le_alpha0(double lpi_i, const unsigned long long *__restrict__ Bl, const LeTrans &a, bool store, double *__restrict__ Am,
                                          int *__restrict__ Ae, double &m, int &e, double &z, int &ez, double &p, int &ep) {
    double pm, bm;
    int pe, bk;
    exp_split(lpi_i, pm, pe);
    emis_unpack(Bl[0], bm, bk);
    m = pm * bm;
    e = floor_add(pe, bk);
    {
        const int x = __builtin_amdgcn_frexp_exp(m);
        m = __builtin_amdgcn_frexp_mant(m);
        e = floor_add(e, x);
    }
    if (store) {
        Am[0] = m;
        Ae[0] = e;
    }
    z = m * a.as_m;
    p = m * a.ao_m;
    ez = floor_add(e, a.as_e);
    ep = floor_add(e, a.ao_e);
}
// alpha_{T-1}(i) = s b_{T-1} from the forward walk's last step (T == 1: alpha_0, which (am, ae) hold already)
__device__ __forceinline__ void le_alpha_last(const unsigned long long *__restrict__ Bl, int N, int T, double s_l, int e_l, double &am, int &ae) {
    if (T > 1) {
        double cb;
        int kb;
        emis_unpack(Bl[(long long)(T - 1) * N], cb, kb);
        am = s_l * cb;
        ae = floor_add(e_l, kb);
    }
}
// beta_{T-1} = 1 (LHMM.py:353-366, quirk Q8), stored; published: w_{T-1}(i) = b_i(o_{T-1}) * 1 along a_ii and the transition INTO
// the state (an); a lane beyond N: zero
__device__ __forceinline__ void le_beta_last(const unsigned long long *__restrict__ Bl, int N, int T, bool act, const LeTrans &a, double an_m, int an_e,
                                             double *__restrict__ Bm, int *__restrict__ Be, long long sstride, double &z, int &ez, double &p, int &ep) {
    double bm;
    int bk;
    Bm[(long long)(T - 1) * sstride] = 1.0;
    Be[(long long)(T - 1) * sstride] = 0;
    emis_unpack(Bl[(long long)(T - 1) * N], bm, bk);
    z = bm * a.as_m;
    p = bm * an_m;
    ez = act ? floor_add(bk, a.as_e) : LE_FLOOR;
    ep = act ? floor_add(bk, an_e) : LE_FLOOR;
}
// Q = LSE_i alpha_{T-1}(i) (LHMM.py:412-422, datasize == 1 on this path) = le_log(S, eM) with eM the largest exponent and S the sum of
// these terms; util.log_sum_exp returns the maximum itself when it is -inf (quirk Q4), as le_log does
__device__ __forceinline__ double le_q_term(bool act, double am, int ae, int eM) { return act ? le_align(am, ae, eM) : 0.0; }

// One walk along the chain: `nsteps` steps starting at frame t0 (forward: t0, t0 + 1, ...; backward: t0, t0 - 1, ...).
// State in / out: the lane's two published values (z for itself, p for its neighbour) with their exponents.
//   forward  (FWD):  neighbour = lane before (wave_shr); stored value of a step = alpha_t = s b_t       (STORE only)
//   backward (!FWD): neighbour = lane after  (wave_shl); stored value of a step = beta_t  = s           (always stored)
// (as, ap) = the transitions the published values travel along.  Bl = packed emissions + the lane's column (any valid
// column), bstride = N.  Called by EVERY lane of the wave (a lane beyond N carries a zero in its exponent and a stride of 0):
// the loop body itself has NO branch and every load and store in it is unconditional, so the compiler counts its s_waitcnt
// exactly -- with a predicated store or load inside the loop it falls back to vmcnt(0) in every block, which waits for the
// block's own prefetch and for the stores' acknowledgements (~800 cycles) -- and the row addresses stay scalar.
// Returns the last step's (s, e0).
template <bool FWD, bool STORE>
__device__ __forceinline__ void le_chain(const unsigned long long *__restrict__ Bl, long long bstride, int nsteps, int t0, int T, double as_m,
                                         int as_e, double ap_m, int ap_e, double &z, int &ez, double &p, int &ep, double *__restrict__ sm,
                                         int *__restrict__ se, long long sstride, double &s_out, int &e_out) {
    auto frame = [&](int step) {
        const int t = FWD ? t0 + step : t0 - step;
        return min(max(t, 0), T - 1);
    };
    double s_last = s_out;
    int e_last = e_out;
    auto one = [&](unsigned long long wq, int t) {
        double cb, s;
        int kb, e0;
        emis_unpack(wq, cb, kb);
        const LeStep st(cb, kb, as_m, as_e, ap_m, ap_e);
        const double pn = FWD ? shr_d(p) : shl_d(p);
        const int epn = FWD ? shr_i(ep, LE_FLOOR) : shl_i(ep, LE_FLOOR);
        st.sum(z, ez, pn, epn, s, e0);
        if (FWD) {
            if (STORE) {
                sm[(long long)t * sstride] = s * cb;
                se[(long long)t * sstride] = floor_add(e0, kb);
            }
        } else {
            sm[(long long)t * sstride] = s;
            se[(long long)t * sstride] = e0;
        }
        s_last = s;
        e_last = e0;
        st.publish(s, e0, z, ez, p, ep);
    };
    // two register sets of packed emissions, used alternately (a copy "next -> current" at the end of a block is hoisted by
    // the compiler to right behind the loads, with a wait for them: the prefetch would be waited for inside its own block)
    unsigned long long qa[FBL_BLK], qb[FBL_BLK];
    auto load = [&](unsigned long long (&q)[FBL_BLK], int blk) {
#pragma unroll
        for (int k = 0; k < FBL_BLK; ++k) q[k] = Bl[(long long)frame(blk * FBL_BLK + k) * bstride];
        // the loads stay HERE, ahead of the block's stores: the memory counter retires in order, and loads queued behind the
        // stores could only be waited for together with the stores' acknowledgements
        __builtin_amdgcn_sched_barrier(0);
    };
    auto block = [&](unsigned long long (&q)[FBL_BLK], int blk) {
#pragma unroll
        for (int k = 0; k < FBL_BLK; ++k) one(q[k], FWD ? t0 + blk * FBL_BLK + k : t0 - blk * FBL_BLK - k);
        le_renorm(z, ez, p, ep);
    };
    auto tail = [&](unsigned long long (&q)[FBL_BLK], int blk, int rem) {      // rem < FBL_BLK steps whose frames are in q already
#pragma unroll
        for (int k = 0; k < FBL_BLK - 1; ++k)
            if (k < rem) one(q[k], FWD ? t0 + blk * FBL_BLK + k : t0 - blk * FBL_BLK - k);
        if (rem > 0) le_renorm(z, ez, p, ep);
    };
    const int nblk = nsteps / FBL_BLK, rem = nsteps - nblk * FBL_BLK;
    load(qa, 0);
    int b = 0;
    for (; b + 2 <= nblk; b += 2) {
        load(qb, b + 1);
        block(qa, b);
        load(qa, b + 2);
        block(qb, b + 1);
    }
    if (b < nblk) {
        load(qb, b + 1);
        block(qa, b);
        tail(qb, b + 1, rem);
    } else {
        tail(qa, b, rem);
    }
    s_out = s_last;
    e_out = e_last;
}

// ------------------------------------------------------------------------------------------------
// The pass loop.  128 threads: wave 0 walks alpha (once per pass), wave 1 walks beta (once per call).  Lane i <-> state i.
// A lane PUBLISHES, after every step, its value already multiplied by the transition it will travel along:
//   forward:  z = alpha_t(i) a_ii  (for itself)       p = alpha_t(i) a_{i,i+1}  (for lane i + 1, read through wave_shr)
//   backward: z = w_t(i) a_ii      (for itself)       p = w_t(i) a_{i-1,i}      (for lane i - 1, read through wave_shl)
// with w_t(j) = b_j(o_t) beta_t(j); the multiplications by b_j(o_{t+1}) a.. of the NEXT step are folded into two constants
// per frame that do not depend on the chain.  The loop-carried chain of a step is  mul -> (DPP) -> ldexp -> add.
// ------------------------------------------------------------------------------------------------
// (3 waves per SIMD = at most 170 VGPRs, 149 used: what ONE retiring wave of the scoring kernel frees (154) -- with more, the two
//  waves of an utterance wait until two scoring waves of a SIMD retire together; profiles/r03_fb.txt)
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(3, 3))) void hmm_fbl_kernel(const UttDesc *__restrict__ utts, const unsigned long long *__restrict__ Bp,
                                                     const int *__restrict__ kmax, const int *__restrict__ row_ptr,
                                                     const int *__restrict__ col_idx, const double *__restrict__ csr_val,
                                                     const double *__restrict__ logpi_in, double *__restrict__ alpha,
                                                     int *__restrict__ alpha_e, double *__restrict__ beta, int *__restrict__ beta_e,
                                                     double *__restrict__ pi_out, double *__restrict__ logp, double *__restrict__ qtrace,
                                                     int32_t *__restrict__ npass_out, int fix_pi, double threshold, const double *__restrict__ Bt,
                                                     const int *__restrict__ col_ptr, const int *__restrict__ row_idx,
                                                     const double *__restrict__ csc_val, const double2 *__restrict__ softplus, double *__restrict__ dump) {
    const UttDesc d = utts[blockIdx.x];
    const int N = d.N, T = d.T;
    if (!pcl_fb_linear_ok(kmax, blockIdx.x, T)) {                    // outside the exponent range: the log-domain recursion (block-uniform)
        hmm_fb2_body(utts, Bt, row_ptr, col_idx, csr_val, col_ptr, row_idx, csc_val, logpi_in, alpha, beta, pi_out, logp, qtrace, npass_out, fix_pi,
                     threshold, softplus);
        return;
    }
    __builtin_amdgcn_s_setprio(3);
    __shared__ double a0s[64], b0s[64], lpi[64];
    __shared__ double s_q;
    const int w = threadIdx.x >> 6, i = threadIdx.x & 63;
    const bool act = i < N;
    // Round 6 (VERDICT r5 next #6): EVERY lane walks the chain.  Rounds 3-5 wrapped the walk in `if (act)` and relied on that branch staying
    // an EXEC mask, so that the DPP shift of the last state's lane found "no source" behind it -- right on this compiler, but nothing in the
    // language says a divergent branch may not become a select.  Now a lane beyond N is an ordinary lane that carries a zero: exponent at
    // LE_FLOOR, every transition a zero factor (LE_ZADD), so whatever its mantissa holds is 2^-(2^28) of anything real and the lane before
    // it adds exactly 0.0 (ldexp by less than -1100).  It reads column 0 (any valid column) and "stores" into a dump slot with stride 0,
    // as the lanes beyond N of hmm_fblm_kernel always did.  Same bits in every result of a real state (tools/fb_linear_fuzz.py).
    const unsigned long long *Bl = Bp + d.b_off + (act ? i : 0);
    double *dm = dump + i;
    int *de = reinterpret_cast<int *>(dump + 64) + i;
    double *Am = act ? alpha + d.b_off + i : dm, *Bm = act ? beta + d.b_off + i : dm;
    int *Ae = act ? alpha_e + d.b_off + i : de, *Be = act ? beta_e + d.b_off + i : de;
    const long long sstride = act ? N : 0;
    const LeTrans a = le_transitions(d, i, act, row_ptr, col_idx, csr_val);
    // the transition INTO this lane from the one before it (= that lane's a_{i-1,i}): what the backward chain publishes with
    const double an_m = __hiloint2double(shr_i(__double2hiint(a.ao_m), 0x3ff00000), shr_i(__double2loint(a.ao_m), 0));
    const int an_e = shr_i(a.ao_e, LE_ZADD);
    if (w == 0) lpi[i] = act ? logpi_in[d.vec_off + i] : -INFINITY;
    __syncthreads();
    FbPassRule rule(fix_pi, threshold);
    double *const trace = qtrace + (long long)blockIdx.x * PCL_MAX_PASS;
    bool beta_done = false;
    for (;;) {
        bool store = rule.may_be_last();
        FbPassRule::Verdict v{false, false};
        double qnew = 0.0;
        for (;;) {
            if (w == 0) {
                // ---------------------------------------------------------------- forward (LHMM.py:335-351)
                double m, z, p, am, s_l = 0.0;                            // (am, ae): alpha_{T-1}(i)
                int e, ez, ep, ae, e_l = LE_FLOOR;
                le_alpha0(act ? lpi[i] : -INFINITY, Bl, a, store, Am, Ae, m, e, z, ez, p, ep);
                a0s[i] = act ? le_log(m, e) : -INFINITY;
                if (store) le_chain<true, true>(Bl, N, T - 1, 1, T, a.as_m, a.as_e, a.ao_m, a.ao_e, z, ez, p, ep, Am, Ae, sstride, s_l, e_l);
                else le_chain<true, false>(Bl, N, T - 1, 1, T, a.as_m, a.as_e, a.ao_m, a.ao_e, z, ez, p, ep, Am, Ae, sstride, s_l, e_l);
                am = m;
                ae = e;
                le_alpha_last(Bl, N, T, s_l, e_l, am, ae);
                const int eM = wave_max_i(act ? ae : LE_FLOOR);
                const double S = wave_sum_d(le_q_term(act, am, ae, eM));
                if (i == 0) s_q = le_log(S, eM);
            } else if (!beta_done) {
                // ---------------------------------------------------------------- backward (LHMM.py:353-366)
                double z, p, s_l = 1.0;
                int ez, ep, e_l = 0;
                le_beta_last(Bl, N, T, act, a, an_m, an_e, Bm, Be, sstride, z, ez, p, ep);
                le_chain<false, true>(Bl, N, T - 1, T - 2, T, a.as_m, a.as_e, an_m, an_e, z, ez, p, ep, Bm, Be, sstride, s_l, e_l);
                b0s[i] = act ? le_log(s_l, e_l) : -INFINITY;             // ln beta_0(i) (T == 1: ln 1 = 0)
            }
            beta_done = true;
            __syncthreads();
            qnew = s_q;
            v = rule.judge(qnew);
            if (!FbPassRule::replay(v, store)) break;
            store = true;                                                // the pass turned out to be the last: once more, with alpha going to HBM
            __syncthreads();
        }
        rule.record(v, qnew, trace, threadIdx.x == 0);
        // ---------------------------------------------------------------- pi (LHMM.py:447-452,470-471), wave 0
        if (w == 0) {
            if (!fix_pi) {
                const double p0 = act ? a0s[i] + b0s[i] : -INFINITY;
                double mx = p0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
                const double n0 = isinf(mx) ? mx : mx + log(wave_sum_d(exp(p0 - mx)));
                const double pv = exp(p0 - n0);                  // the reference stores pi = exp(.) and takes np.log of it again
                lpi[i] = act ? log(pv) : -INFINITY;
                if (v.final_pass && act) pi_out[d.vec_off + i] = pv;
            } else if (v.final_pass && act) {
                pi_out[d.vec_off + i] = exp(lpi[i]);
            }
        }
        if (v.final_pass) {
            if (threadIdx.x == 0) rule.finish(qnew, logp + blockIdx.x, npass_out + blockIdx.x, trace);
            break;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// xi, gamma and the per-frame posteriors of the last pass (LHMM.py:394-405,431-445,486-500) from the (m, e) alpha / beta the
// chain kernel left: POSTL_W frame blocks per utterance; per lane three running sums (gamma_i, xi_ii, xi_{i,i+1}) as m 2^e pairs,
// merged over the blocks in block order (deterministic, independent of the batch).
//   ln gamma_t(i) - sum_value[t]:  sum_value[t] = LSE_i (alpha + beta) is ln P(O) up to rounding, so with
//   ssum = sum_i gamma / 2^eQ / c0 and c0 = P(O) / 2^eQ:  sum_value[t] = ln P(O) + ln ssum, the logarithm of a number within
//   1e-4 of 1 (three terms of its series; anything else takes log()).
// ------------------------------------------------------------------------------------------------
constexpr int POSTL_W = 8;
// the per-utterance constants of that, from ln P(O)
struct LePostConst {
    double qnew, rc0;                                                // ln P(O); 1 / c0, c0 = P(O) / 2^eQ in [0.7, 1.42]
    int eQ;
    bool dead;                                                       // P(O) = 0: every l is -inf, l - sum_value is NaN as in the reference
    __device__ __forceinline__ explicit LePostConst(double q) : qnew(q) {
        dead = !(qnew > -INFINITY);
        const double kq = rint(qnew * LOG2E);
        eQ = dead ? 0 : (int)kq;
        const double lc0 = dead ? 0.0 : fma(-kq, LN2_LO, fma(-kq, LN2_HI, qnew));
        rc0 = dead ? 1.0 : exp(-lc0);
    }
    // the lane's term of the frame's  sum_i gamma_t(i) / 2^eQ  (times rc0: ssum)
    __device__ __forceinline__ double term(double g, int ge) const { return le_align(g, ge, eQ); }
    // l[i,t] - sum_value[t] (LHMM.py:486-500) of gamma_t(i) = g 2^ge
    __device__ __forceinline__ double lgamma(double g, int ge, double ssum) const {
        const double u1 = ssum - 1.0;
        double corr;                                                 // sum_value[t] - ln P(O)
        if (fabs(u1) < 1.0e-4) corr = u1 * (1.0 - u1 * (0.5 - u1 * (1.0 / 3.0)));
        else corr = log(ssum);
        if (dead) return NAN;
        if (ge < LE_PZ || !(g > 0.0)) return -INFINITY;
        return (fma((double)ge, LN2_HI, fma((double)ge, LN2_LO, log(g))) - qnew) - corr;
    }
};
// A frame's row as the posterior kernels read it: alpha_t, beta_t and the packed emission of the lane's state
struct LeRow {
    double am, bm;
    int ae, be;
    unsigned long long w;
    // gamma_t(i) = alpha beta = g 2^ge, and alpha's exponent (a lane beyond N read column 0: its values count as zero)
    __device__ __forceinline__ void gamma(bool act, double &g, int &ge, int &ae_l) const {
        g = am * bm;
        ae_l = act ? ae : LE_FLOOR;
        ge = act ? floor_add(ae, be) : LE_FLOOR;
    }
    // w_t(i) = b_i(o_t) beta_t(i)
    __device__ __forceinline__ void w_value(bool act, double &wm, int &we) const {
        double bm1;
        int bk1;
        emis_unpack(w, bm1, bk1);
        wm = bm * bm1;
        we = act ? floor_add(be, bk1) : LE_FLOOR;
    }
};
// The rows of the CONTIGUOUS frames [t0, t1) through proc(row t, row t + 1, t): frame t needs alpha_t, beta_t and w_{t+1}, and row
// t + 1 is the block's own next row -- every row is read once (32 B per (t, j); with frames dealt round-robin, t, t + 8, ..., every
// block read its successor's row again: 44 B, and the kernel ran at the HBM's rate).  Three register sets in rotation, two rows
// in flight, loads unconditional (clamped frame, column `col` = 0 for lanes beyond N) so that the compiler counts its waits.
template <class Proc>
__device__ __forceinline__ void le_post_rows(const UttDesc &d, const double *__restrict__ alpha, const int *__restrict__ alpha_e,
                                             const double *__restrict__ beta, const int *__restrict__ beta_e, const unsigned long long *__restrict__ Bp,
                                             long long col, int t0, int t1, Proc proc) {
    const unsigned long long *B = Bp + d.b_off;
    const double *Am = alpha + d.b_off, *Bm = beta + d.b_off;
    const int *Ae = alpha_e + d.b_off, *Be = beta_e + d.b_off;
    const int N = d.N, T = d.T;
    auto ld = [&](LeRow &r, int t) {
        const long long o = (long long)min(t, T - 1) * N + col;
        r.am = Am[o]; r.ae = Ae[o]; r.bm = Bm[o]; r.be = Be[o]; r.w = B[o];
        __builtin_amdgcn_sched_barrier(0);
    };
    if (t0 < t1) {
        LeRow r0, r1, r2;
        ld(r0, t0);
        ld(r1, t0 + 1);
        int t = t0;
        for (;;) {
            ld(r2, t + 2); proc(r0, r1, t); if (++t >= t1) break;
            ld(r0, t + 2); proc(r1, r2, t); if (++t >= t1) break;
            ld(r1, t + 2); proc(r2, r0, t); if (++t >= t1) break;
        }
    }
}
// frame t < T - 1 into the lane's three running sums: gamma_i (LHMM.py:442-445) and
// xi_ij (+)= alpha_t(i) a_ij b_j(o_{t+1}) beta_{t+1}(j) (LHMM.py:394-405) for j = i (w) and j = i + 1 (the neighbour's: wn)
__device__ __forceinline__ void le_post_accumulate(const LeTrans &a, double am, int ae_l, double g, int ge, double wm, int we, double wn, int wen,
                                                   double (&sm)[3], int (&se)[3]) {
    le_accumulate(g, ge, sm[0], se[0]);
    le_accumulate(am * a.as_m * wm, floor_add(floor_add(ae_l, a.as_e), we), sm[1], se[1]);
    le_accumulate(am * a.ao_m * wn, floor_add(floor_add(ae_l, a.ao_e), wen), sm[2], se[2]);
}
// the block's three sums of state i into the utterance's partial sums ([u][3][POSTL_W][NP]) for hmm_postl_merge_kernel
__device__ __forceinline__ void le_post_store_parts(double *__restrict__ part_m, int *__restrict__ part_e, int u, int w, int NP, int i, bool act,
                                                    const double (&sm)[3], const int (&se)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t o = (((size_t)u * 3 + c) * POSTL_W + w) * NP + i;
        part_m[o] = sm[c];
        part_e[o] = act ? se[c] : LE_FLOOR;
    }
}

// ONE wave per workgroup, POSTL_W workgroups per utterance (grid (POSTL_W, U)): beside the scoring kernel a 512-thread workgroup needs
// room for 2 x 114 VGPRs on all four SIMDs of one CU at once -- two of the CU's three scoring workgroups gone together -- and the
// scoring kernel refills every slot the moment ONE retires, so the eight-wave kernel of rounds 3-4 spanned 9.6 ms per call inside the
// C4 loop (0.17 ms of work; profiles/r04_bench_kernel_stats.csv); one wave of 114 VGPRs fits where a single scoring wave (154) retired.
// The waves' partial sums go through HBM (18 KB per utterance) to hmm_postl_merge_kernel, which adds them in wave order.
__global__ __launch_bounds__(64) void hmm_postl_kernel(const UttDesc *__restrict__ utts, const unsigned long long *__restrict__ Bp,
                                                                const int *__restrict__ kmax, const int *__restrict__ row_ptr,
                                                                const int *__restrict__ col_idx, const double *__restrict__ csr_val,
                                                                const double *__restrict__ alpha, const int *__restrict__ alpha_e,
                                                                const double *__restrict__ beta, const int *__restrict__ beta_e,
                                                                double *__restrict__ lgam, double *__restrict__ ksai,
                                                                double *__restrict__ gamma_out, const double *__restrict__ logp,
                                                                const double *__restrict__ Bt, double *__restrict__ dump,
                                                                double *__restrict__ part_m, int *__restrict__ part_e) {
    const int u = blockIdx.y, w = blockIdx.x, i = threadIdx.x;
    const UttDesc d = utts[u];
    const int N = d.N, T = d.T;
    if (!pcl_fb_linear_ok(kmax, u, T)) {                             // alpha / beta of this utterance are logarithms: the log-domain posteriors,
        if (w == 0) hmm_post_body<1>(utts, u, Bt, row_ptr, col_idx, csr_val, alpha, beta, lgam, ksai, gamma_out, logp);   // one wave, every frame
        return;
    }
    const bool act = i < N;
    for (long long e = w * 64 + i; e < (long long)N * N; e += 64 * POSTL_W) ksai[d.mat_off + e] = -INFINITY;   // LHMM.py:404: ln 0 entries (the merge kernel writes the stored ones)
    const LeTrans a = le_transitions(d, i, act, row_ptr, col_idx, csr_val);
    const LePostConst pc(logp[u]);
    double sm[3] = {0.0, 0.0, 0.0};
    int se[3] = {LE_FLOOR, LE_FLOOR, LE_FLOOR};
    const int chunk = (T + POSTL_W - 1) / POSTL_W, t0 = w * chunk, t1 = min(T, t0 + chunk);
    double *Gl = act ? lgam + d.b_off + i : dump + i;                      // lanes beyond N "store" into a dump slot (stride 0)
    const long long gstride = act ? N : 0;
    le_post_rows(d, alpha, alpha_e, beta, beta_e, Bp, act ? i : 0, t0, t1, [&](const LeRow &r, const LeRow &n, int t) {
        double g, wm;
        int ge, ae_l, we;
        r.gamma(act, g, ge, ae_l);
        const double ssum = wave_sum_d(pc.term(g, ge)) * pc.rc0;
        Gl[(long long)t * gstride] = pc.lgamma(g, ge, ssum);
        if (t < T - 1) {
            n.w_value(act, wm, we);
            le_post_accumulate(a, r.am, ae_l, g, ge, wm, we, shl_d(wm), shl_i(we, LE_FLOOR), sm, se);
        }
    });
    le_post_store_parts(part_m, part_e, u, w, 64, i, act, sm, se);
}

// the partial sums of the POSTL_W frame blocks of an utterance, added in block order (deterministic, independent of the batch): ln gamma_i,
// ln xi_ii, ln xi_{i,i+1}; blockDim = NP = the posterior kernel's (64 for hmm_postl_kernel, 64 NWC for hmm_postlm_kernel<NWC>)
__global__ __launch_bounds__(256) void hmm_postl_merge_kernel(const UttDesc *__restrict__ utts, const int *__restrict__ kmax, const int *__restrict__ row_ptr,
                                                             const int *__restrict__ col_idx, const double *__restrict__ part_m,
                                                             const int *__restrict__ part_e, double *__restrict__ ksai, double *__restrict__ gamma_out) {
    const int u = blockIdx.x, i = threadIdx.x, NP = blockDim.x;
    const UttDesc d = utts[u];
    if (!pcl_fb_linear_ok(kmax, u, d.T) || i >= d.N) return;         // (the log-domain kernel wrote its results itself)
    double outv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t o = ((size_t)u * 3 + c) * POSTL_W * NP + i;
        int E = LE_FLOOR;
#pragma unroll
        for (int v = 0; v < POSTL_W; ++v) E = max(E, part_e[o + (size_t)v * NP]);
        double tsum = 0.0;
#pragma unroll
        for (int v = 0; v < POSTL_W; ++v) tsum += le_align(part_m[o + (size_t)v * NP], part_e[o + (size_t)v * NP], E);
        outv[c] = le_log(tsum, E);
    }
    gamma_out[d.vec_off + i] = outv[0];
    const int sr0 = row_ptr[d.ptr_off + i] + d.nnz_off, sr1 = row_ptr[d.ptr_off + i + 1] + d.nnz_off;
    for (int k = sr0; k < sr1; ++k) {
        const int j = col_idx[k];
        if (j == i) ksai[d.mat_off + (long long)i * d.N + i] = outv[1];
        else if (j == i + 1) ksai[d.mat_off + (long long)i * d.N + i + 1] = outv[2];
    }
}

// (m, e) -> ln, for PCL_GET_ALPHA / PCL_GET_BETA; utterances the log-domain kernels handled are copied
__global__ __launch_bounds__(256) void hmm_to_log_kernel(const UttDesc *__restrict__ utts, const int *__restrict__ kmax,
                                                        const double *__restrict__ m, const int *__restrict__ e, double *__restrict__ out) {
    const UttDesc d = utts[blockIdx.y];
    const long long n = (long long)d.N * d.T;
    const bool lin = pcl_fb_linear_ok(kmax, blockIdx.y, d.T);
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += 8 * 256)
        out[d.b_off + k] = lin ? le_log(m[d.b_off + k], e[d.b_off + k]) : m[d.b_off + k];
}

