// hmm_fb_linear_mw.inc -- the scaled linear-domain forward-backward of hmm_fb_linear.inc for sentence HMMs of MORE than 64 states
// (included by hmm_dp.hip behind it; same reference lines, same helpers, same pass rule, same range test).
//
// A label of 21 units already has 65 states (AcousticModel.embedded: N = 3 L + 2); the log-domain multi-wave kernel (hmm_fb_kernel<2>)
// takes 11x the time per utterance there.  Here a chain is spread over NWC = ceil(N / 64) wavefronts (N <= 256): state i sits on lane
// i % 64 of chain wave i / 64; inside a wave the neighbour's value still comes through a DPP wave shift, and the ONE value that crosses
// a wave boundary per step (lane 63 -> lane 0 of the next wave, forward; lane 0 -> lane 63 of the wave before, backward) goes through
// LDS: the publishing lane writes its (mantissa, exponent) pair into a slot of the step's parity, all waves of the workgroup meet at one
// barrier per step, the reading lane picks it up -- two slots per wave, so that a wave running ahead cannot overwrite what a slower one
// still has to read.  The workgroup is 2 NWC waves: the first NWC walk alpha, the others walk beta once (and then only stand at the
// barriers: the same step loop, the same barrier, nothing to do in between).  Lanes beyond N are not switched off (every wave must reach
// every barrier, and a batch mixes utterances of different lengths): they carry zeros in their exponents, read column 0 and "store"
// into a dump slot with stride 0.  An utterance outside the exponent range is left to hmm_fb_kernel<2>, launched behind with the
// range record, which returns at once for the others.

template <int NWC>
struct MwShared {
    double xm[2][NWC][2];          // [direction][wave of the chain][parity of the step]: the value that crosses the wave boundary
    int xe[2][NWC][2];
    double red_d[NWC];
    int red_i[NWC];
};

// One walk along the chain (see le_chain) for EVERY wave of the workgroup, whatever it has to do in this pass: a forward chain wave (alpha),
// a backward chain wave (beta), or a backward wave whose beta is done and which only has to be at the barriers.
// Every wave of the workgroup runs the SAME instance in any given pass (two exist: with and without stores in the loop, chosen
// workgroup-uniformly), with ONE step loop and ONE barrier in it: the programming model promises that the waves of a workgroup meet at
// ONE `__syncthreads()`, not that barriers of different call sites count as the same one (a walk with an instance per role and a bare
// barrier loop for the idle waves was 14-20 % faster; DESIGN.md section 4.3, profiles/r06_fb_barrier_ab.txt).  The loop body is
// straight-line code for every role: the direction is DATA (`fwd`, wave-uniform: both wave shifts are made and
// one is selected; what is stored is selected the same way), a forward walk that keeps nothing and an idle wave store into the dump slot
// with stride 0 and read column 0.  (A first version chose the role by wave-uniform BRANCHES around the loads and stores: 45-60 % slower,
// because with memory operations under control flow the compiler waits for vmcnt(0) in every block instead of counting -- see le_chain.)
// c = this wave's place in its chain; `par` = parity of the boundary slots the NEXT read uses.
template <bool ANY_STORE, int NWC>
__device__ __forceinline__ void le_chain_mw(const bool fwd, const unsigned long long *__restrict__ Bl, long long bstride, int nsteps, int t0, int T, double as_m,
                                            int as_e, double ap_m, int ap_e, double &z, int &ez, double &p, int &ep, double *__restrict__ sm,
                                            int *__restrict__ se, long long sstride, double &s_out, int &e_out, int c, int lane,
                                            MwShared<NWC> &sh, int &par) {
    const int dir = fwd ? 0 : 1, tstep = fwd ? 1 : -1;
    const int nb = fwd ? c - 1 : c + 1;                      // the chain wave whose boundary lane feeds this wave's edge lane
    const bool has_nb = nb >= 0 && nb < NWC;
    const bool edge_in = lane == (fwd ? 0 : 63), edge_out = lane == (fwd ? 63 : 0);
    auto frame = [&](int step) { return min(max(t0 + tstep * step, 0), T - 1); };
    double s_last = s_out;
    int e_last = e_out;
    auto one = [&](unsigned long long wq, int t, bool renorm_now) {
        double cb, s;
        int kb, e0;
        emis_unpack(wq, cb, kb);
        const LeStep st(cb, kb, as_m, as_e, ap_m, ap_e);
        const double pr = shr_d(p), pl = shl_d(p);
        const int er = shr_i(ep, LE_FLOOR), el = shl_i(ep, LE_FLOOR);
        double pn = fwd ? pr : pl;
        int epn = fwd ? er : el;
        if (has_nb) {                                        // (wave-uniform, LDS only) the value from across the wave boundary, published one step ago
            const double xl = sh.xm[dir][nb][par];
            const int xe_ = sh.xe[dir][nb][par];
            pn = edge_in ? xl : pn;
            epn = edge_in ? xe_ : epn;
        }
        st.sum(z, ez, pn, epn, s, e0);
        if (ANY_STORE) {                                     // (workgroup-uniform, compile time: a pass in which NO wave keeps anything has no store in its loop)
            sm[(long long)t * sstride] = fwd ? s * cb : s;   // alpha_t = s b_t, beta_t = s (a wave that keeps nothing in this pass: the dump slot, stride 0)
            se[(long long)t * sstride] = fwd ? floor_add(e0, kb) : e0;
        }
        s_last = s;
        e_last = e0;
        st.publish(s, e0, z, ez, p, ep);
        if (renorm_now) le_renorm(z, ez, p, ep);
        if (edge_out) {
            sh.xm[dir][c][par ^ 1] = p;
            sh.xe[dir][c][par ^ 1] = ep;
        }
        __syncthreads();                                     // THE barrier of a step: every wave of the workgroup, whatever its role, here
        par ^= 1;
    };
    unsigned long long qa[FBL_BLK], qb[FBL_BLK];
    auto load = [&](unsigned long long (&q)[FBL_BLK], int blk) {
#pragma unroll
        for (int k = 0; k < FBL_BLK; ++k) q[k] = Bl[(long long)frame(blk * FBL_BLK + k) * bstride];
        __builtin_amdgcn_sched_barrier(0);
    };
    auto block = [&](unsigned long long (&q)[FBL_BLK], int blk) {
#pragma unroll
        for (int k = 0; k < FBL_BLK; ++k) one(q[k], t0 + tstep * (blk * FBL_BLK + k), k == FBL_BLK - 1);
    };
    auto tail = [&](unsigned long long (&q)[FBL_BLK], int blk, int rem) {
#pragma unroll
        for (int k = 0; k < FBL_BLK - 1; ++k)
            if (k < rem) one(q[k], t0 + tstep * (blk * FBL_BLK + k), k == rem - 1);
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

template <int NWC>
__global__ __launch_bounds__(128 * NWC) void hmm_fblm_kernel(const UttDesc *__restrict__ utts, const unsigned long long *__restrict__ Bp,
                                                            const int *__restrict__ kmax, const int *__restrict__ row_ptr,
                                                            const int *__restrict__ col_idx, const double *__restrict__ csr_val,
                                                            const double *__restrict__ logpi_in, double *__restrict__ alpha,
                                                            int *__restrict__ alpha_e, double *__restrict__ beta, int *__restrict__ beta_e,
                                                            double *__restrict__ pi_out, double *__restrict__ logp, double *__restrict__ qtrace,
                                                            int32_t *__restrict__ npass_out, int fix_pi, double threshold, double *__restrict__ dump) {
    constexpr int NP = 64 * NWC;
    const UttDesc d = utts[blockIdx.x];
    const int N = d.N, T = d.T;
    if (!pcl_fb_linear_ok(kmax, blockIdx.x, T)) return;              // hmm_fb_kernel<2>, launched behind, takes it (block-uniform)
    __builtin_amdgcn_s_setprio(3);
    __shared__ double a0s[NP], b0s[NP], lpi[NP], aom[NP];
    __shared__ int aoe[NP];
    __shared__ MwShared<NWC> sh;
    __shared__ double s_q;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool fwd = wave < NWC;
    const int c = fwd ? wave : wave - NWC, i = c * 64 + lane;
    const bool act = i < N;
    const unsigned long long *Bl = Bp + d.b_off + (act ? i : 0);
    double *dm = dump + lane;
    int *de = reinterpret_cast<int *>(dump + 64) + lane;
    double *Am = act ? alpha + d.b_off + i : dm, *Bm = act ? beta + d.b_off + i : dm;
    int *Ae = act ? alpha_e + d.b_off + i : de, *Be = act ? beta_e + d.b_off + i : de;
    const long long sstride = act ? N : 0;
    const LeTrans a = le_transitions(d, i, act, row_ptr, col_idx, csr_val);
    if (fwd) {
        aom[i] = a.ao_m;
        aoe[i] = a.ao_e;
        lpi[i] = act ? logpi_in[d.vec_off + i] : -INFINITY;
    }
    __syncthreads();
    const double an_m = i > 0 ? aom[i - 1] : 1.0;                    // the transition INTO this state from the one before it
    const int an_e = i > 0 ? aoe[i - 1] : LE_ZADD;
    FbPassRule rule(fix_pi, threshold);
    double *const trace = qtrace + (long long)blockIdx.x * PCL_MAX_PASS;
    int par = 0;
    bool beta_done = false;
    for (;;) {
        bool store = rule.may_be_last();
        FbPassRule::Verdict v{false, false};
        double qnew = 0.0;
        for (;;) {
            double z = 0.0, p = 0.0, am = 0.0, s_l = 0.0;
            int ez = LE_FLOOR, ep = LE_FLOOR, ae = LE_FLOOR, e_l = LE_FLOOR;
            const bool walk_b = !fwd && !beta_done;
            if (fwd) {
                // ---------------------------------------------------------------- forward (LHMM.py:335-351): alpha_0
                le_alpha0(act ? lpi[i] : -INFINITY, Bl, a, store, Am, Ae, am, ae, z, ez, p, ep);
                a0s[i] = act ? le_log(am, ae) : -INFINITY;
                if (lane == 63) {
                    sh.xm[0][c][par] = p;
                    sh.xe[0][c][par] = ep;
                }
            } else if (walk_b) {
                // ---------------------------------------------------------------- backward (LHMM.py:353-366)
                le_beta_last(Bl, N, T, act, a, an_m, an_e, Bm, Be, sstride, z, ez, p, ep);
                s_l = 1.0;
                e_l = 0;
                if (lane == 0) {
                    sh.xm[1][c][par] = p;
                    sh.xe[1][c][par] = ep;
                }
            }
            __syncthreads();                                             // the first boundary values are there
            // every wave of the workgroup through the SAME walk (one call, one step loop, one barrier per step).  A forward wave in a pass that
            // keeps nothing and a backward wave whose beta is done write into the dump slot (stride 0); the idle wave also walks on zeros
            // (its z / p start at the floor and it publishes what nobody reads -- the slots of direction 1 belong to the backward chain alone)
            const bool keep = fwd ? store : walk_b;
            // (which of the two instances: a WORKGROUP-uniform choice -- every wave takes the same one, so the barrier inside is the same barrier)
            if (store || !beta_done)
                le_chain_mw<true, NWC>(fwd, keep || fwd ? Bl : Bp + d.b_off, N, T - 1, fwd ? 1 : T - 2, T, a.as_m, a.as_e, fwd ? a.ao_m : an_m, fwd ? a.ao_e : an_e, z, ez, p, ep,
                                       keep ? (fwd ? Am : Bm) : dm, keep ? (fwd ? Ae : Be) : de, keep ? sstride : 0, s_l, e_l, c, lane, sh, par);
            else
                le_chain_mw<false, NWC>(fwd, keep || fwd ? Bl : Bp + d.b_off, N, T - 1, fwd ? 1 : T - 2, T, a.as_m, a.as_e, fwd ? a.ao_m : an_m, fwd ? a.ao_e : an_e, z, ez, p, ep,
                                        dm, de, 0, s_l, e_l, c, lane, sh, par);
            if (fwd) le_alpha_last(Bl, N, T, s_l, e_l, am, ae);
            else if (walk_b) b0s[i] = act ? le_log(s_l, e_l) : -INFINITY;             // ln beta_0(i) (T == 1: ln 1 = 0)
            beta_done = true;
            // Q over the chain's waves
            if (fwd) {
                const int em = wave_max_i(act ? ae : LE_FLOOR);
                if (lane == 0) sh.red_i[c] = em;
            }
            __syncthreads();
            int eM = LE_FLOOR;
#pragma unroll
            for (int k = 0; k < NWC; ++k) eM = max(eM, sh.red_i[k]);
            if (fwd) {
                const double sc = wave_sum_d(le_q_term(act, am, ae, eM));
                if (lane == 0) sh.red_d[c] = sc;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                double S = 0.0;
#pragma unroll
                for (int k = 0; k < NWC; ++k) S += sh.red_d[k];
                s_q = le_log(S, eM);
            }
            __syncthreads();
            qnew = s_q;
            v = rule.judge(qnew);
            if (!FbPassRule::replay(v, store)) break;
            store = true;                                                // the pass turned out to be the last: once more, with alpha going to HBM
            __syncthreads();
        }
        rule.record(v, qnew, trace, threadIdx.x == 0);
        // ---------------------------------------------------------------- pi (LHMM.py:447-452,470-471), the forward waves
        if (!fix_pi) {
            const double p0 = (fwd && act) ? a0s[i] + b0s[i] : -INFINITY;
            double mx = p0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
            if (fwd && lane == 0) sh.red_d[c] = mx;
            __syncthreads();
            double M = -INFINITY;
#pragma unroll
            for (int k = 0; k < NWC; ++k) M = fmax(M, sh.red_d[k]);
            __syncthreads();
            const double part = wave_sum_d((fwd && act && !isinf(M)) ? exp(p0 - M) : 0.0);
            if (fwd && lane == 0) sh.red_d[c] = part;
            __syncthreads();
            double tot = 0.0;
#pragma unroll
            for (int k = 0; k < NWC; ++k) tot += sh.red_d[k];
            const double n0 = isinf(M) ? M : M + log(tot);
            const double pv = exp(p0 - n0);                      // the reference stores pi = exp(.) and takes np.log of it again
            if (fwd) {
                lpi[i] = act ? log(pv) : -INFINITY;
                if (v.final_pass && act) pi_out[d.vec_off + i] = pv;
            }
        } else if (v.final_pass && fwd && act) {
            pi_out[d.vec_off + i] = exp(lpi[i]);
        }
        if (v.final_pass) {
            if (threadIdx.x == 0) rule.finish(qnew, logp + blockIdx.x, npass_out + blockIdx.x, trace);
            break;
        }
        __syncthreads();
    }
}

// xi, gamma, per-frame posteriors for N <= 64 NWC states: workgroup (w, u) of NWC waves takes the contiguous frames [t0, t1) like
// hmm_postl_kernel; wave c holds the states 64 c .. 64 c + 63.  What crosses a wave per frame -- the partial sum of the frame's
// normaliser and the one neighbour value w_{t+1}(64 (c + 1)) -- goes through LDS slots of the row's parity, one barrier per row.
template <int NWC>
__global__ __launch_bounds__(64 * NWC) void hmm_postlm_kernel(const UttDesc *__restrict__ utts, const unsigned long long *__restrict__ Bp,
                                                             const int *__restrict__ kmax, const int *__restrict__ row_ptr,
                                                             const int *__restrict__ col_idx, const double *__restrict__ csr_val,
                                                             const double *__restrict__ alpha, const int *__restrict__ alpha_e,
                                                             const double *__restrict__ beta, const int *__restrict__ beta_e,
                                                             double *__restrict__ lgam, double *__restrict__ ksai, const double *__restrict__ logp,
                                                             double *__restrict__ dump, double *__restrict__ part_m, int *__restrict__ part_e) {
    constexpr int NP = 64 * NWC;
    const int u = blockIdx.y, w = blockIdx.x, c = threadIdx.x >> 6, lane = threadIdx.x & 63, i = c * 64 + lane;
    const UttDesc d = utts[u];
    const int N = d.N, T = d.T;
    if (!pcl_fb_linear_ok(kmax, u, T)) return;                       // (hmm_fb_kernel<2> wrote this utterance's results itself)
    __shared__ double ps[2][NWC], wbm[2][NWC];
    __shared__ int wbe[2][NWC];
    const bool act = i < N;
    for (long long e = w * NP + threadIdx.x; e < (long long)N * N; e += (long long)NP * POSTL_W) ksai[d.mat_off + e] = -INFINITY;   // LHMM.py:404
    const LeTrans a = le_transitions(d, i, act, row_ptr, col_idx, csr_val);
    const LePostConst pc(logp[u]);
    double sm[3] = {0.0, 0.0, 0.0};
    int se[3] = {LE_FLOOR, LE_FLOOR, LE_FLOOR};
    const int chunk = (T + POSTL_W - 1) / POSTL_W, t0 = w * chunk, t1 = min(T, t0 + chunk);
    double *Gl = act ? lgam + d.b_off + i : dump + lane;
    const long long gstride = act ? N : 0;
    int par = 0;
    le_post_rows(d, alpha, alpha_e, beta, beta_e, Bp, act ? i : 0, t0, t1, [&](const LeRow &r, const LeRow &n, int t) {
        double g, wm;
        int ge, ae_l, we;
        r.gamma(act, g, ge, ae_l);
        const double part = wave_sum_d(pc.term(g, ge));
        n.w_value(act, wm, we);
        if (lane == 0) {
            ps[par][c] = part;
            wbm[par][c] = wm;
            wbe[par][c] = we;
        }
        __syncthreads();
        double ssum = 0.0;
#pragma unroll
        for (int k = 0; k < NWC; ++k) ssum += ps[par][k];
        ssum *= pc.rc0;
        double wn = shl_d(wm);
        int wen = shl_i(we, LE_FLOOR);
        if (c + 1 < NWC) {                                               // lane 63's neighbour sits on the next wave
            const double xm_ = wbm[par][c + 1];
            const int xe_ = wbe[par][c + 1];
            wn = lane == 63 ? xm_ : wn;
            wen = lane == 63 ? xe_ : wen;
        }
        par ^= 1;
        Gl[(long long)t * gstride] = pc.lgamma(g, ge, ssum);
        if (t < T - 1) le_post_accumulate(a, r.am, ae_l, g, ge, wm, we, wn, wen, sm, se);
    });
    le_post_store_parts(part_m, part_e, u, w, NP, i, act, sm, se);
}
