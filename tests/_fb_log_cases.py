"""Inputs, float64 twins and long-double references of the log-domain forward-backward tests (tests/test_gpu_fb_log_edges.py on the
device, tests/test_fb_log_cases.py on the CPU).  pcl_launch_forward_backward (csrc/hmm_dp.hip) sends a batch whose HMMs all have at most
two predecessors and successors per state to hmm_fb2_kernel + hmm_post_kernel (N <= 64) or to hmm_fb_kernel<2> (N > 64); the drawn HMMs of
tests/test_gpu_fuzz_hmm.py essentially never have that shape unless they are left to right, so the cases here are built, not drawn.

  A  lse2_tab alone: T = 2, N = 64, ln pi = 0, every stored ln a = 0, states in (source, sink) pairs -- the source has its self-loop, the sink is
     entered from the source and from itself.  With the operands (hi, lo) in B[:, 0] of the pair and B[:, 1] = 0, alpha_1(sink) IS
     lse2_tab(hi, lo): m = 0 adds no rounding.  With them in B[:, 1], beta_0(source) is.  `lse2_tab_twin` restates the kernel's table step in
     float64 NumPy; the reference is np.log1p(np.exp(-d)) in long double.
  B  structure: rings, right-to-left chains, skip chains, two chains woven into each other, permutations with self-loops; each with a state
     nobody leaves, a state nobody enters, a state with its self-loop only; N and T at the edges of the wave, of the FB_AHEAD = 4 blocks and of
     the POST_W = 8 waves.  Reference: oracle/poccala_oracle.py baum_welch.
  C  the posterior kernel's own arithmetic (exp_neg, online_lse, the merge over 8 waves): the N <= 64 cases of B with |b| <= 8, the summed
     ln xi / ln gamma against a long-double restatement of LHMM.py:394-405, 431-445 on the oracle's float64 alpha / beta; `post_twin` is the
     kernel's arithmetic in float64 NumPy, wave by wave.

Everything is NumPy and the oracle.  A case is a dict: name, kind, variant, a (N, N) and pi (N,) as probabilities, B (N, T), lr (the library's
left-to-right rule holds for it), impossible (P(O) = 0 by construction)."""
import functools

import numpy as np

from oracle import poccala_oracle as po

LD = np.longdouble
SP_N, SP_MAX = 1281, 39.98                 # csrc/hmm_dp.hip: nodes of the table, and from where on lse2_tab returns the maximum itself
FB_AHEAD, POST_W, MAX_PASS = 4, 8, 16      # frames in flight in hmm_fb2_body, waves of hmm_post_kernel, PCL_MAX_PASS
KEYS = ('alpha', 'beta', 'lgamma', 'ksai', 'gamma', 'pi', 'logp', 'npass', 'qtrace')
SETTINGS = ((True, 0.64), (False, 0.64), (False, 1e9), (False, 1e-13))     # (fix_pi, threshold); with pi locked every threshold gives two passes


# ================================================================== A: the table log-sum-exp
@functools.lru_cache(maxsize=None)
def lse_d_set():
    """every d >= 0 the table step is held at (float64, sorted, unique): the 1281 nodes k / 32; the 1280 ties k / 32 + 1 / 64 of the round to
    nearest even, with the doubles next to each on both sides; 0, the smallest subnormal, 2^-53; 39.98 with two doubles on either side, 40, 41;
    4096 uniform draws on [0, 40)."""
    k = np.arange(SP_N, dtype=np.float64)
    t = tie_set()
    edge = [SP_MAX]
    for to in (0.0, np.inf):
        v = SP_MAX
        for _ in range(2):
            v = float(np.nextafter(v, to))
            edge.append(v)
    draws = np.random.default_rng(4021).uniform(0.0, 40.0, 4096)
    return np.unique(np.concatenate([k / 32.0, t, np.nextafter(t, 0.0), np.nextafter(t, np.inf), [0.0, 5e-324, 2.0 ** -53], edge, [40.0, 41.0], draws]))


def tie_set():
    return (np.arange(SP_N - 1, dtype=np.float64) + 0.5) / 32.0


@functools.lru_cache(maxsize=None)
def lse_operands():
    """(hi, lo) of every log-sum-exp of section A, padded to a multiple of 32 (a 64-state utterance holds 32 pairs): (0, -d) for the d-set,
    then d = +inf beside a finite operand and both operands -inf (quirk Q4)."""
    d = lse_d_set()
    hi = np.concatenate([np.zeros(d.size), [0.0, -np.inf]])
    lo = np.concatenate([-d, [-np.inf, -np.inf]])
    pad = -hi.size % 32
    return np.concatenate([hi, np.zeros(pad)]), np.concatenate([lo, np.zeros(pad)])


def lse_expected(hi, lo):
    """long double: -inf when both are (Q4), hi exactly from d = 39.98 on, hi + log1p(exp(-d)) below."""
    hi, lo = np.asarray(hi, np.float64), np.asarray(lo, np.float64)
    out = hi.astype(LD)
    with np.errstate(invalid='ignore'):
        d = hi - lo
        add = np.isfinite(hi) & (d < SP_MAX)
    out[add] += np.log1p(np.exp(-d[add].astype(LD)))
    return out


@functools.lru_cache(maxsize=None)
def softplus_table():
    """(f, s) at d = k / 32 as pcl_launch_forward_backward fills it."""
    d = np.arange(SP_N) / 32.0
    return np.log1p(np.exp(-d)), 1.0 / (1.0 + np.exp(d))


def lse2_tab_twin(a, b, c6_sign=1.0):
    """lse2_tab of csrc/hmm_dp.hip in float64 NumPy: the same table, coefficients and Horner order, every fma as a multiply and an add.
    c6_sign = -1: the mutant with the sixth-order coefficient's sign flipped (what the bound has to tell from the kernel)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    f, s = softplus_table()
    m, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid='ignore'):
        plain = np.isinf(m) | ~(m - lo < SP_MAX)
        d = np.where(plain, 0.0, m - lo)
    k = np.rint(d * 32.0).astype(np.int64)                    # __double2int_rn: ties to even
    x = d - k / 32.0                                          # (exact, as the kernel's fma is)
    sg = s[k]
    q = sg - sg * sg
    h = 1.0 - 2.0 * sg
    qh = q * h
    c6 = c6_sign * (q * (q * (120.0 * q - 30.0) + 1.0) * (1.0 / 720.0))
    c5 = qh * (1.0 - 12.0 * q) * (-1.0 / 120.0)
    c4 = q * (1.0 - 6.0 * q) * (1.0 / 24.0)
    c3 = qh * (-1.0 / 6.0)
    r = x * c6 + c5
    r = x * r + c4
    r = x * r + c3
    r = x * r + 0.5 * q
    r = x * r - sg
    return np.where(plain, m, m + (x * r + f[k]))


@functools.lru_cache(maxsize=None)
def lse_twin_error(c6_sign=1.0):
    """the twin's worst absolute error against the long-double reference over the d-set; the device is held to twice this."""
    hi, lo = lse_operands()
    want = lse_expected(hi, lo)
    fin = np.isfinite(hi)
    return float(np.abs(lse2_tab_twin(hi[fin], lo[fin], c6_sign).astype(LD) - want[fin]).max())


def lse_pairs(cross):
    """(source, sink) of the 32 pairs.  Neighbours (2k, 2k + 1): every lane's operands are its own and the lane's before / after it, the
    utterance takes the wave-shift branch of hmm_fb2_body.  cross: the first pair is (0, 63), the others (2k - 1, 2k): lane 63 reads lane 0
    and lane 0 reads lane 63, the utterance takes the cross-lane branch with the same arithmetic."""
    if not cross:
        return [(2 * k, 2 * k + 1) for k in range(32)]
    return [(0, 63)] + [(2 * k - 1, 2 * k) for k in range(1, 32)]


def lse_batch(order, cross):
    """one batch of section A: U / 2 utterances whose alpha_1(sink) and U / 2 whose beta_0(source) are the log-sum-exps of lse_operands().
    order 0: the larger operand sits on the source (the first stored predecessor / successor), 1: on the sink (the second).
    -> dict(a (64, 64) 0 / 1, Bs, alpha_read / beta_read (utterance, state) index arrays in the order of lse_operands())."""
    hi, lo = lse_operands()
    pairs = np.array(lse_pairs(cross))
    src, snk = pairs[:, 0], pairs[:, 1]
    a = np.zeros((64, 64))
    a[np.arange(64), np.arange(64)] = 1.0
    a[src, snk] = 1.0
    first, second = (hi, lo) if order == 0 else (lo, hi)
    C = hi.size // 32
    Bs = []
    for col in (0, 1):                                        # operands in frame 0: alpha_1; in frame 1: beta_0
        for c in range(C):
            B = np.zeros((64, 2))
            B[src, col] = first[32 * c:32 * c + 32]
            B[snk, col] = second[32 * c:32 * c + 32]
            Bs.append(B)
    utt = np.repeat(np.arange(C), 32)
    return dict(a=a, Bs=Bs, alpha_read=(utt, np.tile(snk, C)), beta_read=(utt + C, np.tile(src, C)))


# ================================================================== B: structures of degree <= 2
KINDS = ('ring', 'r2l', 'skip', 'weave', 'perm')
VARIANTS = ('plain', 'nosucc', 'nopred', 'selfonly')
T_FB = (1, 2, 3, 4, 5, 6, 8, 9)                # every tail of the FB_AHEAD = 4 blocks, forward (T - 1 steps) and backward
T_POST = (7, 8, 9, 15, 16, 17)                 # POST_W = 8: waves without a frame, one and two frames per wave, the tails
T_SMALL = tuple(sorted(set(T_FB + T_POST)))
N_SMALL = (2, 3, 63, 64)
N_WIDE = (65, 128, 129, 257)
T_WIDE = (1, 2, 3, 20)
EMIS = ('near', 'far', 'holes')


def successor(kind, n, rng):
    """the second transition of every state besides its self-loop (-1: none)."""
    i = np.arange(n)
    if kind == 'ring':
        return (i + 1) % n
    if kind == 'r2l':
        return i - 1
    if kind == 'skip':
        return np.where(i + 2 < n, i + 2, -1)
    if kind == 'weave':                        # even states left to right, odd states right to left
        return np.where(i % 2 == 0, np.where(i + 2 < n, i + 2, -1), i - 2).clip(-1)
    if kind == 'l2r':
        return np.where(i + 1 < n, i + 1, -1)
    assert kind == 'perm'
    s = np.arange(n)                           # one cycle through every state (Sattolo): no fixed point
    for k in range(n - 1, 0, -1):
        j = int(rng.integers(0, k))
        s[k], s[j] = s[j], s[k]
    return s


def structure(kind, variant, n, rng):
    nxt = successor(kind, n, rng)
    x = rng.uniform(0.1, 0.9, n)
    a = np.zeros((n, n))
    for i in range(n):
        if nxt[i] < 0 or nxt[i] == i:
            a[i, i] = 1.0
        else:
            a[i, i], a[i, nxt[i]] = x[i], 1.0 - x[i]
    s = n // 2
    if variant == 'nosucc':
        a[s, :] = 0.0
    elif variant == 'nopred':
        a[:, s] = 0.0
    elif variant == 'selfonly':
        a[s, :] = 0.0
        a[s, s] = 1.0
    else:
        assert variant == 'plain'
    pi = np.zeros(n)                           # exact zeros everywhere but on the first, the altered and the last state
    sup = support(n)
    pi[sup] = rng.dirichlet(np.ones(len(sup)))
    return a, pi


def support(n):
    return sorted({0, n // 2, n - 1})


def emissions(emis, n, T, rng):
    """near / holes: a few nats around -85.  The states pi starts in differ by 80 nats each in the first frame, so that the re-estimation of
    pi (the only thing the pass loop changes) settles in a few passes: the gain of pass k is about e^(-25 k), and a threshold of 1e-13 is
    met after several passes, not after more than PCL_MAX_PASS.  State 0 has pi > 0, its self-loop and no hole: P(O) > 0."""
    if emis == 'near':
        b = -85.0 + 4.0 * rng.standard_normal((n, T))
        b[support(n), 0] = -85.0 - 80.0 * np.arange(len(support(n)))
        return b
    if emis == 'far':                          # aligned speech: the wrong states are hopeless
        return -3000.0 + 900.0 * rng.standard_normal((n, T))
    if emis == 'unit':
        return rng.uniform(-8.0, 8.0, (n, T))
    assert emis == 'holes'
    b = -85.0 + 4.0 * rng.standard_normal((n, T))
    b[rng.random((n, T)) < 0.08] = -np.inf
    b[0] = np.where(np.isfinite(b[0]), b[0], -85.0)
    b[support(n), 0] = -85.0 - 80.0 * np.arange(len(support(n)))
    return b


def is_left_right(a):
    """pcl_batch_upload_sparse: every stored transition goes to the state itself or the next one."""
    i, j = np.nonzero(a)
    return bool(((j == i) | (j == i + 1)).all())


def case(kind, variant, n, T, emis, salt=0):
    rng = np.random.default_rng([KINDS.index(kind) if kind in KINDS else 9, VARIANTS.index(variant), n, T, EMIS.index(emis) if emis in EMIS else 9, salt])
    a, pi = structure(kind, variant, n, rng)
    return dict(name='%s/%s N=%d T=%d %s' % (kind, variant, n, T, emis), kind=kind, variant=variant, a=a, pi=pi, B=emissions(emis, n, T, rng),
                lr=is_left_right(a), impossible=False)


def impossible(c, t):
    c = dict(c, name=c['name'] + ' impossible', B=c['B'].copy(), impossible=True)
    c['B'][:, t] = -np.inf                     # a frame nobody can emit
    return c


def small_cases(emis_of):
    """every kind x variant x N of N_SMALL; T walks through T_SMALL, the emissions through emis_of(index)."""
    out = []
    for kind in KINDS:
        for variant in VARIANTS:
            for n in N_SMALL:
                k = len(out)
                out.append(case(kind, variant, n, T_SMALL[k % len(T_SMALL)], emis_of(k)))
    return out


@functools.lru_cache(maxsize=None)
def groups():
    """name -> list of cases: one batch each.  'lr_alone' holds the left-to-right HMMs of 'mixed' and nothing else."""
    g = {}
    g['small'] = small_cases(lambda k: EMIS[(k // len(T_SMALL) + k) % 3]) + [impossible(case('ring', 'plain', 64, 9, 'near'), 4)]
    g['sweep'] = [case('ring', 'plain', 64, T, EMIS[k % 2]) for k, T in enumerate(T_SMALL)] + [case('r2l', 'plain', 63, T, 'near') for T in T_SMALL]
    lr = [case('l2r', 'plain', 64, 17, 'near'), case('l2r', 'plain', 62, 6, 'holes'), case('l2r', 'plain', 3, 9, 'far')]
    g['lr_alone'] = lr
    g['mixed'] = [lr[0], case('ring', 'plain', 64, 16, 'near'), lr[1], case('perm', 'plain', 63, 5, 'far'), lr[2]]
    g['wide128'] = [case(kind, 'plain', n, T, EMIS[(i + j + k) % 3]) for i, n in enumerate((65, 128)) for j, kind in enumerate(('ring', 'skip'))
                    for k, T in enumerate(T_WIDE)]
    g['wide192'] = [case(kind, 'plain', 129, T, EMIS[(j + k) % 3]) for j, kind in enumerate(('ring', 'skip')) for k, T in enumerate(T_WIDE)]
    g['wide192'] += [case(kind, v, 129, 20, EMIS[(j + k) % 3]) for j, kind in enumerate(('ring', 'skip')) for k, v in enumerate(VARIANTS[1:])]
    g['wide192'] += [case(kind, 'plain', 129, 20, 'near') for kind in ('r2l', 'weave', 'perm')] + [impossible(case('ring', 'plain', 129, 20, 'near'), 11)]
    # (salt: the first draw of the 257-state ring at T = 20 has a pass whose gain lies 27 ulps of ln P(O) from the 1e-13 threshold, see decisive())
    g['wide320'] = [case(kind, 'plain', 257, T, EMIS[(j + k + 1) % 3], salt=int((kind, T) == ('ring', 20))) for j, kind in enumerate(('ring', 'skip'))
                    for k, T in enumerate(T_WIDE)]
    g['wide_gap'] = [case('ring', 'plain', 5, 20, 'near'), case('ring', 'plain', 129, 20, 'far')]      # NP = 192: the 5-state HMM leaves two waves empty
    g['wide_lr'] = [case('l2r', 'plain', 257, 20, 'near')]                                             # beyond the scaled route's 256 states
    return g


SMALL_GROUPS = ('small', 'sweep', 'mixed', 'lr_alone')
WIDE_GROUPS = ('wide128', 'wide192', 'wide320', 'wide_gap', 'wide_lr')


def dispatch(cases, linear=False):
    """the kernel pcl_launch_forward_backward runs for a batch of these HMMs (PCL_FB_LINEAR=1: linear), from the matrices alone."""
    outdeg = max(int((c['a'] != 0).sum(axis=1).max()) for c in cases)
    indeg = max(int((c['a'] != 0).sum(axis=0).max()) for c in cases)
    lr = all(is_left_right(c['a']) for c in cases)
    NP = (max(c['a'].shape[0] for c in cases) + 63) // 64 * 64
    if indeg > 2 or outdeg > 2:
        return 'hmm_fb_kernel<0>'
    if NP == 64:
        return 'hmm_fbl_kernel' if lr and linear else 'hmm_fb2_kernel'
    return 'hmm_fblm_kernel' if lr and linear and NP <= 256 else 'hmm_fb_kernel<2>'


@functools.lru_cache(maxsize=None)
def oracle(group, index, fix_pi, threshold):
    """oracle/poccala_oracle.py baum_welch of one case, computed once per session and never written to."""
    c = groups_all()[group][index]
    with np.errstate(all='ignore'):
        return po.baum_welch(c['a'], c['pi'], [c['B']], fix_code=1 if fix_pi else 0, threshold=threshold)


def decisive(bw, threshold):
    """every pass decision of the oracle's loop is one that rounding cannot turn: the gain is exactly 0 (pi has settled to the bit: the pass
    repeats the one before) or further than 64 ulps of ln P(O) from the threshold.  Then the device, which rounds elsewhere, counts the same
    passes."""
    q = np.concatenate([bw['q_trace'], [bw['q_final']]])
    with np.errstate(invalid='ignore'):
        g = np.diff(q)
    return bool(((g == 0.0) | (np.abs(g - threshold) > 64 * np.spacing(abs(q[-1])))).all())


def tolerance(c):
    """tests/test_gpu_fuzz_hmm.py: the log-domain oracle rounds once per frame at the size of ln alpha ~ |b| T."""
    B, T = c['B'], c['B'].shape[1]
    big = float(np.abs(B[np.isfinite(B)]).max()) * T if np.isfinite(B).any() else 1.0
    return max(1e-9, 32 * 2.2e-16 * big * np.sqrt(T))


# ================================================================== C: the posterior kernel's arithmetic
@functools.lru_cache(maxsize=None)
def post_cases():
    """the N <= 64 structures of section B with |b| <= 8, and a ring in which one state's posterior is driven below e^-745 for three
    frames (past exp_neg's cut-off)."""
    out = small_cases(lambda k: 'unit')
    c = case('ring', 'plain', 64, 17, 'unit', salt=1)
    c['B'][32, 5:8] = -800.0
    c['name'] += ' driven'
    return out + [c]


def groups_all():
    return dict(groups(), post=post_cases())


def exp_neg_twin(x):
    """exp_neg of csrc/hmm_dp.hip for x <= 0 in float64 NumPy (k ln2_hi is exact for |k| < 2^11, so the first reduction step rounds once, as
    the kernel's fma does)."""
    x = np.asarray(x, np.float64)
    ok = x > -745.0
    xs = np.where(ok, x, 0.0)
    k = np.rint(xs * 1.4426950408889634074)
    r = xs - k * 6.93147180369123816490e-01
    r = r - k * 1.90821492927058770002e-10
    p = np.full_like(xs, 1.0 / 479001600.0)
    for c in (39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0, 1.0, 1.0):
        p = p * r + 1.0 / c
    return np.where(ok, np.ldexp(p, k.astype(np.int64)), 0.0)


def online_lse_twin(x, m, s):
    with np.errstate(invalid='ignore'):
        up = x > m
        add = ~up & (x > -np.inf)
        s_up = s * exp_neg_twin(np.where(up, m - x, 0.0)) + 1.0
        s_add = s + exp_neg_twin(np.where(add, x - m, 0.0))
    return np.where(up, x, m), np.where(up, s_up, np.where(add, s_add, s))


def post_terms(c, alpha, beta, dtype):
    """(terms of ln gamma_i (N, T - 1), terms of ln xi_ij (nnz, T - 1), (i, j) of the stored transitions) in `dtype`, associated as
    hmm_post_body does: alpha_t(i) + (ln a_ij + (b_j(o_t+1) + beta_t+1(j)))."""
    with np.errstate(divide='ignore'):
        la = np.log(c['a'])
    ii, jj = np.nonzero(c['a'])
    A, Bv, B = alpha.astype(dtype), beta.astype(dtype), c['B'].astype(dtype)
    with np.errstate(invalid='ignore'):
        g = A[:, :-1] + Bv[:, :-1]
        x = A[ii, :-1] + (la[ii, jj].astype(dtype)[:, None] + (B[jj, 1:] + Bv[jj, 1:]))
    return g, x, (ii, jj)


def lse_ld(v):
    """long-double log-sum-exp along the last axis; -inf where every term is."""
    v = np.asarray(v, LD)
    m = v.max(axis=-1)
    safe = np.where(np.isfinite(m), m, LD(0))
    with np.errstate(divide='ignore'):
        return np.where(np.isfinite(m), safe + np.log(np.exp(v - safe[..., None]).sum(axis=-1)), m)


def post_reference(c, alpha, beta):
    """long double: the summed ln gamma (N,) and ln xi (N, N) of LHMM.py:394-405, 431-445 from float64 alpha / beta."""
    g, x, (ii, jj) = post_terms(c, alpha, beta, LD)
    n = c['a'].shape[0]
    ksai = np.full((n, n), -np.inf, dtype=LD)
    ksai[ii, jj] = lse_ld(x)
    return lse_ld(g), ksai


def post_twin(c, alpha, beta):
    """float64: the same two sums as hmm_post_body takes them -- wave w of POST_W folds its frames t = w, w + 8, ... < T - 1 into an online
    (max, sum) pair with exp_neg, and the pairs are merged in wave order."""
    g, x, (ii, jj) = post_terms(c, alpha, beta, np.float64)

    def merged(v):
        ms = []
        for w in range(POST_W):
            m, s = np.full(v.shape[0], -np.inf), np.zeros(v.shape[0])
            for t in range(w, v.shape[1], POST_W):
                m, s = online_lse_twin(v[:, t], m, s)
            ms.append((m, s))
        M = np.max([m for m, _ in ms], axis=0)
        tsum = np.zeros(v.shape[0])
        for m, s in ms:
            with np.errstate(invalid='ignore'):
                tsum = tsum + np.where(m > -np.inf, s * np.exp(np.where(m > -np.inf, m - M, 0.0)), 0.0)
        with np.errstate(divide='ignore'):
            return np.where(M > -np.inf, M + np.log(tsum), -np.inf)
    n = c['a'].shape[0]
    ksai = np.full((n, n), -np.inf)
    ksai[ii, jj] = merged(x)
    return merged(g), ksai


@functools.lru_cache(maxsize=None)
def post_twin_error():
    """the twin's worst absolute error in ln gamma / ln xi against the long-double reference over post_cases() (T > 1); the device is held
    to four times this."""
    worst = 0.0
    for k, c in enumerate(post_cases()):
        if c['B'].shape[1] < 2:
            continue
        bw = oracle('post', k, True, 0.64)
        want, got = post_reference(c, bw['alpha'][0], bw['beta'][0]), post_twin(c, bw['alpha'][0], bw['beta'][0])
        for a, b in zip(got, want):
            fin = np.isfinite(b)
            assert np.array_equal(np.isfinite(a), fin), c['name']
            if fin.any():
                worst = max(worst, float(np.abs(a[fin].astype(LD) - b[fin]).max()))
    return worst
