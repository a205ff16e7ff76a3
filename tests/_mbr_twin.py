"""The rule of pcl_batch_mbr (include/poccala_hip.h, row f19; csrc/hmm_mbr.hip) in NumPy, operation for operation and sum for sum in the
kernel's order: the forward-backward under an acoustic scale kappa with the expected frame accuracy beside alpha and beta.  `dtype`
= np.longdouble runs the same code in extended precision (the yardstick of the allowance).  `depart` switches in one wrong variant at a
time, for the tests that show an omission would be caught."""
import numpy as np

from oracle import poccala_oracle as po

DEPARTURES = ('A_at_t', 'no_kappa_in_g', 'unnormalised_c_avg')


def rows_sum(v):
    """The kernel's sum across rows: row i in lane i % 64 of wave i // 64, lanes past N hold 0; a butterfly over the wave with partner lane
    ^ 32, 16, 8, 4, 2, 1 (the same tree as halving the wave five times), then the waves' sums in ascending order."""
    n = len(v)
    nw = (n + 63) // 64
    p = np.zeros(nw * 64, dtype=v.dtype)
    p[:n] = v
    p = p.reshape(nw, 64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p[:, :o] + p[:, o:2 * o]
    s = p[0, 0]
    for k in range(1, nw):
        s = s + p[k, 0]
    return s


def rows_lse(v):
    """log-sum-exp across rows, quirk Q4 (a maximum of +-inf is returned as itself), the sum in rows_sum's order"""
    m = v.max()
    if np.isinf(m):
        return m
    return m + np.log(rows_sum(np.exp(v - m)))


def step(x, y, W):
    """One step of either recursion for every target row at once.  x, y (N,): what the source rows published (value, accuracy);
    W[k, j] = ln weight of source k into target j (-inf: no entry; an entry of ln 0 adds exp(-inf) = 0 to both sums, so the dense walk has
    the bits of the kernel's sparse one).  Two passes: the maximum, then s = sum e_k and sp = sum e_k y_k in ascending k.
    -> (m + ln s, sp / s); (m, 0) where m is +-inf."""
    n = len(x)
    with np.errstate(all='ignore'):
        v = x[:, None] + W
        m = v.max(axis=0)
        ok = ~np.isinf(m)
        ms = np.where(ok, m, 0)
        s, sp = np.zeros(n, dtype=x.dtype), np.zeros(n, dtype=x.dtype)
        for k in range(n):
            e = np.exp(v[k] - ms)
            s = s + e
            sp = sp + e * y[k]
        value = np.where(ok, m + np.log(np.where(ok, s, 1)), m)
        acc = np.where(ok, sp / np.where(ok, s, 1), 0)
    return value, acc


def accuracy(row_state, ref, group):
    """A (N, T): 1 where row j's state and frame t's reference state fall into the same group"""
    rs, r = np.asarray(row_state).astype(np.int64), np.asarray(ref).astype(np.int64)
    return ((rs[:, None] >= 0) & (r[None, :] >= 0) & (rs[:, None] // group == r[None, :] // group)).astype(np.float64)


def mbr(la, lpi, B, row_state, ref, kappa=1.0, group=1, dtype=np.float64, depart=None):
    """la (N, N) = ln a (-inf where there is no transition), lpi (N,) = ln pi, B (N, T) emissions -> dict(logp, c_avg, lgamma, g, alpha,
    beta, alphap, betap): backward first, c_avg at frame 0, then forward -- the kernel's order."""
    assert depart is None or depart in DEPARTURES
    la, lpi, B = np.asarray(la, dtype=dtype), np.asarray(lpi, dtype=dtype), np.asarray(B, dtype=dtype)
    N, T = B.shape
    A = accuracy(row_state, ref, group).astype(dtype)
    kappa = dtype(kappa)
    zero = dtype(0)
    with np.errstate(all='ignore'):
        bs = kappa * B
        beta, betap = np.zeros((N, T), dtype=dtype), np.zeros((N, T), dtype=dtype)
        for t in range(T - 2, -1, -1):
            wy = betap[:, t + 1] + (A[:, t] if depart == 'A_at_t' else A[:, t + 1])
            beta[:, t], betap[:, t] = step(bs[:, t + 1] + beta[:, t + 1], wy, la.T)
        alpha, alphap = np.zeros((N, T), dtype=dtype), np.zeros((N, T), dtype=dtype)
        lgamma, g = np.zeros((N, T), dtype=dtype), np.zeros((N, T), dtype=dtype)
        c_avg = zero
        for t in range(T):
            if t == 0:
                alpha[:, 0] = lpi + bs[:, 0]
                alphap[:, 0] = A[:, 0]
            else:
                r, y = step(alpha[:, t - 1], alphap[:, t - 1], la)
                alpha[:, t] = r + bs[:, t]
                alphap[:, t] = np.where(alpha[:, t] == -np.inf, zero, y + A[:, t])
            l = alpha[:, t] + beta[:, t]
            lgamma[:, t] = l - rows_lse(l)
            gam = np.exp(lgamma[:, t])
            both = alphap[:, t] + betap[:, t]
            if t == 0:
                wgt = np.exp(l) if depart == 'unnormalised_c_avg' else gam
                c_avg = rows_sum(np.where(wgt > 0, wgt * both, zero))
            scale = gam if depart == 'no_kappa_in_g' else kappa * gam
            g[:, t] = np.where(gam > 0, scale * (both - c_avg), zero)
        logp = rows_lse(alpha[:, T - 1])
    return dict(logp=logp, c_avg=c_avg, lgamma=lgamma, g=g, alpha=alpha, beta=beta, alphap=alphap, betap=betap)


def ln_part(g, which):
    """what pcl_batch_mbr_posteriors(which) makes of g: ln max(g, 0) / ln max(-g, 0)"""
    with np.errstate(divide='ignore'):
        return np.log(np.maximum(g if which > 0 else -g, 0))


# ------------------------------------------------------------------ all paths, one by one
def brute_force(a, pi, B, row_state, ref, kappa=1.0, group=1):
    """Every one of the N^T paths (every row may end): P(path) = pi b^kappa prod a b^kappa, acc(path) = sum_t A_t(q_t).
    -> dict(logp, c_avg = E[acc], gamma (N, T), g (N, T) = kappa sum over the paths through (t, j) of P(path) (acc - c_avg) / P)"""
    import itertools
    N, T = B.shape
    A = accuracy(row_state, ref, group)
    with np.errstate(all='ignore'):
        eb = np.exp(kappa * B)
    P, pa, through, through_acc = 0.0, 0.0, np.zeros((N, T)), np.zeros((N, T))
    for q in itertools.product(range(N), repeat=T):
        p = pi[q[0]] * eb[q[0], 0]
        for t in range(1, T):
            p *= a[q[t - 1], q[t]] * eb[q[t], t]
        if p == 0.0:
            continue
        acc = sum(A[q[t], t] for t in range(T))
        P += p
        pa += p * acc
        for t in range(T):
            through[q[t], t] += p
            through_acc[q[t], t] += p * acc
    c = pa / P
    return dict(logp=np.log(P), c_avg=c, gamma=through / P, g=kappa * (through_acc - c * through) / P)


# ------------------------------------------------------------------ allowances of the device against this twin
def allowances(t64, tld, kappa):
    """What the device may differ from the float64 twin by, per quantity: 4 x |float64 twin - long-double twin| plus an absolute term.

    The absolute term.  The kernel runs the twin's operations in the twin's order; what differs is the library: the device's exp and log
    against NumPy's, each within 1 ulp of its result.  In one step of a recursion, value = m + ln(sum exp(v - m)) + bs: the exps move the
    sum by 1 ulp relatively, which is 2^-52 absolutely in its logarithm, the log adds its own ulp, and the result is then rounded at the
    magnitude of alpha -- so a step moves alpha (or beta) by at most 2 ulp(amax), amax the largest finite |alpha|, |beta| of the utterance
    (the terms below that, a few 2^-52, are inside the 2).  ln gamma_t(j) = alpha + beta - normaliser chains t forward steps, T - 1 - t
    backward steps and the normaliser's log-sum-exp: T + 1 steps at the most, so
        d = 2 (T + 1) ulp(amax)                      for ln gamma and ln P.
    Every weight of a mean (e_k / s), every gamma and every path weight inside alpha' / beta' is the exp of such differences, so it is
    off by at most d relatively.  alpha' and beta' are means of accuracies in [0, T]: off by at most T d each, c_avg (a gamma-weighted
    sum of alpha' + beta' <= T) by at most 3 T d with them.  g = kappa gamma ((alpha' + beta') - c_avg): gamma <= 1 off by d relatively,
    the bracket (at most T) off by 2 T d + 3 T d; together at most kappa (T d + 5 T d):
        3 T d  for c_avg,        6 kappa T d  for g."""
    T = t64['lgamma'].shape[1]
    both = np.concatenate([t64['alpha'].ravel(), t64['beta'].ravel()])
    fin = np.abs(both[np.isfinite(both)])
    d = 2.0 * (T + 1) * np.spacing(max(fin.max() if fin.size else 1.0, 1.0))       # (amax at least 1: the 2^-52 terms of the derivation)
    term = dict(logp=d, lgamma=d, c_avg=3.0 * T * d, g=6.0 * kappa * T * d)
    out = {}
    for key, add in term.items():
        a = np.asarray(t64[key], dtype=np.float64)
        with np.errstate(invalid='ignore'):
            dist = np.abs(a - np.asarray(tld[key])).astype(np.float64)
        out[key] = 4.0 * np.where(np.isfinite(dist), dist, 0.0) + add
    return out


# ------------------------------------------------------------------ the structures the tests run on
def chain_structure(N, rng):
    """a left-to-right chain of N rows as AcousticModel.embedded builds them (entry row -> row 1, every emitting row to itself and to the
    next, the exit row without a successor; at most two predecessors and successors), uniform pi = 1 / N: (a, pi)"""
    a = np.zeros((N, N))
    a[0, 1] = 1.0
    for k in range(1, N - 1):
        stay = rng.uniform(0.3, 0.8)
        a[k, k], a[k, k + 1] = stay, 1.0 - stay
    return a, np.ones(N) / N


def dense_structure(N, rng):
    """a random dense matrix with holes (about a third of the entries), a row no path reaches (row 1: its column and its pi are 0), and an
    exit row (the last) without successors: (a, pi)"""
    a = rng.uniform(0.05, 1.0, (N, N)) * (rng.uniform(size=(N, N)) > 0.35)
    a[:, 1] = 0.0
    a[N - 1, :] = 0.0
    a[np.arange(N - 1), (np.arange(N - 1) + 2) % N] += 0.1          # every row but the exit keeps a successor other than row 1
    a[0, 0] += 0.1                                                  # (N = 3: row 0 is the only row a path can be in)
    a[:, 1] = 0.0
    rs = a.sum(axis=1, keepdims=True)
    a = a / np.where(rs > 0, rs, 1.0)
    pi = rng.uniform(0.1, 1.0, N)
    pi[1] = 0.0
    return a, pi / pi.sum()


# ------------------------------------------------------------------ end to end: sMBR iterations through the oracle and the twins
E2E = dict(kappa=0.1, E=2.0, tau=0.0, iters=3, group=1)


def _b_matrix(model, x, rows):
    mean, var, w = model
    return np.vstack([np.zeros(len(x))] + [po.gmm_point(x, mean[j], var[j], w[j]) for j in rows] + [np.full(len(x), -np.inf)])


def _accumulate(model, x, rows, lg, out):
    """oracle accumulate of one utterance whose emitting rows 1 .. N-2 are the states `rows`, from ln gamma (N, T)"""
    import _ebw_twin as ebw
    mean, var, w = model
    for r, j in enumerate(rows):
        gam = np.exp(lg[1 + r])
        comp = po.gmm_component_loglik(x, mean[j], var[j], w[j])
        gm = gam[:, None] * np.exp(comp - po.lse(comp, axis=1)[:, None])
        out['acc'][j] += gm.sum(axis=0)
        out['alpha_acc'][j] += gam.sum()
        out['mean_acc'][j] += gm.T @ (x + ebw.BIAS)
        out['cov_acc'][j] += np.einsum('tm,tmd->md', gm, (x[:, None, :] - mean[j][None]) ** 2)


_E2E_CACHE = {}


def e2e_reference():
    """The sMBR loop on the CPU over _ebw_twin's corpus: per iteration the numerator alignment (oracle scoring and Viterbi over the label
    graph), the MBR twin over the unit loop, oracle accumulates of the positive and the negative part, _ebw_twin.update with tau = 0.
    -> dict(c_avg = per iteration the per-utterance c_avg (iters + 1, U), the last after the last update; logp likewise; refs = the
    alignments of every iteration; bsum = per iteration sum over utterances and frames of max_j |B|; model = the final model)"""
    if _E2E_CACHE:
        return _E2E_CACHE
    import _ebw_twin as ebw
    from poccala_amd.engine import embedded_structure, loop_structure
    model, trans, frames, labels, lens, begin = ebw.e2e_setup()
    c, cm = ebw.E2E, E2E
    J, e = model[0].shape[0], 3
    a_den, pi_den = loop_structure(trans)
    with np.errstate(divide='ignore'):
        la_den, lpi_den = np.log(a_den), np.log(pi_den)
    rs_den = np.concatenate([[-1], np.arange(J), [-2]])
    cav, lps, refs, bsum = [], [], [], []
    for it in range(cm['iters'] + 1):
        zero = lambda: dict(acc=np.zeros((J, c['M'])), alpha_acc=np.zeros(J), mean_acc=np.zeros((J, c['M'], c['D'])), cov_acc=np.zeros((J, c['M'], c['D'])))
        pos, neg = zero(), zero()
        cav.append([]), lps.append([]), refs.append([]), bsum.append(0.0)
        for u, lab in enumerate(labels):
            x = frames[begin[u]:begin[u] + lens[u]]
            a, pi = embedded_structure(len(lab), [trans[i] for i in lab])
            rows = (np.asarray(lab)[:, None] * e + np.arange(e)[None, :]).reshape(-1)
            _, path = po.viterbi(a, pi, _b_matrix(model, x, rows))
            rs_num = np.concatenate([[-1], rows, [-1]])
            ref = rs_num[np.asarray(path, dtype=np.int64)].astype(np.int32)
            Bd = _b_matrix(model, x, np.arange(J))
            t = mbr(la_den, lpi_den, Bd, rs_den, ref, kappa=cm['kappa'], group=cm['group'])
            cav[-1].append(t['c_avg']), lps[-1].append(t['logp']), refs[-1].append(ref)
            bsum[-1] += np.abs(Bd[1:-1]).max(axis=0).sum()
            if it < cm['iters']:
                _accumulate(model, x, np.arange(J), ln_part(t['g'], +1), pos)
                _accumulate(model, x, np.arange(J), ln_part(t['g'], -1), neg)
        if it < cm['iters']:
            up = ebw.update(*model, pos, neg, E=cm['E'], tau=cm['tau'])
            model = (up['mean'], up['var'], up['w'])
    _E2E_CACHE.update(c_avg=np.array(cav), logp=np.array(lps), refs=refs, bsum=np.array(bsum), model=model)
    return _E2E_CACHE
