"""NumPy float64 twin of csrc/frame_mllt.hip: the MLLT rule of include/poccala_hip.h (pcl_batch_accumulate_mllt, pcl_mllt_estimate).
G_i is held twice: by its centred DEFINITION straight from the posteriors, and in the EXPANDED form the device uses -- the frame side F_i
from p_i(t), the mixture side C_i from acc, s and the means -- together with the sum of the ABSOLUTE terms of every element, the scale of
the bounds.  The sweeps run on _fmllr_twin's Cholesky, triangular solves and Gauss-Jordan inversion, in any NumPy float type.
tests/test_mllt_twin.py holds the twin's own invariants; tests/test_gpu_mllt.py compares the device with it."""
import numpy as np

import _fmllr_twin as ft

OK, LOW_OCCUPANCY, NOT_POSITIVE_DEFINITE, SINGULAR = 0, 1, 2, 3
BIAS = 100.0                                     # mean_acc of the statistics block holds sum gamma (o + bias)


# ------------------------------------------------------------------ statistics
def posteriors(model, frames, T, begin, row_states, lgamma, lnb, utt_keep=None, state_keep=None):
    """yields (x (T_u, D), j, gamma (T_u, M)) for every kept utterance and every GMM row of a kept state, rows in ascending order"""
    for u in range(len(T)):
        if T[u] == 0 or (utt_keep is not None and not utt_keep[u]):
            continue
        x = np.asarray(frames[begin[u]:begin[u] + T[u]], dtype=np.float64)
        for r, j in enumerate(row_states[u]):
            if j < 0 or (state_keep is not None and not state_keep[j]):
                continue
            yield x, j, ft.mixture_posteriors(model, x, lgamma[u][r], lnb[u][r], j)


def centred(model, post):
    """the definition: G_i = sum_t sum_jm gamma_t(j,m) / var_jm,i (x_t - mu_jm)(x_t - mu_jm)^T, beta = sum gamma -> (G (D, D, D), beta)"""
    mean, var, w = model
    D = mean.shape[2]
    G, beta = np.zeros((D, D, D)), 0.0
    for x, j, g in post:
        for m in np.flatnonzero(g.any(axis=0)):
            d = x - mean[j, m][None]
            S = np.einsum('t,ta,tb->ab', g[:, m], d, d)
            G += S[None] / var[j, m][:, None, None]
            beta += g[:, m].sum()
    return G, beta


def block_stats(model, post):
    """what pcl_batch_accumulate leaves for these posteriors: acc (J, M), mean_acc (J, M, D) = sum gamma (x + bias)"""
    mean, var, w = model
    acc, macc = np.zeros(mean.shape[:2]), np.zeros(mean.shape)
    for x, j, g in post:
        acc[j] += g.sum(axis=0)
        macc[j] += g.T @ (x + BIAS)
    return acc, macc


def frame_side(model, post):
    """F_i = sum_t p_i(t) x_t x_t^T, p_i(t) = sum_jm gamma_t(j,m) / var_jm,i -> dict(F, Fabs (D, D, D), beta)"""
    mean, var, w = model
    D = mean.shape[2]
    F, Fabs, beta = np.zeros((D, D, D)), np.zeros((D, D, D)), 0.0
    for x, j, g in post:
        p = g @ (1.0 / var[j])
        xa = np.abs(x)
        F += np.einsum('ti,ta,tb->iab', p, x, x)
        Fabs += np.einsum('ti,ta,tb->iab', p, xa, xa)
        beta += g.sum()
    return dict(F=F, Fabs=Fabs, beta=beta)


def mixture_side(model, acc, macc, state_keep=None):
    """C_i = sum_jm (s mu^T + mu s^T - n mu mu^T) / var_i over the kept states' mixtures with a finite acc > 0, n = acc, s = mean_acc -
    bias acc -> dict(C, Cabs (D, D, D): Cabs = sum (|s_a mu_b| + |mu_a s_b| + n |mu_a mu_b|) / var_i, occ = sum n)"""
    mean, var, w = model
    J, M, D = mean.shape
    C, Cabs, occ = np.zeros((D, D, D)), np.zeros((D, D, D)), 0.0
    for j in range(J):
        if state_keep is not None and not state_keep[j]:
            continue
        for m in range(M):
            n = acc[j, m]
            if not (np.isfinite(n) and n > 0):
                continue
            mu, s = mean[j, m], macc[j, m] - BIAS * n
            T = np.outer(s, mu) + np.outer(mu, s) - n * np.outer(mu, mu)
            Ta = np.outer(np.abs(s), np.abs(mu)) + np.outer(np.abs(mu), np.abs(s)) + n * np.outer(np.abs(mu), np.abs(mu))
            C += T[None] / var[j, m][:, None, None]
            Cabs += Ta[None] / var[j, m][:, None, None]
            occ += n
    return dict(C=C, Cabs=Cabs, occ=occ)


def expanded(model, post, acc, macc, state_keep=None):
    """G = F - C and Gabs = Fabs + Cabs, the per-element sum of absolute terms"""
    f, c = frame_side(model, post), mixture_side(model, acc, macc, state_keep)
    return dict(f, **c, G=f['F'] - c['C'], Gabs=f['Fabs'] + c['Cabs'])


# ------------------------------------------------------------------ estimate
def aux(A, G, beta, logdet=None):
    """Q(A) = beta ln|det A| - 1/2 sum_i a_i G_i a_i^T"""
    if logdet is None:
        logdet = np.linalg.slogdet(np.asarray(A, dtype=np.float64))[1]
    with np.errstate(invalid='ignore'):                            # (beta = inf at A = I: nan, as the device gives)
        return beta * logdet - sum(A[i] @ (G[i] @ A[i]) for i in range(A.shape[0])) / 2


def estimate(G, beta, n_iter=20, min_occ=1000.0, dtype=np.float64):
    """-> dict(A (D, D), logdet, q_trace (n_iter + 1,), status) in `dtype`: the header's sweeps from A = I"""
    D = G.shape[0]
    G, beta = np.asarray(G, dtype=dtype), dtype(beta)
    refused = lambda st: dict(A=np.eye(D, dtype=dtype), logdet=dtype(0), q_trace=np.full(n_iter + 1, np.nan, dtype=dtype), status=st)
    if beta < min_occ:
        return refused(LOW_OCCUPANCY)
    L = [ft.cholesky(G[i]) for i in range(D)]
    if any(f is None for f in L):
        return refused(NOT_POSITIVE_DEFINITE)
    A, Ai, ld = np.eye(D, dtype=dtype), np.eye(D, dtype=dtype), dtype(0)
    trace = [aux(A, G, beta, ld)]
    for _ in range(n_iter):
        for i in range(D):
            c = Ai[:, i].copy()
            v = ft.chol_solve(L[i], c)
            a = dtype(0)
            for q in range(D):
                a = a + c[q] * v[q]
            disc = 4 * a * beta
            if not (np.isfinite(a) and a > 0) or not (np.isfinite(disc) and disc >= 0):
                return refused(SINGULAR)
            alpha = np.sqrt(disc) / (2 * a)
            if not np.isfinite(alpha):
                return refused(SINGULAR)
            an = alpha * v
            denom = dtype(0)
            for q in range(D):
                denom = denom + an[q] * c[q]
            if not (np.isfinite(denom) and abs(denom) > 0):
                return refused(SINGULAR)
            z = ((an - A[i]) @ Ai) / denom
            Ai -= c[:, None] * z[None]
            A[i] = an
        Ai, ld = ft.invert(A)
        if Ai is None:
            return refused(SINGULAR)
        trace.append(aux(A, G, beta, ld))
    return dict(A=A, logdet=ld, q_trace=np.array(trace, dtype=dtype), status=OK)


# ------------------------------------------------------------------ planted data: diagonal classes behind a fixed mixing matrix
def planted(D, n_classes=4, n_per=400, seed=5):
    """z has per-class DIAGONAL covariances of clearly different shape (every class its own variances between 0.05 and 5) and class means
    apart; x = R z with a fixed-seed, well-conditioned, NON-orthogonal R.  -> dict(x (N, D), cls (N,), R, and one Gaussian per class with
    the ML mean and diagonal variance of x: mean, var (C, 1, D), w (C, 1))"""
    rng = np.random.default_rng(seed + 100 * D)
    Q1, _ = np.linalg.qr(rng.standard_normal((D, D)))
    Q2, _ = np.linalg.qr(rng.standard_normal((D, D)))
    R = Q1 @ np.diag(np.linspace(0.6, 1.8, D)) @ Q2                 # singular values 0.6 .. 1.8: cond 3, not orthogonal
    sd = np.exp(rng.uniform(np.log(0.05), np.log(5.0), (n_classes, D)) / 2)
    mz = 2.0 * rng.standard_normal((n_classes, D))
    cls = np.repeat(np.arange(n_classes), n_per)
    z = mz[cls] + sd[cls] * rng.standard_normal((len(cls), D))
    x = z @ R.T
    mean = np.stack([x[cls == c].mean(axis=0) for c in range(n_classes)])[:, None, :]
    var = np.stack([x[cls == c].var(axis=0) for c in range(n_classes)])[:, None, :]
    return dict(x=x, cls=cls, R=R, mean=mean, var=var, w=np.ones((n_classes, 1)))


def hard_stats(p):
    """G (centred, hard posteriors), beta and the classes' full covariances Sigma_c (C, D, D) and counts of the planted data"""
    x, cls, mean, var = p['x'], p['cls'], p['mean'], p['var']
    C, D = mean.shape[0], x.shape[1]
    G, Sig, n = np.zeros((D, D, D)), np.zeros((C, D, D)), np.zeros(C)
    for c in range(C):
        d = x[cls == c] - mean[c, 0][None]
        S = d.T @ d
        n[c] = len(d)
        Sig[c] = S / n[c]
        G += S[None] / var[c, 0][:, None, None]
    return G, float(n.sum()), Sig, n


def offdiag_ratio(A, Sig, n):
    """the occupancy-weighted ratio of off-diagonal to diagonal energy of A Sigma_c A^T"""
    off = dia = 0.0
    for c in range(len(n)):
        S = A @ Sig[c] @ A.T
        d = np.diag(S)
        dia += n[c] * (d ** 2).sum()
        off += n[c] * ((S ** 2).sum() - (d ** 2).sum())
    return off / dia


def diag_loglik(y, cls, n_classes):
    """ln p(y) under one diagonal Gaussian per class with the ML mean and variance of y"""
    total = 0.0
    for c in range(n_classes):
        yc = y[cls == c]
        v = yc.var(axis=0)
        total += -0.5 * len(yc) * (np.log(2 * np.pi * v).sum() + y.shape[1])
    return total


# ------------------------------------------------------------------ the inputs the GPU tests run on (tests/test_gpu_mllt.py)
J, M = 4, 3
T_UTT = np.array([1, 40, 65], dtype=np.int32)
UTT_KEEP = np.array([0, 1, 1], dtype=np.int32)                      # the 1-frame utterance is skipped (test_gpu_mllt keeps it in its two-batch case)
STATE_KEEP = np.array([1, 1, 0, 1], dtype=np.int32)                 # state 2 is dropped
GAPS = np.array([2, 0, 3], dtype=np.int64)


def make_case(D, seed=0):
    """J = 4 one-state units, M = 3: mixture (1, 2) has weight 0, mixture (3, 1) lies far from every frame (its posterior underflows to an
    exact 0: it gathers nothing).  A state's mixtures overlap (their means lie within a fraction of a standard deviation), so a frame's
    posterior is spread over them and G_i has full rank from the kept frames at D = 47.  Three utterances of 1 / 40 / 65 frames with
    unowned rows around them, one label sequence each, frames drawn along the labels from the live mixtures and pushed through a mild
    mixing matrix, so that the classes are correlated.  -> (model, labels, frames (F, D) float64, T, begin, align: the state of every frame)"""
    rng = np.random.default_rng(2300 + 17 * D + seed)
    mean = 1.5 * rng.standard_normal((J, 1, D)) + 0.12 * rng.standard_normal((J, M, D))
    var = rng.uniform(0.5, 2.0, (J, M, D))
    w = rng.uniform(0.5, 1.5, (J, M))
    w[1, 2] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    mean[3, 1] += 400.0
    begin = (np.cumsum(GAPS) + np.concatenate([[0], np.cumsum(T_UTT[:-1].astype(np.int64))])).astype(np.int64)
    F = int(begin[-1] + T_UTT[-1] + 2)
    frames = rng.standard_normal((F, D))
    R = np.eye(D) + 0.15 * rng.standard_normal((D, D))
    labels, align = [], []
    for u, T in enumerate(T_UTT):
        lab = rng.permutation(J)[:max(1, min(J, T // 8))].astype(np.int32)
        labels.append(lab)
        st = lab[np.minimum(np.arange(T) * len(lab) // T, len(lab) - 1)]
        align.append(st)
        y = np.empty((T, D))
        for t in range(T):
            live = [m for m in range(M) if w[st[t], m] > 0 and not (st[t] == 3 and m == 1)]
            m = live[rng.integers(0, len(live))]
            y[t] = mean[st[t], m] + np.sqrt(var[st[t], m]) * rng.standard_normal(D)
        frames[begin[u]:begin[u] + T] = y @ R.T
    # the model lives in the mixed space too (or every posterior would collapse onto one mixture): push the means through R
    mean = mean @ R.T
    return (mean, var, w), labels, frames, T_UTT.copy(), begin, align
