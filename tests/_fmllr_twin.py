"""NumPy twin of csrc/frame_adapt.hip: the fMLLR rule of include/poccala_hip.h (pcl_batch_accumulate_fmllr, pcl_fmllr_estimate,
pcl_frames_transform) with the header's operation order, in float64 or -- the estimate -- in any NumPy float type (np.longdouble gives the
reference the device's W is held to).  Cholesky, the triangular solves and the in-place Gauss-Jordan inversion are written out, so that
they run in that type.  tests/test_fmllr_twin.py holds the twin's own invariants; tests/test_gpu_fmllr.py compares the device with it."""
import numpy as np

import _adapt_twin as at

OK, LOW_OCCUPANCY, NOT_POSITIVE_DEFINITE, SINGULAR = 0, 1, 2, 3
LN_2PI = 1.8378770664093454836


def identity(D, dtype=np.float64):
    return np.concatenate([np.zeros((D, 1), dtype=dtype), np.eye(D, dtype=dtype)], axis=1)


# ------------------------------------------------------------------ statistics
def mixture_posteriors(model, x, lgamma_row, lnb_row, j):
    """gamma_t(j, m) (T, M) = exp(ln gamma_t(row) + ln w_jm + ln N(x_t; mu_jm, var_jm) - ln b_j(x_t)) with the reference's density
    (util.py:29: -1/2 sum(var) in the constant); a mixture without a finite weight > 0 and a frame with ln gamma or ln b = -inf give 0"""
    mean, var, w = model
    live = np.isfinite(w[j]) & (w[j] > 0)
    with np.errstate(all='ignore'):
        lw = np.where(live, np.log(np.where(live, w[j], 1.0)), -np.inf)
        d2 = ((x[:, None, :] - mean[j][None]) ** 2 / (2 * var[j][None])).sum(axis=2)
        lp = lw[None] - 0.5 * mean.shape[2] * LN_2PI - 0.5 * var[j].sum(axis=1)[None] - d2
        ok = np.isfinite(lgamma_row) & np.isfinite(lnb_row)
        g = np.exp(lp + np.where(ok, lgamma_row - lnb_row, -np.inf)[:, None])
    return np.where(live[None] & ok[:, None], g, 0.0)


def frame_stats(model, frames, T, begin, row_states, lgamma, lnb, utt_speaker, S):
    """-> dict(G (S, D, n, n), k (S, D, n), beta (S,), and Gabs / kabs / betaabs: the sums of the ABSOLUTE terms).  row_states[u] (N_u,):
    state of every row (< 0: not a GMM row); lgamma[u], lnb[u] (N_u, T_u) as Batch.get returns them."""
    mean, var, w = model
    D, n = mean.shape[2], mean.shape[2] + 1
    G, Gabs = np.zeros((S, D, n, n)), np.zeros((S, D, n, n))
    k, kabs = np.zeros((S, D, n)), np.zeros((S, D, n))
    beta = np.zeros(S)
    for u, s in enumerate(utt_speaker):
        if s < 0 or T[u] == 0:
            continue
        x = np.asarray(frames[begin[u]:begin[u] + T[u]], dtype=np.float64)
        p, q, b = np.zeros((T[u], D)), np.zeros((T[u], D)), np.zeros(T[u])
        qa = np.zeros((T[u], D))
        for r, j in enumerate(row_states[u]):
            if j < 0:
                continue
            g = mixture_posteriors(model, x, lgamma[u][r], lnb[u][r], j)
            p += g @ (1.0 / var[j])
            q += g @ (mean[j] / var[j])
            qa += g @ np.abs(mean[j] / var[j])
            b += g.sum(axis=1)
        zeta = np.concatenate([np.ones((T[u], 1)), x], axis=1)
        za = np.abs(zeta)
        G[s] += np.einsum('ti,tp,tq->ipq', p, zeta, zeta)
        Gabs[s] += np.einsum('ti,tp,tq->ipq', p, za, za)
        k[s] += np.einsum('ti,tp->ip', q, zeta)
        kabs[s] += np.einsum('ti,tp->ip', qa, za)
        beta[s] += b.sum()
    return dict(G=G, k=k, beta=beta, Gabs=Gabs, kabs=kabs, betaabs=beta.copy())


# ------------------------------------------------------------------ linear algebra in any float type
def cholesky(G):
    """lower L with G = L L^T, or None when a pivot is not finite or not > 0"""
    n = G.shape[0]
    A = G.copy()
    for j in range(n):
        piv = A[j, j]
        if not (np.isfinite(piv) and piv > 0):
            return None
        d = np.sqrt(piv)
        A[j, j] = d
        A[j + 1:, j] = A[j + 1:, j] / d
        for r in range(j + 1, n):
            A[r, j + 1:r + 1] -= A[r, j] * A[j + 1:r + 1, j]
    return np.tril(A)


def chol_solve(L, b):
    n = len(b)
    v = b.copy()
    for j in range(n):
        v[j] = v[j] / L[j, j]
        v[j + 1:] -= L[j + 1:, j] * v[j]
    for j in range(n - 1, -1, -1):
        v[j] = v[j] / L[j, j]
        v[:j] -= L[j, :j] * v[j]
    return v


def invert(A):
    """in-place Gauss-Jordan with row pivoting, as the header states it -> (inverse, ln|det|), or (None, None) when a pivot is 0 or not finite"""
    D = A.shape[0]
    M = A.copy()
    perm, ld = [], M.dtype.type(0)
    for kk in range(D):
        col = np.abs(M[kk:, kk])
        r = kk + int(np.argmax(col))                       # (argmax: the FIRST largest)
        perm.append(r)
        if r != kk:
            M[[kk, r]] = M[[r, kk]]
        piv = M[kk, kk]
        if not (np.isfinite(piv) and abs(piv) > 0):
            return None, None
        ld = ld + np.log(abs(piv))
        colk = M[:, kk].copy()
        M[kk, kk] = 1
        rk = M[kk] / piv
        M[:, kk] = 0
        others = np.arange(D) != kk
        M[others] = M[others] - colk[others, None] * rk[None]
        M[kk] = rk
    for kk in range(D - 1, -1, -1):
        r = perm[kk]
        if r != kk:
            M[:, [kk, r]] = M[:, [r, kk]]
    return M, ld


def aux(W, G, k, beta, logdet=None):
    """Q = beta ln|det A| - 1/2 sum_i (w_i G_i w_i^T - 2 w_i k_i^T) of one speaker"""
    if logdet is None:
        logdet = np.linalg.slogdet(np.asarray(W[:, 1:], dtype=np.float64))[1]
    quad = sum(W[i] @ (G[i] @ W[i]) - 2 * (W[i] @ k[i]) for i in range(W.shape[0]))
    return beta * logdet - quad / 2


def row_update(i, W, Ai, L, g, beta, p_scale=1):
    """steps 1 - 5 of the header for row i, in place -> False when the step is singular"""
    D = W.shape[0]
    dt = W.dtype.type
    p = np.concatenate([[dt(0)], Ai[:, i]]) * dt(p_scale)
    v = chol_solve(L[i], p)
    a, c = dt(0), dt(0)
    for q in range(D + 1):
        a = a + p[q] * v[q]
        c = c + p[q] * g[i][q]
    disc = c * c + 4 * a * beta
    if not (np.isfinite(a) and a > 0) or not (np.isfinite(disc) and disc >= 0):
        return False
    sq = np.sqrt(disc)
    a1, a2 = (-c + sq) / (2 * a), (-c - sq) / (2 * a)
    with np.errstate(all='ignore'):
        f1 = beta * np.log(abs(a1 * a + c)) - a * a1 * a1 / 2
        f2 = beta * np.log(abs(a2 * a + c)) - a * a2 * a2 / 2
    alpha = a1 if (f1 >= f2 or np.isnan(f2)) else a2
    if not np.isfinite(alpha):
        return False
    wn = alpha * v + g[i]
    u = Ai[:, i].copy()
    denom = dt(0)
    for q in range(D):
        denom = denom + wn[1 + q] * u[q]
    if not (np.isfinite(denom) and abs(denom) > 0):
        return False
    z = ((wn[1:] - W[i, 1:]) @ Ai) / denom
    Ai -= u[:, None] * z[None]
    W[i] = wn
    return True


def estimate(G, k, beta, n_iter=20, min_occ=1000.0, dtype=np.float64, W0=None, p_scale=1, on_row=None):
    """-> dict(W (S, D, n), logdet (S,), q_trace (S, n_iter), status (S,) int32) in `dtype`.  W0 (S, D, n): start the sweeps there instead
    of at [0 | I]; p_scale: the cofactor row is scaled by it (the update must not care); on_row(s, W): called after every row update."""
    S, D, n, _ = G.shape
    G, k, beta = np.asarray(G, dtype=dtype), np.asarray(k, dtype=dtype), np.asarray(beta, dtype=dtype)
    W = np.stack([identity(D, dtype)] * S)
    logdet, q_trace, status = np.zeros(S, dtype=dtype), np.full((S, n_iter), np.nan, dtype=dtype), np.zeros(S, dtype=np.int32)
    for s in range(S):
        if beta[s] < min_occ:
            status[s] = LOW_OCCUPANCY
            continue
        L = [cholesky(G[s, i]) for i in range(D)]
        if any(f is None for f in L):
            status[s] = NOT_POSITIVE_DEFINITE
            continue
        g = [chol_solve(L[i], k[s, i]) for i in range(D)]
        Ws = (identity(D, dtype) if W0 is None else np.asarray(W0[s], dtype=dtype)).copy()
        Ai, ld = invert(Ws[:, 1:])
        ok, trace = Ai is not None, []
        for it in range(n_iter):
            for i in range(D):
                ok = ok and row_update(i, Ws, Ai, L, g, beta[s], p_scale)
                if ok and on_row is not None:
                    on_row(s, Ws)
            if ok:
                Ai, ld = invert(Ws[:, 1:])
                ok = Ai is not None
            if not ok:
                break
            trace.append(aux(Ws, G[s], k[s], beta[s], ld))
        if not ok:
            status[s] = SINGULAR
            continue
        W[s], logdet[s], q_trace[s] = Ws, ld, trace
    return dict(W=W, logdet=logdet, q_trace=q_trace, status=status)


# ------------------------------------------------------------------ apply, compose
def apply(frames, W, T, begin, utt_speaker):
    """y = b + A x for the rows of the utterances with a speaker whose W is not exactly [0 | I]: the offset first, then the products in
    ascending feature order, one rounding each -> (float64 array, its float32 rounding)"""
    out = np.array(frames, dtype=np.float64)
    D = out.shape[1]
    for u, s in enumerate(utt_speaker):
        if s < 0 or np.array_equal(W[s], identity(D)):
            continue
        x = out[begin[u]:begin[u] + T[u]].copy()
        y = np.broadcast_to(W[s][:, 0], x.shape).copy()
        for e in range(D):
            y = y + W[s][None, :, 1 + e] * x[:, e:e + 1]
        out[begin[u]:begin[u] + T[u]] = y
    return out, out.astype(np.float32)


def compose(W_run, logdet_run, W_new, logdet_new):
    """first W_run, then W_new: A <- A_new A, b <- A_new b + b_new"""
    out = np.empty_like(W_run)
    for s in range(len(W_run)):
        out[s, :, 1:] = W_new[s, :, 1:] @ W_run[s, :, 1:]
        out[s, :, 0] = W_new[s, :, 1:] @ W_run[s, :, 0] + W_new[s, :, 0]
    return out, np.asarray(logdet_run) + np.asarray(logdet_new)


# ------------------------------------------------------------------ population moments (the exact-recovery test)
def population_stats(mu, var, w, A0, b0, count=1000.0):
    """G, k, beta (one speaker) of count frames x = A0^-1 (y - b0), y drawn from the mixture (mu (M, D), var (M, D), w (M,)) with every
    frame given to its own Gaussian: E[zeta zeta^T | m] in closed form"""
    M, D = mu.shape
    Ainv = np.linalg.inv(A0)
    G, k = np.zeros((D, D + 1, D + 1)), np.zeros((D, D + 1))
    for m in range(M):
        mx, Cx = Ainv @ (mu[m] - b0), Ainv @ np.diag(var[m]) @ Ainv.T
        mz = np.concatenate([[1.0], mx])
        Ez = np.outer(mz, mz)
        Ez[1:, 1:] += Cx
        for i in range(D):
            G[i] += count * w[m] / var[m, i] * Ez
            k[i] += count * w[m] * mu[m, i] / var[m, i] * mz
    return G[None], k[None], np.array([count])


# ------------------------------------------------------------------ the inputs the GPU tests run on (tests/test_gpu_fmllr.py)
J, M, S_SPK, MIN_OCC = at.J, at.M, 4, 50.0
T_UTT = np.array([63, 64, 1, 130, 30, 65, 20], dtype=np.int32)
SPEAKER = np.array([0, 1, 2, 0, -1, 1, 2], dtype=np.int32)        # speaker 2: 21 frames, below MIN_OCC; speaker 3: no utterance
GAPS = np.array([5, 0, 3, 1, 0, 7, 2], dtype=np.int64)            # unowned rows before / between the utterances; 4 more behind the last


def make_case(D, seed=0):
    """_adapt_twin.make_case's (7, 70, D) model (dead mixtures in states 2 and 5), one label sequence per utterance over the 7 one-state
    units, and frames drawn along the labels from the model's live mixtures, then pushed through the INVERSE of a per-speaker affine map
    -> (model, labels, frames (F, D) float64, T, begin, speaker, the maps W_true (S, D, D+1))"""
    model = at.make_case(D, seed)[0]
    mean, var, w = model
    rng = np.random.default_rng(77 * D + seed)
    begin = (np.cumsum(GAPS) + np.concatenate([[0], np.cumsum(T_UTT[:-1].astype(np.int64))])).astype(np.int64)
    F = int(begin[-1] + T_UTT[-1] + 4)
    frames = rng.standard_normal((F, D))
    W_true = np.stack([identity(D)] * S_SPK)
    for s in range(S_SPK):
        W_true[s, :, 1:] = np.eye(D) * rng.uniform(0.8, 1.2, D) + 0.05 * rng.standard_normal((D, D))
        W_true[s, :, 0] = 0.5 * rng.standard_normal(D)
    labels = []
    for u, T in enumerate(T_UTT):
        L = max(1, min(4, T // 8))
        lab = rng.integers(0, J, size=L)
        labels.append(lab.astype(np.int32))
        st = lab[np.minimum(np.arange(T) * L // T, L - 1)]
        y = np.empty((T, D))
        for t in range(T):
            live = np.flatnonzero(w[st[t]] > 0)
            m = live[rng.integers(0, len(live))]
            y[t] = mean[st[t], m] + np.sqrt(var[st[t], m]) * rng.standard_normal(D)
        s = SPEAKER[u]
        Wt = W_true[max(s, 0)]
        frames[begin[u]:begin[u] + T] = np.linalg.solve(Wt[:, 1:], (y - Wt[:, 0]).T).T
    return model, labels, frames, T_UTT.copy(), begin, SPEAKER.copy(), W_true
