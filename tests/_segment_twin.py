"""Float64 NumPy twin of segmental GMM training: the stand-alone EM of the reference (E1-E3 below) and the k-means protocol of
include/poccala_hip.h (pcl_seg_kmeans).  Test helper only; pinned to the reference by golden G18 (tests/test_segment_em_twin.py).

E1  loop body: expectation from the current parameters, maximization, the new parameters stored, Q; repeated while
    Q - Q_prev > threshold (Q_prev = -inf at the start); the parameters of the step that fails the test are kept.
E2  mean = sum gamma x / Gamma; variance = sum gamma (x - NEW mean)^2 / Gamma floored at c_covariance; weight = Gamma / n.
E3  Q uses this iteration's gamma with the parameters after the M-step; closed form in `q_closed`.
E4  (include/poccala_hip.h, pcl_seg_em; not the reference, which gives NaN there) a mixture no frame reaches, Gamma = 0: weight 0, its
    mean and variance kept, nothing added to Q.  `maximization` needs the parameters the E-step used (`prev`) to keep them.
The Gaussian is the reference's (util.gaussian_function, quirk Q1): constant -D/2 ln 2 pi - 1/2 sum(var).
"""
import numpy as np

LN2PI = np.log(2 * np.pi)
_M64 = (1 << 64) - 1


def log_gauss(x, mean, var, logdet=False):
    """(n, M) ln N(x_i; mean_m, var_m) as the reference evaluates it."""
    d = x.shape[1]
    const = -0.5 * d * LN2PI - 0.5 * (np.log(var).sum(1) if logdet else var.sum(1))
    diff = x[:, None, :] - mean[None]
    return const[None] - 0.5 * (diff * diff / var[None]).sum(2)


def expectation(x, mean, var, w, logdet=False):
    with np.errstate(divide='ignore'):
        lg = log_gauss(x, mean, var, logdet) + np.log(w)[None]
    top = lg.max(1, keepdims=True)
    lse = top + np.log(np.exp(lg - top).sum(1, keepdims=True))
    return np.exp(lg - lse)


def maximization(x, gamma, c_covariance, prev=None):
    """-> mean, floored variance, weight, un-floored variance, Gamma.  prev = (mean, var) of the E-step: what a mixture with Gamma = 0
    keeps (E4; its un-floored variance is reported as 0); without prev such a mixture gets the reference's NaN."""
    big = gamma.sum(0)
    dead = ~(big > 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = gamma.T @ x / big[:, None]
        s2 = np.einsum('im,imd->md', gamma, (x[:, None, :] - mean[None]) ** 2) / big[:, None]
    var = np.maximum(s2, c_covariance)
    if prev is not None and dead.any():
        mean[dead], var[dead], s2[dead] = prev[0][dead], prev[1][dead], 0.0
    return mean, var, big / len(x), s2, big


def q_closed(big, w, var, s2, logdet=False):
    """E3: Q = sum_m Gamma_m [ln w_m - 1/2 sum_d (ln 2 pi + g(var) + s2 / var)], g(v) = v (quirk Q1) or ln v."""
    g = np.log(var) if logdet else var
    live = big > 0                                              # E4: 0 ln 0 taken as 0
    return float((big[live] * (np.log(w[live]) - 0.5 * (LN2PI + g + s2 / var).sum(1)[live])).sum())


def q_literal(x, gamma, mean, var, w, logdet=False):
    """The double loop of q_function, literally."""
    v1 = float((gamma.sum(0) * np.log(w)).sum())
    lg = log_gauss(x, mean, var, logdet)
    v2 = 0.0
    for m in range(mean.shape[0]):
        for i in range(len(x)):
            v2 += gamma[i, m] * lg[i, m]
    return v1 + v2


def em(x, mean, var, w, c_covariance=1e-3, threshold=1.28, max_iters=1000, logdet=False):
    """-> dict(mean, var, w, q_seq (every loop body's Q), iters (loop bodies run), q (last accepted))"""
    x = np.asarray(x, dtype=np.float64)
    mean, var, w = (np.array(a, dtype=np.float64) for a in (mean, var, w))
    q_old, q_seq = -np.inf, []
    for _ in range(max_iters):
        gamma = expectation(x, mean, var, w, logdet)
        mean, var, w, s2, big = maximization(x, gamma, c_covariance, prev=(mean, var))
        q_new = q_closed(big, w, var, s2, logdet)
        q_seq.append(q_new)
        if q_new - q_old > threshold:
            q_old = q_new
        else:
            break
    return dict(mean=mean, var=var, w=w, q_seq=np.array(q_seq), iters=len(q_seq), q=q_old)


# ---------------------------------------------------------------------- k-means protocol
def uniform(seed, j, k):
    x = (seed * 0x9E3779B97F4A7C15 + (j << 32) + k + 1) & _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return (x >> 11) * 2.0 ** -53


def seeds(x, k, seed, j):
    """k-means++ seeding of one state -> (positions, margin): margin = the smallest |u total - prefix boundary| / total met
    (inf where no D^2 draw happened): the device matches wherever it is above its summation error."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    idx = [min(int(uniform(seed, j, 0) * n), n - 1)]
    d2 = None
    margin = np.inf
    for kk in range(1, k):
        new = ((x - x[idx[-1]]) ** 2).sum(1)
        d2 = new if d2 is None else np.minimum(d2, new)
        total = d2.sum()
        u = uniform(seed, j, kk)
        if not total > 0:
            idx.append(min(int(u * n), n - 1))
            continue
        pre = np.cumsum(d2)
        hit = np.nonzero(pre > u * total)[0]
        if len(hit) == 0:
            idx.append(int(np.nonzero(d2 > 0)[0][-1]))
            margin = 0.0
            continue
        idx.append(int(hit[0]))
        margin = min(margin, float(np.abs(pre - u * total).min() / total))
    return np.array(idx, dtype=np.int32), margin


def lloyd(x, centres, max_sweeps=100, dtype=np.float64):
    """-> (assign, sweeps, centres, margin): margin = the smallest relative gap between a frame's best and second-best squared
    distance over all sweeps (inf for K = 1)."""
    x = np.asarray(x, dtype=np.float64)
    c = np.array(centres, dtype=np.float64)
    n, k = len(x), len(c)
    assign = np.full(n, -1, dtype=np.int32)
    margin, sweeps = np.inf, 0
    xs = x.astype(dtype)
    for _ in range(max_sweeps):
        d2 = ((xs[:, None, :] - c.astype(dtype)[None]) ** 2).sum(2).astype(np.float64)
        new = d2.argmin(1).astype(np.int32)                     # the lowest index wins a tie
        if k > 1:
            srt = np.sort(d2, axis=1)
            margin = min(margin, float(((srt[:, 1] - srt[:, 0]) / np.maximum(srt[:, 1], 1e-300)).min()))
        sweeps += 1
        if np.array_equal(new, assign):
            break
        assign = new
        for kk in range(k):
            sel = assign == kk
            if sel.any():
                c[kk] = x[sel].mean(0)                           # an empty cluster keeps its centre
    return assign, sweeps, c, margin


def cluster_model(x, assign, centres):
    """The model after clustering: cluster mean, max(mean squared deviation, 1e-4), n_k / n (empty cluster: centre, 1e-4, 0)."""
    x = np.asarray(x, dtype=np.float64)
    k = len(centres)
    mean = np.array(centres, dtype=np.float64)
    var = np.full_like(mean, 1e-4)
    w = np.zeros(k)
    for kk in range(k):
        sel = assign == kk
        if sel.any():
            mean[kk] = x[sel].mean(0)
            var[kk] = np.maximum(((x[sel] - mean[kk]) ** 2).mean(0), 1e-4)
            w[kk] = sel.sum() / len(x)
    return mean, var, w


def kmeans(x, k, seed, j=0, max_sweeps=100, init_centres=None):
    x = np.asarray(x, dtype=np.float64)
    c0 = x[seeds(x, k, seed, j)[0]] if init_centres is None else init_centres
    assign, sweeps, c, _ = lloyd(x, c0, max_sweeps)
    return cluster_model(x, assign, c) + (assign, sweeps)


def frame_state_of(frame_unit, frame_k, gmm_num, dropped=None):
    """pcl_batch_regroup's two arrays -> the owner state of every frame (-1: not used)."""
    fu, fk = np.asarray(frame_unit, dtype=np.int64), np.asarray(frame_k, dtype=np.int64)
    out = np.where((fu >= 0) & (fk >= 0), fu * gmm_num + fk, -1)
    if dropped is not None:
        out = np.where(np.asarray(dropped, dtype=bool), -1, out)
    return out.astype(np.int32)
