"""NumPy twin of csrc/model_adapt.hip: the adaptation rules of include/poccala_hip.h (pcl_mllr_estimate, pcl_model_transform_means,
pcl_mstep_map) in float64, with a straightforward loop over the mixtures for G and k and np.linalg.cholesky for the solve.
tests/test_adapt_twin.py holds the twin's own invariants; tests/test_gpu_adapt.py compares the device with it."""
import numpy as np

BIAS = 100.0                                   # mean_acc = sum gamma (o + BIAS): the accumulate pass's constant
OK, LOW_OCCUPANCY, FEW_MIXTURES, NOT_POSITIVE_DEFINITE = 0, 1, 2, 3


def identity(D):
    return np.concatenate([np.zeros((D, 1)), np.eye(D)], axis=1)


def contributes(acc):
    return np.isfinite(acc) & (acc > 0)


def mllr_estimate(mean, var, acc, mean_acc, state_class=None, n_classes=1, min_occ=1000.0):
    """-> dict(W (R, D, D+1), occ (R,), status (R,) int32, and per class and dimension G (R, D, n, n), k (R, D, n), the sums of the
    absolute terms Gabs / kabs, cond (R, D) = cond(G[r, i]) (nan for a class without a contributing mixture))"""
    J, M, D = mean.shape
    R, n = int(n_classes), D + 1
    cls = np.zeros(J, dtype=np.int64) if state_class is None else np.asarray(state_class, dtype=np.int64)
    if R < 1 or cls.shape != (J,) or (cls < -1).any() or (cls >= R).any() or not (np.isfinite(min_occ) and min_occ >= 0):
        raise ValueError('mllr_estimate: bad classes or min_occ')
    s = mean_acc - BIAS * acc[:, :, None]
    W = np.stack([identity(D)] * R)
    occ, status = np.zeros(R), np.zeros(R, dtype=np.int32)
    G, Gabs = np.zeros((R, D, n, n)), np.zeros((R, D, n, n))
    k, kabs = np.zeros((R, D, n)), np.zeros((R, D, n))
    cond = np.full((R, D), np.nan)
    for r in range(R):
        count = 0
        for j in np.flatnonzero(cls == r):
            for m in range(M):
                if not contributes(acc[j, m]):
                    continue
                count += 1
                occ[r] += acc[j, m]
                xi = np.concatenate([[1.0], mean[j, m]])
                outer = np.outer(xi, xi)
                c = acc[j, m] / var[j, m]                                   # (D,)
                G[r] += c[:, None, None] * outer[None]
                Gabs[r] += np.abs(c)[:, None, None] * np.abs(outer)[None]
                sv = s[j, m] / var[j, m]
                k[r] += sv[:, None] * xi[None]
                kabs[r] += np.abs(sv)[:, None] * np.abs(xi)[None]
        if count:
            with np.errstate(all='ignore'):
                cond[r] = [np.linalg.cond(G[r, i]) if np.isfinite(G[r, i]).all() else np.inf for i in range(D)]
        if occ[r] < min_occ:
            status[r] = LOW_OCCUPANCY
            continue
        if count < n:
            status[r] = FEW_MIXTURES
            continue
        rows = []
        for i in range(D):
            try:
                if not np.isfinite(G[r, i]).all():
                    raise np.linalg.LinAlgError('not finite')
                L = np.linalg.cholesky(G[r, i])
                if not (np.isfinite(np.diag(L)).all() and (np.diag(L) > 0).all()):
                    raise np.linalg.LinAlgError('pivot')
            except np.linalg.LinAlgError:
                status[r] = NOT_POSITIVE_DEFINITE
                break
            y = np.linalg.solve(L, k[r, i])
            rows.append(np.linalg.solve(L.T, y))
        if status[r] == OK:
            W[r] = np.stack(rows)
    return dict(W=W, occ=occ, status=status, G=G, k=k, Gabs=Gabs, kabs=kabs, cond=cond)


def transform_means(mean, W, state_class=None):
    """mean[j, m] <- b_r + A_r mean[j, m]: the offset first, then the products in ascending feature order, one rounding each (the device's
    order); states of class -1 and classes whose W is exactly [0 | I] keep their bits.  Also returns the sum of the absolute terms."""
    J, M, D = mean.shape
    cls = np.zeros(J, dtype=np.int64) if state_class is None else np.asarray(state_class, dtype=np.int64)
    out, scale = mean.copy(), np.abs(mean)
    for j in range(J):
        r = cls[j]
        if r < 0 or np.array_equal(W[r], identity(D)):
            continue
        acc = np.broadcast_to(W[r][:, 0], (M, D)).copy()
        ab = np.abs(acc)
        for e in range(D):
            acc = acc + W[r][None, :, 1 + e] * mean[j, :, e:e + 1]
            ab = ab + np.abs(W[r][None, :, 1 + e] * mean[j, :, e:e + 1])
        out[j], scale[j] = acc, ab
    return out, scale


def map_means(mean, acc, mean_acc, tau):
    """mean <- (tau mean + s) / (tau + acc) where acc is finite and > 0"""
    if not (np.isfinite(tau) and tau >= 0):
        raise ValueError('map_means: tau = %r' % (tau,))
    s = mean_acc - BIAS * acc[:, :, None]
    live = contributes(acc)
    with np.errstate(all='ignore'):
        new = (tau * mean + s) / (tau + acc)[:, :, None]
    return np.where(live[:, :, None], new, mean)


# ------------------------------------------------------------------ the inputs the GPU tests run on (tests/test_gpu_adapt.py)
J, M = 7, 70
CLASSES3 = np.array([-1, 0, 0, 0, 0, 1, 2], dtype=np.int32)     # state 0 left alone; class 1 = state 5 (few mixtures); class 2 = state 6 (low occupancy)
MIN_OCC3 = 10.0
ALIVE5 = 10                                                      # state 5 keeps 10 mixtures with a weight: fewer than D + 1 for every D >= 10 the tests use (12 .. 48);
                                                                 # at D = 1 and 2 it is NOT short of mixtures, and the tests take the statuses from the twin


def make_case(D, seed=0, frames_n=900):
    """A (7, 70, D) model -- means ~ N(0, 1) per dimension, variances in [0.5, 2], a third of state 2's weights zero, state 5 with ALIVE5
    live mixtures -- and an adaptation batch: frames drawn from the model's live mixtures with shifted and scaled means, state posteriors
    that put 0.6 on the state a frame came from and spread the rest (state 6 gets a hundredth of its share).
    -> (mean, var, w), frames (F, D), gamma (F, J)"""
    rng = np.random.default_rng(1000 * D + seed)
    mean = rng.standard_normal((J, M, D))
    var = rng.uniform(0.5, 2.0, (J, M, D))
    w = rng.uniform(0.2, 1.0, (J, M))
    w[2, ::3] = 0.0
    w[5, ALIVE5:] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    live = np.argwhere(w > 0)
    pick = live[rng.integers(0, len(live), frames_n)]
    scale, shift = rng.uniform(0.8, 1.2, D), rng.standard_normal(D) * 0.5
    mu, vr = mean[pick[:, 0], pick[:, 1]], var[pick[:, 0], pick[:, 1]]
    frames = scale * mu + shift + np.sqrt(vr) * rng.standard_normal((frames_n, D))
    gamma = rng.uniform(0.2, 1.0, (frames_n, J))
    gamma[:, 6] *= 0.01
    gamma = 0.4 * gamma / gamma.sum(axis=1, keepdims=True)
    gamma[np.arange(frames_n), pick[:, 0]] += 0.6
    gamma[:, 6] *= 0.01
    return (mean, var, w), frames, gamma / gamma.sum(axis=1, keepdims=True)


def numpy_stats(model, frames, gamma):
    """acc (J, M) and mean_acc (J, M, D) as the accumulate pass defines them: gamma_t(j, m) = gamma_t(j) x the mixture's share of b_j(o_t)
    (the reference's density, util.py:29: -1/2 sum(var) in the constant)"""
    mean, var, w = model
    Jn, Mn, D = mean.shape
    acc, macc = np.zeros((Jn, Mn)), np.zeros((Jn, Mn, D))
    for j in range(Jn):
        with np.errstate(divide='ignore'):
            lw = np.log(w[j])
        d2 = ((frames[:, None, :] - mean[j][None]) ** 2 / (2 * var[j][None])).sum(axis=2)          # (F, M)
        lp = lw[None] - 0.5 * var[j].sum(axis=1)[None] - d2
        lp -= lp.max(axis=1, keepdims=True)
        p = np.exp(lp)
        g = gamma[:, j:j + 1] * p / p.sum(axis=1, keepdims=True)
        acc[j] = g.sum(axis=0)
        macc[j] = g.T @ (frames + BIAS)
    return acc, macc
