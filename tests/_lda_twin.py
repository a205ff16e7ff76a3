"""NumPy float64 twin of csrc/frame_lda.hip and Engine.lda_estimate (row f12; the rule: include/poccala_hip.h): splice, class
statistics, the LDA estimate, the projection.  tests/test_lda_twin.py holds its own invariants; tests/test_gpu_lda.py compares the device
with it."""
import numpy as np


def splice(frames, T, begin, left, right):
    """(F, (left + right + 1) D) float64: for every row of a listed utterance the rows clamp(g + k, begin, begin + T - 1), k = -left .. right,
    side by side; rows of no utterance are zero.  owned (F,) bool marks the rows of the utterances."""
    x = np.asarray(frames, dtype=np.float64)
    F, D = x.shape
    out = np.zeros((F, (left + right + 1) * D))
    owned = np.zeros(F, dtype=bool)
    for t, b in zip(T, begin):
        t, b = int(t), int(b)
        if t == 0:
            continue
        g = np.arange(b, b + t)
        owned[g] = True
        for j, k in enumerate(range(-left, right + 1)):
            out[g, j * D:(j + 1) * D] = x[np.clip(g + k, b, b + t - 1)]
    return out, owned


def fold(frame_state, state_class):
    """owner states -> classes: -1 stays -1, state j becomes state_class[j] (None: identity)"""
    st = np.asarray(frame_state)
    if state_class is None:
        return st.copy()
    sc = np.asarray(state_class)
    return np.where(st >= 0, sc[np.maximum(st, 0)], -1).astype(st.dtype)


def stats(frames, T, begin, frame_class, R, left, right):
    """dict n (R,), s (R, Ds), S (R, Ds, Ds) and sabs / Sabs, the sums of the ABSOLUTE terms (what an error bound is taken from)"""
    xs, owned = splice(frames, T, begin, left, right)
    cls = np.where(owned, np.asarray(frame_class), -1)
    Ds = xs.shape[1]
    out = dict(n=np.zeros(R), s=np.zeros((R, Ds)), S=np.zeros((R, Ds, Ds)), sabs=np.zeros((R, Ds)), Sabs=np.zeros((R, Ds, Ds)))
    for r in range(R):
        x = xs[cls == r]
        out['n'][r] = len(x)
        out['s'][r] = x.sum(axis=0)
        out['S'][r] = x.T @ x
        out['sabs'][r] = np.abs(x).sum(axis=0)
        out['Sabs'][r] = np.abs(x).T @ np.abs(x)
    return out


def estimate(n, s, S, D_out, eps=1e-10):
    """(A (D_out, Ds), b (D_out,), eigenvalues (D_out,) descending) by the header's eight steps"""
    n, s, S = np.asarray(n, dtype=np.float64), np.asarray(s, dtype=np.float64), np.asarray(S, dtype=np.float64)
    Ds = s.shape[1]
    live = np.flatnonzero(n > 0)
    N = n[live].sum()
    m = s[live].sum(axis=0) / N
    W, B = np.zeros((Ds, Ds)), np.zeros((Ds, Ds))
    for r in live:
        W += S[r] - np.outer(s[r], s[r]) / n[r]
        d = s[r] / n[r] - m
        B += n[r] * np.outer(d, d)
    W /= N
    B /= N
    W = 0.5 * (W + W.T)
    W[np.diag_indices(Ds)] += eps * np.trace(W) / Ds
    L = np.linalg.cholesky(W)
    Li = np.linalg.solve(L, np.eye(Ds))
    M = Li @ B @ Li.T
    lam, V = np.linalg.eigh(0.5 * (M + M.T))
    top = np.argsort(-lam, kind='stable')[:D_out]
    A = V[:, top].T @ Li
    b = -A @ m
    flip = A[np.arange(D_out), np.abs(A).argmax(axis=1)] < 0
    A[flip] = -A[flip]
    b[flip] = -b[flip]
    return A, b, lam[top]


def project(frames, T, begin, left, right, A, b):
    """(y64 (F, D_out), y32 = float32(y64), mag (F, D_out) = |b_i| + sum_p |A_ip x_p|): b first, then the terms in ascending index order;
    rows of no utterance are zero"""
    xs, owned = splice(frames, T, begin, left, right)
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    y = np.tile(b, (len(xs), 1))
    for p in range(xs.shape[1]):
        y = y + A[:, p][None, :] * xs[:, p][:, None]
    mag = np.abs(b)[None, :] + np.abs(xs) @ np.abs(A).T
    y[~owned] = 0.0
    mag[~owned] = 0.0
    return y, y.astype(np.float32), mag


def class_covariances(y, cls, R):
    """(within, between, mean) of projected rows y with classes cls (-1 skipped), both divided by the number of kept rows"""
    keep = cls >= 0
    N = keep.sum()
    m = y[keep].mean(axis=0)
    W, B = np.zeros((y.shape[1],) * 2), np.zeros((y.shape[1],) * 2)
    for r in range(R):
        x = y[cls == r]
        if len(x):
            d = x - x.mean(axis=0)
            W += d.T @ d
            B += len(x) * np.outer(x.mean(axis=0) - m, x.mean(axis=0) - m)
    return W / N, B / N, m


def nearest_mean_error(y, cls, R):
    """share of the kept rows whose nearest class mean (Euclidean, lowest class on a tie) is not their own class's"""
    keep = np.flatnonzero(cls >= 0)
    live = [r for r in range(R) if (cls == r).any()]
    means = np.stack([y[cls == r].mean(axis=0) for r in live])
    d = ((y[keep][:, None, :] - means[None, :, :]) ** 2).sum(axis=2)
    return float((np.asarray(live)[d.argmin(axis=1)] != cls[keep]).mean())


def principal_angle(A2, basis):
    """the largest principal angle (radians) between the row space of A2 (k, Ds) and the column space of basis (Ds, k)"""
    qa = np.linalg.qr(np.asarray(A2).T)[0]
    qb = np.linalg.qr(np.asarray(basis))[0]
    sv = np.linalg.svd(qa.T @ qb, compute_uv=False)
    return float(np.arccos(np.clip(sv.min(), -1.0, 1.0)))


# ------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
LENGTHS = [1, 2, 3, 9, 40, 64, 65]
R_CASE = 5


def make_case(D, seed=0):
    """The statistics case of the GPU test: 7 utterances of LENGTHS with gaps between them, neighbouring utterances offset by +-1000 (a read
    across a boundary cannot hide), R = 5 with class 3 empty and some rows -1.  -> frames (F, D) float64, T, begin, frame_class (F,)"""
    rng = np.random.default_rng(100 + seed + D)
    T = np.array(LENGTHS, dtype=np.int32)
    begin = np.empty(len(T), dtype=np.int64)
    row = 3
    for u, t in enumerate(T):
        begin[u] = row
        row += int(t) + int(rng.integers(1, 4))
    F = row + 2
    frames = rng.standard_normal((F, D)) * 5 + 7777.0          # rows of no utterance: far from everything
    cls = np.full(F, -1, dtype=np.int32)
    for u, (t, b) in enumerate(zip(T, begin)):
        frames[b:b + t] = rng.standard_normal((t, D)) + (1000.0 if u % 2 else -1000.0) + np.arange(D)
        c = rng.choice([0, 1, 2, 4], size=t).astype(np.int32)
        c[rng.random(t) < 0.15] = -1
        cls[b:b + t] = c
    cls[begin[4]:begin[4] + 30] = 2                             # class 2 spans several chunks of 16 inside one utterance
    cls[:3] = 1                                                 # labelled rows outside every utterance: not kept
    return frames, T, begin, cls


def planted_case(seed=7, D=3, left=1, right=1, R=4, U=12, T_each=60):
    """Planted data: the class means of the SPLICED vectors differ only inside a known 2-dimensional subspace (basis (Ds, 2)), the noise is
    isotropic.  A frame's class is constant inside its utterance, so the spliced vector of a row is (mean_c, mean_c, mean_c) + noise with
    mean_c = centre + basis_D coefficients: the subspace is span{(v1, v1, v1), (v2, v2, v2)}.  -> frames, T, begin, frame_class, basis"""
    rng = np.random.default_rng(seed)
    v = np.linalg.qr(rng.standard_normal((D, 2)))[0]
    coef = rng.standard_normal((R, 2)) * 4
    T = np.full(U, T_each, dtype=np.int32)
    begin = (np.arange(U) * (T_each + 2) + 1).astype(np.int64)
    F = int(begin[-1] + T_each + 1)
    frames = np.zeros((F, D))
    cls = np.full(F, -1, dtype=np.int32)
    for u in range(U):
        c = u % R
        frames[begin[u]:begin[u] + T_each] = 2.0 + coef[c] @ v.T + rng.standard_normal((T_each, D))
        cls[begin[u]:begin[u] + T_each] = c
    basis = np.concatenate([v] * (left + right + 1), axis=0)
    return frames, T, begin, cls, basis
