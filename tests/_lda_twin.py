"""NumPy float64 twin of csrc/frame_lda.hip and Engine.lda_estimate (row f12; the rule: include/poccala_hip.h): splice, class
statistics, the LDA estimate, the projection.  tests/test_lda_twin.py holds its own invariants; tests/test_gpu_lda.py and
tests/test_gpu_lda_edges.py compare the device with it."""
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


# ------------------------------------------------------------------ the edges of the device's tiling (tests/test_gpu_lda_edges.py)
TILE, KSTEP_ROWS, STEP_ROWS, CHUNK_DEFAULT, ROUND = 16, 4, 32, 1024, 1024      # frame_lda.hip: a tile's order, rows per MFMA, KB, LDA_CHUNK_DEFAULT, LDA_ROUND

# (D, left, right, order n = Ds + 1, tile rows NT): every NT the launcher has an instance for.  n = 16, 64, 112, 128: no zero padding column,
# the ones column is the last column of the last tile; n = 17, 65: the ones column alone in its tile; n = 128: the cap
EDGE_SHAPES = [(1, 0, 0, 2, 1), (5, 1, 1, 16, 1), (16, 0, 0, 17, 2), (13, 1, 1, 40, 3), (7, 4, 4, 64, 4), (16, 2, 1, 65, 5), (5, 9, 8, 91, 6),
               (37, 1, 1, 112, 7), (1, 63, 63, 128, 8)]

# one class per row count, an empty class in the middle and one at the end
KEDGE_COUNTS = [1, 3, 4, 5, 15, 16, 17, 0, 31, 32, 33, 63, 64, 65, 97, 0]
KEDGE_LENGTHS = [1, 2, 3, 9, 40, 64, 65, 130, 150]
# PCL_LDA_CHUNK=1: class 0 ends ON the edge of round 0, class 1 is empty at that edge, class 2 lies in rounds 1 and 2
ROUND_COUNTS = [1024, 0, 1500, 0, 30, 0]
ROUND_LENGTHS = [1, 2, 3, 700, 900, 1000]
# ... and at order 40 (6 tiles per chunk) the edge of round 0 falls inside class 2
ROUND40_COUNTS = [1000, 0, 70, 0, 30, 0]
ROUND40_LENGTHS = [1, 2, 3, 400, 750]
LONG_ROWS = 64 * 256 + 300                                    # behind what one pass of the key kernel's grid covers
LONG_LENGTHS = [5, LONG_ROWS, 3]
# two projections in a row, (D, left, right, D_out) each: the first leaves 40 dimensions, held at a row stride of 47, for the second to splice
CHAIN = [(13, 2, 1, 40), (40, 1, 0, 64)]
DEVICE_DIMS = (13, 26, 39, 47, 48, 64)                        # the row strides the device holds a frame matrix at (pcl_api.hip, device_dim)
LONG_PERIOD, LONG_R = 7, 6                                     # the class of row t of an utterance: t mod 7, 6 -> not kept


def place(lengths, D, rng):
    """make_case's layout for any list of lengths: gaps of 1 .. 3 rows between the utterances, rows of no utterance far from everything,
    neighbouring utterances offset by +-1000.  -> frames (F, D), T, begin, owned (F,) bool"""
    T = np.array(lengths, dtype=np.int32)
    begin = np.empty(len(T), dtype=np.int64)
    row = 3
    for u, t in enumerate(T):
        begin[u] = row
        row += int(t) + int(rng.integers(1, 4))
    F = row + 2
    frames = rng.standard_normal((F, D)) * 5 + 7777.0
    owned = np.zeros(F, dtype=bool)
    for u, (t, b) in enumerate(zip(T, begin)):
        frames[b:b + t] = rng.standard_normal((t, D)) + (1000.0 if u % 2 else -1000.0) + np.arange(D)
        owned[b:b + t] = True
    return frames, T, begin, owned


def plant_case(D, lengths, counts, seed=0):
    """Utterances of the given lengths with EXACTLY counts[r] rows of class r (0: an empty class), drawn without replacement from all
    the utterances' rows, so that a class is scattered over the utterances; the utterances' other rows are -1.  Every row of NO utterance is
    labelled with the last non-empty class: labelled, and not to be kept.  -> frames (F, D) float64, T, begin, frame_class (F,)"""
    rng = np.random.default_rng(500 + seed + D)
    counts = np.asarray(counts, dtype=np.int64)
    frames, T, begin, owned = place(lengths, D, rng)
    if counts.sum() > owned.sum() or (counts < 0).any() or not (counts > 0).any():
        raise ValueError('%d rows to plant in utterances of %d rows' % (counts.sum(), owned.sum()))
    cls = np.full(len(frames), -1, dtype=np.int32)
    rows = rng.permutation(np.flatnonzero(owned))[:counts.sum()]
    cls[rows] = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    cls[~owned] = np.flatnonzero(counts > 0)[-1]
    return frames, T, begin, cls


def long_case(D=2, seed=0):
    """One utterance of LONG_ROWS rows between two short ones; the class of row t of an utterance is t mod LONG_PERIOD (a period co-prime
    to the key kernel's 256 threads and to the projection's 16-frame tiles), LONG_R = 6 classes, residue 6 not kept; rows of no utterance
    labelled 0."""
    frames, T, begin, owned = place(LONG_LENGTHS, D, np.random.default_rng(900 + seed + D))
    cls = np.zeros(len(frames), dtype=np.int32)
    for t, b in zip(T, begin):
        c = np.arange(t, dtype=np.int32) % LONG_PERIOD
        cls[b:b + t] = np.where(c < LONG_R, c, -1)
    return frames, T, begin, cls


def chunk_plan(counts, chunk=None, round_chunks=ROUND):
    """How pcl_launch_lda_accumulate cuts class counts into K-chunks and launch rounds (chunk None: the default).  -> dict: rows (per chunk),
    cls_chunk0 (R + 1,), chunks, rounds, split (the classes whose chunks lie in more than one round)"""
    chunk = CHUNK_DEFAULT if chunk is None else int(chunk)
    rows, cls_chunk0 = [], [0]
    for c in np.asarray(counts, dtype=np.int64):
        rows += [int(min(chunk, c - v)) for v in range(0, int(c), chunk)]
        cls_chunk0.append(len(rows))
    split = [r for r in range(len(cls_chunk0) - 1)
             if cls_chunk0[r + 1] > cls_chunk0[r] and cls_chunk0[r] // round_chunks != (cls_chunk0[r + 1] - 1) // round_chunks]
    return dict(rows=rows, cls_chunk0=np.array(cls_chunk0), chunks=len(rows), rounds=-(-len(rows) // round_chunks), split=split)


def chunk_steps(n):
    """What the product kernel's loops do for a chunk of n rows: steps = iterations of the k0 loop (32 rows each); second = a wave issues
    its second MFMA k-step (rows 16 .. 31 of a step); early = a wave leaves a step at the break (a step with fewer than 29 rows)"""
    left = [min(STEP_ROWS, n - k0) for k0 in range(0, n, STEP_ROWS)]
    return dict(steps=len(left), second=any(m > 4 * KSTEP_ROWS for m in left), early=any(m <= STEP_ROWS - KSTEP_ROWS for m in left))
