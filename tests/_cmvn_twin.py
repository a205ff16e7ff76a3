"""NumPy twin of the CMVN rule (include/poccala_hip.h, row f14; csrc/frame_cmvn.hip): the statistics, the per-speaker apply and the
sliding-window form in EXACTLY the header's operation order, in float64, plus long-double direct-sum versions to measure them against.
tests/test_cmvn_twin.py holds the twin's own invariants; tests/test_gpu_cmvn.py holds the device to the twin."""
import numpy as np

CH_ROWS, ROW_LANES, SCAN_ROWS = 1024, 4, 64
OK, LOW_COUNT, NOT_FINITE = 0, 1, 2
LD = np.longdouble


def widen(frames):
    """what the device reads: the float64 copy, or the float32 rows widened"""
    return np.asarray(frames).astype(np.float64)


# ------------------------------------------------------------------ statistics
def chunk_sum(x):
    """(rows <= 1024, D) -> the chunk's sum in the header's order: row lane r adds rows r, r + 4, ... ascending from 0; lanes added 0, 1, 2, 3"""
    lanes = np.zeros((ROW_LANES, x.shape[1]))
    for t in range(x.shape[0]):
        lanes[t % ROW_LANES] = lanes[t % ROW_LANES] + x[t]
    s = lanes[0].copy()
    for r in range(1, ROW_LANES):
        s = s + lanes[r]
    return s


def utt_sum(x):
    """the chunks' sums in chunk order from 0"""
    us = np.zeros(x.shape[1])
    for lo in range(0, x.shape[0], CH_ROWS):
        us = us + chunk_sum(x[lo:lo + CH_ROWS])
    return us


def zero(S, D):
    return dict(n=np.zeros(S, dtype=np.int64), s=np.zeros((S, D)), q=np.zeros((S, D)), sabs=np.zeros((S, D)), qabs=np.zeros((S, D)))


def accumulate(st, frames, T, begin, spk):
    """one pcl_cmvn_accumulate onto st (in place, returned): a speaker's utterances with T > 0 in ascending index.  sabs / qabs: the sums
    of the absolute terms (what an error bound scales with)."""
    x = widen(frames)
    with np.errstate(all='ignore'):
        for s in range(len(st['n'])):
            for u in np.flatnonzero(np.asarray(spk) == s):
                if T[u] == 0:
                    continue
                xu = x[begin[u]:begin[u] + T[u]]
                sq = xu * xu
                st['n'][s] += T[u]
                st['s'][s] = st['s'][s] + utt_sum(xu)
                st['q'][s] = st['q'][s] + utt_sum(sq)
                st['sabs'][s] += np.abs(xu).sum(axis=0)
                st['qabs'][s] += sq.sum(axis=0)
    return st


def accumulate_ld(S, frames, T, begin, spk):
    """the same sums, directly, in long double"""
    x = widen(frames).astype(LD)
    s, q = np.zeros((S, x.shape[1]), dtype=LD), np.zeros((S, x.shape[1]), dtype=LD)
    for u in range(len(T)):
        if spk[u] >= 0:
            xu = x[begin[u]:begin[u] + T[u]]
            s[spk[u]] += xu.sum(axis=0)
            q[spk[u]] += (xu * xu).sum(axis=0)
    return s, q


# ------------------------------------------------------------------ the rule
def floor_var(q_over_n, m, var_floor):
    t = q_over_n - m * m
    return np.where(t > var_floor, t, var_floor)


def normalise(x, m, v, norm_vars):
    return (x - m) / np.sqrt(v) if norm_vars else x - m


def statuses(n, s, q, min_count):
    bad = ~(np.isfinite(s).all(axis=1) & np.isfinite(q).all(axis=1))
    return np.where(n < min_count, LOW_COUNT, np.where(bad, NOT_FINITE, OK)).astype(np.int32)


def check_args(F, T, begin, spk=None, S=None, norm_vars=True, var_floor=1e-20, min_count=1):
    """the refusals of the C-ABI that do not depend on the device's state -> a ValueError"""
    T, begin = np.asarray(T, dtype=np.int64), np.asarray(begin, dtype=np.int64)
    if len(T) < 1 or (T < 0).any() or (begin < 0).any() or (begin + T > F).any():
        raise ValueError('an utterance outside the frame matrix')
    spans = sorted((b, b + t) for b, t in zip(begin, T) if t > 0)
    if any(spans[i][0] < spans[i - 1][1] for i in range(1, len(spans))):
        raise ValueError('the utterances overlap')
    if spk is not None and ((np.asarray(spk) < -1).any() or (np.asarray(spk) >= S).any()):
        raise ValueError('a speaker outside [-1, S)')
    if norm_vars and not (np.isfinite(var_floor) and var_floor > 0):
        raise ValueError('var_floor')
    if min_count < 1:
        raise ValueError('min_count')


def apply(frames, T, begin, spk, n, s, q, norm_vars=True, var_floor=1e-20, min_count=1):
    """pcl_frames_cmvn from the statistics (n, s, q) -> (y64 (F, D): what the float64 copy holds afterwards -- or would, were there one
    --, status (S,)).  The float32 rows hold y64.astype(float32) where a row was normalised, their old bits elsewhere (apply32)."""
    check_args(len(frames), T, begin, spk, len(n), norm_vars, var_floor, min_count)
    y = widen(frames).copy()
    st = statuses(n, s, q, min_count)
    with np.errstate(all='ignore'):
        for u in range(len(T)):
            sp = spk[u]
            if sp < 0 or st[sp] != OK:
                continue
            nn = np.float64(n[sp])
            m = s[sp] / nn
            v = floor_var(q[sp] / nn, m, var_floor)
            rows = slice(begin[u], begin[u] + T[u])
            y[rows] = normalise(y[rows], m, v, norm_vars)
    return y, st


def touched(F, T, begin, keep=None):
    """rows of the matrix that a call rewrites"""
    on = np.zeros(F, dtype=bool)
    for u in range(len(T)):
        if keep is None or keep[u]:
            on[begin[u]:begin[u] + T[u]] = True
    return on


def as_rows32(frames32, y64, on):
    """the float32 rows after a call: float32(y) on the rewritten rows, the old bits elsewhere"""
    out = np.array(frames32, dtype=np.float32, copy=True)
    out[on] = y64[on].astype(np.float32)
    return out


# ------------------------------------------------------------------ sliding window
def window_bounds(t, T, window, min_window, center):
    if center:
        lo = t - window // 2
        hi = lo + window
        if lo < 0:
            hi -= lo
            lo = 0
        if hi > T:
            lo = max(0, lo - (hi - T))
            hi = T
    else:
        lo = max(0, t - window + 1)
        hi = t + 1
        if hi - lo < min_window:
            hi = min(T, lo + min_window)
    return lo, hi


def window_bounds_all(T, window, min_window, center):
    """window_bounds for every t at once (the same integer rule, vectorised)"""
    t = np.arange(T, dtype=np.int64)
    if center:
        lo = t - window // 2
        hi = lo + window
        neg = lo < 0
        hi = np.where(neg, hi - lo, hi)
        lo = np.where(neg, 0, lo)
        over = hi > T
        lo = np.where(over, np.maximum(0, lo - (hi - T)), lo)
        hi = np.where(over, T, hi)
    else:
        lo = np.maximum(0, t - window + 1)
        hi = t + 1
        hi = np.where(hi - lo < min_window, np.minimum(T, lo + min_window), hi)
    return lo, hi


def prefix(x):
    """(T, D) -> P (T + 1, D) in the header's order: blocks of 64 rows, the local inclusive prefix in ascending row order from 0, the block
    totals scanned in ascending block order from 0, P[r + 1] = offset[block of r] + local[r], P[0] = 0"""
    T, D = x.shape
    P = np.zeros((T + 1, D))
    off = np.zeros(D)
    for lo in range(0, T, SCAN_ROWS):
        blk = x[lo:lo + SCAN_ROWS]
        local = np.zeros(blk.shape)
        a = np.zeros(D)
        for r in range(blk.shape[0]):
            a = a + blk[r]
            local[r] = a
        P[lo + 1:lo + 1 + blk.shape[0]] = off + local
        off = off + a
    return P


def sliding(frames, T, begin, window, min_window, center, norm_vars=False, var_floor=1e-20):
    """pcl_frames_cmvn_sliding -> y64 (F, D)"""
    check_args(len(frames), T, begin, norm_vars=norm_vars, var_floor=var_floor)
    if not (1 <= min_window <= window <= 1 << 20):
        raise ValueError('window limits')
    y = widen(frames).copy()
    with np.errstate(all='ignore'):
        for u in range(len(T)):
            if T[u] == 0:
                continue
            x = y[begin[u]:begin[u] + T[u]].copy()
            Ps, Pq = prefix(x), prefix(x * x)
            lo, hi = window_bounds_all(int(T[u]), window, min_window, center)
            n = (hi - lo).astype(np.float64)[:, None]
            m = (Ps[hi] - Ps[lo]) / n
            v = floor_var((Pq[hi] - Pq[lo]) / n, m, var_floor) if norm_vars else None
            y[begin[u]:begin[u] + T[u]] = normalise(x, m, v, norm_vars)
    return y


def sliding_ld(x, window, min_window, center, norm_vars=False, var_floor=1e-20):
    """one utterance (T, D), window sums taken directly in long double -> y (long double)"""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    y = np.empty(x.shape, dtype=LD)
    for t in range(len(x)):
        lo, hi = window_bounds(t, len(x), window, min_window, center)
        w = x[lo:hi]
        m = w.sum(axis=0) / LD(hi - lo)
        c = x[t] - m
        if norm_vars:
            v = (w * w).sum(axis=0) / LD(hi - lo) - m * m
            c = c / np.sqrt(np.where(v > var_floor, v, LD(var_floor)))
        y[t] = c
    return y


# ------------------------------------------------------------------ the inputs the GPU tests run on (tests/test_gpu_cmvn.py)
S_SPK, MIN_COUNT = 4, 50
T_UTT = np.array([63, 64, 1, 130, 30, 65, 20, 0], dtype=np.int32)
SPEAKER = np.array([0, 1, 2, 0, -1, 1, 2, 0], dtype=np.int32)     # speaker 2: 21 frames, below MIN_COUNT; speaker 3: no utterance
GAPS = np.array([5, 0, 3, 1, 0, 7, 2, 1], dtype=np.int64)         # unowned rows before / between the utterances; 4 more behind the last


def layout(T, gaps, tail=4):
    T = np.asarray(T, dtype=np.int32)
    begin = (np.cumsum(gaps) + np.concatenate([[0], np.cumsum(T[:-1].astype(np.int64))])).astype(np.int64)
    return T, begin, int(begin[-1] + T[-1] + tail)


def make_case(D, seed=0, T=T_UTT, gaps=GAPS):
    """-> (frames (F, D) float64 with a per-utterance offset and per-column scale, column 0 of speaker 1 constant, T, begin, speaker)"""
    T, begin, F = layout(T, gaps)
    rng = np.random.default_rng(1000 * D + seed)
    frames = rng.standard_normal((F, D))
    scale = rng.uniform(0.2, 5.0, D)
    for u in range(len(T)):
        frames[begin[u]:begin[u] + T[u]] = frames[begin[u]:begin[u] + T[u]] * scale + 3.0 * rng.standard_normal(D)
    spk = SPEAKER[:len(T)].copy() if len(T) <= len(SPEAKER) else np.zeros(len(T), dtype=np.int32)
    for u in np.flatnonzero(spk == 1):
        frames[begin[u]:begin[u] + T[u], 0] = 2.5                  # a constant column: its variance is 0 or rounding, the floor decides
    return frames, T, begin, spk
