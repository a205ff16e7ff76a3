"""NumPy float64 definition of the pitch and voicing features (rule P1-P5 of include/poccala_hip.h, pcl_pitch): the reference has no
pitch code, so this twin IS the definition the device kernels (csrc/pitch.hip) are held against.

  geometry  size = int(rate * sampletime), step = int(size * overlap), T = max(1, 1 + ceil((n - size) / step)), frame t starts at sample
            t * step, samples beyond the signal are zero: the MFCC's rows.  Lags Lmin = ceil(rate / f_max) .. Lmax = floor(rate / f_min).
  P1  w = x[t*step : t*step + size + Lmax] - mean(first `size` samples of it); the mean's sum: 64 partial sums, partial j = 0 + w[j] +
      w[j + 64] + ... (ascending), then 0 + partial 0 + partial 1 + ... (ascending), then one division by size
  P2  a = w[0:size], b_l = w[l : l + size]; p = a.b_l, e0 = a.a, el = b_l.b_l, each summed over the sample index in ascending order, one
      multiplication and one addition at a time, starting from 0 (el directly, not incrementally);
      nccf_raw = p / sqrt(e0 * el), 0 where e0 * el == 0; nccf_bal = p / sqrt(e0 * el + ballast), 0 where that sum is 0
  P3  c(t, l) = 1 - nccf_bal(t, l) * (1 - soft_min_f0 * l / rate)
  P4  best(0, l) = c(0, l); best(t, l) = c(t, l) + min_l' [best(t-1, l') + pf * (g[l] - g[l'])^2], g = ln(lag), ties to the smallest l';
      the last frame takes the smallest l of its minimum, then the back-pointers are followed
  P5  v = nccf_raw(t, l*); ln f0 = ln(rate / (l* + shift)), shift = the vertex of the parabola through nccf_raw at l* - 1, l*, l* + 1 clamped
      to +-0.5 (0 at the ends of the lag grid and where the parabola's second difference is not negative); delta of ln f0 = ((x[t+1] - x[t-1]) +
      2 (x[t+2] - x[t-2])) / 10 with the frame indices clamped to the utterance (the MFCC's +-2-frame rule; a constant gives exactly 0)
Every step is one correctly rounded float64 operation at a time, in the order written here, so that the kernels can match it bit for bit
(everything but the final ln, which is the platform's).
"""
import math

import numpy as np

BALLAST, SOFT_MIN_F0, PF = 7000.0, 10.0, 0.1


def geometry(rate, sampletime=0.025, overlap=0.5, f_min=50.0, f_max=400.0):
    size = int(rate * sampletime)
    step = int(size * overlap)
    lmin, lmax = int(math.ceil(rate / f_max)), int(math.floor(rate / f_min))
    return size, step, lmin, lmax


def frame_count(n, size, step):
    return max(1, 1 + int(math.ceil((n - size) / step)))


def log_lags(lmin, lmax):
    """g of P4: what the caller hands to the device."""
    return np.log(np.arange(lmin, lmax + 1, dtype=np.float64))


def windows(x, size, step, lmax):
    """P1: (T, size + lmax) mean-free windows."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    T = frame_count(len(x), size, step)
    W = size + lmax
    pad = np.zeros((T - 1) * step + W)
    pad[:min(len(x), len(pad))] = x[:len(pad)]
    w = np.stack([pad[t * step:t * step + W] for t in range(T)])
    part = np.zeros((T, 64))
    for i0 in range(0, size, 64):                       # partial j: ascending i = j, j + 64, ...
        blk = w[:, i0:min(i0 + 64, size)]
        part[:, :blk.shape[1]] = part[:, :blk.shape[1]] + blk
    tot = np.zeros(T)
    for j in range(64):
        tot = tot + part[:, j]
    return w - (tot / float(size))[:, None]


def nccf(x, rate, sampletime=0.025, overlap=0.5, f_min=50.0, f_max=400.0, ballast=BALLAST):
    """P1-P2: (nccf_bal, nccf_raw), each (T, L)."""
    size, step, lmin, lmax = geometry(rate, sampletime, overlap, f_min, f_max)
    w = windows(x, size, step, lmax)
    T, L = len(w), lmax - lmin + 1
    p, e0, el = np.zeros((T, L)), np.zeros((T, 1)), np.zeros((T, L))
    for i in range(size):                               # ascending sample index, one multiplication and one addition at a time
        a = w[:, i:i + 1]
        b = w[:, lmin + i:lmin + i + L]
        p = p + a * b
        e0 = e0 + a * a
        el = el + b * b
    den = e0 * el
    with np.errstate(all='ignore'):
        raw = np.where(den == 0.0, 0.0, p / np.sqrt(den))
        db = den + ballast
        bal = np.where(db == 0.0, 0.0, p / np.sqrt(db))
    return bal, raw


def track(bal, rate, lmin, g, soft_min_f0=SOFT_MIN_F0, pf=PF):
    """P3-P4 on one utterance's (T, L) nccf_bal: (T,) lag indices (0 = Lmin)."""
    bal = np.asarray(bal, dtype=np.float64)
    T, L = bal.shape
    lag = np.arange(lmin, lmin + L, dtype=np.float64)
    fac = 1.0 - soft_min_f0 * lag / float(rate)
    c = 1.0 - bal * fac[None, :]
    d = g[:, None] - g[None, :]                         # [l, l']
    trans = pf * (d * d)
    best = c[0].copy()
    bp = np.zeros((T, L), dtype=np.int64)
    for t in range(1, T):
        cand = best[None, :] + trans
        arg = np.argmin(cand, axis=1)                   # the first of equal minima: the smallest l'
        best = c[t] + cand[np.arange(L), arg]
        bp[t] = arg
    idx = np.zeros(T, dtype=np.int64)
    idx[T - 1] = int(np.argmin(best))
    for t in range(T - 1, 0, -1):
        idx[t - 1] = bp[t, idx[t]]
    return idx


def delta(x):
    """The MFCC's +-2-frame rule with clamped edges, sum_i i x[t + i] / 10, written as differences so that a constant column gives
    exactly 0: ((x[t+1] - x[t-1]) + 2 (x[t+2] - x[t-2])) / 10."""
    x = np.asarray(x, dtype=np.float64)
    T = len(x)
    t = np.arange(T)

    def at(i):
        return x[np.clip(t + i, 0, T - 1)]
    return ((at(1) - at(-1)) + 2.0 * (at(2) - at(-2))) / 10.0


def refine(raw, idx, lmin):
    """P5's fractional lag: (T,) float64."""
    raw = np.asarray(raw, dtype=np.float64)
    T, L = raw.shape
    out = np.empty(T)
    for t in range(T):
        li = int(idx[t])
        shift = 0.0
        if 0 < li < L - 1:
            ym, y0, yp = raw[t, li - 1], raw[t, li], raw[t, li + 1]
            den = (ym - 2.0 * y0) + yp
            if den < 0.0:
                shift = min(0.5, max(-0.5, 0.5 * (ym - yp) / den))
        out[t] = float(lmin + li) + shift
    return out


def outputs(raw, idx, rate, lmin):
    """P5: (T, 3) = [v, ln f0, delta ln f0]."""
    raw = np.asarray(raw, dtype=np.float64)
    v = raw[np.arange(len(idx)), idx]
    lnf0 = np.log(float(rate) / refine(raw, idx, lmin))
    return np.stack([v, lnf0, delta(lnf0)], axis=1)


def pitch(x, rate, sampletime=0.025, overlap=0.5, f_min=50.0, f_max=400.0, ballast=BALLAST, soft_min_f0=SOFT_MIN_F0, pf=PF):
    """dict(out (T, 3), lag (T,) in samples, bal, raw (T, L)) of one signal."""
    _, _, lmin, lmax = geometry(rate, sampletime, overlap, f_min, f_max)
    bal, raw = nccf(x, rate, sampletime, overlap, f_min, f_max, ballast)
    idx = track(bal, rate, lmin, log_lags(lmin, lmax), soft_min_f0, pf)
    return dict(out=outputs(raw, idx, rate, lmin), lag=idx + lmin, bal=bal, raw=raw)
