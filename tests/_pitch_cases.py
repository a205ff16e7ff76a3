"""Inputs and twin expectations of the pitch edge tests (tests/test_gpu_pitch_edges.py on the device, tests/test_pitch_cases.py on the
CPU): the smallest calls that put each kernel of poccala_amd/csrc/pitch.hip on a line no other test reaches.  Everything is NumPy and
tests/_pitch_twin.py, from fixed seeds.

A case is a dict: name, rate, sigs (list of 1-d arrays: int16 travels as int16, float64 as float64), kw (the keyword arguments of
pitch_batch beside the signals and the rate: geometry, lag range, ballast, soft_min_f0, pf), nccf (None, or (bal_list, raw_list) for
PCL_PITCH_NCCF_IN: `sigs` then only give the lengths).  `expect(case)` is the twin's answer per utterance: dict(out, lag, bal, raw).
Cases are built once per process (functools.lru_cache) and never changed by a test.

No case holds a non-finite sample: rule P1-P5 does not define them."""
import functools

import numpy as np

import _pitch_twin as pt

GEOM_KEYS = ('sampletime', 'overlap', 'f_min', 'f_max')
TWIN_KEYS = GEOM_KEYS + ('ballast', 'soft_min_f0', 'pf')
LDS_LIMIT = 65536                  # frontend_host.h PITCH_LDS_LIMIT; the window needs (size + Lmax + 64) * 8 bytes (pitch_lds_bytes)
L65 = dict(f_min=95.0)             # 8 kHz: lags 20 .. 84, one wave and one lane


# ------------------------------------------------------------------ the twin on a case
def geometry(case):
    """(size, step, lmin, lmax) of the case's call"""
    return pt.geometry(case['rate'], **{k: case['kw'][k] for k in GEOM_KEYS if k in case['kw']})


def lags(case):
    _, _, lmin, lmax = geometry(case)
    return lmax - lmin + 1


def lds_bytes(case):
    size, _, _, lmax = geometry(case)
    return (size + lmax + 64) * 8


def frames(case):
    size, step, _, _ = geometry(case)
    return [pt.frame_count(len(x), size, step) for x in case['sigs']]


def row_off(case):
    return np.concatenate([[0], np.cumsum(frames(case))])


def track_kw(case):
    return {k: case['kw'][k] for k in ('soft_min_f0', 'pf') if k in case['kw']}


_EXPECT = {}


def expect(case):
    """the twin's dict(out, lag, bal, raw) of every utterance, computed once per case"""
    if case['name'] not in _EXPECT:
        rate = case['rate']
        _, _, lmin, lmax = geometry(case)
        res = []
        with np.errstate(all='ignore'):                  # (the overflow case: e0 * el = inf is what it is there for)
            if case['nccf'] is None:
                res = [pt.pitch(x, rate, **{k: v for k, v in case['kw'].items() if k in TWIN_KEYS}) for x in case['sigs']]
            else:
                g = pt.log_lags(lmin, lmax)
                for bal, raw in zip(*case['nccf']):
                    idx = pt.track(bal, rate, lmin, g, **track_kw(case))
                    res.append(dict(out=pt.outputs(raw, idx, rate, lmin), lag=idx + lmin, bal=bal, raw=raw))
        _EXPECT[case['name']] = res
    return _EXPECT[case['name']]


# ------------------------------------------------------------------ signals
def voiced(rate, n, f_lo=120.0, f_hi=180.0, seed=1, noise=200.0, amp=6000.0):
    """int16: three harmonics of a pitch that glides from f_lo to f_hi over n samples, on a noise floor"""
    f = np.linspace(f_lo, f_hi, n)
    ph = 2 * np.pi * np.cumsum(f) / rate
    s = sum((amp / k) * np.sin(k * ph) for k in range(1, 4)) + noise * np.random.default_rng(seed).standard_normal(n)
    return np.round(s).astype(np.int16)


def samples_of(T, size, step, short=0):
    """a length that gives T frames: the last frame starts `short` samples before the signal ends being a whole frame (0 <= short < step
    for T > 1: step does not divide n - size unless short = 0)"""
    return size + (T - 1) * step - short


def case(name, rate, sigs, nccf=None, **kw):
    return dict(name=name, rate=rate, sigs=sigs, kw=kw, nccf=nccf)


# ------------------------------------------------------------------ the lag grid's ends
LAG_GRID = {2: (8000, 380.0, 400.0, 370.0, 410.0),      # L: rate, f_min, f_max, and the glide's range
            63: (8000, 97.5, 400.0, 120.0, 180.0),
            1023: (16000, 15.41, 1000.0, 200.0, 400.0),
            1024: (16000, 15.39, 1000.0, 200.0, 400.0)}


@functools.lru_cache(maxsize=None)
def lag_grid(L):
    """a short glide and a T = 1 utterance on a grid of exactly L lags"""
    rate, f_min, f_max, f_lo, f_hi = LAG_GRID[L]
    size, step, _, _ = pt.geometry(rate, f_min=f_min, f_max=f_max)
    x = voiced(rate, samples_of(9 if L < 1000 else 6, size, step, 31), f_lo, f_hi, seed=L)
    return case('lag-grid-%d' % L, rate, [x, x[40:40 + size - 17].copy()], f_min=f_min, f_max=f_max)


# ------------------------------------------------------------------ the LDS limit
@functools.lru_cache(maxsize=None)
def lds(extra=0):
    """16 kHz, lags 40 .. 320, a frame of 7808 (+ extra) samples: (size + 320 + 64) * 8 = 65536 (+ 8 * extra) bytes.  Three frames.
    sampletime is the middle of the interval that int(rate * sampletime) maps to the intended size."""
    rate, size = 16000, LDS_LIMIT // 8 - 64 - 320 + extra
    sampletime = (size + 0.5) / rate
    step = int(size * 0.5)
    return case('lds-%d' % (LDS_LIMIT + 8 * extra), rate, [voiced(rate, samples_of(3, size, step, 5), 90.0, 140.0, seed=3)], sampletime=sampletime)


# ------------------------------------------------------------------ frame geometry
@functools.lru_cache(maxsize=None)
def overlap_one():
    """step = size = 200; 4 frames whose last is partly padding, and a T = 1 utterance"""
    x = voiced(8000, samples_of(4, 200, 200, 37), seed=4)
    return case('overlap-1', 8000, [x, x[:150].copy()], overlap=1.0, **L65)


@functools.lru_cache(maxsize=None)
def odd_size():
    """size = 201, step = 100, n - size = 433"""
    return case('odd-size', 8000, [voiced(8000, 201 + 433, seed=5), voiced(8000, 201 + 100, seed=6)], sampletime=201.5 / 8000, **L65)


@functools.lru_cache(maxsize=None)
def ragged_tail(alone=False):
    """utterance 0: n = size + 3 step exactly, so its last frame's `size` samples are the signal's last and the whole lag tail
    w[size .. size + Lmax) is padding (zeros enter b, not a); every earlier frame has its tail inside the signal.  Unless `alone`,
    utterance 1 follows with full-scale samples, which a kernel without the k < n test would read as utterance 0's tail."""
    a = voiced(8000, samples_of(4, 200, 100), seed=7)
    full = np.where((np.arange(900) // 23) % 2 == 0, 32767, -32768).astype(np.int16)
    return case('ragged-tail' + ('-alone' if alone else ''), 8000, [a] if alone else [a, full], **L65)


# ------------------------------------------------------------------ more than 256 rows
STRADDLE_T = 60                    # the two long utterances


@functools.lru_cache(maxsize=None)
def straddle_frames():
    """T of every utterance: 44 short ones of 1 .. 20 frames, and two of STRADDLE_T frames put where the rows pass 256 and 512"""
    rng = np.random.default_rng(11)
    short = list(rng.permutation(20) + 1) + list(rng.permutation(20) + 1) + [1, 20, 7, 13]
    T, rows, marks = [], 0, [256 - 30, 512 - 32]
    for t in short:
        if marks and rows >= marks[0]:
            T.append(STRADDLE_T)
            rows += STRADDLE_T
            marks.pop(0)
        T.append(int(t))
        rows += int(t)
    assert not marks
    return tuple(T)


@functools.lru_cache(maxsize=None)
def straddle(given=False):
    """8 kHz, L = 65, every utterance its own pitch range so that ln f0 differs across every utterance boundary.  given: the same rows
    through PCL_PITCH_NCCF_IN with random correlations on a coarse grid."""
    rate = 8000
    size, step, lmin, lmax = pt.geometry(rate, **L65)
    rng = np.random.default_rng(12)
    sigs = []
    for u, T in enumerate(straddle_frames()):
        n = samples_of(T, size, step, int(rng.integers(0, step))) if T > 1 else int(rng.integers(30, size + 1))
        f = rng.uniform(100.0, 330.0)
        sigs.append(voiced(rate, n, f, f * rng.uniform(0.8, 1.25), seed=100 + u))
    if not given:
        return case('straddle', rate, sigs, **L65)
    L = lmax - lmin + 1
    bal = [np.round(rng.uniform(-1, 1, (T, L)), 1) for T in straddle_frames()]
    raw = [np.round(rng.uniform(-1, 1, (T, L)), 2) for T in straddle_frames()]
    return case('straddle-given', rate, [np.zeros(len(x), dtype=np.int16) for x in sigs], nccf=(bal, raw), **L65)


def straddling(c):
    """[(u, k)]: utterance u has at least two rows on each side of row 256 k"""
    off = row_off(c)
    return [(u, k) for u in range(len(c['sigs'])) for k in range(1, int(off[-1]) // 256 + 1) if off[u] + 2 <= 256 * k <= off[u + 1] - 2]


# ------------------------------------------------------------------ P2's branches
def _p2_sigs(scale=1.0, offset=0.0):
    s = voiced(8000, samples_of(6, 200, 100, 41), seed=8).astype(np.float64)
    return [scale * (0.37 * s + 0.123) + offset, scale * (0.37 * s[60:60 + 170] + 0.123) + offset]


@functools.lru_cache(maxsize=None)
def p2(which):
    if which == 'underflow':                             # e0 * el ~ 1e-340 rounds to 0 while p ~ 1e-170 does not
        return case('p2-underflow', 8000, _p2_sigs(1e-90), **L65)
    if which == 'overflow':                              # e0 * el ~ 1e338 is inf, p ~ 1e169 finite: p / sqrt(inf) = 0
        return case('p2-overflow', 8000, _p2_sigs(1e80), **L65)
    if which == 'ballast0-silence':                      # den + ballast == 0
        return case('p2-ballast0-silence', 8000, [np.zeros(650, dtype=np.int16), np.zeros(90, dtype=np.int16)], ballast=0.0, **L65)
    if which == 'ballast0':                              # nccf_bal IS nccf_raw
        return case('p2-ballast0', 8000, [voiced(8000, 659, seed=9), voiced(8000, 170, seed=10)], ballast=0.0, **L65)
    if which == 'int16-extremes':                        # every sample -32768 or 32767: a square wave of period 54
        n = np.arange(659)
        x = np.where((n // 27) % 2 == 0, 32767, -32768).astype(np.int16)
        return case('p2-int16-extremes', 8000, [x, x[5:5 + 170].copy()], **L65)
    if which == 'dc-offset':                             # the mean is ~ 3e7 on samples that are no integers: its partial sums round
        return case('p2-dc-offset', 8000, _p2_sigs(1.0, 3.0e7), **L65)
    raise KeyError(which)


P2_CASES = ('underflow', 'overflow', 'ballast0-silence', 'ballast0', 'int16-extremes', 'dc-offset')


def p2_terms(c, u):
    """(p, den, den + ballast) of utterance u as the twin sums them (pt.nccf's loop, kept beside it)"""
    size, step, lmin, lmax = geometry(c)
    w = pt.windows(c['sigs'][u], size, step, lmax)
    return nccf_terms(w, size, lmin, lmax, c['kw'].get('ballast', pt.BALLAST))


def nccf_terms(w, size, lmin, lmax, ballast):
    T, L = len(w), lmax - lmin + 1
    p, e0, el = np.zeros((T, L)), np.zeros((T, 1)), np.zeros((T, L))
    for i in range(size):
        a = w[:, i:i + 1]
        b = w[:, lmin + i:lmin + i + L]
        p = p + a * b
        e0 = e0 + a * a
        el = el + b * b
    with np.errstate(all='ignore'):
        den = e0 * el
        return p, den, den + ballast


def nccf_of_windows(w, size, lmin, lmax, ballast):
    """P2 on given windows: pt.nccf's (bal, raw) when w = pt.windows(...)"""
    p, den, db = nccf_terms(w, size, lmin, lmax, ballast)
    with np.errstate(all='ignore'):
        return np.where(db == 0.0, 0.0, p / np.sqrt(db)), np.where(den == 0.0, 0.0, p / np.sqrt(den))


# ------------------------------------------------------------------ P5's branches
P5_KINDS = ('end0', 'endL', 'flat', 'convex', 'clamp+', 'clamp-', 'exact+', 'free', 'free-at-1', 'free-at-L-2')


def _p5_frame(rng, L, kind):
    """(bal row, raw row): bal has one peak at the lag the track is to take, raw the neighbourhood that P5 is to read there"""
    li = {'end0': 0, 'endL': L - 1, 'free-at-1': 1, 'free-at-L-2': L - 2}.get(kind, int(rng.integers(2, L - 2)))
    bal = np.round(rng.uniform(0.0, 0.1, L), 2)
    bal[li] = 0.9
    raw = np.round(rng.uniform(-1, 1, L), 2)
    if kind == 'end0':                                   # (a kernel that wrapped to L - 1 would find a concave triple here)
        raw[0], raw[1], raw[L - 1] = 0.9, 0.3, 0.5
    elif kind == 'endL':
        raw[L - 1], raw[L - 2], raw[0] = 0.9, 0.3, 0.5
    elif kind == 'flat':                                 # second difference exactly 0
        raw[li - 1:li + 2] = 0.5
    elif kind == 'convex':
        raw[li - 1:li + 2] = 0.9, 0.1, 0.8
    elif kind == 'clamp+':                               # 0.5 (0 - 0.9) / -0.1 = 4.5
        raw[li - 1:li + 2] = 0.0, 0.5, 0.9
    elif kind == 'clamp-':
        raw[li - 1:li + 2] = 0.9, 0.5, 0.0
    elif kind == 'exact+':                               # 0.5 (0 - 1) / -1 = 0.5: on the clamp, not over it
        raw[li - 1:li + 2] = 0.0, 1.0, 1.0
    else:
        y0 = rng.uniform(0.5, 1.0)
        raw[li - 1:li + 2] = y0 - rng.uniform(0.05, 0.4), y0, y0 - rng.uniform(0.05, 0.4)
    return bal, raw


@functools.lru_cache(maxsize=None)
def p5():
    """8 kHz, L = 65 through PCL_PITCH_NCCF_IN, default soft_min_f0 and pf (a peak of 0.9 outweighs the largest jump, 0.1 ln(84 / 20)^2):
    one utterance of three rounds over P5_KINDS, one T = 1 utterance per end of the grid, one of a single interior kind each"""
    rate = 8000
    size, step, lmin, lmax = pt.geometry(rate, **L65)
    L = lmax - lmin + 1
    rng = np.random.default_rng(13)
    plan = [list(P5_KINDS) * 3, ['end0'], ['endL'], ['clamp+', 'clamp-'], ['free', 'flat', 'free']]
    rows = [[_p5_frame(rng, L, k) for k in kinds] for kinds in plan]
    bal = [np.stack([r[0] for r in utt]) for utt in rows]
    raw = [np.stack([r[1] for r in utt]) for utt in rows]
    sigs = [np.zeros(samples_of(len(k), size, step), dtype=np.int16) for k in plan]
    return case('p5', rate, sigs, nccf=(bal, raw), **L65)


def p5_branches(raw, idx):
    """how often each branch of P5 is taken on (T, L) raw at lag indices idx, by the twin's own arithmetic"""
    L = raw.shape[1]
    n = dict.fromkeys(('li == 0', 'li == L - 1', 'den >= 0', 'clamped +0.5', 'clamped -0.5', 'unclamped'), 0)
    for t, li in enumerate(idx):
        if li == 0 or li == L - 1:
            n['li == 0' if li == 0 else 'li == L - 1'] += 1
            continue
        ym, y0, yp = raw[t, li - 1], raw[t, li], raw[t, li + 1]
        den = (ym - 2.0 * y0) + yp
        if den >= 0.0:
            n['den >= 0'] += 1
            continue
        s = 0.5 * (ym - yp) / den
        n['clamped +0.5' if s > 0.5 else 'clamped -0.5' if s < -0.5 else 'unclamped'] += 1
    return n


# ------------------------------------------------------------------ the track over many frames
def _given(name, rate, lens, seed, bal_step=0.1, **kw):
    size, step, lmin, lmax = pt.geometry(rate, **{k: kw[k] for k in GEOM_KEYS if k in kw})
    L = lmax - lmin + 1
    rng = np.random.default_rng(seed)
    bal = [np.round(rng.uniform(-1, 1, (T, L)) / bal_step) * bal_step for T in lens]
    raw = [np.round(rng.uniform(-1, 1, (T, L)), 2) for T in lens]
    return case(name, rate, [np.zeros(samples_of(T, size, step), dtype=np.int16) for T in lens], nccf=(bal, raw), **kw)


@functools.lru_cache(maxsize=None)
def track(which):
    """correlations on a coarse grid (ties everywhere) through PCL_PITCH_NCCF_IN"""
    if which == 'T600-L65':
        return _given('track-T600-L65', 8000, [600], 21, **L65)
    if which == 'T300-L281':
        return _given('track-T300-L281', 16000, [300], 22)
    if which == 'mixed':                                 # one workgroup each; 257 is one frame past a multiple of 256
        return _given('track-mixed', 8000, [1, 2, 3, 257, 1], 23, **L65)
    if which == 'pf0':                                   # soft_min_f0 = 0 as well: the local cost is on the grid too, so columns hold ties
        return _given('track-pf0', 8000, [40, 1, 5, 2], 24, bal_step=0.5, pf=0.0, soft_min_f0=0.0, **L65)
    if which == 'negative-fac':                          # 1 - 200 l / 8000: 0.5 at lag 20, -1.1 at lag 84
        return _given('track-negative-fac', 8000, [30, 1, 4], 25, soft_min_f0=200.0, **L65)
    raise KeyError(which)


TRACK_CASES = ('T600-L65', 'T300-L281', 'mixed', 'pf0', 'negative-fac')


def fac(c):
    """P3's factor per lag"""
    _, _, lmin, lmax = geometry(c)
    return 1.0 - c['kw'].get('soft_min_f0', pt.SOFT_MIN_F0) * np.arange(lmin, lmax + 1, dtype=np.float64) / float(c['rate'])
