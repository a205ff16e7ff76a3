"""The pitch twin (tests/_pitch_twin.py: the definition of rule P1-P5) against answers known in advance: synthetic tones whose period is
known, noise that has none, silence, the shortest utterances and the tie rule.  No GPU."""
import numpy as np
import pytest

import _pitch_twin as pt

# (rate, f0): every tone below is tracked within one lag on both signal shapes.  Left out on purpose: 390 Hz at 8 kHz (a period of 20.5
# samples falls between two lags and the harmonic signal goes an octave down), 55 and 60 Hz at 16 kHz (two lags short).
TONES = [(8000, f) for f in (100, 150.3, 220, 310)] + [(16000, f) for f in (100, 150.3, 220, 310, 390)]
KINDS = ('sine', 'harmonics8000', 'harmonics300')      # a sine of amplitude 8000; harmonics k = 1 .. 5 of amplitude 8000 / k, and of 300 / k


def tone(rate, f0, kind, seconds=0.4):
    t = np.arange(int(rate * seconds)) / rate
    if kind == 'sine':
        s = 8000 * np.sin(2 * np.pi * f0 * t)
    else:
        amp = float(kind[len('harmonics'):])
        s = sum((amp / k) * np.sin(2 * np.pi * k * f0 * t) for k in range(1, 6))
    return np.round(s).astype(np.int16)


_CACHE = {}


def tone_result(rate, f0, kind):
    """computed once, shared with tests/test_gpu_pitch.py, never changed"""
    key = (rate, f0, kind)
    if key not in _CACHE:
        _CACHE[key] = pt.pitch(tone(rate, f0, kind), rate)
    return _CACHE[key]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rate,f0', TONES)
def test_tones_are_tracked_within_one_lag_and_are_voiced(rate, f0, kind):
    r = tone_result(rate, f0, kind)
    lag, v = r['lag'][:-3], r['out'][:-3, 0]             # the last three frames run into the zero padding
    print(rate, f0, kind, 'lags', lag.min(), lag.max(), 'period', rate / f0, 'min v', v.min())
    assert np.all(np.abs(lag - rate / f0) <= 1.0)
    assert np.all(v >= 0.98)
    # ln f0 follows the refined lag: within the grid's resolution of the true pitch
    assert np.all(np.abs(r['out'][:-3, 1] - np.log(f0)) <= np.log1p(1.0 / (rate / f0 - 1.0)))


@pytest.mark.parametrize('rate', [8000, 16000])
def test_white_noise_is_unvoiced(rate):
    x = np.round(1000 * np.random.default_rng(rate).standard_normal(int(0.4 * rate))).astype(np.int16)
    r = pt.pitch(x, rate)
    print(rate, 'max |v|', np.abs(r['out'][:, 0]).max())
    assert np.abs(r['out'][:, 0]).max() < 0.3


def test_silence_is_lag_min_unvoiced_and_flat():
    rate = 8000
    size, step, lmin, lmax = pt.geometry(rate)
    r = pt.pitch(np.zeros(1500), rate)
    assert len(r['lag']) == pt.frame_count(1500, size, step) > 3
    assert np.all(r['lag'] == lmin) and np.all(r['out'][:, 0] == 0.0) and np.all(r['out'][:, 2] == 0.0)
    assert np.all(r['out'][:, 1] == np.log(rate / float(lmin)))
    assert np.all(r['bal'] == 0.0) and np.all(r['raw'] == 0.0)


@pytest.mark.parametrize('n,T', [(37, 1), (200, 1), (201, 2), (300, 2), (301, 3)])
def test_the_shortest_utterances(n, T):
    rate = 8000
    size, step, lmin, lmax = pt.geometry(rate)
    assert (size, step) == (200, 100)
    x = np.round(3000 * np.sin(2 * np.pi * 140 * np.arange(n) / rate)).astype(np.int16)
    r = pt.pitch(x, rate)
    assert r['out'].shape == (T, 3) and r['bal'].shape == (T, lmax - lmin + 1)
    assert np.isfinite(r['out']).all()
    if T == 1:                                           # no track: the frame's own cheapest lag, and a delta over one row is 0
        c = 1.0 - r['bal'][0] * (1.0 - pt.SOFT_MIN_F0 * np.arange(lmin, lmax + 1) / rate)
        assert r['lag'][0] == lmin + int(np.argmin(c)) and r['out'][0, 2] == 0.0
    if T == 2:                                           # both rows clamp to the same pair: (-2 x0 - x0 + x1 + 2 x1) / 10
        x0, x1 = r['out'][:, 1]
        assert r['out'][0, 2] == r['out'][1, 2] == ((x1 - x0) + 2.0 * (x1 - x0)) / 10.0


def test_ties_go_to_the_smallest_lag():
    rate, lmin, L = 8000, 20, 141
    g = pt.log_lags(lmin, lmin + L - 1)
    for T in (1, 2, 7):
        # soft_min_f0 = 0 makes the local cost the same at every lag: every minimum is a tie
        assert np.all(pt.track(np.full((T, L), 0.25), rate, lmin, g, soft_min_f0=0.0) == 0)
    # two equal peaks in every frame: the one at the smaller lag is taken, in the last frame and through the back-pointers
    bal = np.zeros((6, L))
    bal[:, 30] = bal[:, 90] = 0.5
    assert np.all(pt.track(bal, rate, lmin, g, soft_min_f0=0.0) == 30)


def test_delta_is_the_mfcc_rule():
    x = np.array([1.0, 4.0, 9.0, 16.0, 25.0, 36.0])
    want = [(-2 * 1 - 1 + 4 + 2 * 9) / 10, (-2 * 1 - 1 + 9 + 2 * 16) / 10, (-2 * 1 - 4 + 16 + 2 * 25) / 10, (-2 * 4 - 9 + 25 + 2 * 36) / 10,
            (-2 * 9 - 16 + 36 + 2 * 36) / 10, (-2 * 16 - 25 + 36 + 2 * 36) / 10]
    assert np.allclose(pt.delta(x), want, rtol=1e-15)
    assert pt.delta(np.array([3.5]))[0] == 0.0


def test_parabola_refinement():
    raw = np.array([[0.1, 0.5, 0.9, 0.7, 0.2],           # peak between 2 and 3
                    [0.9, 0.5, 0.1, 0.0, 0.0],           # the track sits at the grid's end: no refinement
                    [0.5, 0.5, 0.5, 0.5, 0.5],           # flat: second difference 0, no refinement
                    [0.0, 0.0, 1.0, 0.999999, 0.0]])     # the vertex is clamped to half a lag
    l = pt.refine(raw, np.array([2, 0, 2, 2]), 40)
    assert l[0] == 42 + 0.5 * (0.5 - 0.7) / ((0.5 - 2.0 * 0.9) + 0.7) and 42 < l[0] < 42.5
    assert l[1] == 40 and l[2] == 42 and 42.49 < l[3] <= 42.5
