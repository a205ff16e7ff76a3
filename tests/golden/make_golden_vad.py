#!/usr/bin/env python3
"""Golden vectors for the voice-activity detector (row f6) by RUNNING the reference's AudioProcessing.VAD
(StatisticalModel/AudioProcessing.py:450-543).  Build container only.

    python tests/golden/make_golden_vad.py        # writes tests/golden/G19_vad.npz

Per case: the input matrix, mel_distance, osf, the kept row indices, the threshold and (simple_size, alpha, beta).
  speech39 / speech13   the reference's own MFCC of two synthetic signals: a noise lead-in, a voiced stretch, a noise tail
  t16 .. t40            random matrices at the edges of the filter's range (T = s, s+1, 2s-1, 2s, 2s+1, 40)
  s8                    simple_size = 8 with osf(beta=0.8): at the default beta h + 1 = 16 is outside the window of 16 and the reference raises
  piecewise             mel_distance(alpha=0.3) and osf(beta=0.8) called directly
Every committed case keeps |osf_t - thr| / thr >= 1e-6 on every frame (asserted here), so a test may demand the exact kept set.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402
from make_golden_mfcc import FakeWav  # noqa: E402

MIN_GAP = 1e-6


def speech_signal(rng, n, rate, lead, tail):
    """Noise, then a voiced stretch (harmonics with a slow amplitude envelope) on the same noise floor, then noise."""
    t = np.arange(n) / rate
    s = 60 * rng.standard_normal(n)
    a, b = int(lead * n), int((1 - tail) * n)
    env = np.zeros(n)
    env[a:b] = np.hanning(b - a) ** 0.5
    s += env * (3000 * np.sin(2 * np.pi * 180 * t) + 1800 * np.sin(2 * np.pi * 360 * t + 0.4) + 900 * np.sin(2 * np.pi * 1500 * t))
    s = np.round(s).astype(np.int16)
    s[s == 0] = 1                      # init_audio deletes zero samples; keep the fixture explicit
    return s


def run(AudioProcessing, x, s=16, alpha=None, beta=None):
    """The reference's three steps; alpha / beta None = its defaults through VAD.mfcc()'s own calls."""
    v = AudioProcessing.VAD(s)
    v.init_mfcc(x)
    dist = v.mel_distance() if alpha is None else v.mel_distance(alpha=alpha)
    sm = v.osf(dist) if beta is None else v.osf(dist, beta=beta)
    rows = v.detect(sm)
    a, b = (0.5 if alpha is None else alpha), (0.93 if beta is None else beta)
    # the threshold and the kept indices: detect() returns rows only, so restate its last three lines on ITS smoothed distances
    thr = sm[int(s / 2)] * (sm.max() - sm.min()) / sm.max()
    kept = np.nonzero(sm - thr > 0)[0]
    assert np.array_equal(x[kept], rows), 'kept indices do not reproduce detect()'
    if alpha is None and beta is None:
        assert np.array_equal(v.mfcc(), rows)
    gap = np.abs(sm - thr) / abs(thr)
    assert gap.min() >= MIN_GAP, 'a frame sits %.3g from the threshold' % gap.min()
    return dict(x=x, dist=dist, osf=sm, kept=kept.astype(np.int32), thr=np.float64(thr), params=np.array([s, a, b], dtype=np.float64)), gap.min()


def main():
    import_reference()
    from StatisticalModel.AudioProcessing import AudioProcessing
    rng = np.random.default_rng(1919)
    cases = {}
    for tag, n, rate, d1, d2 in (('speech39', 12000, 16000, True, True), ('speech13', 20000, 16000, False, False)):
        sig = speech_signal(rng, n, rate, 0.3, 0.25)
        m = AudioProcessing.MFCC(13)
        m._MFCC__wdata = sig
        m._MFCC__wav = FakeWav(rate, n)
        cases[tag] = run(AudioProcessing, m.mfcc(d1=d1, d2=d2))
    for T in (16, 17, 31, 32, 33, 40):
        x = rng.standard_normal((T, 13)) * np.linspace(0.5, 3.0, T)[:, None]
        cases['t%d' % T] = run(AudioProcessing, x)
    cases['s8'] = run(AudioProcessing, rng.standard_normal((29, 26)) * np.linspace(0.5, 3.0, 29)[:, None], s=8, beta=0.8)
    cases['piecewise'] = run(AudioProcessing, rng.standard_normal((60, 13)) * np.linspace(0.5, 3.0, 60)[:, None], alpha=0.3, beta=0.8)
    out = {'cases': np.array(sorted(cases))}
    for tag, (c, gap) in cases.items():
        print('%-10s T=%4d D=%2d kept=%4d thr=%.6g min gap=%.3g' % (tag, c['x'].shape[0], c['x'].shape[1], len(c['kept']), c['thr'], gap))
        for k, v in c.items():
            out['%s_%s' % (tag, k)] = v
    path = os.path.join(HERE, 'G19_vad.npz')
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 128 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
