"""Device time of the pitch features (row f15, csrc/pitch.hip) beside the host route they stand in for.

    python tools/pitch_bench.py [--utts 256] [--seconds 3.0] [--rate 16000] [--repeats 5] [--host-utts 8] [--out FILE]

A corpus-shaped batch: --utts ragged utterances of int16 PCM, between a third of --seconds and --seconds long (a noise floor with a voiced
stretch of moving pitch).  Medians of --repeats runs through pcl_kernel_time (HIP events around the launches) after one uncounted run that
allocates:
  pitch_nccf   P1-P2, one workgroup per frame          (multiply-adds: frames x lags x frame size x 3)
  pitch_track  P3-P4, one workgroup per utterance      (candidates: frames x lags^2)
  pitch_out    P5
and the wall clock of the whole pcl_pitch_pcm16 call (upload, kernels, the (rows, 3) result down).  The host route on the first --host-utts
utterances, scaled to the batch by frames: the NCCF as ONE BLAS call per utterance (the windows' lag matrix against the frames, np.einsum
for the energies) -- faster than the twin's loop and not bit-equal to it, a fair host figure -- plus the twin's track (tests/_pitch_twin.py).
Not a gate."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def utterance(rng, n, rate):
    s = 60 * rng.standard_normal(n)
    a, b = int(0.25 * n), int(0.8 * n)
    f = np.linspace(rng.uniform(90, 160), rng.uniform(160, 300), b - a)
    ph = 2 * np.pi * np.cumsum(f) / rate
    s[a:b] += np.hanning(b - a) ** 0.5 * (3000 * np.sin(ph) + 1500 * np.sin(2 * ph + 0.4) + 700 * np.sin(5 * ph))
    return np.round(s).astype(np.int16)


def host_nccf(x, rate, ballast=7000.0):
    """P1-P2 with the twin's windows and the dot products as one matrix product per frame block"""
    import _pitch_twin as pt
    size, step, lmin, lmax = pt.geometry(rate)
    w = pt.windows(x, size, step, lmax)
    L = lmax - lmin + 1
    idx = lmin + np.arange(L)[:, None] + np.arange(size)[None, :]
    b = w[:, idx]                                       # (T, L, size)
    a = w[:, :size]
    p = np.matmul(b, a[:, :, None])[:, :, 0]            # BLAS
    e0 = np.einsum('ti,ti->t', a, a)[:, None]
    el = np.einsum('tli,tli->tl', b, b)
    den = e0 * el
    with np.errstate(all='ignore'):
        raw = np.where(den == 0, 0.0, p / np.sqrt(den))
        bal = p / np.sqrt(den + ballast)
    return bal, raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=3.0)
    ap.add_argument('--rate', type=int, default=16000)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-utts', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import _pitch_twin as pt
    from poccala_amd import Engine
    from poccala_amd.StatisticalModel.AudioProcessing import pitch_batch
    rng = np.random.default_rng(0)
    rate = a.rate
    sigs = [utterance(rng, int(rng.uniform(a.seconds / 3, a.seconds) * rate), rate) for _ in range(a.utts)]
    size, step, lmin, lmax = pt.geometry(rate)
    L = lmax - lmin + 1
    frames = sum(pt.frame_count(len(s), size, step) for s in sigs)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('pitch_bench: %d utterances, %d frames, %d samples, rate %d, frame %d / %d, lags %d .. %d (L = %d)' % (
        a.utts, frames, sum(len(s) for s in sigs), rate, size, step, lmin, lmax, L))
    eng = Engine(0)
    eng.enable_timing(True)
    groups = ('pitch_nccf', 'pitch_track', 'pitch_out')
    ms = {g: [] for g in groups}
    wall = []
    rows = None
    for r in range(a.repeats + 1):
        for g in groups:
            eng.kernel_time(g)
        eng.sync()
        t0 = time.perf_counter()
        rows = pitch_batch(sigs, rate, engine=eng)
        t1 = time.perf_counter()
        got = {g: eng.kernel_time(g)[0] for g in groups}
        if r:                                           # (the first run allocates)
            wall.append(1e3 * (t1 - t0))
            for g in groups:
                ms[g].append(got[g])
    med = {g: float(np.median(ms[g])) for g in groups}
    say('pitch_nccf   median of %d: %.3f ms  (%.2f T multiply-adds / s)' % (a.repeats, med['pitch_nccf'], frames * L * size * 3 / med['pitch_nccf'] / 1e9))
    say('pitch_track  median of %d: %.3f ms  (%.2f G candidates / s)' % (a.repeats, med['pitch_track'], frames * L * L / med['pitch_track'] / 1e6))
    say('pitch_out    median of %d: %.3f ms' % (a.repeats, med['pitch_out']))
    say('pcl_pitch_pcm16, whole call, wall clock: median %.2f ms, %.0f x real time' % (
        float(np.median(wall)), sum(len(s) for s in sigs) / rate / (np.median(wall) / 1e3)))
    eng.enable_timing(False)
    # the host route
    n_host = min(a.host_utts, len(sigs))
    host_frames = sum(pt.frame_count(len(s), size, step) for s in sigs[:n_host])
    t_n, t_t = [], []
    g = pt.log_lags(lmin, lmax)
    for r in range(a.repeats):
        t0 = time.perf_counter()
        cors = [host_nccf(s, rate) for s in sigs[:n_host]]
        t1 = time.perf_counter()
        for c in cors:
            pt.track(c[0], rate, lmin, g)
        t2 = time.perf_counter()
        t_n.append(1e3 * (t1 - t0))
        t_t.append(1e3 * (t2 - t1))
    scale = frames / host_frames
    say('host, %d utterances (%d frames): NCCF by BLAS median %.1f ms, track %.1f ms; scaled to the batch: %.0f ms + %.0f ms' % (
        n_host, host_frames, np.median(t_n), np.median(t_t), np.median(t_n) * scale, np.median(t_t) * scale))
    # the two routes differ in summation order only: the same lag on all but a few frames where two candidates are close
    lags = pitch_batch(sigs[:n_host], rate, details=True, engine=eng)[1]['lag']
    agree = np.mean(np.concatenate([pt.track(c[0], rate, lmin, g) + lmin == l for c, l in zip(cors, lags)]))
    say('frames on which the BLAS route and the device pick the same lag: %.4f' % agree)
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
