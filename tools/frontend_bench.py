#!/usr/bin/env python3
"""Front-end on the device against the route through the host: PCM -> frames resident on the GPU, ready for a batch.

  fused   Engine.frontend: MFCC, voice-activity detector and compaction without the features leaving the device
  host    the route available before the detector ran on the device: mfcc_batch to the host, the NumPy restatement of the
          detector (tests/_vad_twin.py), load_frames of the survivors

Shapes: 1024 signals of 300 frames at 16 kHz, D = 39 (the shape tools/mfcc_bench.py times), and one ragged batch.  Both routes run in the
same process after a warm-up of each, alternating (fused, host, fused, host, ...) so that a drift of the machine reaches both alike; each
figure is the median of `--reps` calls (minimum and maximum beside it).  Kernel times are HIP-event
times from pcl_kernel_time, summed per group over one call.

    python tools/frontend_bench.py [--reps 5] [--out FILE]        # writes profiles/r08_frontend.txt unless told otherwise
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402

import _vad_twin as vt  # noqa: E402
from poccala_amd import Engine  # noqa: E402
from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch  # noqa: E402

GROUPS = ('mfcc', 'vad_dist', 'vad_osf', 'vad_select', 'vad_gather')


def signals(U, frames, rng, ragged=False):
    out = []
    for _ in range(U):
        f = int(rng.integers(40, frames + 1)) if ragged else frames
        n = 400 + (f - 1) * 200
        t = np.arange(n) / 16000.0
        env = np.zeros(n)
        a, b = int(0.3 * n), int(0.75 * n)
        env[a:b] = np.hanning(b - a) ** 0.5
        out.append(np.round(60 * rng.standard_normal(n) + env * (3000 * np.sin(2 * np.pi * 180 * t) + 1500 * np.sin(2 * np.pi * 1500 * t))))
    return out


def stats(xs):
    return float(np.median(xs)), min(xs), max(xs)


def fused(eng, sigs):
    t0 = time.perf_counter()
    lens, begin = eng.frontend(sigs, 16000)
    eng.sync()
    return time.perf_counter() - t0, lens


def host_route(eng, sigs):
    t0 = time.perf_counter()
    mats = mfcc_batch(sigs, 16000, d1=True, d2=True, engine=eng)
    t1 = time.perf_counter()
    lens, begin, rows = vt.vad_batch(mats)
    t2 = time.perf_counter()
    eng.load_frames(np.float32(rows))
    eng.sync()
    t3 = time.perf_counter()
    return t3 - t0, (t1 - t0, t2 - t1, t3 - t2), lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r08_frontend.txt'))
    a = ap.parse_args()
    eng = Engine(0)
    eng.enable_timing(True)
    lines = ['# tools/frontend_bench.py: %s, %d CUs; fused = Engine.frontend, host = mfcc_batch -> NumPy detector -> load_frames'
             % (eng.device_info()['name'], eng.device_info()['cus']),
             '# wall times: median (min .. max) of the repetitions, the two routes alternating after one warm-up call of each, same process; kernel times: HIP events']
    rng = np.random.default_rng(0)
    for tag, sigs in (('1024 x 300 frames', signals(1024, 300, rng)), ('ragged 777 x 40..600 frames', signals(777, 600, rng, ragged=True))):
        fused(eng, sigs)                                       # warm-up of both routes: pool, code objects, page tables
        host_route(eng, sigs)
        for g in GROUPS:
            eng.kernel_time(g)
        walls, kern, hw, parts = [], {g: [] for g in GROUPS}, [], []
        for _ in range(a.reps):                                # the two routes alternate
            w, lens = fused(eng, sigs)
            walls.append(w * 1e3)
            for g in GROUPS:
                kern[g].append(eng.kernel_time(g)[0])
            w, p, hl = host_route(eng, sigs)
            hw.append(w * 1e3)
            parts.append(p)
            eng.kernel_time('mfcc')                            # (the host route's MFCC launch is not the fused call's)
        total = int(sum(1 + (len(s) - 400 + 199) // 200 for s in sigs))
        lines.append('%s: %d MFCC frames, %d kept' % (tag, total, int(lens.sum())))
        lines.append('  fused call wall        %8.2f ms (%.2f .. %.2f)' % stats(walls))
        for g in GROUPS:
            lines.append('    kernels %-11s  %8.3f ms (%.3f .. %.3f)' % ((g,) + stats(kern[g])))
        vad_ms = sum(stats(kern[g])[0] for g in GROUPS[1:])
        lines.append('    detector kernels together %.3f ms = %.1f %% of the MFCC kernels' % (vad_ms, 100 * vad_ms / max(stats(kern['mfcc'])[0], 1e-9)))
        assert np.array_equal(hl, lens), 'the two routes kept different frames'
        lines.append('  host route wall        %8.2f ms (%.2f .. %.2f): mfcc_batch %.1f + NumPy detector %.1f + load_frames %.1f ms'
                     % (stats(hw) + tuple(1e3 * float(np.median([p[k] for p in parts])) for k in range(3))))
        lines.append('  fused / host           %8.3f' % (stats(walls)[0] / stats(hw)[0]))
    eng.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
