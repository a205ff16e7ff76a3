#!/usr/bin/env python3
"""Front-end on the device against the route through the host: PCM -> frames resident on the GPU, ready for a batch.

  fused   Engine.frontend on float64 samples: MFCC, voice-activity detector and compaction without the features leaving the device
  int16   the same call on the same samples as np.int16 arrays (cast once, outside the timed region): int16 on the wire through the
          context's page-locked staging, converted in the MFCC kernel -- the same frames, bit for bit
  host    the route available before the detector ran on the device: mfcc_batch to the host, the NumPy restatement of the
          detector (tests/_vad_twin.py), load_frames of the survivors

Shapes: 1024 signals of 300 frames at 16 kHz, D = 39 (the shape tools/mfcc_bench.py times), and one ragged batch.  The three routes run in
the same process after a warm-up of each, alternating (int16, fused, host, int16, fused, host, ...) so that a drift of the machine reaches
all alike; each figure is the median of `--reps` calls (minimum and maximum beside it).  Kernel times are HIP-event times from
pcl_kernel_time, summed per group over one call; so is "H2D" of the int16 route (its chunks' copies on the staging stream, which overlap
the staging memcpy: the two do not add up); "staging memcpy" and the float64 route's one blocking copy are host-clock times taken inside
the library.

    python tools/frontend_bench.py [--reps 5] [--out FILE]        # writes profiles/r09_frontend_pcm16.txt unless told otherwise
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
TRANSFER = ('pcm_stage', 'pcm_h2d')


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


def report(lines, title, walls, kern, wire_bytes):
    lines.append('  %-22s %8.2f ms (%.2f .. %.2f), %.0f MB of samples on the wire' % ((title,) + stats(walls) + (wire_bytes / 1e6,)))
    if stats(kern['pcm_stage'])[0] > 0:
        lines.append('    staging memcpy       %8.3f ms (%.3f .. %.3f)' % stats(kern['pcm_stage']))
    lines.append('    H2D of the samples   %8.3f ms (%.3f .. %.3f)' % stats(kern['pcm_h2d']))
    for g in GROUPS:
        lines.append('    kernels %-11s  %8.3f ms (%.3f .. %.3f)' % ((g,) + stats(kern[g])))
    k = sum(stats(kern[g])[0] for g in GROUPS)
    # the staging memcpy and the chunks' copies overlap: the longer of the two is what the transfer costs the wall clock
    moved = max(stats(kern['pcm_stage'])[0], stats(kern['pcm_h2d'])[0])
    lines.append('    kernels together %.3f ms, transfer %.3f ms, everything else (concatenation, tables, descriptors, allocation, Python) %.2f ms'
                 % (k, moved, stats(walls)[0] - k - moved))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r09_frontend_pcm16.txt'))
    a = ap.parse_args()
    eng = Engine(0)
    eng.enable_timing(True)
    lines = ['# tools/frontend_bench.py: %s, %d CUs; fused = Engine.frontend on float64 samples, int16 = on the same samples as int16, host = mfcc_batch -> NumPy detector -> load_frames'
             % (eng.device_info()['name'], eng.device_info()['cus']),
             '# wall times: median (min .. max) of the repetitions, the three routes alternating after one warm-up call of each, same process; kernel and H2D times: HIP events; staging memcpy: host clock']
    rng = np.random.default_rng(0)
    for tag, sigs in (('1024 x 300 frames', signals(1024, 300, rng)), ('ragged 777 x 40..600 frames', signals(777, 600, rng, ragged=True))):
        sigs16 = [s.astype(np.int16) for s in sigs]            # the same samples (rounded, |s| < 32768), cast once outside the timed region
        assert all(np.array_equal(a16, s) for a16, s in zip(sigs16, sigs))
        fused(eng, sigs16)                                     # warm-up of the three routes: pool, staging, code objects, page tables
        fused(eng, sigs)
        host_route(eng, sigs)
        for g in GROUPS + TRANSFER:
            eng.kernel_time(g)
        new = lambda: {g: [] for g in GROUPS + TRANSFER}       # noqa: E731
        walls16, walls, kern16, kern, hw, parts = [], [], new(), new(), [], []
        for _ in range(a.reps):                                # the three routes alternate
            w, lens16 = fused(eng, sigs16)
            walls16.append(w * 1e3)
            for g in GROUPS + TRANSFER:
                kern16[g].append(eng.kernel_time(g)[0])
            w, lens = fused(eng, sigs)
            walls.append(w * 1e3)
            for g in GROUPS + TRANSFER:
                kern[g].append(eng.kernel_time(g)[0])
            w, p, hl = host_route(eng, sigs)
            hw.append(w * 1e3)
            parts.append(p)
            for g in ('mfcc',) + TRANSFER:                     # (the host route's MFCC launch is not the fused call's)
                eng.kernel_time(g)
        cat16, cat64 = [], []                                  # what Engine.frontend does on the host before it calls the library
        for _ in range(a.reps):
            t0 = time.perf_counter()
            np.concatenate(sigs16)
            t1 = time.perf_counter()
            np.concatenate(sigs)
            cat16.append((t1 - t0) * 1e3)
            cat64.append((time.perf_counter() - t1) * 1e3)
        total = int(sum(1 + (len(s) - 400 + 199) // 200 for s in sigs))
        n_samples = int(sum(len(s) for s in sigs))
        assert np.array_equal(lens16, lens), 'the int16 and the float64 call kept different frames'
        assert np.array_equal(hl, lens), 'the two routes kept different frames'
        lines.append('%s: %d MFCC frames, %d kept, %d samples' % (tag, total, int(lens.sum()), n_samples))
        report(lines, 'int16 fused call wall', walls16, kern16, 2 * n_samples)
        report(lines, 'fused call wall', walls, kern, 8 * n_samples)
        lines.append('  int16 / float64 fused  %8.3f  (%.2fx faster); mfcc kernels int16 / float64 %.3f'
                     % (stats(walls16)[0] / stats(walls)[0], stats(walls)[0] / stats(walls16)[0], stats(kern16['mfcc'])[0] / max(stats(kern['mfcc'])[0], 1e-9)))
        lines.append('  np.concatenate of the signals alone: int16 %.2f ms (%.2f .. %.2f), float64 %.2f ms (%.2f .. %.2f)' % (stats(cat16) + stats(cat64)))
        lines.append('  host route wall        %8.2f ms (%.2f .. %.2f): mfcc_batch %.1f + NumPy detector %.1f + load_frames %.1f ms'
                     % (stats(hw) + tuple(1e3 * float(np.median([p[k] for p in parts])) for k in range(3))))
        lines.append('  fused / host           %8.3f    int16 fused / host %8.3f' % (stats(walls)[0] / stats(hw)[0], stats(walls16)[0] / stats(hw)[0]))
    eng.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
