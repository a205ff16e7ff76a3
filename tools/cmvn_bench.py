"""Device time of CMVN on resident frames (row f14, csrc/frame_cmvn.hip) beside the host route it replaces.

    python tools/cmvn_bench.py [--utts 1024] [--frames 300] [--dim 39] [--speakers 64] [--long 1000000] [--window 600] [--repeats 5] [--out FILE]

Random frames, config 4's shard shape (1024 x 300 frames, D = 39) with 64 speakers, once as float64 frames (the context holds the float64
copy and the float32 rows) and once as float32 frames; then ONE utterance of --long frames for the sliding form.  Medians of --repeats
runs through pcl_kernel_time (HIP events around the launches) after one uncounted run that allocates:
  cmvn_stats    the chunk partials and the per-speaker sums          (bytes: every element of the listed rows read once)
  cmvn_apply    statuses, m and sqrt(v), the elementwise apply       (bytes: every element read once; written once to each copy held)
  cmvn_sliding  the blocked prefix and the apply from window sums    (bytes: the apply's, plus the rows read once more and the prefix block
                                                                     -- 16 bytes per element -- written once and read once)
Bytes count the row stride (the padding columns travel with the rows).  The figure to hold a first run against: the apply near the fill
bandwidth DESIGN section 7 (f7) records, ~4.8 TB/s; not a gate.  The host route on the same frames: Engine.frames_download + NumPy +
Engine.load_frames, wall clock, median of --repeats."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stride(D):
    for o in (13, 26, 39, 47, 48, 64):
        if D <= o:
            return o
    raise ValueError(D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--dim', type=int, default=39)
    ap.add_argument('--speakers', type=int, default=64)
    ap.add_argument('--long', type=int, default=1000000)
    ap.add_argument('--window', type=int, default=600)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from poccala_amd import Engine
    U, T, D, S = a.utts, a.frames, a.dim, a.speakers
    F, FD = U * T, stride(a.dim)
    rng = np.random.default_rng(0)
    eng = Engine(0)
    eng.enable_timing(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(group, call, reload):
        ms = []
        for r in range(a.repeats + 1):
            reload()
            eng.kernel_time(group)
            call()
            ms.append(eng.kernel_time(group)[0])
        return float(np.median(ms[1:]))

    def rate(nbytes, ms):
        return '%8.3f ms = %6.3f TB/s' % (ms, nbytes / (ms * 1e-3) / 1e12)

    say('# tools/cmvn_bench.py: %d x %d frames, D = %d (row stride %d), %d speakers, median of %d (%s)'
        % (U, T, D, FD, S, a.repeats, eng.device_info()['name']))
    lens, begin = np.full(U, T, dtype=np.int32), np.arange(U, dtype=np.int64) * T
    spk = (np.arange(U) % S).astype(np.int32)
    for dtype in (np.float64, np.float32):
        frames = (rng.standard_normal((F, D)) * 2 + 1).astype(dtype)
        held = 12 if dtype == np.float64 else 4                     # bytes per element of the copies the context holds
        read = 8 if dtype == np.float64 else 4

        def reload():
            eng._frames_key = None
            eng.load_frames(frames)
            eng.cmvn_zero(S)

        def reload_with_stats():
            reload()
            eng.cmvn_accumulate(lens, begin, spk)

        name = np.dtype(dtype).name
        say('%s frames  cmvn_stats    %s' % (name, rate(F * FD * read, timed('cmvn_stats', lambda: eng.cmvn_accumulate(lens, begin, spk), reload))))
        say('%s frames  cmvn_apply    %s' % (name, rate(F * FD * (read + held), timed('cmvn_apply', lambda: eng.cmvn_apply(lens, begin, spk), reload_with_stats))))
        say('%s frames  cmvn_sliding  %s  (window %d, causal, mean and variance)'
            % (name, rate(F * FD * (2 * read + held) + F * D * 32, timed('cmvn_sliding', lambda: eng.cmvn_sliding(lens, begin, a.window, 100, False, True), reload)), a.window))
        host = []
        for r in range(a.repeats):
            reload()
            t0 = time.perf_counter()
            x = eng.frames_download(dtype).astype(np.float64)
            for s in range(S):
                rows = np.concatenate([np.arange(begin[u], begin[u] + lens[u]) for u in np.flatnonzero(spk == s)])
                m = x[rows].mean(axis=0)
                v = np.maximum((x[rows] * x[rows]).mean(axis=0) - m * m, 1e-20)
                x[rows] = (x[rows] - m) / np.sqrt(v)
            eng._frames_key = None
            eng.load_frames(x.astype(dtype))
            host.append((time.perf_counter() - t0) * 1e3)
        say('%s frames  host route (frames_download + NumPy + load_frames) %8.3f ms' % (name, float(np.median(host))))
    # one long utterance, the sliding form
    L = a.long
    frames = (rng.standard_normal((L, D)) * 2 + 1)
    lens, begin = np.array([L], dtype=np.int32), np.zeros(1, dtype=np.int64)

    def reload_long():
        eng._frames_key = None
        eng.load_frames(frames)

    for center in (False, True):
        ms = timed('cmvn_sliding', lambda: eng.cmvn_sliding(lens, begin, a.window, 100, center, True), reload_long)
        say('float64 frames  one utterance of %d frames, window %d, %s  cmvn_sliding %s'
            % (L, a.window, 'centred' if center else 'causal', rate(L * FD * 28 + L * D * 32, ms)))
    eng.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
