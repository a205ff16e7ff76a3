"""Wall time of the two model-free initialisers at BASELINE config 4's model shape, device route against host route.

    python tools/bootstrap_bench.py [--states 3000] [--mix 2048] [--dim 39] [--utts 1024] [--frames 300] [--repeats 5] [--out FILE]

Medians of --repeats runs, one line per figure (also written to --out; profiles/r09_bootstrap.txt is such a file):
  flat start, device   Engine.flat_start: moments of the resident frames -> pcl_model_flat_start's fill -> derive pass
                       (split by pcl_kernel_time: "moments", "flat_fill", "derive")
  flat start, host     what the library offered before: NumPy moments of the host frames, np.repeat to (J, M, D) on the host,
                       Engine.load_model (pcl_model_upload: pad, copy over PCIe, derive)
  uniform map, device  Engine.uniform_segments (map + counting sort + gather on the device)
  uniform map, host    the NumPy twin of the map (tests/_bootstrap_twin.py) + Engine.segments (map uploaded, same sort + gather)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--states', type=int, default=3000)
    ap.add_argument('--mix', type=int, default=2048)
    ap.add_argument('--dim', type=int, default=39)
    ap.add_argument('--utts', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--labels', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import _bootstrap_twin as tw
    from poccala_amd import Engine
    J, M, D, U, T = a.states, a.mix, a.dim, a.utts, a.frames
    rng = np.random.default_rng(0)
    frames = (rng.standard_normal((U * T, D), dtype=np.float32) * 2 + 1).astype(np.float32)
    lens, begin = np.full(U, T, dtype=np.int32), np.arange(U, dtype=np.int64) * T
    coeff = (rng.random(M) - rng.random(M)) * 0.1
    n_utts = int(U * 0.25)
    eng = Engine(0)
    eng.load_frames(frames)
    eng.enable_timing(True)
    lines = ['# tools/bootstrap_bench.py: J = %d, M = %d, D = %d, %d x %d frames, median of %d (%s)' % (J, M, D, U, T, a.repeats, eng.device_info()['name'])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev, parts = [], dict(moments=[], flat_fill=[], derive=[])
    for r in range(a.repeats + 1):                                   # the first run allocates: not counted
        for k in parts:
            eng.kernel_time(k)
        eng.sync()
        t0 = time.perf_counter()
        eng.flat_start(lens, begin, J, M, n_utts=n_utts, step=1, coeff=coeff)
        eng.sync()
        dt = time.perf_counter() - t0
        if r:
            dev.append(dt)
            for k in parts:
                parts[k].append(eng.kernel_time(k)[0])
        print('device flat start run %d: %.1f ms' % (r, dt * 1e3), flush=True)
    med = lambda v: float(np.median(v))
    say('flat start, device route (Engine.flat_start):            %9.1f ms   kernels: moments %.2f ms, fill %.2f ms, derive %.2f ms (%.0f %% of the call)'
        % (med(dev) * 1e3, med(parts['moments']), med(parts['flat_fill']), med(parts['derive']), 100 * med(parts['derive']) / (med(dev) * 1e3)))
    gb = 2 * J * ((M + 3) // 4 * 4) * D * 8 / 1e9
    say('   the fill writes %.2f GB: %.0f GB/s' % (gb, gb / (med(parts['flat_fill']) * 1e-3)))
    host, hparts = [], dict(moments=[], repeat=[], upload=[])
    for r in range(a.repeats):
        t0 = time.perf_counter()
        x = frames[tw.sample_rows(lens, begin, n_utts, 1)].astype(np.float64)
        mean = x.mean(0)
        var = np.sqrt(np.maximum(((x - mean) ** 2).mean(0), 1e-4)) ** 2
        t1 = time.perf_counter()
        g_mean = (mean[None, :].repeat(M, axis=0) + coeff[:, None] * var)[None].repeat(J, axis=0)
        g_var = var[None, None, :].repeat(M, axis=1).repeat(J, axis=0)
        w = np.full((J, M), 1.0 / M)
        t2 = time.perf_counter()
        eng._model_key = None
        eng.load_model(g_mean, g_var, w)
        eng.sync()
        t3 = time.perf_counter()
        del g_mean, g_var
        host.append(t3 - t0)
        hparts['moments'].append(t1 - t0)
        hparts['repeat'].append(t2 - t1)
        hparts['upload'].append(t3 - t2)
        print('host flat start run %d: %.1f ms' % (r, (t3 - t0) * 1e3), flush=True)
    say('flat start, host route (NumPy + Engine.load_model):      %9.1f ms   NumPy moments %.1f ms, np.repeat %.1f ms, load_model %.1f ms'
        % (med(host) * 1e3, med(hparts['moments']) * 1e3, med(hparts['repeat']) * 1e3, med(hparts['upload']) * 1e3))
    say('   device route / host route: %.4f' % (med(dev) / med(host)))
    units = J // 3
    labels = rng.integers(0, units, (U, a.labels)).astype(np.int32)
    d_t, h_t, h_map = [], [], []
    for r in range(a.repeats + 1):
        eng.sync()
        t0 = time.perf_counter()
        seg = eng.uniform_segments(labels, lens, begin, 3, units * 3)
        t1 = time.perf_counter()
        seg.close()
        t2 = time.perf_counter()
        state = tw.uniform_map(U * T, labels, lens, begin, 3)
        t3 = time.perf_counter()
        seg = eng.segments(state, J=units * 3)
        t4 = time.perf_counter()
        seg.close()
        if r:
            d_t.append(t1 - t0)
            h_t.append(t4 - t2)
            h_map.append(t3 - t2)
    say('uniform segments, device route (Engine.uniform_segments): %8.1f ms' % (med(d_t) * 1e3))
    say('uniform segments, host route (twin map + Engine.segments): %7.1f ms   of which the NumPy map %.1f ms' % (med(h_t) * 1e3, med(h_map) * 1e3))
    eng.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
