"""Wall time of growing a resident model by mix-up at BASELINE config 4's shape, device route against host route.

    python tools/mixup_bench.py [--states 3000] [--mix 1024] [--to 2048] [--dim 39] [--repeats 5] [--out FILE]

Medians of --repeats runs, the routes alternating, each from the same freshly uploaded (J, M, D) model; one line per figure (also
written to --out; the bench table of profiles/r13_mixup.txt is such a file):
  device   Engine.mixup: plan + fill on the device (pcl_kernel_time "mixup"), then the derive pass every new model gets ("derive")
  host     what the library offered before: Engine.model_download, the NumPy twin of the rule (tests/_mixup_twin.py),
           Engine.load_model (pcl_model_upload: pad, copy over PCIe, derive)
The run before the counted ones also downloads the device-grown model and compares it with the twin's, bit for bit."""
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
    ap.add_argument('--mix', type=int, default=1024)
    ap.add_argument('--to', type=int, default=2048)
    ap.add_argument('--dim', type=int, default=39)
    ap.add_argument('--perturb', type=float, default=0.2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import _mixup_twin as tw
    from poccala_amd import Engine
    J, M, M_new, D = a.states, a.mix, a.to, a.dim
    rng = np.random.default_rng(0)
    mean = rng.standard_normal((J, M, D))
    var = rng.uniform(0.5, 2.0, (J, M, D))
    w = rng.standard_exponential((J, M))
    w /= w.sum(axis=1, keepdims=True)
    eng = Engine(0)
    eng.enable_timing(True)
    lines = ['# tools/mixup_bench.py: J = %d, M = %d -> %d, D = %d, perturb %g, median of %d, routes alternating (%s)'
             % (J, M, M_new, D, a.perturb, a.repeats, eng.device_info()['name'])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def base():
        eng._model_key = None
        eng.load_model(mean, var, w)
        eng.sync()
        for k in ('mixup', 'derive'):
            eng.kernel_time(k)

    dev, parts = [], dict(mixup=[], derive=[])
    host, hparts = [], dict(download=[], twin=[], upload=[])
    for r in range(a.repeats + 1):                                   # the first run allocates: not counted
        base()
        t0 = time.perf_counter()
        eng.mixup(M_new, perturb=a.perturb)
        eng.sync()
        dt = time.perf_counter() - t0
        kt = {k: eng.kernel_time(k)[0] for k in parts}
        if r:
            dev.append(dt)
            for k in parts:
                parts[k].append(kt[k])
        print('device run %d: %.1f ms (mixup %.2f ms, derive %.2f ms)' % (r, dt * 1e3, kt['mixup'], kt['derive']), flush=True)
        grown = eng.model_download() if r == 0 else None
        base()
        t0 = time.perf_counter()
        old = eng.model_download()
        t1 = time.perf_counter()
        new = tw.mixup(*old, M_new, a.perturb)
        t2 = time.perf_counter()
        eng.load_model(*new[:3])
        eng.sync()
        t3 = time.perf_counter()
        if r:
            host.append(t3 - t0)
            hparts['download'].append(t1 - t0)
            hparts['twin'].append(t2 - t1)
            hparts['upload'].append(t3 - t2)
        print('host run %d: %.1f ms' % (r, (t3 - t0) * 1e3), flush=True)
        if grown is not None:
            same = [g.tobytes() == n.tobytes() for g, n in zip(grown, new[:3])]
            say('device-grown model against the twin at this shape (mean, var, weight bit-equal): %s; max |d mean| = %.3e'
                % (same, float(np.abs(grown[0] - new[0]).max())))
        del old, new, grown
    med = lambda v: float(np.median(v))
    say('mix-up, device route (Engine.mixup):                     %9.1f ms   kernels: plan + fill %.2f ms, derive %.2f ms (%.0f %% of the call)'
        % (med(dev) * 1e3, med(parts['mixup']), med(parts['derive']), 100 * med(parts['derive']) / (med(dev) * 1e3)))
    pad = lambda m: (m + 3) // 4 * 4
    dd = next(o for o in (13, 26, 39, 47, 48, 64) if D <= o)          # the padded feature dimension
    rd, wr = 2 * J * pad(M) * dd * 8 / 1e9, 2 * J * pad(M_new) * dd * 8 / 1e9
    say('   the fill reads the old master copy (%.2f GB, every row for itself and for its children) and writes the new one (%.2f GB): '
        '%.0f GB/s over "mixup", plan included' % (rd, wr, (rd + wr) / (med(parts['mixup']) * 1e-3)))
    say('mix-up, host route (download + NumPy twin + load_model): %9.1f ms   model_download %.1f ms, twin %.1f ms, load_model %.1f ms'
        % (med(host) * 1e3, med(hparts['download']) * 1e3, med(hparts['twin']) * 1e3, med(hparts['upload']) * 1e3))
    say('   device route / host route: %.4f' % (med(dev) / med(host)))
    eng.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
