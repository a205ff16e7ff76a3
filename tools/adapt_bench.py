"""Wall time of adapting a resident model's means by MLLR at BASELINE config 4's shape, device route against host route.

    python tools/adapt_bench.py [--units 1000] [--mix 2048] [--dim 39] [--classes 1,8] [--repeats 5] [--host-repeats 5] [--out FILE]

The statistics are those of one config-4 batch (1024 utterances x 300 frames, labels of 20 units): score + forward-backward + accumulate
under PCL_F32.  Per class count R, medians of --repeats runs, the routes alternating, every run from the same freshly uploaded model and
a fresh accumulate pass; one line per figure (also written to --out; the bench table of profiles/r14_adapt.txt is such a file):
  device   Engine.mllr_estimate (pcl_kernel_time "adapt_gk": the GEMM and its reduction, "adapt_solve": the factorisations) +
           Engine.transform_means(None) ("adapt" of that call: the apply kernel; "derive": the pass behind it), with the GEMM on the
           float64 matrix pipe (default) and on the VALU (PCL_MLLR_VALU=1), and Engine.mstep_map beside them
  host     what the library offered before: Engine.stats_download + Engine.model_download + the twin's rule as BLAS calls (one
           (D+1) x K x (D+1) product per class and dimension, np.linalg.cholesky) + Engine.load_model
The first device run's W is compared with the host route's."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def host_mllr(mean, var, acc, mean_acc, cls, R, min_occ):
    """tests/_adapt_twin.py:mllr_estimate with the loop over mixtures replaced by matrix products (the same sums in BLAS's order)"""
    import _adapt_twin as tw
    J, M, D = mean.shape
    W = np.stack([tw.identity(D)] * R)
    status = np.zeros(R, dtype=np.int32)
    for r in range(R):
        sel = np.flatnonzero(cls == r)
        a = acc[sel].reshape(-1)
        live = tw.contributes(a)
        a = a[live]
        if a.sum() < min_occ:
            status[r] = tw.LOW_OCCUPANCY
            continue
        if len(a) < D + 1:
            status[r] = tw.FEW_MIXTURES
            continue
        mu, vr = mean[sel].reshape(-1, D)[live], var[sel].reshape(-1, D)[live]
        s = mean_acc[sel].reshape(-1, D)[live] - tw.BIAS * a[:, None]
        xi = np.concatenate([np.ones((len(a), 1)), mu], axis=1)
        rows = []
        for i in range(D):
            c = a / vr[:, i]
            G = xi.T @ (xi * c[:, None])
            k = xi.T @ (s[:, i] / vr[:, i])
            try:
                L = np.linalg.cholesky(G)
            except np.linalg.LinAlgError:
                status[r] = tw.NOT_POSITIVE_DEFINITE
                break
            rows.append(np.linalg.solve(L.T, np.linalg.solve(L, k)))
        if status[r] == 0:
            W[r] = np.stack(rows)
    return W, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--units', type=int, default=1000)
    ap.add_argument('--mix', type=int, default=2048)
    ap.add_argument('--dim', type=int, default=39)
    ap.add_argument('--utts', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--label', type=int, default=20)
    ap.add_argument('--classes', default='1,8')
    ap.add_argument('--min-occ', type=float, default=1000.0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-repeats', type=int, default=None, help='runs of the host route (default: --repeats)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import _adapt_twin as tw
    from poccala_amd import Engine, PCL_F32, synth
    from poccala_amd.engine import make_sentence_batch
    units, M, D, S = a.units, a.mix, a.dim, 5
    J = units * (S - 2)
    host_n = a.repeats if a.host_repeats is None else a.host_repeats
    mean, var, w, trans = synth.make_model(units, M, D)
    frames, lens, begin = synth.make_frames(a.utts, a.frames, D)
    labels = synth.make_labels(a.utts, a.label, units)
    eng = Engine(0)
    eng.enable_timing(True)
    lines = ['# tools/adapt_bench.py: J = %d, M = %d, D = %d, statistics of one batch of %d x %d frames (PCL_F32), min_occ %g, medians of %d '
             '(host route: %d), routes alternating (%s)' % (J, M, D, a.utts, a.frames, a.min_occ, a.repeats, host_n, eng.device_info()['name'])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng.load_frames(frames)
    groups = ('adapt', 'adapt_gk', 'adapt_solve', 'derive')

    def base():
        """the same model and the same statistics in front of every run"""
        eng._model_key = None
        eng.load_model(mean, var, w)
        b, _ = make_sentence_batch(eng, labels, lens, begin, trans)
        b.score(PCL_F32)
        b.forward_backward(fix_pi=False)
        eng.stats_zero()
        b.accumulate(PCL_F32)
        eng.sync()
        b.close()
        for k in groups:
            eng.kernel_time(k)

    med = lambda v: float(np.median(v)) if len(v) else float('nan')
    dd = next(o for o in (13, 26, 39, 47, 48, 64) if D <= o)          # the padded feature dimension
    NT = (D + 2 + 15) // 16
    ntiles = NT * (NT + 1) // 2
    for R in [int(x) for x in a.classes.split(',')]:
        cls = ((np.arange(J) // (S - 2)) % R).astype(np.int32)
        res = {}
        for valu in (False, True):
            key = 'valu' if valu else 'mfma'
            res[key] = dict(est=[], gk=[], solve=[], apply_call=[], apply=[], derive=[], W=None, status=None)
        res['map'] = dict(call=[], kernel=[], derive=[])
        host = dict(total=[], stats=[], model=[], twin=[], upload=[], W=None)
        for r in range(a.repeats + 1):                                 # the first run allocates: not counted
            for valu in (False, True):
                d = res['valu' if valu else 'mfma']
                os.environ['PCL_MLLR_VALU'] = '1' if valu else '0'
                base()
                t0 = time.perf_counter()
                W, occ, status = eng.mllr_estimate(cls, R, a.min_occ)
                t1 = time.perf_counter()
                kt = {k: eng.kernel_time(k)[0] for k in groups}
                t2 = time.perf_counter()
                eng.transform_means(None, cls, R)
                t3 = time.perf_counter()
                ka = {k: eng.kernel_time(k)[0] for k in groups}
                if r:
                    d['est'].append(t1 - t0), d['gk'].append(kt['adapt_gk']), d['solve'].append(kt['adapt_solve'])
                    d['apply_call'].append(t3 - t2), d['apply'].append(ka['adapt']), d['derive'].append(ka['derive'])
                else:
                    d['W'], d['status'], d['occ'] = W, status, occ
                print('R = %d %s run %d: estimate %.1f ms (gemm %.2f, solve %.2f), apply %.1f ms (kernel %.2f, derive %.2f)'
                      % (R, 'VALU' if valu else 'MFMA', r, (t1 - t0) * 1e3, kt['adapt_gk'], kt['adapt_solve'], (t3 - t2) * 1e3, ka['adapt'], ka['derive']), flush=True)
            os.environ['PCL_MLLR_VALU'] = '0'
            if R == 1:
                base()
                t0 = time.perf_counter()
                eng.mstep_map(10.0)
                t1 = time.perf_counter()
                km = {k: eng.kernel_time(k)[0] for k in groups}
                if r:
                    res['map']['call'].append(t1 - t0), res['map']['kernel'].append(km['adapt']), res['map']['derive'].append(km['derive'])
            if r <= host_n:                                            # (run 0 is the comparison run of both routes)
                base()
                t0 = time.perf_counter()
                st = eng.stats_download()
                t1 = time.perf_counter()
                old = eng.model_download()
                t2 = time.perf_counter()
                Wh, sh = host_mllr(old[0], old[1], st['acc'], st['mean_acc'], cls, R, a.min_occ)
                new = tw.transform_means(old[0], Wh, cls)[0]
                t3 = time.perf_counter()
                eng.load_model(new, old[1], old[2])
                eng.sync()
                t4 = time.perf_counter()
                if r:
                    host['total'].append(t4 - t0), host['stats'].append(t1 - t0), host['model'].append(t2 - t1)
                    host['twin'].append(t3 - t2), host['upload'].append(t4 - t3)
                else:
                    host['W'], host['status'] = Wh, sh
                print('R = %d host run %d: %.1f ms' % (R, r, (t4 - t0) * 1e3), flush=True)
                del st, old, new
        say('R = %d: statuses %s (host route %s), occupancies %.4g .. %.4g' % (R, res['mfma']['status'].tolist(), host['status'].tolist(),
                                                                             res['mfma']['occ'].min(), res['mfma']['occ'].max()))
        scale = np.abs(host['W']).max(axis=-1, keepdims=True)
        say('   W, device (MFMA) against the host route, relative to the largest element of a row: %.3e; VALU against MFMA: %.3e'
            % (float((np.abs(res['mfma']['W'] - host['W']) / scale).max()), float((np.abs(res['valu']['W'] - res['mfma']['W']) / scale).max())))
        mixt = int((cls >= 0).sum()) * M
        flop_tiles, flop_full = mixt * D * ntiles * 512.0, mixt * D * 2.0 * (D + 1) * (D + 2)
        logical = mixt * D * (D + 3) * 8.0
        unique = mixt * (2 * dd + 1 + dd) * 8.0
        for key, name in (('mfma', 'float64 matrix pipe'), ('valu', 'float64 VALU       ')):
            d = res[key]
            say('R = %d, GEMM on the %s: estimate %8.1f ms = G, k %8.2f ms + solve %6.2f ms + the rest (lists up, statuses down); '
                'apply %7.1f ms = kernel %6.2f ms + derive %6.2f ms' % (R, name, med(d['est']) * 1e3, med(d['gk']), med(d['solve']), med(d['apply_call']) * 1e3,
                                                                      med(d['apply']), med(d['derive'])))
            say('   G, k: %.1f GFLOP in the upper-triangular 16 x 16 tiles (%.1f for [G | k] without padding or symmetry): %.2f TFLOP/s float64 '
                '(%.2f); %.2f GB of model and statistics touched once, %.1f GB requested by the workgroups: %.0f GB/s of unique bytes'
                % (flop_tiles / 1e9, flop_full / 1e9, flop_tiles / (med(d['gk']) * 1e-3) / 1e12, flop_full / (med(d['gk']) * 1e-3) / 1e12, unique / 1e9, logical / 1e9,
                   unique / (med(d['gk']) * 1e-3) / 1e9))
        if R == 1:
            m = res['map']
            say('MAP means (Engine.mstep_map): %7.1f ms = kernel %6.2f ms + derive %6.2f ms' % (med(m['call']) * 1e3, med(m['kernel']), med(m['derive'])))
        dev = med(res['mfma']['est']) + med(res['mfma']['apply_call'])
        say('R = %d, host route (stats_download + model_download + BLAS twin + load_model): %9.1f ms = %.1f + %.1f + %.1f + %.1f ms'
            % (R, med(host['total']) * 1e3, med(host['stats']) * 1e3, med(host['model']) * 1e3, med(host['twin']) * 1e3, med(host['upload']) * 1e3))
        say('   device route (estimate + apply, matrix pipe) / host route: %.5f' % (dev / med(host['total'])))
    eng.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
