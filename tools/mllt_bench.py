"""Kernel time of MLLT (row f13) at BASELINE config 4's shape, through pcl_kernel_time.

    python tools/mllt_bench.py [--units 1000] [--mix 2048] [--dim 39] [--utts 1024] [--frames 300] [--chunks 512,1024,...] [--repeats 5] [--out FILE]

One batch of --utts x --frames frames (labels of 20 units) is scored and aligned once (PCL_F32) and accumulated, so that the statistics
block is that of a real E-step.  The model is (--units x 3 states) x --mix mixtures where memory allows; otherwise --mix is halved until
the model fits, and the first line says which shape ran.  Medians of --repeats runs, the float64 matrix pipe and the VALU form
(PCL_MLLR_VALU=1) alternating; one line per figure (also written to --out; profiles/r17_mllt.txt is such a file):
  frames     Batch.accumulate_mllt: "mllt_frames" (the reduction p_i(t), beta(t)) and "mllt_gk" (the frame-side GEMM, ONE group, and its
             reduction), the latter for every PCL_MLLT_CHUNK of --chunks: the sweep the default chunk length is chosen from
  mixtures   Engine.mllt_estimate: "mllt_gk" (the mixture-side GEMM over 2 x J x M K-elements and its reduction) and "mllt_solve"
  beside     on the same build, machine and batch: Batch.accumulate_fmllr with one speaker ("fmllr_frames": the same loop with q, in two
             halves at D >= 39; "fmllr_gk") and Engine.mllr_estimate with one class ("adapt_gk": the same template at half the K)
with the fraction of the 78.6 TFLOP/s float64 matrix peak the issued MFMAs amount to."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--units', type=int, default=1000)
    ap.add_argument('--mix', type=int, default=2048)
    ap.add_argument('--dim', type=int, default=39)
    ap.add_argument('--utts', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--label', type=int, default=20)
    ap.add_argument('--chunks', default='512,1024,2048,4096,8192,16384,65536')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--n-iter', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from poccala_amd import Engine, PCL_F32, PoccalaHipError, synth
    from poccala_amd.engine import make_sentence_batch
    units, M, D, S = a.units, a.mix, a.dim, 5
    J = units * (S - 2)
    eng = Engine(0)
    eng.enable_timing(True)
    frames, lens, begin = synth.make_frames(a.utts, a.frames, D)
    labels = synth.make_labels(a.utts, a.label, units)
    eng.load_frames(frames)
    while True:
        mean, var, w, trans = synth.make_model(units, M, D)
        try:
            eng.load_model(mean, var, w)
            b, _ = make_sentence_batch(eng, labels, lens, begin, trans)
            b.score(PCL_F32)
            b.forward_backward(fix_pi=False)
            eng.stats_zero()
            b.accumulate(PCL_F32)
            eng.mllt_zero()
            b.accumulate_mllt()                                   # (allocates the float64 scoring rows and the call's scratch: not counted)
            eng.sync()
            break
        except (PoccalaHipError, MemoryError) as e:
            if M <= 1:
                raise
            print('M = %d does not fit (%s): halving' % (M, e), flush=True)
            M //= 2
    V = int(lens.sum())
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# tools/mllt_bench.py: J = %d, M = %d, D = %d (asked for M = %d), one batch of %d x %d = %d frames, medians of %d, MFMA and VALU '
             'alternating (%s)' % (J, M, D, a.mix, a.utts, a.frames, V, a.repeats, eng.device_info()['name']))
    groups = ('mllt', 'mllt_frames', 'mllt_gk', 'mllt_solve', 'fmllr_frames', 'fmllr_gk', 'adapt_gk')
    med = lambda v: float(np.median(v))
    NT = (D + 15) // 16
    ntiles = NT * (NT + 1) // 2
    NTf = (D + 2 + 15) // 16
    ntf = NTf * (NTf + 1) // 2

    def timed(call, valu, chunk=None):
        os.environ['PCL_MLLR_VALU'] = '1' if valu else '0'
        if chunk is None:
            os.environ.pop('PCL_MLLT_CHUNK', None)
        else:
            os.environ['PCL_MLLT_CHUNK'] = str(chunk)
        for k in groups:
            eng.kernel_time(k)
        call()
        eng.sync()
        return {k: eng.kernel_time(k)[0] for k in groups}

    def series(call, keys, chunk=None):
        got = {(v, k): [] for v in (False, True) for k in keys}
        for r in range(a.repeats + 1):                            # the first run allocates: not counted
            for valu in (False, True):
                t = timed(call, valu, chunk)
                if r:
                    for k in keys:
                        got[(valu, k)].append(t[k])
        return {vk: med(x) for vk, x in got.items()}

    # ---- the frame side, over the chunk sweep
    def acc_mllt():
        eng.mllt_zero()
        b.accumulate_mllt()

    flop_f = V * D * ntiles * 512.0
    for chunk in [None] + [int(c) for c in a.chunks.split(',')]:
        m = series(acc_mllt, ('mllt_frames', 'mllt_gk'), chunk)
        n_chunks = '(library default)' if chunk is None else '%5d chunks x %d = %6d workgroups' % (-(-V // chunk), D, -(-V // chunk) * D)
        say('frames, PCL_MLLT_CHUNK = %7s %s: mllt_frames %8.2f ms; mllt_gk MFMA %8.3f ms = %5.2f TFLOP/s float64 = %4.1f %% of the matrix peak; '
            'VALU %8.3f ms' % ('unset' if chunk is None else chunk, n_chunks, m[(False, 'mllt_frames')], m[(False, 'mllt_gk')],
                              flop_f / (m[(False, 'mllt_gk')] * 1e-3) / 1e12, 100 * flop_f / (m[(False, 'mllt_gk')] * 1e-3) / PEAK, m[(True, 'mllt_gk')]))
    # ---- the mixture side and the solve
    m = series(lambda: eng.mllt_estimate(a.n_iter, 1.0), ('mllt_gk', 'mllt_solve'))
    flop_c = 2.0 * J * M * D * ntiles * 512.0
    say('mixtures, %d K-elements, default chunk: mllt_gk MFMA %8.2f ms = %5.2f TFLOP/s float64 = %4.1f %% of the matrix peak; VALU %8.2f ms; '
        'mllt_solve (%d sweeps) %7.2f ms' % (2 * J * M, m[(False, 'mllt_gk')], flop_c / (m[(False, 'mllt_gk')] * 1e-3) / 1e12,
                                           100 * flop_c / (m[(False, 'mllt_gk')] * 1e-3) / PEAK, m[(True, 'mllt_gk')], a.n_iter, m[(False, 'mllt_solve')]))
    est = eng.mllt_estimate(a.n_iter, 1.0)
    say('   status %d, occupancies %.6g (frames) %.6g (statistics block, PCL_F32 accumulate), ln|det A| %.6f' % (est['status'], est['occ'][0], est['occ'][1], est['logdet']))
    # ---- beside them: fMLLR with one speaker, MLLR with one class
    spk = np.zeros(a.utts, dtype=np.int32)

    def acc_fmllr():
        eng.fmllr_zero(1)
        b.accumulate_fmllr(spk)

    f = series(acc_fmllr, ('fmllr_frames', 'fmllr_gk'))
    flop_ff = V * D * ntf * 512.0
    say('beside: fmllr_frames %8.2f ms (mllt_frames / fmllr_frames above); fmllr_gk (one speaker, PCL_MLLR_CHUNK default) MFMA %8.3f ms = %5.2f TFLOP/s'
        % (f[(False, 'fmllr_frames')], f[(False, 'fmllr_gk')], flop_ff / (f[(False, 'fmllr_gk')] * 1e-3) / 1e12))
    g = series(lambda: eng.mllr_estimate(None, 1, 1.0), ('adapt_gk',))
    flop_a = 1.0 * J * M * D * ntf * 512.0
    say('beside: adapt_gk (one class, %d K-elements) MFMA %8.2f ms = %5.2f TFLOP/s; the mixture-side mllt_gk / adapt_gk = %.2f'
        % (J * M, g[(False, 'adapt_gk')], flop_a / (g[(False, 'adapt_gk')] * 1e-3) / 1e12, m[(False, 'mllt_gk')] / g[(False, 'adapt_gk')]))
    b.close()
    eng.close()
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
