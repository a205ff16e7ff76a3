"""Device time of the LDA accumulate pass and of the projection (row f12, csrc/frame_lda.hip), MFMA form against VALU form.

    python tools/lda_bench.py [--utts 1024] [--frames 300] [--dim 13] [--context 4] [--classes 3000 150] [--out-dim 40] [--repeats 5] [--out FILE]

Random float64 frames, every row labelled with a uniformly drawn class.  Per class count R, medians of --repeats runs through
pcl_kernel_time (HIP events around the launches), the two forms alternating, after one uncounted run that allocates:
  lda_sort     keys + counting sort of the rows by class
  lda_stats    the [x | 1][x | 1]^T product over (chunk, tile group) work items and the reduction of the chunks' partials
  lda_project  Engine.splice_project to --out-dim dimensions (once per R: it does not depend on the form)
and the fraction of the float64 matrix peak (78.6 TFLOP/s, the MI355X data sheet) that the MFMAs ISSUED by lda_stats amount to: 512 flops
per row for each of the NT (NT + 1) / 2 upper-triangular 16 x 16 tiles, NT = ceil((Ds + 1) / 16).  The first run also compares the two
forms' statistics (n exactly, S to 1e-10 of the largest element)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F64_MATRIX = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--dim', type=int, default=13)
    ap.add_argument('--context', type=int, default=4)
    ap.add_argument('--classes', type=int, nargs='+', default=[3000, 150])
    ap.add_argument('--out-dim', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from poccala_amd import Engine
    U, T, D, c = a.utts, a.frames, a.dim, a.context
    F, Ds = U * T, (2 * c + 1) * D
    NT = (Ds + 1 + 15) // 16
    flops = F * 512.0 * NT * (NT + 1) / 2
    rng = np.random.default_rng(0)
    frames = rng.standard_normal((F, D))
    lens, begin = np.full(U, T, dtype=np.int32), (np.arange(U, dtype=np.int64) * T)
    A, b = rng.standard_normal((a.out_dim, Ds)) / Ds, rng.standard_normal(a.out_dim)
    eng = Engine(0)
    eng.enable_timing(True)
    lines = ['# tools/lda_bench.py: %d x %d frames, D = %d, +-%d (order %d, %d tiles), median of %d (%s)'
             % (U, T, D, c, Ds + 1, NT * (NT + 1) // 2, a.repeats, eng.device_info()['name'])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(lines.pop())
    for R in a.classes:
        cls = rng.integers(0, R, size=F).astype(np.int32)
        eng.load_frames(frames)
        times = {form: dict(lda_sort=[], lda_stats=[]) for form in ('mfma', 'valu')}
        ref = None
        for r in range(a.repeats + 1):
            for form in ('mfma', 'valu'):
                os.environ['PCL_LDA_VALU'] = '1' if form == 'valu' else '0'
                eng.lda_zero(R, c, c)
                for k in ('lda_sort', 'lda_stats'):
                    eng.kernel_time(k)
                eng.lda_accumulate(lens, begin, cls)
                got = {k: eng.kernel_time(k)[0] for k in ('lda_sort', 'lda_stats')}
                if r == 0:
                    n, s, S = eng.lda_stats()
                    if ref is None:
                        ref = (n, S)
                    else:
                        assert np.array_equal(n, ref[0]) and np.abs(S - ref[1]).max() <= 1e-10 * np.abs(ref[1]).max()
                        ref = None
                else:
                    for k in got:
                        times[form][k].append(got[k])
        for form in ('mfma', 'valu'):
            sort_ms, stats_ms = (float(np.median(times[form][k])) for k in ('lda_sort', 'lda_stats'))
            say('R = %5d  %s  lda_sort %8.3f ms  lda_stats %8.3f ms  = %5.2f TFLOP/s issued, %5.2f %% of the float64 matrix peak'
                % (R, form, sort_ms, stats_ms, flops / stats_ms / 1e9, 100.0 * flops / (stats_ms * 1e-3) / PEAK_F64_MATRIX))
        os.environ.pop('PCL_LDA_VALU', None)
        proj = []
        for r in range(a.repeats + 1):
            eng._frames_key = None
            eng.load_frames(frames)
            eng.kernel_time('lda_project')
            eng.splice_project(lens, begin, c, c, A, b)
            proj.append(eng.kernel_time('lda_project')[0])
        say('R = %5d  lda_project -> %d dimensions %8.3f ms' % (R, a.out_dim, float(np.median(proj[1:]))))
    eng.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
