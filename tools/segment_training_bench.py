"""Wall time of segmental training (Segments.kmeans + Segments.em) at a BASELINE-like shape, per phase.

    python tools/segment_training_bench.py [--states 549] [--mix 64] [--dim 39] [--frames 1000000] [--sweeps 10] [--iters 5]
                                           [--embedded] [--twin-states N]

Prints one line per phase; under rocprofv3 --kernel-trace --stats the per-kernel split comes from the profiler.
--embedded      afterwards one embedded EM iteration (scoring + forward-backward + accumulate + pcl_mstep) on the SAME frames with the
                model just trained: utterances of 300 frames, 20 label units each (60 label states per frame), second of two runs
--twin-states N the float64 NumPy twin (tests/_segment_twin.py) on the first N states' frames, for the record"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--states', type=int, default=549)
    ap.add_argument('--mix', type=int, default=64)
    ap.add_argument('--dim', type=int, default=39)
    ap.add_argument('--frames', type=int, default=1000000)
    ap.add_argument('--sweeps', type=int, default=10)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--f64', action='store_true')
    ap.add_argument('--embedded', action='store_true')
    ap.add_argument('--twin-states', type=int, default=0)
    a = ap.parse_args()
    from poccala_amd import Engine, PCL_F32, PCL_F64
    prec = PCL_F64 if a.f64 else PCL_F32
    rng = np.random.default_rng(0)
    state = rng.integers(0, a.states, a.frames).astype(np.int32)
    blobs = rng.standard_normal((a.states, 8, a.dim)).astype(np.float32) * 3
    frames = blobs[state, rng.integers(0, 8, a.frames)] + rng.standard_normal((a.frames, a.dim)).astype(np.float32)
    eng = Engine(0)
    eng.load_frames(frames)
    t = [time.perf_counter()]
    seg = eng.segments(state, J=a.states)
    t.append(time.perf_counter())
    sweeps = seg.kmeans(a.mix, seed=1, max_sweeps=a.sweeps, precision=prec)
    eng.sync()
    t.append(time.perf_counter())
    iters, q = seg.em(max_iters=a.iters, precision=prec)
    eng.sync()
    t.append(time.perf_counter())
    seg.close()
    emb = None
    if a.embedded:
        from poccala_amd import synth
        units, T, L = a.states // 3, 300, 20
        U = a.frames // T
        eng.load_units(np.stack([synth.flat_start_transmat()] * units))
        labels = np.random.default_rng(2).integers(0, units, (U, L)).astype(np.int32)
        b = eng.label_batch(labels, np.full(U, T, dtype=np.int32), np.arange(U, dtype=np.int64) * T)
        for _ in range(2):
            eng.sync()
            t0 = time.perf_counter()
            b.score(prec)
            b.forward_backward()
            eng.stats_zero()
            b.accumulate(prec)
            eng.mstep(1e-3)
            eng.sync()
            emb = time.perf_counter() - t0
        b.close()
    eng.close()
    print('shape: %d states x %d mixtures, D = %d, %d frames, %s' % (a.states, a.mix, a.dim, a.frames, 'f64' if a.f64 else 'f32'))
    print('segments (sort + gather)   %8.1f ms' % (1e3 * (t[1] - t[0])))
    print('kmeans (seed + %2d sweeps max, ran %d..%d) %8.1f ms' % (a.sweeps, sweeps.min(), sweeps.max(), 1e3 * (t[2] - t[1])))
    print('em (%d loop bodies max, ran %d..%d)  %8.1f ms  = %.1f ms per loop body = %.2f M frames/s' %
          (a.iters, iters.min(), iters.max(), 1e3 * (t[3] - t[2]), 1e3 * (t[3] - t[2]) / iters.max(), a.frames * iters.max() / (t[3] - t[2]) / 1e6))
    if emb is not None:
        print('embedded EM iteration on the same frames (score + forward-backward + accumulate + mstep, %d x 300 frames, 60 label states per frame) %8.1f ms'
              % (a.frames // 300, 1e3 * emb))
    if a.twin_states:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
        import _segment_twin as tw
        t0 = time.perf_counter()
        n = 0
        for j in range(a.twin_states):
            x = frames[state == j].astype(np.float64)
            n += len(x)
            mean, var, w, assign, sw = tw.kmeans(x, a.mix, 1, j, a.sweeps)
            t1 = time.perf_counter()
            r = tw.em(x, mean, var, np.maximum(w, 1e-300), max_iters=a.iters)
        print('CPU twin, %d states (%d frames): kmeans + em %8.1f ms (em of the last state: %d loop bodies, %.1f ms)'
              % (a.twin_states, n, 1e3 * (time.perf_counter() - t0), r['iters'], 1e3 * (time.perf_counter() - t1)))


if __name__ == '__main__':
    main()
