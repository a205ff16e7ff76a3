#!/usr/bin/env python
"""Kernel time of pcl_mstep_ebw (group "ebw") beside pcl_mstep's (group "mstep", which includes its derive pass; "derive" is timed alone behind
pcl_mstep_ebw) at the config-4 shape J = 3000, M = 2048, D = 39, on synthetic statistics made on the device by two small accumulate passes.
Median of 7 calls after a warm-up.  Traffic of the update: two statistics blocks read once, means and variances read and written once.
    python tools/ebw_bench.py [--J 3000 --M 2048 --D 39 --frames 64 --out profiles/ebw_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK = 8.0e12            # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--J', type=int, default=3000)
    ap.add_argument('--M', type=int, default=2048)
    ap.add_argument('--D', type=int, default=39)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--weight-iters', type=int, default=100)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from poccala_amd import Engine, PCL_F32
    J, M, D, F = a.J, a.M, a.D, a.frames
    rng = np.random.default_rng(4)
    mean = rng.standard_normal((J, M, D), dtype=np.float32).astype(np.float64)
    var = rng.uniform(0.5, 2.0, (J, M, D))
    w = np.full((J, M), 1.0 / M)
    frames = rng.standard_normal((F, D), dtype=np.float32)
    eng = Engine(0)
    eng.enable_timing(True)

    def fill(seed, scale):                                       # one accumulate pass with random state posteriors
        g = np.random.default_rng(seed).uniform(0.1, 1.0, (J, F)) * scale
        lg = np.concatenate([np.full((1, F), -np.inf), np.log(g), np.full((1, F), -np.inf)])
        b.set_posteriors([lg])
        eng.stats_zero()
        b.accumulate(PCL_F32)

    times = dict(ebw=[], derive=[], mstep=[])
    for rep in range(8):                                         # the first is the warm-up
        eng.load_model(mean, var, w)
        eng.load_frames(frames)
        b = eng.all_state_batch(np.array([F], dtype=np.int32), np.array([0], dtype=np.int64))
        b.score(PCL_F32)
        fill(1, 3.0)
        eng.ebw_hold()
        fill(2, 1.0)
        for k in times:
            eng.kernel_time(k)
        counts = eng.mstep_ebw(weight_iters=a.weight_iters)
        t_ebw, t_der = eng.kernel_time('ebw')[0], eng.kernel_time('derive')[0]
        b.score(PCL_F32)
        fill(1, 3.0)
        eng.kernel_time('mstep')
        eng.mstep()
        t_ms = eng.kernel_time('mstep')[0]
        b.close()
        if rep:
            times['ebw'].append(t_ebw)
            times['derive'].append(t_der)
            times['mstep'].append(t_ms)
    med = {k: float(np.median(v)) for k, v in times.items()}
    elems = J * M * D                                            # what the kernels touch: host dimensions of real mixtures
    bytes_ebw = 8 * (4 * elems + 4 * elems + 2 * J * M)          # mean_acc, cov_acc of both sets; mean, var read and written; the two acc
    bytes_mstep = 8 * (2 * elems + 2 * elems + J * M)            # one block's moments read, mean and var written
    mstep_kernel = max(med['mstep'] - med['derive'], 1e-9)
    res = dict(J=J, M=M, D=D, weight_iters=a.weight_iters, counts=counts, ms=med, mstep_kernel_ms=mstep_kernel,
               ebw_bytes=bytes_ebw, ebw_bytes_per_s=bytes_ebw / (med['ebw'] * 1e-3), ebw_share_of_hbm_peak=bytes_ebw / (med['ebw'] * 1e-3) / HBM_PEAK,
               mstep_bytes_per_s=bytes_mstep / (mstep_kernel * 1e-3), ratio_ebw_to_mstep_kernel=med['ebw'] / mstep_kernel, all_ms=times)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    eng.close()


if __name__ == '__main__':
    main()
