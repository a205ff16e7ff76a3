#!/usr/bin/env python
"""Kernel time of pcl_batch_mbr (group "mbr": one pass under kappa with the expected accuracy) beside pcl_batch_forward_backward's (group "fb",
pi locked: one pass) on the SAME batches: the unit-loop denominator graph over 40 units x 3 states (N = 122, indegree 41 at a unit's first
row: the general lists) and a label batch of 20 units (N = 62: the register lists; forward-backward runs its scaled two-wave kernels there),
128 utterances x 300 frames each.  Median of 7 calls after a warm-up.
    python tools/mbr_bench.py [--units 40 --U 128 --T 300 --L 20 --kappa 0.1 --out profiles/mbr_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--units', type=int, default=40)
    ap.add_argument('--U', type=int, default=128)
    ap.add_argument('--T', type=int, default=300)
    ap.add_argument('--L', type=int, default=20)
    ap.add_argument('--M', type=int, default=4)
    ap.add_argument('--D', type=int, default=39)
    ap.add_argument('--kappa', type=float, default=0.1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from poccala_amd import Engine, PCL_F32, synth
    mean, var, w, trans = synth.make_model(a.units, a.M, a.D, seed=3)
    labels = synth.make_labels(a.U, a.L, a.units, seed=4)
    frames = synth.make_peaked_frames(labels, a.T, mean, var, seed=5)
    lens = np.full(a.U, a.T, dtype=np.int32)
    begin = (np.arange(a.U) * a.T).astype(np.int64)
    eng = Engine(0)
    eng.enable_timing(True)
    eng.load_model(mean, var, w)
    eng.load_units(trans)
    eng.load_frames(frames)
    num = eng.label_batch(labels, lens, begin)
    den = eng.loop_batch(lens, begin, trans)
    num.score(PCL_F32)
    num.viterbi()
    refs = num.ref_states()
    den.score(PCL_F32)
    res = dict(units=a.units, U=a.U, T=a.T, kappa=a.kappa, M=a.M, D=a.D)
    for name, b in (('loop', den), ('label', num)):
        times = dict(mbr=[], fb=[])
        for rep in range(8):                                         # the first is the warm-up
            for k in times:
                eng.kernel_time(k)
            b.mbr(refs, kappa=a.kappa)
            eng.sync()
            t_mbr = eng.kernel_time('mbr')[0]
            b.forward_backward(fix_pi=True)
            eng.sync()
            t_fb = eng.kernel_time('fb')[0]
            if rep:
                times['mbr'].append(t_mbr)
                times['fb'].append(t_fb)
        med = {k: float(np.median(v)) for k, v in times.items()}
        res[name] = dict(N=int(b.N[0]), ms=med, ratio_mbr_to_fb=med['mbr'] / med['fb'], all_ms=times,
                         c_avg_per_frame=float(b.mbr_get(want=('c_avg',))['c_avg'].sum() / (a.U * a.T)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    num.close()
    den.close()
    eng.close()


if __name__ == '__main__':
    main()
