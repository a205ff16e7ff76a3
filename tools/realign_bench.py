"""Wall time of the realignment hop of training scheme 1 -- from "Viterbi done" to "Segments exists" -- at BASELINE config 4's shard
shape, the device route against the host route it replaces in AcousticModel.train_segments_batch.

    python tools/realign_bench.py [--units 1000] [--mix 2] [--dim 39] [--utts 1024] [--frames 300] [--labels 20] [--repeats 5] [--out FILE]

Medians of --repeats runs, the two routes alternating on ONE aligned batch (also written to --out; profiles/r11_realign.txt is such a
file):
  host route     what AcousticModel._align_regroup + Batch.segments do: row_unit built per utterance in NumPy, Batch.regroup
                 (pcl_batch_regroup: two int32 per frame to the host), the drop rule with np.unique per utterance, the owner array
                 filled per utterance, Engine.segments' upload (pcl_seg_create)
  device route   Batch.align_segments (pcl_batch_align_segments: one kernel, then pcl_seg_create's counting sort + gather on the
                 resident map); its kernels split by pcl_kernel_time in a second set of runs with the timers on:
                 "align_segments", "seg_count", "seg_gather" """
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--units', type=int, default=1000)
    ap.add_argument('--mix', type=int, default=2)
    ap.add_argument('--dim', type=int, default=39)
    ap.add_argument('--utts', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--labels', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from poccala_amd import Engine, PCL_F32, synth
    S, e = 5, 3
    U, T, L = a.utts, a.frames, a.labels
    mean, var, w, trans = synth.make_model(a.units, a.mix, a.dim, seed=1)
    mean = mean * 4
    labels = np.stack(synth.make_labels(U, L, a.units, seed=2)).astype(np.int32)
    frames = synth.make_peaked_frames(list(labels), T, mean, var, seed=3)
    lens, begin = np.full(U, T, dtype=np.int32), np.arange(U, dtype=np.int64) * T
    eng = Engine(0)
    eng.load_model(mean, var, w)
    eng.load_units(np.stack(trans))
    eng.load_frames(frames)
    b = eng.label_batch(labels, lens, begin)
    b.score(PCL_F32)
    b.viterbi()
    eng.sync()
    lines = ['# tools/realign_bench.py: %d units, S = %d, M = %d, D = %d, %d x %d frames, L = %d, median of %d (%s)'
             % (a.units, S, a.mix, a.dim, U, T, L, a.repeats, eng.device_info()['name'])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def host_route():
        t0 = time.perf_counter()
        row_unit = []
        for lab in labels:
            ids = np.repeat(lab, e)
            row_unit.append(np.concatenate([[ids[0]], ids, [ids[-1]]]).astype(np.int32))
        t1 = time.perf_counter()
        fu, fk = b.regroup(row_unit, e)
        t2 = time.perf_counter()
        dropped = [u for u, lab in enumerate(labels) if len(np.unique(fu[u])) < len(set(lab.tolist()))]
        t3 = time.perf_counter()
        seg = b.segments(row_unit, e, dropped=dropped, regrouped=(fu, fk))
        t4 = time.perf_counter()
        return seg, dropped, (t4 - t0, t1 - t0, t2 - t1, t3 - t2, t4 - t3)

    def device_route():
        t0 = time.perf_counter()
        seg, dropped = b.align_segments()
        return seg, dropped, time.perf_counter() - t0

    host, dev = [], []
    for r in range(a.repeats + 1):                                   # the first run allocates: not counted
        eng.sync()
        hs, hd, ht = host_route()
        eng.sync()
        ds, dd, dt = device_route()
        if r == 0:
            assert hd == dd and np.array_equal(hs.counts, ds.counts) and np.array_equal(hs.order, ds.order)
            say('both routes: %d of %d utterances dropped, %d of %d frames owned, the same counts and order' % (len(dd), U, int(ds.counts.sum()), U * T))
        else:
            host.append(ht)
            dev.append(dt)
        hs.close()
        ds.close()
        print('run %d: host route %.1f ms, device route %.2f ms' % (r, ht[0] * 1e3, dt * 1e3), flush=True)
    med = lambda v: float(np.median(v))
    hm = [med([h[k] for h in host]) * 1e3 for k in range(5)]
    say('host route (row_unit + regroup + drop rule + Batch.segments):   %8.2f ms   row_unit %.2f ms, Batch.regroup %.2f ms, drop rule %.2f ms, Batch.segments %.2f ms'
        % tuple(hm))
    say('device route (Batch.align_segments):                            %8.2f ms' % (med(dev) * 1e3))
    say('   device route / host route: %.4f%s' % (med(dev) * 1e3 / hm[0], '' if med(dev) * 1e3 <= hm[0] else '   THE DEVICE ROUTE IS SLOWER'))
    eng.enable_timing(True)
    parts = dict(align_segments=[], seg_count=[], seg_gather=[])
    for r in range(a.repeats + 1):
        for k in parts:
            eng.kernel_time(k)
        ds, dd, dt = device_route()
        ds.close()
        if r:
            for k in parts:
                parts[k].append(eng.kernel_time(k)[0])
    say('   kernels of the device route (timers on): align_segments %.3f ms, counting sort %.3f ms, scatter + gather %.3f ms'
        % (med(parts['align_segments']), med(parts['seg_count']), med(parts['seg_gather'])))
    b.close()
    eng.close()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
