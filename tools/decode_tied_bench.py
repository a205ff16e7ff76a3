#!/usr/bin/env python3
"""Decode kernel time untied and tied at BASELINE config 5's shard shape (profiles/r06_decode_summary.txt: 417 utterances x 300
frames, 183 units, a 20 k-word pronunciation tree, 8192 live tokens): pcl_batch_decode, and pcl_batch_decode_tied under the identity
tying (every (unit, k) its own leaf: the same tokens, the same bits, so the difference is the state-id gather alone) on the same
batch.  Median kernel time of `reps` launches after a warm-up, from the library's own events (pcl_kernel_time).

usage: decode_tied_bench.py [--no-tied] [--reps N] [--mixtures M]
  --no-tied  untied decode only, and the tied entry points are not bound: an older build of the library (POCCALA_HIP_LIB) can be
             measured with this script for an A/B on one machine."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--no-tied', action='store_true')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--mixtures', type=int, default=64)
args = ap.parse_args()

from poccala_amd import _lib
if args.no_tied:
    for name in ('pcl_lexicon_tie', 'pcl_lexicon_untie', 'pcl_lexicon_states', 'pcl_batch_decode_tied'):
        _lib.PROTOTYPES.pop(name)
from poccala_amd import Engine, PCL_F32, synth

c = synth.CONFIGS['C5shard']
cap = 8192
tree, lx = synth.make_pronunciation_tree(20000, c['units'])
mean, var, w, trans = synth.make_model(c['units'], args.mixtures, c['D'])
frames, lens, begin = synth.make_frames(c['U'], c['T'], c['D'], seed=6)
eng = Engine(0)
eng.enable_timing(True)
eng.load_model(mean, var, w)
eng.load_units(np.stack(trans))
eng.load_lexicon(tree)
eng.load_frames(frames)
b = eng.all_state_batch(lens, begin)
b.score(PCL_F32)


def timed(**kw):
    res = b.decode(max_tokens=cap, candidate=5, **kw)           # warm-up: workspace, code object
    eng.sync()
    eng.kernel_time('decode')
    ms = []
    for _ in range(args.reps):
        res = b.decode(max_tokens=cap, candidate=5, **kw)
        eng.sync()
        t, k = eng.kernel_time('decode')
        ms.append(t / k)
    return ms, res


out = dict(lib=_lib.LIB_PATH, mixtures=args.mixtures, reps=args.reps)
ms, res = timed()
out['untied_ms'] = [round(x, 3) for x in ms]
out['untied_median_ms'] = round(float(np.median(ms)), 3)
out['mean_live_tokens'] = round(float(np.mean([r['n_tokens'].mean() for r in res])), 1)
if not args.no_tied:
    from poccala_amd.AcousticModel.ContextTree import Tree
    n, P = c['units'] * 3, 3
    z = np.zeros(0)
    eng.load_tying(Tree(P, c['units'], node_cand=np.full(n, -1, np.int32), node_child=np.full((n, 2), -1, np.int32), node_state=np.arange(n, dtype=np.int32),
                        node_n=np.zeros(n, np.int64), split_gain=z, row_state=z.astype(np.int32), event_ctx=np.zeros((0, 3), np.int32),
                        q_member=np.zeros((1, c['units'] + 1), np.uint8), root_of=np.arange(n, dtype=np.int32), leaf_n=z, leaf_s=z, leaf_q=z))
    eng.tie_lexicon()
    ms, res_t = timed(tied=True)
    out['tied_ms'] = [round(x, 3) for x in ms]
    out['tied_median_ms'] = round(float(np.median(ms)), 3)
    out['tied_equals_untied'] = all(a['final'] == t['final'] and a['history'] == t['history'] for a, t in zip(res, res_t))
    eng.enable_timing(True)
    out['lexicon_tie_ms'] = round(eng.kernel_time('lexicon_tie')[0], 3)
b.close()
eng.close()
print(json.dumps(out))
