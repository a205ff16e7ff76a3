#!/usr/bin/env python3
"""Decode kernel time with and without the language model at BASELINE config 5's shard shape (tests/test_gpu_decode.py,
test_c5_decode_at_shard_shape: 417 utterances x 300 frames, 183 units, a 20 k-word pronunciation tree, 8192 live tokens): plain
decode() and decode(lm=True) with a random bigram of about 20 successors per word, `reps` repetitions each, kernel time from the
library's own events (pcl_kernel_time).

usage: decode_lm_bench.py [--no-lm] [--reps N] [--mixtures M]
  --no-lm    plain decode only, and the language-model entry points are not bound: an older build of the library (POCCALA_HIP_LIB)
             can be measured with this script for an A/B on one machine."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--no-lm', action='store_true')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--mixtures', type=int, default=4096)
ap.add_argument('--successors', type=int, default=20)
args = ap.parse_args()

from poccala_amd import _lib
if args.no_lm:
    for name in ('pcl_lm_upload', 'pcl_batch_decode_lm', 'pcl_batch_decode_get_words'):
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
out['plain_ms'] = [round(x, 3) for x in ms]
out['plain_median_ms'] = round(float(np.median(ms)), 3)
out['mean_live_tokens'] = round(float(np.mean([r['n_tokens'].mean() for r in res])), 1)
if not args.no_lm:
    from poccala_amd.LanguageModel import Ngram
    rng = np.random.default_rng(9)
    g = Ngram(2).count([], list(dict.fromkeys(x for ws in tree['words'] for x in ws)))
    W = len(g.words)
    g.uni_count[1:] = rng.integers(0, 50, size=W - 1)
    succ = rng.integers(1, W, size=(W, args.successors))         # (duplicates collapse: about `successors` per word)
    cnt = rng.integers(1, 40, size=(W, args.successors))
    for v in range(W):
        g.bi_count[v] = dict(zip(succ[v].tolist(), cnt[v].tolist()))
    lm = g.compile(tree)
    eng.load_language_model(lm)
    ms, res_lm = timed(lm=True)
    out['lm_ms'] = [round(x, 3) for x in ms]
    out['lm_median_ms'] = round(float(np.median(ms)), 3)
    out['lm_words'], out['lm_bigrams'] = W, int(len(lm['col']))
    out['lm_history_entries'] = int(sum(len(r['history']) for r in res_lm))
    out['lm_mean_live_tokens'] = round(float(np.mean([r['n_tokens'].mean() for r in res_lm])), 1)
b.close()
eng.close()
print(json.dumps(out))
