#!/usr/bin/env python3
"""What the word lattice costs at BASELINE config 5's decode shape (417 utterances x 300 frames, 183 units, a 20 k-word pronunciation
tree, 8192 live tokens): the median of --reps (7) runs each of
  plain decode                      pcl_batch_decode                        pcl_kernel_time "decode"
  decode with the lattice           pcl_batch_decode_lattice                "decode" (the LAT kernels) and "lattice_build" behind it
  the lattice pass                  pcl_batch_lattice_posteriors(kappa)     "lattice_post"
and the arc counts (word-end donors per utterance: n_arcs_wanted), which say what record traffic the LAT kernels add: 36 bytes per arc.
The result goes to profiles/lattice_bench.json (or --out) and is printed as one JSON line.

usage: lattice_bench.py [--plain-only] [--reps N] [--mixtures M] [--max-arcs A] [--out FILE]
  --plain-only   plain decode only, and the lattice entry points are not bound: a build of the library from before the lattice
                 (POCCALA_HIP_LIB) can be measured with this script for an A/B of the plain kernels on one machine."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--plain-only', action='store_true')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--mixtures', type=int, default=256)
ap.add_argument('--max-arcs', type=int, default=0, help='records kept per utterance (default: 64 per frame, grown once if that overflows)')
ap.add_argument('--kappa', type=float, default=0.1)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lattice_bench.json'))
args = ap.parse_args()

from poccala_amd import _lib
NEW = ('pcl_batch_decode_lattice', 'pcl_batch_lattice_get', 'pcl_batch_lattice_posteriors', 'pcl_batch_lattice_results', 'pcl_batch_lattice_set_records')
if args.plain_only:
    for name in NEW:
        _lib.PROTOTYPES.pop(name, None)
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
GROUPS = ('decode', 'lattice_build', 'lattice_post')


def drain():
    for g in GROUPS:
        try:
            eng.kernel_time(g)
        except Exception:
            pass


def per_launch(group):
    t, k = eng.kernel_time(group)
    return t / k if k else 0.0


def timed(run, groups):
    run()                                                       # warm-up: workspace, code object
    eng.sync()
    drain()
    ms = {g: [] for g in groups}
    for _ in range(args.reps):
        run()
        eng.sync()
        for g in groups:
            ms[g].append(per_launch(g))
    return {g: [round(x, 3) for x in v] for g, v in ms.items()}


def median(v):
    return round(float(np.median(v)), 3)


out = dict(lib=_lib.LIB_PATH, mixtures=args.mixtures, reps=args.reps, U=int(c['U']), T=int(c['T']), max_tokens=cap)
ms = timed(lambda: b.decode_launch(max_tokens=cap, candidate=5), ('decode',))
out['plain_ms'], out['plain_median_ms'] = ms['decode'], median(ms['decode'])
if not args.plain_only:
    max_arcs = args.max_arcs or 64 * int(c['T'])
    b.decode_launch(max_tokens=cap, candidate=5, lattice=True, max_arcs=max_arcs)
    wanted = b.lattice_fetch()['n_arcs_wanted']
    if wanted.max() > max_arcs and not args.max_arcs:
        max_arcs = int(wanted.max())
    ms = timed(lambda: b.decode_launch(max_tokens=cap, candidate=5, lattice=True, max_arcs=max_arcs), ('decode', 'lattice_build'))
    out['lattice_decode_ms'], out['lattice_decode_median_ms'] = ms['decode'], median(ms['decode'])
    out['lattice_build_ms'], out['lattice_build_median_ms'] = ms['lattice_build'], median(ms['lattice_build'])
    from poccala_amd.engine import ptr

    def post():
        eng._check(eng._lib.pcl_batch_lattice_posteriors(b._b, float(args.kappa)))
    ms = timed(post, ('lattice_post',))
    out['lattice_post_ms'], out['lattice_post_median_ms'] = ms['lattice_post'], median(ms['lattice_post'])
    raw = b.lattice_fetch()
    res = b.lattice_posteriors(args.kappa)
    out.update(max_arcs=max_arcs, kappa=args.kappa, arcs_wanted_mean=round(float(raw['n_arcs_wanted'].mean()), 1), arcs_wanted_max=int(raw['n_arcs_wanted'].max()),
               arcs_total=int(raw['n_arcs_wanted'].sum()), overflowed=int(raw['overflow'].sum()),
               entries_mean=round(float(np.mean([len(r['best']) for r in res])), 1), record_bytes=int(raw['n_arcs_wanted'].sum()) * 36,
               status_nonzero=int(sum(1 for r in res if r['status'])),
               mean_confidence=round(float(np.mean([x[3] for r in res for x in r['best']])), 4))
b.close()
eng.close()
line = json.dumps(out)
if not args.plain_only:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
print(line)
