"""Device time of the decision-tree statistics pass and of the tree build (row f16, csrc/tree_cluster.hip) at a realistic shape, with the
NumPy twin's CPU time for the same input beside it.

    python tools/tree_bench.py [--utts 1024] [--frames 300] [--dim 39] [--units 40] [--events 20000] [--questions 100] [--leaves 3000]
                               [--min-count 20] [--repeats 3] [--roots centre shared] [--no-twin] [--out FILE]

The default is the C4 shard's frame matrix (1024 x 300 frames of 39 dimensions), --events distinct triphone contexts drawn from all
(units + 1) units (units + 1) and listed in lexicographic order, P = 3 positions, --questions random unit sets, grown to --leaves leaves.
Every frame belongs to a uniformly drawn statistics row and scatters around a mean that depends on the row's left and right neighbour,
its centre and its position, so that the questions have something to find.
Per frame type (float32 rows widened / the float64 copy), medians of --repeats runs through pcl_kernel_time (HIP events around the
launches) after one uncounted run that allocates:
  tree_sort    keys + stable counting sort of the frame rows by statistics row
  tree_stats   the chunks' partial sums and their reduction in chunk order
and the wall time of the call.  Per root layout ('centre': a root per (centre, position), the usual one; 'shared': one root per
position for all centres, the longest row walks the build can meet):
  tree_build   the evaluation and arg-max kernels of all splits (HIP events), next to the wall time of pcl_tree_build, which adds the
               host's share: one descriptor upload, one download and one partition per split
The twin (tests/_tree_twin.py) is timed on the host for the first layout: its statistics pass and its build over the device's sums; its
tree is compared with the device's."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_input(a):
    rng = np.random.default_rng(0)
    nu, P, D = a.units, 3, a.dim
    every = np.array([(l, c, r) for l in range(nu + 1) for c in range(nu) for r in range(nu + 1)], dtype=np.int32)
    event_ctx = every[np.sort(rng.choice(len(every), size=min(a.events, len(every)), replace=False))]
    E = len(event_ctx)
    R = E * P
    sets = []
    while len(sets) < a.questions:
        m = rng.integers(0, 2, size=nu + 1)
        if 0 < m.sum() <= nu:
            sets.append(m)
    q_member = np.array(sets, dtype=np.uint8)
    F = a.utts * a.frames
    frame_row = rng.integers(0, R, size=F).astype(np.int32)
    shift_l, shift_r, shift_c = rng.standard_normal((nu + 1, D)) * 1.5, rng.standard_normal((nu + 1, D)), rng.standard_normal((nu, D)) * 2
    ev = event_ctx[frame_row // P]
    frames = (shift_l[ev[:, 0]] + 0.5 * shift_r[ev[:, 2]] + shift_c[ev[:, 1]] + 0.25 * (frame_row % P)[:, None]
              + rng.standard_normal((F, D))).astype(np.float32)
    lens, begin = np.full(a.utts, a.frames, dtype=np.int32), np.arange(a.utts, dtype=np.int64) * a.frames
    roots = dict(centre=(np.arange(nu * P, dtype=np.int32), nu * P), shared=(np.tile(np.arange(P, dtype=np.int32), nu), P))
    return dict(P=P, D=D, n_units=nu, event_ctx=event_ctx, q_member=q_member, R=R, frames=frames, frame_row=frame_row, T=lens, begin=begin,
                roots=roots)


def twin_build(x, stats, layout, a):
    import _tree_twin as tw
    root_of, R0 = x['roots'][layout]
    t0 = time.perf_counter()
    t = tw.build(stats[0], stats[1], stats[2], x['event_ctx'], x['P'], x['n_units'], x['q_member'], R0, root_of, a.min_count, 0.0, a.leaves,
                 a.var_floor)
    return t, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=1024)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--dim', type=int, default=39)
    ap.add_argument('--units', type=int, default=40)
    ap.add_argument('--events', type=int, default=20000)
    ap.add_argument('--questions', type=int, default=100)
    ap.add_argument('--leaves', type=int, default=3000)
    ap.add_argument('--min-count', type=int, default=20)
    ap.add_argument('--var-floor', type=float, default=1e-3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--roots', nargs='+', default=['centre', 'shared'], choices=['centre', 'shared'])
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from poccala_amd import Engine
    import _tree_twin as tw
    x = make_input(a)
    R, D, P = x['R'], x['D'], x['P']
    eng = Engine(0)
    eng.enable_timing(True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# tools/tree_bench.py: %d x %d frames, D = %d; %d events x P = %d = %d rows, %d units, Q = %d, max_leaves = %d, min_count = %d, '
        'median of %d (%s); every figure below was measured on this run'
        % (a.utts, a.frames, D, R // P, P, R, a.units, a.questions, a.leaves, a.min_count, a.repeats, eng.device_info()['name']))
    stats = None
    for kind, dt in (('float32', np.float32), ('float64', np.float64)):
        eng.load_frames(x['frames'].astype(dt))
        got = dict(tree_sort=[], tree_stats=[], wall=[])
        for r in range(a.repeats + 1):
            eng.tree_zero(R)
            for k in ('tree_sort', 'tree_stats'):
                eng.kernel_time(k)
            t0 = time.perf_counter()
            eng.tree_accumulate(x['T'], x['begin'], x['frame_row'])
            wall = (time.perf_counter() - t0) * 1e3
            if r:
                got['wall'].append(wall)
                for k in ('tree_sort', 'tree_stats'):
                    got[k].append(eng.kernel_time(k)[0])
        med = {k: float(np.median(v)) for k, v in got.items()}
        say('statistics  %s frames  tree_sort %8.3f ms  tree_stats %8.3f ms  (pcl_tree_accumulate, wall: %8.3f ms)'
            % (kind, med['tree_sort'], med['tree_stats'], med['wall']))
        stats = eng.tree_stats()
    say('statistics  %d of %d rows seen, %d frames' % (int((stats[0] > 0).sum()), R, int(stats[0].sum())))
    trees = {}
    for layout in a.roots:
        root_of, R0 = x['roots'][layout]
        dev, wall = [], []
        for r in range(a.repeats + 1):
            eng.kernel_time('tree_build')
            t0 = time.perf_counter()
            tree = eng.tree_build(x['event_ctx'], P, x['n_units'], x['q_member'], root_of, n_roots=R0, min_count=a.min_count, max_leaves=a.leaves,
                                  var_floor=a.var_floor)
            w = (time.perf_counter() - t0) * 1e3
            ms, launches = eng.kernel_time('tree_build')
            if r:
                dev.append(ms)
                wall.append(w)
        trees[layout] = tree
        say('build  roots = %-6s (%3d)  %d leaves, %d splits, %d launches  tree_build %9.3f ms  (pcl_tree_build, wall: %9.3f ms)'
            % (layout, R0, tree.n_states, len(tree.split_gain), launches, float(np.median(dev)), float(np.median(wall))))
    eng.close()
    if not a.no_twin:
        layout = a.roots[0]
        t0 = time.perf_counter()
        st = tw.accumulate(tw.zero(R, D), x['frames'], x['T'], x['begin'], x['frame_row'])
        t_acc = time.perf_counter() - t0
        same_n = bool(np.array_equal(st['n'], stats[0]))
        rel = float(np.max(np.abs(st['s'] - stats[1])) / np.max(np.abs(st['s'])))
        say('twin (NumPy, host CPU)  statistics %8.1f s  (n equal: %s, largest |s - s_twin| / max |s| = %.2e)' % (t_acc, same_n, rel))
        t, secs = twin_build(x, stats, layout, a)
        tree = trees[layout]
        same = all(np.array_equal(getattr(tree, f), t[f]) for f in ('node_cand', 'node_child', 'node_state', 'node_n', 'row_state'))
        worst = float(np.max(np.abs(tree.split_gain - t['split_gain']) / t['gain_B'])) if same and len(t['split_gain']) else float('nan')
        say('twin (NumPy, host CPU)  build, roots = %s: %8.1f s  (%d leaves; the device tree is the twin\'s: %s; largest |gain - gain_twin| / B = %.2e)'
            % (layout, secs, int((t['node_state'] >= 0).sum()), same, worst))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
