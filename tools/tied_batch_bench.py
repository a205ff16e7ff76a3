"""Time of making one batch over tied states by the two routes (row f17, csrc/tying.hip), on the same corpus and the same machine:

  host route    Tree.unit_state_ids per utterance (a Python walk per label position and state position) +
                make_sentence_batch(unit_state_ids=): dense per-utterance matrices built on the host, pcl_batch_create +
                pcl_batch_set_transitions + pcl_batch_set_states
  device route  Engine.label_batch(tied=True): pcl_batch_create_labels_tied, the walks on the device

    python tools/tied_batch_bench.py [--utts 8192] [--min-len 20] [--max-len 60] [--frames 100] [--dim 13] [--units 40] [--questions 60]
                                     [--leaves 2000] [--repeats 3] [--out FILE]

The corpus is synthetic: --utts labels of --min-len .. --max-len units; the tree is grown by Engine.tree_build from statistics of
synth.py frames (one frame row per statistics row drawn uniformly, scattering around a mean that depends on the context), one root per
state position.  Each route runs once uncounted (allocations, page faults), then --repeats times; the median wall time of the whole
route is reported, the host route's two halves separately, and pcl_kernel_time("tying") of the device route's kernel (HIP events).  The
two batches' row -> state maps are compared."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grow_tree(eng, a, rng):
    from poccala_amd import synth
    from poccala_amd.AcousticModel.ContextTree import questions
    nu, P, D = a.units, 3, a.dim
    every = np.array([(l, c, r) for l in range(nu + 1) for c in range(nu) for r in range(nu + 1)], dtype=np.int32)
    event_ctx = every[np.sort(rng.choice(len(every), size=min(20000, len(every)), replace=False))]
    R = len(event_ctx) * P
    F = 8 * R
    frames, _, _ = synth.make_frames(1, F, D, seed=3, ragged=False)
    frame_row = rng.integers(0, R, size=F).astype(np.int32)
    ev = event_ctx[frame_row // P]
    shift = rng.standard_normal((3, nu + 1, D))
    frames = (np.asarray(frames[:F], dtype=np.float32) + 1.5 * shift[0][ev[:, 0]] + 2 * shift[1][ev[:, 1]] + 0.5 * shift[2][ev[:, 2]]
              + 0.25 * (frame_row % P)[:, None]).astype(np.float32)
    sets = []
    while len(sets) < a.questions:
        m = rng.integers(0, 2, size=nu + 1)
        if 0 < m.sum() <= nu:
            sets.append(np.flatnonzero(m).tolist())
    eng.load_frames(frames)
    eng.tree_zero(R)
    eng.tree_accumulate(np.array([F], dtype=np.int32), np.array([0], dtype=np.int64), frame_row)
    return eng.tree_build(event_ctx, P, nu, questions(sets, nu), np.tile(np.arange(P, dtype=np.int32), nu), min_count=8, max_leaves=a.leaves, install=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=8192)
    ap.add_argument('--min-len', type=int, default=20)
    ap.add_argument('--max-len', type=int, default=60)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--dim', type=int, default=13)
    ap.add_argument('--units', type=int, default=40)
    ap.add_argument('--questions', type=int, default=60)
    ap.add_argument('--leaves', type=int, default=2000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from poccala_amd import Engine, synth
    from poccala_amd.engine import make_sentence_batch
    rng = np.random.default_rng(0)
    S = 5
    eng = Engine(0)
    trans = np.stack([synth.random_left_right_transmat(rng, S) for _ in range(a.units)])
    eng.load_units(trans)
    tree = grow_tree(eng, a, rng)
    eng.load_tying(tree)
    U = a.utts
    labels = [rng.integers(0, a.units, size=int(rng.integers(a.min_len, a.max_len + 1))).astype(np.int32) for _ in range(U)]
    lens = np.full(U, a.frames, dtype=np.int32)
    begin = np.zeros(U, dtype=np.int64)                           # (the batches are only made here: every utterance may read the same rows)
    eng.load_frames(np.zeros((a.frames, a.dim), dtype=np.float32))
    n_pos = int(sum(len(l) for l in labels))
    lines = ['tied_batch_bench: %s' % eng.device_info(),
             'corpus: %d utterances, %d label positions (%d .. %d a label), P = 3: %d walks; tree: %d nodes, %d tied states, Q = %d'
             % (U, n_pos, a.min_len, a.max_len, 3 * n_pos, tree.n_nodes, tree.n_states, tree.Q)]
    host, host_ids, host_batch, dev, kern = [], [], [], [], []
    rows_h = rows_d = None
    eng.enable_timing(True)
    for r in range(a.repeats + 1):
        t0 = time.perf_counter()
        ids = [tree.unit_state_ids(l) for l in labels]
        t1 = time.perf_counter()
        hb, _ = make_sentence_batch(eng, labels, lens, begin, trans, S, unit_state_ids=ids)
        eng.sync()
        t2 = time.perf_counter()
        if rows_h is None:
            rows_h = np.concatenate(hb.row_states())
        hb.close()
        eng.kernel_time('tying')
        t3 = time.perf_counter()
        db = eng.label_batch(labels, lens, begin, tied=True)
        eng.sync()
        t4 = time.perf_counter()
        k = eng.kernel_time('tying')
        if rows_d is None:
            rows_d = np.concatenate(db.row_states())
        db.close()
        if r:                                                     # the first run allocates
            host.append(t2 - t0), host_ids.append(t1 - t0), host_batch.append(t2 - t1), dev.append(t4 - t3), kern.append(k)
    med = lambda x: float(np.median(x))
    lines.append('row -> state maps of the two routes equal: %s (%d rows)' % (bool(np.array_equal(rows_h, rows_d)), rows_h.size))
    lines.append('host route,   median of %d: %.3f s  (Tree.unit_state_ids %.3f s + make_sentence_batch(unit_state_ids=) %.3f s)'
                 % (a.repeats, med(host), med(host_ids), med(host_batch)))
    lines.append('device route, median of %d: %.4f s  (Engine.label_batch(tied=True), wall); pcl_kernel_time("tying") = %s ms'
                 % (a.repeats, med(dev), kern))
    lines.append('ratio host / device: %.1f' % (med(host) / med(dev)))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    eng.close()


if __name__ == '__main__':
    main()
