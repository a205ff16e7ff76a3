"""Walk every owner of device memory in the host runtime at the smallest shapes that reach them, twice in one process, and print the pool's
books as one JSON line (tests/test_gpu_ownership.py asserts on it; run with PCL_DESTROY_SYNC=1 so that block reuse does not depend on timing).

Model: 3 units of S = 5 (J = 9), M = 4, D = 13.  Utterances: T = 7, 12, 1 (the one-frame utterance is the known edge), labels of one or two
units, one of them naming a unit twice (duplicate rows).  Every refused call is refused by host-side validation before any launch."""
import json
import sys
import os

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poccala_amd import Engine, PCL_F32, PCL_F64, synth                       # noqa: E402
from poccala_amd._lib import PoccalaHipError                                   # noqa: E402

UNITS, M, D, S = 3, 4, 13, 5
LENS = np.array([7, 12, 1], dtype=np.int32)
BEGIN = np.array([0, 7, 19], dtype=np.int64)
LABELS = [[0, 0], [1, 2], [2]]


def refused(call, what, out):
    """`call` must raise the library's error and leave the number of handed-out blocks where it was."""
    before = Engine.pool_stats()['handed_out_blocks']
    try:
        call()
        out['refused'].append(dict(what=what, raised=False))
        return
    except PoccalaHipError as e:
        code = e.code
    out['refused'].append(dict(what=what, raised=True, code=code, blocks_before=before, blocks_after=Engine.pool_stats()['handed_out_blocks']))


def walk(out):
    rng = np.random.default_rng(5)
    mean, var, w, trans = synth.make_model(UNITS, M, D, seed=3)
    J = mean.shape[0]
    frames = rng.standard_normal((20, D)).astype(np.float32)
    eng = Engine(0)
    # refused before the context holds a model: a non-positive variance
    bad_var = var.copy()
    bad_var[1, 2, 3] = 0.0
    refused(lambda: eng.load_model(mean, bad_var, w), 'model with a non-positive variance', out)
    # 1. model, units, frames
    eng.load_model(mean, var, w)
    eng.load_units(np.stack(trans))
    eng.load_frames(frames)
    refused(lambda: eng.batch([3, 0, 3], LENS, BEGIN), 'batch with N = 0', out)
    plain = eng.batch([3], [5], [0])
    refused(lambda: plain.set_states([np.array([-1, J, -2], dtype=np.int32)]), 'set_states with a state id of J', out)
    plain.close()
    # 2. label batch   3. score in both precisions
    b = eng.label_batch(LABELS, LENS, BEGIN)
    b.score(PCL_F32)
    b.score(PCL_F64)
    # 4. forward-backward, Viterbi, asynchronous fetch (ksai_nz among the results), accumulate, M-step
    b.forward_backward()
    b.viterbi()
    bufs = b.result_buffers()
    b.fetch_async(bufs)
    b.fetch_wait()
    eng.stats_zero()
    b.accumulate(PCL_F32)
    eng.mstep()
    # 5. regroup
    row_unit = []
    for lab in LABELS:
        rep = np.repeat(np.asarray(lab, dtype=np.int32), S - 2)
        row_unit.append(np.concatenate([[rep[0]], rep, [rep[-1]]]).astype(np.int32))
    b.score(PCL_F32)
    b.viterbi()
    b.regroup(row_unit, S - 2)
    # 6. realignment into a segment set, one k-means sweep, one EM iteration
    seg, dropped = b.align_segments()
    seg.kmeans(2, seed=1, max_sweeps=1)                            # (two mixtures: the states the paths gave two frames or more are trained)
    seg.em(max_iters=1)
    seg.close()
    # 7. lexicon and one decode (the two utterances of more than one frame)
    tree, _ = synth.make_pronunciation_tree(0, UNITS, seed=1)
    eng.load_lexicon(tree)
    ab = eng.all_state_batch(LENS[:2], BEGIN[:2])
    ab.score(PCL_F32)
    ab.decode(candidate=2, max_tokens=64)
    ab.close()
    b.close()
    # 8. front-end: half a second of int16 PCM at 16 kHz
    pcm = (3000.0 * np.sin(np.arange(8000) * 0.05) + 200.0 * rng.standard_normal(8000)).astype(np.int16)
    eng.frontend([pcm], 16000, d1=False, d2=False)                 # (13 cepstra, no deltas: the model's dimension, which the flat start checks)
    # 9. flat start   10. a model of another J (the old one goes)
    eng.flat_start_model(J, M, np.zeros(D), np.ones(D))
    mean2, var2, w2, _ = synth.make_model(2, M, D, seed=4)
    eng.load_model(mean2, var2, w2)
    # 11. streaming slots, twice
    for _ in range(2):
        eng.stage_frames(frames)
        eng.swap_frames()
    eng.close()


def main():
    out = dict(refused=[], walks=[])
    for _ in range(2):
        before = Engine.pool_stats()
        walk(out)
        after = Engine.pool_stats()
        out['walks'].append(dict(device_allocs_before=before['device_allocs'], device_waits_before=before['device_waits'], **after))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
