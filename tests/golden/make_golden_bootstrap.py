#!/usr/bin/env python3
"""Golden G20: the two model-free steps the reference's training schemes begin with, made by RUNNING the reference.

    python tests/golden/make_golden_bootstrap.py        # rewrites tests/golden/G20_bootstrap.npz

Like make_golden.py this imports the reference and therefore runs in the build container only; the .npz holds data (inputs and
the reference's outputs), no source text.
  (a) flat start: AcousticModel.__flat_start (AcousticModel.py:479-517) through its mangled name, with __load_audio replaced by a
      function that hands out fixture matrices, __save_parameter replaced by one that captures the GMM parameters, np.random.seed
      and random.seed fixed, and np.random.random wrapped so that the coefficient draw is recorded.  A ragged corpus of 9
      utterances (one of 2 frames, shorter than step 3), D = 5 with feature 4 below the 1e-4 variance floor, proportion 0.6
      (int(5.4) = 5: truncates), step in {1, 3}, differentiation on and off: cases fs0 .. fs3.
  (b) uniform segmentation: __eq_segment(mode='e') with __save_data recording, then __get_gmmdata per unit, for state_num 5 and 4.
      The first data column is the global row number, so the owner state of every row is read back from where the row ended up.
      T not divisible by L, chunk not divisible by S-2, chunk < S-2, T < L, a repeated unit (apart and adjacent): cases us5, us4.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import RecLog, import_reference  # noqa: E402

FS_LENS = [17, 40, 5, 2, 33, 21, 8, 50, 12]
FS_D, FS_M, FS_UNITS = 5, 3, ['a', 'b']
FS_CASES = [dict(step=1, diff=True, coefficient=1.0, seed=11), dict(step=3, diff=True, coefficient=0.5, seed=12),
            dict(step=1, diff=False, coefficient=1.0, seed=13), dict(step=3, diff=False, coefficient=1.0, seed=14)]
FS_PROPORTION = 0.6

US_T = [23, 10, 3, 7, 30, 0 + 9]
US_GAP = [0, 2, 0, 5, 1, 0]                 # rows of the frame matrix left out in front of every utterance
US_LABELS = [['a', 'b', 'a', 'c'], ['b', 'c'], ['a', 'b', 'c', 'a'], ['c', 'a', 'b'], ['c', 'c'], ['d']]
US_UNITS = ['a', 'b', 'c', 'd', 'e']        # 'e' never occurs


def flat_start_cases(AcousticModel, scratch, out):
    rng = np.random.default_rng(20)
    corpus = []
    for n in FS_LENS:
        x = rng.standard_normal((n, FS_D)) * np.array([1.0, 2.5, 0.3, 4.0, 1e-3]) + np.array([0.5, -3.0, 10.0, 0.0, 2.0])
        corpus.append(x)
    out['fs_lens'] = np.array(FS_LENS)
    out['fs_frames'] = np.concatenate(corpus, axis=0)
    out['fs_proportion'] = np.float64(FS_PROPORTION)
    out['fs_n_cases'] = np.int64(len(FS_CASES))
    os.makedirs(os.path.join(os.environ['parameters_file_path'], 'XIF_tone'), exist_ok=True)
    for c, case in enumerate(FS_CASES):
        am = AcousticModel(RecLog(), 'XIF_tone', processes=1, console=False, state_num=5, mix_level=FS_M, dct_num=FS_D, delta_1=False, delta_2=False)
        setattr(am, '_AcousticModel__loaded_units', list(FS_UNITS))
        setattr(am, '_AcousticModel__load_audio', lambda path: corpus[path].copy())
        captured = []

        def save_parameter(unit, hmm):
            for g in hmm.profunction[1:-1]:
                captured.append((np.array(g.mean), np.array([np.diag(cv) for cv in g.covariance]), np.array(g.alpha)))
        setattr(am, '_AcousticModel__save_parameter', save_parameter)
        am.delete_trainInfo = lambda: None
        draws = []
        inner = np.random.random

        def recording(*a, **k):
            r = inner(*a, **k)
            draws.append(np.array(r))
            return r
        np.random.seed(case['seed'])
        random.seed(case['seed'])
        np.random.random = recording
        try:
            getattr(am, '_AcousticModel__flat_start')([[u] for u in range(len(corpus))], len(corpus), proportion=FS_PROPORTION, step=case['step'],
                                                      differentiation=case['diff'], coefficient=case['coefficient'])
        finally:
            np.random.random = inner
        assert len(captured) == len(FS_UNITS) * 3
        if case['diff']:
            # the two draws of :508-509 come first; the GMM constructors of init_unit (:511) draw their throw-away parameters after them
            assert len(draws) >= 2 and draws[0].shape == (FS_M, 1) and draws[1].shape == (FS_M, 1)
            coeff = ((draws[0] - draws[1]) * case['coefficient'])[:, 0]
        else:
            coeff = np.zeros(FS_M)
        out['fs%d_step' % c] = np.int64(case['step'])
        out['fs%d_diff' % c] = np.int64(case['diff'])
        out['fs%d_coeff' % c] = coeff
        out['fs%d_mean' % c] = np.stack([m for m, _, _ in captured])          # (J, M, D)
        out['fs%d_var' % c] = np.stack([v for _, v, _ in captured])
        out['fs%d_weight' % c] = np.stack([w for _, _, w in captured])
        print('fs%d: step %d, diff %s: J = %d, var = %s' % (c, case['step'], case['diff'], len(captured), captured[0][1][0]))


def uniform_cases(AcousticModel, out):
    T, begin, F = np.array(US_T), [], 0
    for t, gap in zip(US_T, US_GAP):
        F += gap
        begin.append(F)
        F += t
    F += 4                                                                  # rows behind the last utterance
    idx = {u: i for i, u in enumerate(US_UNITS)}
    out['us_T'], out['us_begin'], out['us_F'] = T, np.array(begin), np.int64(F)
    out['us_label_len'] = np.array([len(l) for l in US_LABELS])
    out['us_labels'] = np.array([idx[u] for l in US_LABELS for u in l])
    out['us_n_units'] = np.int64(len(US_UNITS))
    for sn in (5, 4):
        am = AcousticModel(RecLog(), 'XIF_tone', processes=1, console=False, state_num=sn)
        saved = {}
        setattr(am, '_AcousticModel__save_data', lambda unit, unit_data: saved.setdefault(unit, []).append(np.array(unit_data)))
        eq_segment = getattr(am, '_AcousticModel__eq_segment')
        get_gmmdata = getattr(am, '_AcousticModel__get_gmmdata')
        for u, lab in enumerate(US_LABELS):
            data = np.stack([np.arange(begin[u], begin[u] + T[u], dtype=np.float64), np.full(T[u], float(u))], axis=1)
            eq_segment(data, lab, mode='e')
        state = np.full(F, -1, dtype=np.int32)
        for unit, blocks in saved.items():
            g = get_gmmdata(blocks)
            assert len(g) == sn - 2
            for k in range(sn - 2):
                rows = np.asarray(g[k]).reshape(-1, 2)[:, 0].astype(np.int64)
                assert np.all(state[rows] == -1)
                state[rows] = idx[unit] * (sn - 2) + k
        out['us%d_frame_state' % sn] = state
        print('us%d: %d of %d rows used' % (sn, int((state >= 0).sum()), F))


def main():
    scratch, _, _, _, AcousticModel = import_reference()
    out = {}
    flat_start_cases(AcousticModel, scratch, out)
    uniform_cases(AcousticModel, out)
    np.savez_compressed(os.path.join(HERE, 'G20_bootstrap.npz'), **out)
    print('G20_bootstrap.npz:', len(out), 'arrays')


if __name__ == '__main__':
    main()
