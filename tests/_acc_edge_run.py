"""Running a case of tests/_acc_edge_cases.py (or of tests/_acc16_cases.py) on an engine: shared by tests/test_gpu_acc_edges.py and by the
child processes of its row-form / segment-form comparison.  As a program (python tests/_acc_edge_run.py): the ragged list-builder cases under
PCL_F64 and the default f32 route, one line `DIGEST <case> <route> <sha256 of acc, alpha_acc, mean_acc, cov_acc>` each; PCL_ACC_ROWS is read
once per process by the library, so the caller starts one process per setting."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import _acc_edge_cases as ec  # noqa: E402

KEYS = ec.KEYS


def engine_with_variant(variant):
    """An engine whose context read PCL_SCORE_VARIANT = variant (None: the default); the environment is left as it was."""
    from poccala_amd import Engine
    old = os.environ.get('PCL_SCORE_VARIANT')
    if variant is not None:
        os.environ['PCL_SCORE_VARIANT'] = str(variant)
    try:
        return Engine(0)
    finally:
        if variant is not None:
            if old is None:
                del os.environ['PCL_SCORE_VARIANT']
            else:
                os.environ['PCL_SCORE_VARIANT'] = old


def statistics(eng, c, prec):
    """load_model, load_frames, the batch (a label batch, or the row -> state maps), the ORACLE'S ln b and the case's ln gamma, stats_zero,
    accumulate, stats_download."""
    from poccala_amd import PCL_F32, PCL_F64, synth
    c = ec.as_batch(c)
    P = PCL_F32 if prec == 'f32' else PCL_F64
    eng.load_model(c['mean'], c['var'], c['w'])
    eng.load_frames(c['frames'])
    if c['labels'] is not None:
        eng.load_units(np.stack([synth.flat_start_transmat()] * (c['mean'].shape[0] // 3)))
        b = eng.label_batch(c['labels'], c['T'], c['begin'])
    else:
        b = eng.batch([len(r) for r in c['rows']], c['T'], c['begin'])
        b.set_states(c['rows'])
    try:
        b.score(P)
        b.set_emissions(ec.emissions(c))
        b.set_posteriors(ec.lgammas(c))
        if c['prune'] is not None:
            eng.accumulate_prune(c['prune'])
        try:
            eng.stats_zero()
            b.accumulate(P)
            return eng.stats_download()
        finally:
            eng.accumulate_prune(-1e300)
    finally:
        b.close()


def digest(st):
    h = hashlib.sha256()
    for k in KEYS:
        h.update(np.ascontiguousarray(st[k], dtype=np.float64).tobytes())
    return h.hexdigest()


def main():
    eng = engine_with_variant(None)
    try:
        for cid, mk in ec.list_cases():
            for prec in ('f64', 'f32'):
                print('DIGEST %s %s %s' % (cid, prec, digest(statistics(eng, mk(), prec))), flush=True)
    finally:
        eng.close()


if __name__ == '__main__':
    main()
