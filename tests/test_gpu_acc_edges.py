"""csrc/gmm_accumulate.hip held to the float64 oracle where tests/test_gpu_acc16_edges.py does not reach: the active-frame list builder
(acc_count* -> acc_scan_kernel -> acc_fill*) on ragged batches, the strict-f32 matrix-pipe kernel (gmm_accumulate_mfma_kernel, route
PCL_ROUTE_MFMA32 under PCL_SCORE_VARIANT=3) and the direct-form kernel (gmm_accumulate_kernel: f32 whole states, every PCL_F64 pass, the
subset launch of split states) at the edges of their own tilings.  tests/_acc_edge_cases.py makes the inputs and
tests/test_acc_edge_cases.py proves on the CPU that each sits on its edge and would show the defect it is aimed at.

Per case (tests/_acc_edge_run.py): load_model, load_frames, the batch, set_emissions with the ORACLE'S float64 ln b, set_posteriors with
the case's ln gamma, stats_zero, accumulate, stats_download; acc, alpha_acc, mean_acc, cov_acc of every state through _parity.hold under a
tag that names case and route.  Bounds are those of tests/test_gpu_accumulate.py: float64 rtol 1e-9, atol 1e-13 of the state's largest
entry; f32 routes rtol 1e-4, atol 1e-6 of the state's largest entry, + _parity.cov_acc_atol for cov_acc.  Routes, one module-scoped
engine per scoring variant (read when the context is created):
  PCL_F64                           every case                                                        (direct form, double)
  PCL_F32, PCL_SCORE_VARIANT=1      every case                                                        (direct form, float)
  PCL_F32, PCL_SCORE_VARIANT=3      every case whose padded D has a matrix-pipe instance, and every case of _acc16_cases unchanged
  PCL_F32, default variant          the ragged list-builder cases                                     (the f16 kernels have their own file)
The row form of the list builder is the default, so all of the above holds IT to the oracle; the last test runs the ragged cases in two
fresh processes, PCL_ACC_ROWS = 0 and 1, and asks for the same bits from the segment form.

MEASURED on the MI355X (largest share of a bound per route, over all cases): PCL_F64 6.2e-5 (dims D=64, cov_acc); f32 direct form 0.32
(dims D=64, cov_acc); f32 split-f16 on the list cases 0.067 (scan 1023, cov_acc); strict-f32 matrix pipe 0.32 (scale, cov_acc; 0.22 on
every other case).
FOUND AND FIXED: test_f16_ladder_on_the_f32_matrix_pipe[scale] had cov_acc at 1.0044 of its bound (max |d| 5.17e-5; acc and mean_acc of
the same case used 0.021).  State (a) of that case puts 32 frames per mixture at the mixture's own mean (sd 0.05), one to three units from
the state's centre: the kernel's f32 raw moments S2, S1, S0 are each ~ acc d^2 and the flush S2 - 2 d S1 + d^2 S0 cancels them to
acc . 0.0025, so the roundings of the running f32 sums are all that is left.  gmm_accumulate_mfma_kernel now keeps one accumulator set
per 16-frame half of a tile and adds the two in float64 at the flush: the same case uses 0.32."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _acc16_cases as ac
import _acc_edge_cases as ec
import _acc_edge_run as run
from _oracle_pool import f32_evaluation_bound_rows
from _parity import hold

pytestmark = pytest.mark.gpu
LIST, ALL, A16 = ec.list_cases(), ec.all_cases(), ac.all_cases()
PIPE = [(i, m) for i, m in ALL if i not in ('dims-48', 'dims-50', 'dims-64')]              # a matrix-pipe instance for the padded D
WORST = {}


def ids(cases):
    return [i for i, _ in cases]


def _engine(variant):
    e = run.engine_with_variant(variant)
    yield e
    e.close()


@pytest.fixture(scope='module')
def eng():
    yield from _engine(None)


@pytest.fixture(scope='module')
def eng1():
    yield from _engine(1)


@pytest.fixture(scope='module')
def eng3():
    yield from _engine(3)


def hold_case(c, st, prec, route):
    """Every state against the oracle; prints and returns the largest share of a bound that was used."""
    ref = ec.reference(ec.as_batch(c))
    tag = 'acc edges %s %s' % (c['name'], route)
    used = 0.0
    for j in range(c['mean'].shape[0]):
        if c['counts'][j] == 0:
            assert all(not np.any(st[k][j]) for k in ec.KEYS), '%s: empty state %d is not zero' % (tag, j)
            continue
        for k in ec.KEYS:
            rt, floor = ec.bounds(ec.as_batch(c), j, k, prec)
            if c['masked'] and prec == 'f32':                            # (_acc16_cases.masked: the bound of tests/test_gpu_acc16_edges.py)
                rt = 1e-4 + 4.0 * float(f32_evaluation_bound_rows([(c['mean'][j], c['var'][j], c['w'][j])], c['frames'][ac.survivors(c, j)]).max())
                assert rt <= 2.1e-3
            used = max(used, hold(tag, k, np.asarray(st[k][j]), np.asarray(ref[k][j]), rt, floor)['used'])
    assert (st['cov_acc'] >= 0.0).all(), tag
    WORST[route] = max(WORST.get(route, 0.0), used)
    print('%s: %.3g of the bound (worst on this route so far: %.3g)' % (tag, used, WORST[route]))
    return used


@pytest.mark.parametrize('mk', [m for _, m in ALL], ids=ids(ALL))
def test_statistics_f64(eng, mk):
    c = mk()
    hold_case(c, run.statistics(eng, c, 'f64'), 'f64', 'f64 direct')


def test_the_pipe_cases_are_all_but_the_direct_only_dimensions():
    assert [i for i, m in ALL if ec.route(3, 'f32', m()['mean'].shape[2]) == 3] == ids(PIPE) and len(PIPE) == len(ALL) - 3


@pytest.mark.parametrize('mk', [m for _, m in ALL], ids=ids(ALL))
def test_statistics_f32_direct_form(eng1, mk):
    c = mk()
    hold_case(c, run.statistics(eng1, c, 'f32'), 'f32', 'f32 direct')


@pytest.mark.parametrize('mk', [m for _, m in PIPE], ids=ids(PIPE))
def test_statistics_f32_matrix_pipe(eng3, mk):
    c = mk()
    assert ec.route(3, 'f32', c['mean'].shape[2]) == 3
    hold_case(c, run.statistics(eng3, c, 'f32'), 'f32', 'f32 mfma32')


@pytest.mark.parametrize('mk', [m for _, m in A16], ids=ids(A16))
def test_f16_ladder_on_the_f32_matrix_pipe(eng3, mk):
    """The cases of tests/_acc16_cases.py unchanged: survivor counts 0, 1, 31, 32, 33, 64, 65, ... through the two-stages-ahead gather, dead
    waves in the last slice, the subset launch over [0, n_good) for the ladder's split state."""
    c = mk()
    hold_case(c, run.statistics(eng3, c, 'f32'), 'f32', 'f32 mfma32')


@pytest.mark.parametrize('mk', [m for _, m in LIST], ids=ids(LIST))
def test_list_builder_default_route(eng, mk):
    c = mk()
    hold_case(c, run.statistics(eng, c, 'f32'), 'f32', 'f32 split16')


def test_conditioning_is_what_the_cases_claim(eng3):
    """The library's own classification: the split state's off-pipe mixtures, the ill-conditioned state as a whole."""
    for c in (ec.split(), ec.ill()):
        eng3.load_model(c['mean'], c['var'], c['w'])
        n_off, _ = eng3.model_split_info()
        assert n_off.tolist() == [int(ec.off_pipe(c['mean'][j], c['var'][j]).sum()) for j in range(3)]
    assert n_off.tolist() == [0, ec.ILL_M, 0]


def test_rows_and_segments_build_the_same_lists():
    """PCL_ACC_ROWS is read once per process: two fresh processes run the ragged cases under PCL_F64 and the default f32 route and print
    one digest of the four statistics arrays per case and route; the two outputs are the same, line for line."""
    outs = []
    for rows in ('0', '1'):
        r = subprocess.run([sys.executable, os.path.join(run.ROOT, 'tests', '_acc_edge_run.py')], env=dict(os.environ, PCL_ACC_ROWS=rows),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('DIGEST ')]
        assert len(lines) == 2 * len(LIST), r.stdout
        outs.append(lines)
    assert outs[0] == outs[1]
