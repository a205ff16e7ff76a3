"""The claims of tests/_acc_edge_cases.py, held on the CPU (tests/test_gpu_acc_edges.py runs the cases on the device).  A NumPy twin of
the list builder (count -> scan -> fill; _acc_edge_cases.twin_lists) turns every case into per-state lists; summed through the oracle they
must give the case's reference, which was computed another way (per occurrence of a state).  Every claim is re-derived from the inputs.
Sensitivity is a condition: with the defect a list case is aimed at applied to the twin -- the entry at the step boundary dropped, written
one slot early or filed with the previous segment, `>` in place of `>=`, the scan's chunk length off by one -- at least one statistic
moves by more than ten times the widest allowance the device test grants it (the f32 one)."""
import math

import numpy as np
import pytest

import _acc16_cases as ac
import _acc_edge_cases as ec
from _oracle_pool import f32_evaluation_bound_rows

LIST, SHAPE, ALL = ec.list_cases(), ec.shape_cases(), ec.all_cases()


def ids(cases):
    return [i for i, _ in cases]


def excess(c, got, prec='f32'):
    """Per state the largest |got - reference| in units of the device test's allowance."""
    ref, out = ec.reference(c), {}
    for j in range(c['mean'].shape[0]):
        worst = 0.0
        for k in ec.KEYS:
            rt, at = ec.bounds(c, j, k, prec)
            tol = at + rt * np.abs(ref[k][j])
            err = np.abs(np.asarray(got[k][j]) - ref[k][j])
            with np.errstate(divide='ignore', invalid='ignore'):
                r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
            worst = max(worst, float(np.max(r)))
        out[j] = worst
    return out


def test_the_case_count():
    assert len(LIST) == 6 and len(SHAPE) == 21 and len(ALL) == ec.N_CASES == 27
    assert len({mk()['name'] for _, mk in ALL} | {mk()['name'] for _, mk in ac.all_cases()}) == 27 + len(ac.all_cases())     # (the references are cached by name)


@pytest.mark.parametrize('mk', [m for _, m in ALL], ids=ids(ALL))
def test_case_is_well_formed(mk):
    c = mk()
    J, M, D = c['mean'].shape
    assert c['frames'].dtype == np.float64 and (c['frames'] + 100.0 > 0).all()
    assert len(c['rows']) == len(c['T']) == len(ec.lgammas(c)) and int(c['T'].sum()) == c['frames'].shape[0]
    assert np.array_equal(c['begin'], np.concatenate([[0], np.cumsum(c['T'][:-1])]))
    counts = np.zeros(J, dtype=np.int64)
    for u, (rows, lg) in enumerate(zip(c['rows'], ec.lgammas(c))):
        assert lg.shape == (len(rows), c['T'][u]) and rows[0] == ec.ENTRY and rows[-1] == ec.EXIT
        assert np.isneginf(lg[rows < 0]).all()
        fin = lg[np.isfinite(lg)]
        assert (fin <= 0.0).all() and (fin >= (ac.LG_LO if c['prune'] is None else -14.0)).all()        # (both precisions cut at the same frames)
        for n, st in enumerate(rows):
            if st >= 0:
                counts[st] += int((lg[n] >= ec.threshold(c)).sum())
    assert np.array_equal(counts, c['counts'])
    assert c['kind'] == 'shape' or (D == 13 and J <= 12 and max(c['T']) <= 130)
    assert c['kind'] == 'list' or c['frames'].shape[0] <= (40 if M > 288 else 130)
    for j in range(J):
        assert np.array_equal(np.flatnonzero(ec.off_pipe(c['mean'][j], c['var'][j])), c['split'].get(j, ()) if not c['claims'].get('valu_states') or j not in c['claims']['valu_states'] else np.arange(M)), j


@pytest.mark.parametrize('mk', [m for _, m in ALL], ids=ids(ALL))
def test_f32_evaluation_bound(mk):
    """What any f32 evaluation of a survivor's exponent may lose (a worst-case sum over the D dimensions, so it grows with D: 2.9e-5 at
    D = 64) stays under half of the 1e-4 the f32 routes are held to; the other half is the accumulation's."""
    c = mk()
    lists = ec.twin_lists(c)
    worst = 0.0
    for j, ent in lists.items():
        if ent:
            x = c['frames'][[e[0] for e in ent]]
            worst = max(worst, float(f32_evaluation_bound_rows([(c['mean'][j], c['var'][j], c['w'][j])], x).max()))
    assert worst <= 5e-5, worst


@pytest.mark.parametrize('mk', [m for _, m in ALL], ids=ids(ALL))
@pytest.mark.parametrize('form', ['rows', 'segs'])
def test_twin_lists_reproduce_the_reference(mk, form):
    """Ascending frames per segment, segments in state-sorted order; the sums of the lists equal the per-occurrence reference at the
    float64 allowance, and the list lengths are the case's counts."""
    c = mk()
    lists = ec.twin_lists(c, form)
    for j in range(c['mean'].shape[0]):
        assert len(lists.get(j, [])) == c['counts'][j]
    assert np.array_equal(sorted(lists), sorted({int(s) for r in c['rows'] for s in r if s >= 0}))
    ex = excess(c, ec.stats_of_lists(c, lists), 'f64')
    assert max(ex.values()) <= 1.0, ex
    assert ec.twin_lists(c, form, prec='f64') == lists                    # PCL_F64 cuts at 2^-1076: the same survivors


@pytest.mark.parametrize('mk', [m for _, m in LIST], ids=ids(LIST))
def test_list_case_shows_its_defects(mk):
    c = mk()
    assert c['defects'] and set(c['defects']) <= set(ec.DEFECTS)
    for defect in c['defects']:
        for form in ('rows', 'segs'):
            if defect in ('drop', 'early', 'prev') and not ec.boundary_owners(c, form):
                assert form == 'segs' and max(c['T']) <= 64, 'no survivor on the %d-frame step' % ec.STEP[form]
                continue
            ex = excess(c, ec.stats_of_lists(c, ec.twin_lists(c, form, defect)))
            assert max(ex.values()) > 10.0, (defect, form, ex)
            if defect == 'drop':                                         # every state that owns such an entry shows its loss
                assert all(ex[j] > 10.0 for j in ec.boundary_owners(c, form)), (form, ex)
    covered = {d for _, m in LIST for d in m()['defects']}
    assert covered == set(ec.DEFECTS)


def test_ragged_claims():
    for c in (ec.ragged(), ec.labels()):
        cl = c['claims']
        assert [int(t) for t in c['T']] == cl['T'] and [len(r) for r in c['rows']] == cl['N']
        assert [-(-len(r) // ec.ROW_GROUP) for r in c['rows']] == cl['wave_groups'] and [-(-len(r) // ec.ROW_BLOCK) for r in c['rows']] == cl['row_blocks']
        assert [(u, n) for u, r in enumerate(c['rows']) for n in range(1, len(r) - 1) if r[n] < 0] == cl['inner_virtual_rows']
        seen = {}
        for (u, n), p in c['patterns'].items():
            t = np.flatnonzero(np.isfinite(c['lgamma'][u][n]))
            assert np.array_equal(t, ec.pattern_frames(p, int(c['T'][u])))
            seen.setdefault(p if not (p == 'mid' and c['T'][u] < 66) else 'every', []).append((u, n))
        assert set(seen) == cl['patterns']
        assert any(np.array_equal(np.flatnonzero(np.isfinite(c['lgamma'][u][n])), [63, 64, 65]) for u, n in seen['mid'])
        # a segment without a survivor between two rows that keep frames, not at the edge of its wave group
        assert any(0 < n % 8 < 7 and c['rows'][u][n - 1] >= 0 and c['rows'][u][n + 1] >= 0 and c['patterns'][(u, n - 1)] != 'none' and c['patterns'][(u, n + 1)] != 'none'
                   and c['rows'][u][n] != ec.EMPTY_STATE for u, n in seen['none'])
        assert c['counts'][cl['empty_state']] == 0 and any((r == cl['empty_state']).any() for r in c['rows'])
        segs = ec.segments(c)
        per_state = np.bincount([s[0] for s in segs], minlength=12)
        assert per_state.max() >= 4 and any(sum(1 for s in segs if s[0] == j and s[1] == u) >= 2 for j in range(12) for u in range(len(c['T'])))
        # survivors on the 64-frame step of the segment form and the 8-frame step of the row form, in first and in later segments of a state
        assert ec.boundary_owners(c, 'segs') and len(ec.boundary_owners(c, 'rows')) >= 6
    c = ec.ragged()
    assert set(ec.RAGGED_T) == {1, 7, 8, 9, 63, 64, 65, 129} and set(ec.RAGGED_N) == {3, 8, 9, 32, 33, 34}
    assert [len(l) for l in ec.LABELS] == [1, 2, 10, 11] and [3 * len(l) + 2 for l in ec.LABELS] == ec.labels()['claims']['N']
    for u, l in enumerate(ec.LABELS):                                     # the rows are what pcl_batch_create_labels derives
        assert np.array_equal(ec.labels()['rows'][u][1:-1], np.repeat(np.asarray(l) * 3, 3) + np.tile(np.arange(3), len(l)))


@pytest.mark.parametrize('n_segs', ec.SCAN_SEGS)
def test_scan_claims(n_segs):
    c = ec.scan(n_segs)
    segs = ec.segments(c)
    assert len(segs) == n_segs == c['claims']['n_segs'] and set(c['T']) == {4}
    assert c['claims']['per'] == -(-n_segs // ec.SCAN_THREADS) == {1023: 1, 1025: 2, 2049: 3}[n_segs]
    kept = [k for k, (j, u, n) in enumerate(segs) if np.isfinite(c['lgamma'][u][n]).any()]
    assert kept == c['claims']['kept_segments']
    edges = {0, n_segs - 1} | {k for e in range(ec.SCAN_THREADS, n_segs, ec.SCAN_THREADS) for k in (e - 1, e)}
    assert edges <= set(kept) and len(kept) >= 40
    assert n_segs - (n_segs // ec.SCAN_THREADS) * ec.SCAN_THREADS >= 1 or n_segs < ec.SCAN_THREADS     # the rounded-down chunk length leaves segments out


def test_prune_claims():
    c = ec.prune()
    thr = c['claims']['thr']
    assert thr == -20.0 * ac.LN2 == ec.threshold(c) == ec.threshold(c, 'f64') and c['prune'] == -20.0
    vals = np.concatenate([c['lgamma'][u][n] for j, u, n in ec.segments(c) if j == 0])
    assert len(vals) == sum(c['claims']['T']) and (np.abs(vals / thr - 1.0) < 2e-12).all()
    assert int((vals == thr).sum()) == c['claims']['at_thr'] and int((vals >= thr).sum()) == c['claims']['kept'] == c['counts'][0]
    assert int((vals < thr).sum()) == len(vals) - c['claims']['kept'] > 50
    others = np.concatenate([c['lgamma'][u][n] for j, u, n in ec.segments(c) if j != 0])
    assert (others[np.isfinite(others)] > ac.LG_LO - 1e-12).all()
    assert math.isclose(ec.reference(c)['alpha_acc'][0], c['claims']['kept'] * 2.0 ** -20, rel_tol=1e-10)


@pytest.mark.parametrize('mk', [m for _, m in SHAPE], ids=ids(SHAPE))
def test_shape_claims(mk):
    c = mk()
    J, M, D = c['mean'].shape
    cl = c['claims']
    assert cl['padded_D'] == min(x for x in (13, 26, 39, 47, 48, 64) if x >= D)
    assert cl['route3'] == (3 if cl['padded_D'] <= 47 else 1) == ec.route(3, 'f32', D) and ec.route(1, 'f32', D) == 1 and ec.route(3, 'f64', D) == 1
    assert cl['Mpad'] == -(-M // 4) * 4 and cl['n_mtiles'] == -(-M // 32)
    assert cl['direct_slices'] == -(-cl['Mpad'] // 256) and cl['nslice'] == -(-cl['n_mtiles'] // 8)
    assert cl['direct_last_live'] == cl['Mpad'] - 256 * (cl['direct_slices'] - 1) and cl['mfma_last_live'] == cl['n_mtiles'] - 8 * (cl['nslice'] - 1)
    assert c['rows'][0].tolist() == [-1] + list(range(J)) + [-2]
    assert ec.accumulate_order(c) == cl.get('order', list(range(J)))


def test_shape_ladders():
    assert ec.SHAPE_M == [1, 33, 224, 255, 256, 257, 288]
    t = {m: ec.tilings(m) for m in ec.SHAPE_M}
    assert [t[m]['n_mtiles'] for m in (224, 255, 256, 257, 288)] == [7, 8, 8, 9, 9] and t[257]['nslice'] == 2 and t[257]['mfma_last_live'] == 1
    assert [t[m]['direct_slices'] for m in ec.SHAPE_M] == [1, 1, 1, 1, 1, 2, 2] and (t[257]['direct_last_live'], t[288]['direct_last_live']) == (4, 32)
    assert t[255]['Mpad'] == 256 and t[33]['Mpad'] == 36 and t[1]['Mpad'] == 4                     # padded lanes beside live ones
    assert set(ec.SHAPE_COUNTS) == {3, ec.FC + 1, 2 * ec.FC + 1}
    assert ec.WIDE == [(1793, 8), (1793, 9), (2048, 8), (2048, 9)]
    for M, J in ec.WIDE:
        c = ec.wide(M, J)
        assert c['claims']['nslice'] == 8 and c['frames'].shape[0] == 40 and c['mean'].shape[2] == 13
        blocks = ec.mfma32_blocks(M, J)
        assert len(blocks) == c['claims']['grid'] == (64 if J == 8 else 128) and c['claims']['dead_blocks'] == (0 if J == 8 else 56)
        live = [b for b in blocks if b is not None]
        assert sorted(live) == [(w, s) for w in range(J) for s in range(8)]                        # every (state, slice) once
        assert all(w % 8 == i % 8 for i, b in enumerate(blocks) if b for w in [b[0]])             # a state's slices share a residue mod 8
        assert c['claims']['mfma_last_live'] == (1 if M == 1793 else 8)
        assert {0, 1, 2, 3, 31, 32, 33, 40} <= set(c['counts'].tolist())
    assert ec.SHAPE_D == [13, 14, 39, 40, 47, 48, 50, 64]
    assert [ec.dims(d)['claims']['padded_D'] for d in ec.SHAPE_D] == [13, 26, 39, 47, 47, 48, 64, 64]
    assert [ec.dims(d)['claims']['route3'] for d in ec.SHAPE_D] == [3, 3, 3, 3, 3, 1, 1, 1]
    c = ec.split()
    assert c['split'] == {1: (2, 68)} and 2 < 32 and 68 >= 64 and c['claims']['n_mtiles'] == 3 and not ec.uses_valu(c, 1)
    c = ec.ill()
    assert [ec.uses_valu(c, j) for j in range(3)] == [False, True, False] and c['claims']['order'] == [0, 2, 1]
    assert ec.off_pipe(c['mean'][1], c['var'][1]).all()


def test_reference_is_shared_and_read_only():
    c = ec.ragged()
    r = ec.reference(c)
    assert ec.reference(c) is r and not r['acc'].flags.writeable
    np.testing.assert_allclose(r['acc'].sum(axis=1), r['alpha_acc'], rtol=1e-10)
    want = sum(float(np.exp(lg[np.isfinite(lg)]).sum()) for lg in c['lgamma'])
    assert math.isclose(r['alpha_acc'].sum(), want, rel_tol=1e-12)
