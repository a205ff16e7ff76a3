"""The cases of tests/_mbr_cases.py carry what they claim, in NumPy and the twin alone: the degrees that select hmm_mbr_kernel<2> or <0>,
the -inf patterns the holes are there for, what an impossible utterance gives, the identities tests/test_gpu_mbr_edges.py holds the
device to (so that a failure there points at the device), every path one by one for a small case with holes, and the size of the batch
that is to send mbr_post_kernel round its grid-stride loop.  No GPU."""
import math

import numpy as np
import pytest

import _mbr_cases as mc
import _mbr_twin as tw
from _mbr_cases import CASES


def twins_of(case, combo, ld=False):
    kappa, group, refkind = combo
    refs = mc.refs_of(case, refkind)
    n = 2 if case['name'] == 'stride' else len(case['utts'])
    return [mc.twin_of((case['name'], u) + tuple(combo), case['utts'][u], refs[u], kappa, group, ld=ld) for u in range(n)], refs


@pytest.mark.parametrize('name', mc.NAMES)
def test_the_degrees_select_the_lists_the_case_is_meant_for(name):
    case = CASES[name]
    indeg, outdeg = mc.degrees(case['utts'][:8])
    print('%s: max in-degree %d, out-degree %d' % (name, indeg, outdeg))
    assert (indeg <= 2 and outdeg <= 2) == case['register']
    assert case['register'] == (case['kind'] == 'chain')
    for la, lpi, rows, B in case['utts'][:8]:
        n = len(rows)
        assert la.shape == (n, n) and lpi.shape == (n,) and B.shape[0] == n and rows[0] == -1 and rows[-1] == -2
        assert (B[0] == 0).all() and np.isneginf(B[-1]).all() and ((rows[1:-1] >= 0) & (rows[1:-1] < mc.J)).all()
        if not case['holes']:
            assert np.isfinite(B[:-1]).all()


def test_the_shapes_are_the_ones_the_kernel_branches_at():
    shapes = lambda name: [u[3].shape for u in CASES[name]['utts']]
    for kind in ('chain', 'dense'):
        got = shapes(kind + '_waves') + shapes(kind + '_big')
        assert {n for n, _ in got} == {127, 128, 129, 256, 257, 1023, 1024, 3}
        assert {t for _, t in got} == ({1, 2, 3, 5})
        assert (1024, 5 if kind == 'chain' else 3) in got and (3, 5) in shapes(kind + '_big')
        assert all(t <= 3 for n, t in got if kind == 'dense' and n > 257)
        assert [s for s in shapes(kind + '_holes')] == [(5, 9), (66, 9), (130, 9)]
    assert any(t == 1 for _, t in shapes('chain_waves')) and any(t == 5 for _, t in shapes('chain_waves'))
    mixed = CASES['mixed']['utts']
    assert all(x is y for a, b in zip(mixed, CASES['chain_waves']['utts']) for x, y in zip(a, b))      # the same arrays, not copies of them
    assert len(mixed) == len(CASES['chain_waves']['utts']) + 1 and mixed[-1][3].shape == (65, 3)
    assert mc.degrees(mixed[:-1]) == (2, 2) and max(mc.degrees(mixed[-1:])) > 2
    assert shapes('imp_chain64')[mc.IMP_AT] == (64, 6) and shapes('imp_chain130')[mc.IMP_AT] == (130, 6) and shapes('imp_dense130')[mc.IMP_AT] == (130, 6)
    assert all(len(CASES[n]['utts']) == 4 for n in mc.IMPOSSIBLE)


@pytest.mark.parametrize('name', ('chain_holes', 'dense_holes', 'brute_holes'))
def test_holes_leave_a_finite_likelihood_and_rows_without_a_path(name):
    case = CASES[name]
    for combo in case['combos']:
        twins, _ = twins_of(case, combo)
        for u, (t64, _) in enumerate(twins):
            la, lpi, rows, B = case['utts'][u]
            n, T = B.shape
            assert np.isneginf(B[1:-1]).any() and np.isfinite(t64['logp'])
            if name == 'brute_holes':
                continue
            al, be = t64['alpha'][1:-1, 1:], t64['beta'][1:-1, :-1]              # emitting rows; t > 0 for alpha, t < T - 1 for beta
            if n > 3:
                dead = np.isneginf(al)
                beside = np.zeros_like(dead)
                beside[1:] |= np.isfinite(al[:-1])
                beside[:-1] |= np.isfinite(al[1:])
                assert (dead & beside).any(), (name, u, 'no alpha = -inf beside a finite neighbour')
            assert np.isneginf(be).any(), (name, u, 'no beta = -inf on an emitting row')
            assert np.isneginf(t64['lgamma']).any() and not np.isnan(t64['lgamma']).any()
            print('%s utt %d (N=%d): ln P %.4f; %d of %d emissions -inf, alpha -inf at %d, beta -inf at %d entries of the emitting rows' % (
                name, u, n, t64['logp'], np.isneginf(B[1:-1]).sum(), B[1:-1].size, np.isneginf(al).sum(), np.isneginf(be).sum()))


@pytest.mark.parametrize('name', mc.IMPOSSIBLE)
def test_an_impossible_utterance_is_all_nan_and_zero(name):
    case = CASES[name]
    kappa, group, refkind = case['combos'][0]
    ref = mc.refs_of(case, refkind)[mc.IMP_AT]
    for t in mc.imp_frames(case):
        la, lpi, rows, B = mc.impossible(case['utts'][mc.IMP_AT], t)
        for dtype in (np.float64, np.longdouble):
            tt = tw.mbr(la, lpi, B, rows, ref, kappa=kappa, group=group, dtype=dtype)
            assert tt['logp'] == -np.inf and tt['c_avg'] == 0 and (tt['g'] == 0).all() and np.isnan(tt['lgamma']).all()
            assert not np.isnan(tw.ln_part(tt['g'].astype(np.float64), +1)).any() and np.isneginf(tw.ln_part(tt['g'].astype(np.float64), -1)).all()
    la, lpi, rows, B = mc.impossible(mc.utterance('chain', 6, 3, np.random.default_rng(6)), 1)      # a 6-row chain, frame 1 of 3: 18 NaNs
    tt = tw.mbr(la, lpi, B, rows, np.zeros(3, dtype=np.int32))
    assert tt['lgamma'].shape == (6, 3) and np.isnan(tt['lgamma']).sum() == 18


# ------------------------------------------------------------------ the identities of tests/test_gpu_mbr_edges.py, in the twin
@pytest.mark.parametrize('name', ('id_chain8', 'id_dense9'))
def test_one_group_makes_c_avg_the_emitting_mass(name):
    case = CASES[name]
    la, lpi, rows, B = case['utts'][0]
    ref = mc.refs_of(case, 'all')[0]
    assert (ref >= 0).all()
    for kappa in (0.1, 1.0):
        t64 = tw.mbr(la, lpi, B, rows, ref, kappa=kappa, group=mc.J)
        tld = tw.mbr(la, lpi, B, rows, ref, kappa=kappa, group=mc.J, dtype=np.longdouble)
        al = tw.allowances(t64, tld, kappa)
        mass = math.fsum(np.exp(t64['lgamma'][1:-1]).ravel())
        margin = mc.one_group_margin(al, B.shape)
        print('%s kappa=%g: c_avg %.15g, emitting mass %.15g, margin %.3g' % (name, kappa, t64['c_avg'], mass, margin))
        assert abs(t64['c_avg'] - mass) <= margin and 0 < mass < B.shape[1]


@pytest.mark.parametrize('name', ('id_chain8', 'id_dense9'))
@pytest.mark.parametrize('k', (0.1, 3.0))
def test_kappa_moves_into_the_emissions(name, k):
    case = CASES[name]
    la, lpi, rows, B = case['utts'][0]
    ref = mc.refs_of(case, 'partly')[0]
    s, u = tw.mbr(la, lpi, B, rows, ref, kappa=k, group=mc.CD_GROUP), tw.mbr(la, lpi, k * B, rows, ref, kappa=1.0, group=mc.CD_GROUP)
    assert (s['g'] != 0).any()                                       # (something to compare: kappa = 3 leaves one path nearly all the mass)
    mc.hold_kappa_moved(s, u, k)


def test_the_central_difference_has_something_to_measure():
    case = CASES['id_chain8']
    la, lpi, rows, B = case['utts'][0]
    ref = mc.refs_of(case, 'all')[0]
    t64 = tw.mbr(la, lpi, B, rows, ref, kappa=mc.CD_KAPPA, group=mc.CD_GROUP)
    j, f = mc.central_entry(t64, B)
    assert 1 <= j < B.shape[0] - 1 and np.isfinite(B[j, f])
    up, dn = B.copy(), B.copy()
    up[j, f] += mc.CD_H
    dn[j, f] -= mc.CD_H
    d = (tw.mbr(la, lpi, up, rows, ref, kappa=mc.CD_KAPPA, group=mc.CD_GROUP)['c_avg'] - tw.mbr(la, lpi, dn, rows, ref, kappa=mc.CD_KAPPA, group=mc.CD_GROUP)['c_avg']) / (2 * mc.CD_H)
    tol = mc.central_tolerance(B.shape[1], mc.CD_KAPPA)
    print('entry (%d, %d): difference quotient %.9g, g %.9g, tolerance %.3g' % (j, f, d, t64['g'][j, f], tol))
    assert abs(d - t64['g'][j, f]) <= tol and abs(t64['g'][j, f]) > 1e3 * tol


def test_every_path_one_by_one_with_holes():
    case = CASES['brute_holes']
    la, lpi, rows, B = case['utts'][0]
    assert B.shape[0] <= 4 and B.shape[1] <= 5 and np.isneginf(B[1:-1]).any()
    for kappa, group, refkind in case['combos']:
        ref = mc.refs_of(case, refkind)[0]
        t = tw.mbr(la, lpi, B, rows, ref, kappa=kappa, group=group)
        bf = tw.brute_force(np.exp(la), np.exp(lpi), B, rows, ref, kappa=kappa, group=group)
        close = lambda got, want: np.all(np.abs(np.asarray(got) - np.asarray(want)) <= 1e-12 * np.maximum(1.0, np.abs(want)))     # tests/test_mbr_twin.py: RTOL
        with np.errstate(all='ignore'):
            gamma = np.exp(t['lgamma'])
        assert close(t['logp'], bf['logp']) and close(t['c_avg'], bf['c_avg']) and close(gamma, bf['gamma']) and close(t['g'], bf['g'])


def test_the_stride_batch_is_past_the_grid():
    blocks, threads = mc.stride_limit()
    case = CASES['stride']
    total = sum(u[3].size for u in case['utts'])
    print('mbr_post_kernel: %d blocks of %d threads = %d; the batch has %d elements in %d utterances' % (blocks, threads, blocks * threads, total, len(case['utts'])))
    assert total > blocks * threads
    assert total - case['utts'][-1][3].size <= blocks * threads      # and by less than an utterance: no larger than it has to be
    assert all(u is case['utts'][k % 2] for k, u in enumerate(case['utts']))
    assert not mc.same_bits(case['utts'][0][3], case['utts'][1][3])
