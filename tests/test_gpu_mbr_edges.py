"""pcl_batch_mbr (csrc/hmm_mbr.hip) at its wave, list and batch edges: the shapes tests/test_gpu_mbr.py does not reach.  The cases are
tests/_mbr_cases.py (tests/test_mbr_cases.py holds on the CPU that they carry what they claim, and that the identities below hold in the
twin, so a failure here points at the device).

  a  wave counts: N in {127, 128, 129, 256, 257, 1023, 1024} with T in {1, 2, 3, 5}, chain (register lists) and dense (general lists); an
     N = 3 utterance beside the N = 1024 one (a workgroup of sixteen waves, fifteen of them without a row), a T = 1 beside a T = 5
  b  the limit: N = 1025 is refused by mbr (nothing before it refuses the batch), mbr_get stays refused, a batch of N = 1024 made afterwards runs
  c  hmm_mbr_kernel<2> against hmm_mbr_kernel<0>: the same chains alone and beside one dense utterance, byte for byte -- no twin involved
  d  -inf emissions on emitting rows (alpha = -inf, beta = -inf beside finite rows; P(O) > 0)
  e  an utterance with P(O) = 0 beside possible ones: what it gives, that its neighbours do not notice it, what the three posterior sets
     hold for it, and that the accumulate pass gets nothing from it
  f  mbr_post_kernel's grid-stride loop: a batch of more than 2048 x 256 elements
  4  identities that do not go through the twin: one group (c_avg is the emitting mass), kappa moved into the emissions, a central
     difference of c_avg against g

Bound: tests/test_gpu_mbr.py's, unchanged -- _mbr_twin.allowances(float64 twin, long-double twin, kappa), whose derivation does not
depend on N (the twin repeats the cross-row order; only the library's exp / log differ).  Every share is printed before it is asserted;
WORST collects the worst per quantity over this file.  The twins are made once per (case, utterance, combination) and left unchanged."""
import math

import numpy as np
import pytest

import _mbr_cases as mc
import _mbr_twin as tw
from _mbr_cases import CASES, INVALID, STATE, against_twin, refused, same_bits, share
from _parity import hold

pytestmark = pytest.mark.gpu
F64_RTOL = 1e-9              # PCL_F64
WORST = {}
KEYS = ('logp', 'c_avg', 'lgamma', 'g')


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def batch_of(eng, case, utts=None):
    """the batch of a case (or of `utts` in place of its own), its emissions in place and read back -> (batch, per_utt, setup)"""
    s = mc.batch_setup(case, utts)
    b, per_utt = mc.make_batch(eng, s)
    assert all(same_bits(x, u[3]) for x, u in zip(b.get('B'), s['utts']))          # the twin is fed what the batch holds
    return b, per_utt, s


def held(tag, b, per_utt, utts, refs, combo, keys, only=None):
    """mbr under the combination, held to the twins (made once per key) -> (device results, twins, allowances)"""
    kappa, group, _ = combo
    b.mbr(refs, kappa=kappa, group=group)
    twins = [mc.twin_of(keys[u] + tuple(combo), utts[u], refs[u], kappa, group) if only is None or u in only else None for u in range(len(utts))]
    out = against_twin(tag, b, per_utt, [u[3] for u in utts], refs, kappa, group, twins=twins, worst=WORST, only=only)
    print('worst share of the allowance per quantity so far: %s' % WORST)
    return out


def run_case(eng, name, combo):
    case = CASES[name]
    b, per_utt, _ = batch_of(eng, case)
    refs = mc.refs_of(case, combo[2])
    got, twins, allows = held('mbr edges %s kappa=%g group=%d ref=%s' % ((name,) + tuple(combo)), b, per_utt, case['utts'], refs, combo,
                              [(name, u) for u in range(len(case['utts']))])
    return b, got, twins, allows, refs


def one(got, u):
    return {k: got[k][u] for k in KEYS}


def equal_bits(x, y):
    return all(same_bits(x[k], y[k]) for k in KEYS)


# ------------------------------------------------------------------ a, d: wave counts and holes against the twin
@pytest.mark.parametrize('combo', mc.EDGE_COMBOS)
@pytest.mark.parametrize('name', ('chain_waves', 'dense_waves', 'chain_big', 'dense_big', 'chain_holes', 'dense_holes'))
def test_waves_and_holes_against_the_twin(eng, name, combo):
    b, got, twins, _, _ = run_case(eng, name, combo)
    if CASES[name]['holes']:                                         # (share has held the finite / -inf / NaN patterns equal)
        assert all(np.isneginf(g['lgamma'][1:-1]).any() and not np.isnan(g['lgamma']).any() and np.isfinite(g['logp']) for g in twins)
    b.close()


# ------------------------------------------------------------------ b: the limit
def test_the_row_limit(eng):
    """Nothing before mbr refuses a 1025-row batch: it is created and filled, mbr names both numbers, and the refusal leaves nothing."""
    from poccala_amd.engine import Batch
    la, lpi, rows, B = mc.utterance('chain', 1025, 2, np.random.default_rng(mc.seed_of('limit')))
    s = mc.batch_setup(dict(name='limit'), [(la, lpi, rows, B)])
    b, _ = mc.make_batch(eng, s)
    e = refused(INVALID, lambda: b.mbr([np.zeros(2, dtype=np.int32)]))
    assert '1025' in str(e) and '1024' in str(e), e
    refused(STATE, b.mbr_get)
    refused(STATE, lambda: b.mbr_posteriors(0))
    b.close()
    b2, _, _, _, _ = run_case(eng, 'chain_big', mc.EDGE_COMBOS[0])
    b2.close()


# ------------------------------------------------------------------ c: the two list forms, bit for bit
@pytest.mark.parametrize('combo', mc.EDGE_COMBOS)
def test_register_lists_and_general_lists_give_the_same_bits(eng, combo):
    """hmm_mbr.hip's header: a padded register entry is ln 0 and `leaves every bit as the general lists give it`.  The selection is made
    per batch, so one dense utterance beside the chains sends them through the general lists."""
    alone, mixed = CASES['chain_waves'], CASES['mixed']
    n = len(alone['utts'])
    assert max(mc.degrees(alone['utts'])) <= 2 < max(mc.degrees(mixed['utts']))
    b1, first, _, _, refs = run_case(eng, 'chain_waves', combo)
    b1.close()
    refs = refs + [mc.refs_of(mixed, combo[2])[-1]]
    b2, per_utt, _ = batch_of(eng, mixed)
    second, _, _ = held('mbr edges mixed kappa=%g group=%d ref=%s' % tuple(combo), b2, per_utt, mixed['utts'], refs, combo,
                        [('chain_waves', u) for u in range(n)] + [('mixed', n)])
    for u in range(n):
        assert equal_bits(one(first, u), one(second, u)), 'utterance %d (N=%d) differs between the list forms' % (u, len(per_utt[u][2]))
    b2.close()


# ------------------------------------------------------------------ e: P(O) = 0 beside P(O) > 0
@pytest.mark.parametrize('which_frame', (0, 1, 2))
@pytest.mark.parametrize('name', mc.IMPOSSIBLE)
def test_an_impossible_utterance_beside_possible_ones(eng, name, which_frame):
    """The accumulate pass after mbr_posteriors(+1) is held BYTE-EQUAL with and without the impossible utterance: its posteriors are all
    ln 0, the pass compacts the frames that carry something in a fixed order (no atomics), so the sums see the same terms in
    the same order."""
    from poccala_amd import PCL_F64
    case = CASES[name]
    combo = case['combos'][0]
    at, frame = mc.IMP_AT, mc.imp_frames(case)[which_frame]
    possible = case['utts']
    utts = list(possible)
    utts[at] = mc.impossible(possible[at], frame)
    others = [u for u in range(len(utts)) if u != at]
    refs = mc.refs_of(case, combo[2])
    tag = 'mbr edges %s frame %d kappa=%g group=%d ref=%s' % ((name, frame) + tuple(combo))
    b, per_utt, s = batch_of(eng, case, utts)
    b.forward_backward(fix_pi=True)                                  # (so that PCL_GET_LGAMMA may be read)
    got, _, _ = held(tag, b, per_utt, utts, refs, combo, [(name, u, frame if u == at else None) for u in range(len(utts))])
    assert got['logp'][at] == -np.inf and got['c_avg'][at] == 0.0 and (got['g'][at] == 0.0).all() and np.isnan(got['lgamma'][at]).all()
    assert all(np.isfinite(got['logp'][u]) for u in others)
    b.mbr_posteriors(0)
    lg = b.get('lgamma')
    assert all(same_bits(lg[u], got['lgamma'][u]) for u in others) and np.isnan(lg[at]).all()
    with_it = None
    for which in (-1, +1):                                           # an impossible utterance adds nothing to either set: ln 0, never NaN
        b.mbr_posteriors(which)
        lg = b.get('lgamma')
        assert np.isneginf(lg[at]).all()
        assert all(np.array_equal(np.isneginf(lg[u]), ~(which * got['g'][u] > 0)) and not np.isnan(lg[u]).any() for u in others)
    if which_frame == 1:
        eng.stats_zero()
        b.accumulate(PCL_F64)
        with_it = eng.stats_download()
    b.set_emissions([u[3] for u in possible])                        # the same batch, the utterance possible again
    again, _, _ = held(tag + ' possible again', b, per_utt, possible, refs, combo, [(name, u, None) for u in range(len(utts))])
    assert np.isfinite(again['logp'][at]) and not np.isnan(again['lgamma'][at]).any()
    for u in others:
        assert equal_bits(one(got, u), one(again, u)), 'utterance %d noticed its impossible neighbour' % u
    b.close()
    if with_it is not None:
        from poccala_amd.engine import Batch
        b3 = Batch(eng, s['N'][others], s['T'][others], s['begin'][others])        # the neighbours alone, over the same frames
        b3.set_transitions([possible[u][0] for u in others], [possible[u][1] for u in others])
        b3.set_states([possible[u][2] for u in others])
        b3.set_emissions([possible[u][3] for u in others])
        b3.mbr([refs[u] for u in others], kappa=combo[0], group=combo[1])
        alone = b3.mbr_get()
        assert all(equal_bits(one(got, u), one(alone, k)) for k, u in enumerate(others))
        b3.mbr_posteriors(+1)
        eng.stats_zero()
        b3.accumulate(PCL_F64)
        without = eng.stats_download()
        assert with_it['acc'].sum() > 0
        for k in ('acc', 'alpha_acc', 'mean_acc', 'cov_acc'):
            hold(tag, k + ' with / without the impossible utterance', with_it[k], without[k], F64_RTOL)
            print('%s: %s %s' % (tag, k, 'byte-equal' if same_bits(with_it[k], without[k]) else 'NOT byte-equal'))
            assert same_bits(with_it[k], without[k])
        b3.close()


# ------------------------------------------------------------------ f: the posteriors kernel's stride loop
def test_the_posteriors_kernel_goes_round_its_grid(eng):
    """N = 130, T = 5, 807 utterances: 524 550 elements against the grid's 2048 x 256 = 524 288.  (N = 1024 would need 171 utterances, and
    the batch's dense (N, N) transition upload and xi buffer 1.4 GB each: the condition on sum N T is kept, N is smaller and U larger.)"""
    case = CASES['stride']
    combo = case['combos'][0]
    blocks, threads = mc.stride_limit()
    assert sum(u[3].size for u in case['utts']) > blocks * threads
    b, per_utt, _ = batch_of(eng, case)
    b.forward_backward(fix_pi=True)
    refs = mc.refs_of(case, combo[2])
    got, twins, allows = held('mbr edges stride', b, per_utt, case['utts'], refs, combo, [('stride', u % 2) for u in range(len(case['utts']))], only=(0, 1))
    assert not equal_bits(one(got, 0), one(got, 1))
    for u in range(2, len(case['utts'])):
        assert equal_bits(one(got, u), one(got, u % 2)), 'copy %d differs from the first of its kind' % u
    flat = lambda xs: np.concatenate([np.ravel(x) for x in xs])
    b.mbr_posteriors(0)
    assert same_bits(flat(b.get('lgamma')), flat(got['lgamma']))
    g, parts = flat(got['g']), {}
    for which in (+1, -1):
        b.mbr_posteriors(which)
        with np.errstate(over='ignore'):
            parts[which] = np.exp(flat(b.get('lgamma')))
    pos, neg = parts[+1], parts[-1]
    assert not ((pos > 0) & (neg > 0)).any()                         # disjoint ...
    with np.errstate(divide='ignore', invalid='ignore'):
        trip = (2.0 + np.abs(np.log(np.abs(g)))) * 2.0 ** -52 * np.abs(g)
    trip = np.where(g == 0, 0.0, trip)
    assert (np.abs((pos - neg) - g) <= trip).all()                   # ... and their difference is g, the last element included
    assert (g[-650:] != 0).any() and (g != 0).sum() > 1000
    for u in (0, 1):
        tr = trip[u * 650:(u + 1) * 650].reshape(130, 5)
        share('mbr edges stride', 'positive part', pos[u * 650:(u + 1) * 650].reshape(130, 5), np.maximum(twins[u]['g'], 0), allows[u]['g'] + tr, WORST)
        share('mbr edges stride', 'negative part', neg[u * 650:(u + 1) * 650].reshape(130, 5), np.maximum(-twins[u]['g'], 0), allows[u]['g'] + tr, WORST)
    print('worst share of the allowance per quantity so far: %s' % WORST)
    b.close()


# ------------------------------------------------------------------ 4: identities that do not go through the twin
def small_batch(eng, name):
    """-> (batch, per utterance (la, lpi, rows), J of its model): id_chain8 / id_dense9, or tests/test_gpu_mbr.py's loop3 on real scoring"""
    if name == 'loop3':
        import test_gpu_mbr as base
        s = base.setup_of('loop3')
        return base.make_batch(eng, s) + (s['J'],)
    b, per_utt, _ = batch_of(eng, CASES[name])
    return b, per_utt, mc.J


def small_refs(b, J, name, kind):
    rng = np.random.default_rng(mc.seed_of(name, 'small', kind))
    refs = [rng.integers(0, J, t).astype(np.int32) for t in b.T]
    if kind == 'partly':
        for r in refs:
            r[::2] = -1
    return refs


@pytest.mark.parametrize('name', ('id_chain8', 'id_dense9', 'loop3'))
def test_one_group_makes_c_avg_the_emitting_mass(eng, name):
    """group >= J and a reference at every frame: every emitting row is accurate at every frame, the entry and the exit row never, so
    c_avg = sum_t sum_{emitting j} gamma_t(j).  Margin: c_avg's allowance plus N T times ln gamma's (gamma <= 1)."""
    b, per_utt, J = small_batch(eng, name)
    Bs = b.get('B')
    refs = small_refs(b, J, name, 'all')
    for kappa in (0.1, 1.0):
        b.mbr(refs, kappa=kappa, group=J)
        got = b.mbr_get()
        for u, (la, lpi, rows) in enumerate(per_utt):
            t64 = tw.mbr(la, lpi, Bs[u], rows, refs[u], kappa=kappa, group=J)
            tld = tw.mbr(la, lpi, Bs[u], rows, refs[u], kappa=kappa, group=J, dtype=np.longdouble)
            margin = mc.one_group_margin(tw.allowances(t64, tld, kappa), Bs[u].shape)
            mass = math.fsum(np.exp(got['lgamma'][u][1:-1]).ravel())
            print('%s kappa=%g utt %d: c_avg %.15g, emitting mass %.15g, margin %.3g' % (name, kappa, u, got['c_avg'][u], mass, margin))
            assert abs(got['c_avg'][u] - mass) <= margin and mass > 0
    b.close()


@pytest.mark.parametrize('k', (0.1, 3.0))
@pytest.mark.parametrize('name', ('id_chain8', 'id_dense9', 'loop3'))
def test_kappa_moves_into_the_emissions(eng, name, k):
    """mbr(kappa = k) on B against mbr(kappa = 1) on the float64 product k B formed on the host: the kernel forms kappa b as one rounded
    product and 1.0 x is x, so ln P, c_avg and ln gamma have the same bits; g = (k gamma) x against k (gamma x) is within 2 ulp."""
    b, per_utt, J = small_batch(eng, name)
    group = 3 if name == 'loop3' else mc.CD_GROUP
    refs = small_refs(b, J, name, 'partly')
    Bs = b.get('B')
    b.mbr(refs, kappa=k, group=group)
    s = b.mbr_get()
    b.set_emissions([k * x for x in Bs])
    b.mbr(refs, kappa=1.0, group=group)
    u = b.mbr_get()
    assert any((g != 0).any() for g in s['g'])
    for i in range(b.U):
        mc.hold_kappa_moved(one(s, i), one(u, i), k)
    b.close()


def test_g_is_the_central_difference_of_c_avg(eng):
    """tests/test_mbr_twin.py's central difference, once on the device: step and margin are that test's (h = 1e-4; h^2 16 T kappa^3 / 6 +
    8 eps T / h); the device's two c_avg carry their allowance each, which adds 2 allowance(c_avg) / 2h."""
    case = CASES['id_chain8']
    la, lpi, rows, B = case['utts'][0]
    kappa, group, h = mc.CD_KAPPA, mc.CD_GROUP, mc.CD_H
    b, per_utt, _ = batch_of(eng, case)
    ref = mc.refs_of(case, 'all')
    t64 = tw.mbr(la, lpi, B, rows, ref[0], kappa=kappa, group=group)
    tld = tw.mbr(la, lpi, B, rows, ref[0], kappa=kappa, group=group, dtype=np.longdouble)
    al = tw.allowances(t64, tld, kappa)
    j, f = mc.central_entry(t64, B)
    b.mbr(ref, kappa=kappa, group=group)
    g = b.mbr_get()['g'][0][j, f]
    c = {}
    for sign in (+1, -1):
        moved = B.copy()
        moved[j, f] += sign * h
        b.set_emissions([moved])
        b.mbr(ref, kappa=kappa, group=group)
        c[sign] = b.mbr_get(want=('c_avg',))['c_avg'][0]
    d = (c[+1] - c[-1]) / (2 * h)
    tol = mc.central_tolerance(B.shape[1], kappa) + 2.0 * float(al['c_avg']) / (2 * h)
    print('entry (%d, %d): difference quotient %.12g, g %.12g, |difference| %.3e, tolerance %.3e' % (j, f, d, g, abs(d - g), tol))
    assert abs(d - g) <= tol and abs(g) > 1e3 * tol
    b.close()
