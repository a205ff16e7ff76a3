"""The claims of tests/_logdet_cases.py, held on the CPU (tests/test_gpu_logdet.py runs the cases on the device): every device case must
be able to fail.

  identity      the oracle's gmm_point with w' = w exp(1/2 (sum var - sum ln var)) IS the plain log-determinant reference (1e-12 relative)
                and w' is finite: the oracle serves the E-step and the M-step unchanged.
  whole site    a site that ignored PCL_MODEL_LOGDET altogether: the Q1 reference differs from the log-determinant one by at least D/2 nats
                on every compared element (v - ln v >= 1 per feature).
  partial site  sites 3 to 6 handle only SOME mixtures: the off-pipe list of a split state (the subset launch of
                gmm_score.hip, the coarse pass, the subset pass of the accumulate), the on-pipe list of a split state (the compact-main
                kernel), every mixture of a flagged tile (the fix-up).  A mutant reference gives exactly those mixtures the Q1 constant; the
                case assigned to the site holds at least 8 compared elements at which mutant and truth differ by 100 allowances or more.
  membership    which mixtures are off the pipe is re-derived from model_derive.hip's rule at the documented threshold (96); the device test
                asserts that pcl_model_split_info counts the same.
  regime        what the float64 reference itself loses when mean and var are rounded to f32 stays below half of every allowance: the
                bounds are used in the regime they were measured in."""
import numpy as np
import pytest

import _logdet_cases as lc
from oracle import poccala_oracle as po

SCORE_CASES = [('ladder-13', lambda: lc.ladder(13)), ('ladder-20', lambda: lc.ladder(20)), ('ladder-39', lambda: lc.ladder(39)), ('broad', lc.broad), ('outlier', lc.outlier),
               ('split', lc.split), ('collapsed', lc.collapsed)]
IDS = [i for i, _ in SCORE_CASES]


@pytest.fixture(scope='module')
def refs():
    """Per case the log-determinant and the Q1 reference on every (state, frame), computed once."""
    out = {}
    for i, mk in SCORE_CASES:
        c = mk()
        out[i] = (lc.point_states(c['frames'], c['mean'], c['var'], c['w']), lc.point_states(c['frames'], c['mean'], c['var'], c['w'], True))
    return out


def f32_class(cid, c, limit_share=0.99):
    """The states whose ln b the device test holds to the f32-class bound: any off-pipe mixture; every state of the outlier case."""
    if cid == 'outlier':
        return np.ones(c['mean'].shape[0], dtype=bool)
    return lc.off_pipe(c['mean'], c['var']).any(axis=1)


def split_states(c, limit):
    """States that stay split at `limit` off-pipe mixtures (more: the whole state goes to the direct form, whose rows derive_kernel writes)."""
    n_off = lc.off_pipe(c['mean'], c['var']).sum(axis=1)
    return (n_off > 0) & (n_off <= limit)


@pytest.mark.parametrize('cid', IDS)
def test_the_oracle_with_q1_weights_is_the_plain_reference(cid, refs):
    c = dict(SCORE_CASES)[cid]()
    with np.errstate(over='ignore'):
        wp = lc.q1_weights(c['var'], c['w'])
    if cid == 'broad':                                                  # sum var - sum ln var ~ 5e4: no E-step runs on it, the plain reference serves alone
        assert not np.isfinite(wp).all() and np.isfinite(refs[cid][0]).all()
        return
    assert np.isfinite(wp).all() and (wp >= 0).all() and ((wp == 0) == (c['w'] == 0)).all()
    expo = 0.5 * (c['var'].sum(-1) - np.log(c['var']).sum(-1))
    assert expo.max() < 300.0                                           # (far below ln(DBL_MAX) = 709)
    got = np.stack([po.gmm_point(c['frames'].astype(np.float64), c['mean'][j], c['var'][j], wp[j]) for j in range(len(wp))])
    ref = refs[cid][0]
    assert np.isfinite(ref).all()
    rel = np.abs(got - ref) / np.abs(ref)
    print('%s: oracle with w\' against the plain reference: %.2e relative, largest exponent of w\' %.1f' % (cid, rel.max(), expo.max()))
    assert rel.max() <= 1e-12


@pytest.mark.parametrize('cid', IDS)
def test_a_site_without_the_flag_moves_every_element_by_half_d(cid, refs):
    c = dict(SCORE_CASES)[cid]()
    D = c['mean'].shape[2]
    ld, q1 = refs[cid]
    cmp = lc.compared(c)
    assert cmp.sum() >= 100 and (ld - q1)[cmp].min() >= 0.5 * D


def test_case_shapes_and_membership():
    for D in lc.LADDER_DIMS:
        c = lc.ladder(D)
        assert c['mean'].shape == (4, 70, D) and c['frames'].shape == (130, D) and c['frames'].dtype == np.float32
        assert not lc.off_pipe(c['mean'], c['var']).any()               # ordinary states: the 5e-5 bound applies
        assert (c['w'] == 0).sum() == 1 and c['w'][lc.ZERO_WEIGHT] == 0 and np.allclose(c['w'].sum(1), 1)
        s = np.resize(lc.LADDER_SCALES, 70)
        tail_ld, tail_q1 = np.log(c['var']).sum(-1), c['var'].sum(-1)
        assert (tail_ld[:, s == 4.0].min(axis=1) - tail_ld[:, s == 0.25].max(axis=1) > 0.8 * np.log(16.0) * D).all()
        assert np.corrcoef(tail_ld.ravel(), tail_q1.ravel())[0, 1] > 0.5    # both grow with s: -1/2 tail orders the mixtures alike, the SIZES differ
        assert (tail_q1[:, s == 4.0].mean() - tail_q1[:, s == 0.25].mean()) > 3.0 * D
    o = lc.outlier()
    assert o['frames'].shape == (260, 39) and o['mean'] is lc.ladder(39)['mean']
    assert lc.OUTLIER_FRAMES[0] < 256 <= lc.OUTLIER_FRAMES[1]            # one frame in each 256-frame workgroup
    sig = np.sqrt(o['var'][:, :, lc.OUTLIER_FEATURE])
    for t in lc.OUTLIER_FRAMES:
        assert ((o['frames'][t, lc.OUTLIER_FEATURE] - o['mean'][:, :, lc.OUTLIER_FEATURE]) / sig).min() >= 400.0
    c = lc.split()
    J, M, D = c['mean'].shape
    assert (J, M, D) == (6, 48, 39) and [len(t) for t in c['tight']] == [0, 3, 6, 9, 0, 48]
    off = lc.off_pipe(c['mean'], c['var'])
    for j in range(J):
        assert np.array_equal(np.flatnonzero(off[j]), c['tight'][j])
    assert split_states(c, int(np.float32(0.5) * np.float32(M))).tolist() == [False, True, True, True, False, False]
    assert split_states(c, int(np.float32(0.99) * np.float32(M))).tolist() == [False, True, True, True, False, False]     # 48 > 47: whole
    assert all(len(r) == 11 for r in c['rows']) and c['frames'].shape == (225, 39) and {u for l in c['labels'] for u in l} == {0, 1}
    c = lc.collapsed()
    off = lc.off_pipe(c['mean'], c['var'])
    assert off.sum(axis=1).tolist() == [160, 140, 0] and all(np.array_equal(np.flatnonzero(off[j]), c['tight'][j]) for j in range(3))
    assert c['mean'].shape == (3, 160, 39) and c['frames'].shape == (386, 39)
    cons = -0.5 * np.log(c['var']).sum(-1)
    assert cons[1][off[1]].max() - cons[1][~off[1]].min() > 250.0        # a collapsed mixture's constant hundreds of nats above a broad one's
    for j in (0, 1):                                                      # frames on both sides of the split
        own = c['comp'][c['state'] == j]
        assert off[j, own].sum() >= 30 and (j == 0 or (~off[j, own]).sum() >= 100)


def test_site_1_k0_with_the_q1_constant_costs_the_bits():
    """state_prepass_kernel's K0 = max_m k'_m over the on-pipe mixtures; derive_kernel stores k'_m - K0 in two f16 pieces and the kernel
    sums them with the quadratic terms in f32.  Both take the constant from the flag on their own: with the prepass alone on Q1's
    constant, K0 lies below EVERY k'_m of the `broad` case by 2^14 log2 units or more -- inside f16 (beyond it the kernel flags the tile
    and the fix-up repairs the score, which no comparison sees), where one f32 spacing is 2^-9 log2 units = 1.35e-3 nats, 27 allowances
    of 5e-5; with the flag in both, every piece lies in (-5e4, 0].  On the ladder the same defect moves K0 by less than 2^10 log2 units
    (a spacing of 2^-14: nothing a bound sees), which is why `broad` exists."""
    c = lc.broad()
    assert not lc.off_pipe(c['mean'], c['var']).any() and c['mean'].shape == (4, 70, 39)
    kp, kq1 = lc.k_prime(c['mean'], c['var'], c['w']), lc.k_prime(c['mean'], c['var'], c['w'], q1=True)
    rel = kp - kp.max(axis=1, keepdims=True)
    assert rel.max() == 0.0 and rel.min() > -5.0e4
    shift = kp - kq1.max(axis=1, keepdims=True)
    assert shift.min() >= 2.0 ** 14 and shift.max() < lc.F16_MAX
    assert 2.0 ** -9 * np.log(2.0) >= 25.0 * lc.F32_LOGLIK_ATOL
    for D in lc.LADDER_DIMS:
        l = lc.ladder(D)
        fin = l['w'] > 0
        shift = lc.k_prime(l['mean'], l['var'], l['w'])[fin].max() - lc.k_prime(l['mean'], l['var'], l['w'], q1=True)[fin].max()
        assert abs(shift) < 1024.0


# (site, case, which mixtures take the Q1 constant): DESIGN.md section 7a
def mutants():
    sp, co, ou = lc.split(), lc.collapsed(), lc.outlier()
    M = sp['mean'].shape[1]
    out = []
    for site, c, cid, limit, on in ((3, sp, 'split', int(np.float32(0.5) * np.float32(M)), False), (4, sp, 'split', int(np.float32(0.99) * np.float32(M)), False),
                                    (5, sp, 'split', int(np.float32(0.99) * np.float32(M)), True), (4, co, 'collapsed', lc.COLLAPSED_M, False),
                                    (5, co, 'collapsed', lc.COLLAPSED_M, True)):
        off = lc.off_pipe(c['mean'], c['var'])
        mask = (~off if on else off) & split_states(c, limit)[:, None]
        out.append(('site %d %s: %s-pipe list of the split states' % (site, cid, 'on' if on else 'off'), cid, c, mask, None))
    frames = np.zeros(ou['frames'].shape[0], dtype=bool)
    frames[list(lc.OUTLIER_FRAMES)] = True
    out.append(('site 3 outlier: every mixture of a flagged tile', 'outlier', ou, np.ones(ou['w'].shape, dtype=bool), frames))
    return out


MUTANTS = mutants()


@pytest.mark.parametrize('k', range(len(MUTANTS)), ids=[m[0] for m in MUTANTS])
def test_a_site_that_drops_the_flag_for_its_own_mixtures_shows(k, refs):
    what, cid, c, mask, frames = MUTANTS[k]
    ref = refs[cid][0]
    mut = lc.point_states(c['frames'], c['mean'], c['var'], c['w'], mask)
    if frames is not None:                                                # only the rescored frames read the mutated rows
        mut = np.where(frames[None, :], mut, ref)
    allow = lc.allowance(c, ref, f32_class(cid, c))
    hit = (np.abs(mut - ref) >= 100.0 * allow) & lc.compared(c)
    print('%s: %d compared elements 100 allowances or more away (of %d), smallest shift among them %.1f nats' % (
        what, hit.sum(), lc.compared(c).sum(), np.abs(mut - ref)[hit].min() if hit.any() else 0.0))
    assert mask.any() and hit.sum() >= 8


def test_site_6_the_accumulate_pass_dropping_the_flag_for_the_off_pipe_list_shows():
    """The statistics of (state, mixture) cells: the accumulate pass alone (alpha, beta, ln b the true ones) takes the Q1 constant for the
    off-pipe list of the states it keeps split (up to half of M): their cells lose their occupancy; allowance of the f32 statistics."""
    c = lc.split()
    M = c['mean'].shape[1]
    off = lc.off_pipe(c['mean'], c['var'])
    mask = off & split_states(c, int(np.float32(0.5) * np.float32(M)))[:, None]
    ref, mut = lc.estep(c)['stats'], lc.estep(c, acc_q1_mask=mask)['stats']
    allow = 1e-4 * np.abs(ref['acc']) + 1e-6 * np.abs(ref['acc']).max()
    hit = np.abs(mut['acc'] - ref['acc']) >= 100.0 * allow
    print('site 6 split: %d (state, mixture) cells of acc 100 allowances or more away, all on the off-pipe list: %s' % (hit.sum(), bool((hit <= mask).all())))
    assert hit.sum() >= 8 and (hit <= mask).all()
    assert (ref['acc'][off] > 0).sum() > 20                               # the off-pipe mixtures carry real occupancy


@pytest.mark.parametrize('cid', IDS)
def test_the_cases_stay_in_the_regime_of_their_bounds(cid, refs):
    c = dict(SCORE_CASES)[cid]()
    ref = refs[cid][0]
    loss = lc.f32_parameter_loss(c['frames'], c['mean'], c['var'], c['w'])
    share = (loss / lc.allowance(c, ref, f32_class(cid, c)))[lc.compared(c)]
    print('%s: the reference with f32-rounded parameters moves by up to %.2e nats, %.3f of the allowance; |ln b| up to %.1f' % (
        cid, loss[lc.compared(c)].max(), share.max(), np.abs(ref[lc.compared(c)]).max()))
    assert share.max() < 0.5


def test_survives_inputs():
    c = lc.survives()
    J, M, D = c['mean'].shape
    assert (J, M, D) == (6, 8, 13) and len(c['labels']) == 7 and c['W'].shape == (1, D, D + 1) and np.linalg.cond(c['W'][0][:, 1:]) < 10.0
    assert [int((c['frame_state'] == j).sum()) for j in range(J)] == [40] * J and c['frames'].shape[0] == int(c['lens'].sum()) >= 240
    x = c['frames']
    assert (lc.point_states(x, c['mean'], c['var'], c['w']) - lc.point_states(x, c['mean'], c['var'], c['w'], True)).min() >= 0.5 * D
    e = lc.estep(c)
    assert np.isfinite(e['logp']).all() and (e['stats']['acc'] > 0).all()   # every mixture is reached: the M-step has no guard to take
    for j in range(J):                                                     # the M-step reference gives weights that sum to one either way
        assert abs(po.gmm_update_param(e['log'][j])[0].sum() - 1.0) < 1e-12
