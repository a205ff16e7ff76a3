"""Minimum Bayes risk on the device (csrc/hmm_mbr.hip: pcl_batch_mbr / pcl_batch_mbr_get / pcl_batch_mbr_posteriors; Batch.mbr / mbr_get /
mbr_posteriors / ref_states) against the NumPy statement of the rule (tests/_mbr_twin.py, whose own invariants tests/test_mbr_twin.py holds).

Everything goes through the C-ABI; the twin is fed the emissions the batch holds (get('B')), the transitions and ln pi as they were set.
Shapes: batches of 5 utterances of unequal N and T, N in {3, 62, 64, 65, 130} (one wave, a full wave, the two-wave edge, three waves),
T in {1, 2, 3, 17}; a left-to-right chain (the register lists), a dense random matrix with holes, an unreachable row and an exit row that
emits nothing (the general lists), and Engine.loop_batch over 3 and over 22 units (N = 11 and 68) on real scoring.
The shapes this file does not reach are in tests/test_gpu_mbr_edges.py (cases: tests/_mbr_cases.py): up to sixteen waves and the 1024-row
limit, the two list forms against each other bit for bit, -inf emissions on emitting rows, utterances with P(O) = 0 beside possible ones,
mbr_post_kernel's grid-stride loop, and identities that do not go through the twin.  The helpers shared with it live in _mbr_cases.py.

Bound.  Nothing here is a float32 path.  Per utterance the float64 twin is measured against the same code in long double; the device may
differ from the float64 twin by 4x that distance plus an absolute term derived in _mbr_twin.allowances from ulp(max |alpha|) and the
number of chained steps.  What mbr_posteriors leaves is read back through PCL_GET_LGAMMA and compared in the linear domain
(exp(ln max(g, 0)) against max(g, 0)): one log and one exp lie between, the log rounds at |ln g| 2^-53 absolutely, which the exp turns
into that much relatively, plus an ulp for each library call: (2 + |ln g|) 2^-52 relative.  Every figure is printed before it is asserted.

End to end (6 units, J = 18, M = 2, D = 4, 8 x 40 frames, the unit loop against the Viterbi alignment of the label batches, three sMBR
iterations with kappa = 0.1, E = 2, tau = 0): ln b under PCL_F64 is held to 1e-9 relative; c_avg moves with B by
g, and sum_j |g_t(j)| <= kappa max |alpha' + beta' - c_avg| <= kappa T, so an iteration's summed c_avg may differ from the host chain's by
1e-9 kappa T sum_{u,t} max_j |B|; every update divides by g + D >= gn + gd (tau = 0, D >= 2 gd), below the factor 10 the MMI test allows
per update, so iteration k is held to 10^k times that, and the final model to the MMI test's 1e-7 relative plus 1e-7 absolute."""
import numpy as np
import pytest

import _ebw_twin as ebw
import _mbr_cases as mc
import _mbr_twin as tw
from _mbr_cases import INVALID, STATE, WORST, against_twin, logs, refused, same_bits, share
from _parity import hold

pytestmark = pytest.mark.gpu
F64_RTOL = 1e-9              # PCL_F64
NS, TS = [3, 62, 64, 65, 130], [1, 2, 3, 17, 17]
COMBOS = [(1.0, 1, 'viterbi'), (1.0, 3, 'random'), (0.1, 1, 'partly'), (0.1, 3, 'none'), (0.1, 1, 'viterbi'), (1.0, 1, 'partly'),
          (0.1, 3, 'random'), (1.0, 3, 'viterbi')]
STRUCTURES = ('chain', 'dense', 'loop3', 'loop22')


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


_SETUPS = {}


def setup_of(kind):
    """host side of a structure, made once: model, frames, and per utterance (la, lpi, row_state, B or None)"""
    if kind in _SETUPS:
        return _SETUPS[kind]
    from poccala_amd import synth
    rng = np.random.default_rng(dict(chain=1, dense=2, loop3=3, loop22=4)[kind])
    units = 3 if kind == 'loop3' else 22
    mean, var, w, trans = synth.make_model(units, 2, 4, seed=5)
    J = units * 3
    s = dict(kind=kind, model=(mean, var, w), trans=trans, J=J)
    if kind in ('chain', 'dense'):
        N = NS if kind == 'chain' else NS[::-1]
        T = TS if kind == 'chain' else [17, 3, 2, 1, 17]
        s['N'], s['T'], s['utts'] = np.array(N, dtype=np.int32), np.array(T, dtype=np.int32), []
        for n, t in zip(N, T):
            a, pi = tw.chain_structure(n, rng) if kind == 'chain' else tw.dense_structure(n, rng)
            rows = np.concatenate([[-1], rng.integers(0, J, n - 2), [-2]]).astype(np.int32)
            B = mc.emissions(n, t, rng)                              # uniform(-40, 0), the entry row's ln 1 and the exit row's ln 0
            if kind == 'chain' and t == 1:
                B[0] = -3.0                                          # (one frame: something other than the entry row has to be possible)
            s['utts'].append(logs(a, pi) + (rows, B))
        s['begin'] = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)        # (set_states wants frames behind the batch; the emissions are set)
        s['frames'] = rng.standard_normal((sum(T), 4))
    else:
        T = [1, 2, 3, 17, 9]
        s['T'] = np.array(T, dtype=np.int32)
        s['begin'] = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
        s['frames'] = (rng.standard_normal((sum(T), 4)) * 1.5).astype(np.float32).astype(np.float64)
    _SETUPS[kind] = s
    return s


def make_batch(eng, s):
    """the batch of a structure with its emissions in place -> (batch, per utterance (la, lpi, row_state))"""
    from poccala_amd import PCL_F64
    from poccala_amd.engine import loop_structure
    if s['kind'] in ('chain', 'dense'):
        return mc.make_batch(eng, s)
    eng.load_model(*s['model'])
    eng.load_frames(s['frames'])
    b = eng.loop_batch(s['T'], s['begin'], s['trans'])
    b.score(PCL_F64)
    la, lpi = logs(*loop_structure(s['trans']))
    rows = np.concatenate([[-1], np.arange(s['J']), [-2]]).astype(np.int32)
    return b, [(la, lpi, rows)] * len(s['T'])


def refs_of(b, kind, J, rng):
    if kind == 'viterbi':
        b.viterbi()
        return b.ref_states()
    out = [rng.integers(0, J, t).astype(np.int32) for t in b.T]
    if kind == 'none':
        out = [np.full(t, -1, dtype=np.int32) for t in b.T]
    if kind == 'partly':
        for r in out:
            r[::2] = -1
    return out


@pytest.mark.parametrize('kind', STRUCTURES)
def test_the_pass_is_the_twins(eng, kind):
    s = setup_of(kind)
    b, per_utt = make_batch(eng, s)
    b.forward_backward(fix_pi=True)                                  # (so that PCL_GET_LGAMMA may be read; the pass itself does not need it)
    Bs = b.get('B')
    rng = np.random.default_rng(9)
    for kappa, group, refkind in COMBOS:
        tag = 'mbr %s kappa=%g group=%d ref=%s' % (kind, kappa, group, refkind)
        refs = refs_of(b, refkind, s['J'], rng)
        b.mbr(refs, kappa=kappa, group=group)
        got, twins, allows = against_twin(tag, b, per_utt, Bs, refs, kappa, group)
        if refkind == 'none':
            assert (got['c_avg'] == 0).all() and all((g == 0).all() for g in got['g'])
        b.mbr_posteriors(0)
        assert all(same_bits(x, y) for x, y in zip(b.get('lgamma'), got['lgamma']))
        parts = {}
        for which in (+1, -1):
            b.mbr_posteriors(which)
            with np.errstate(over='ignore'):
                parts[which] = [np.exp(x) for x in b.get('lgamma')]
        for u in range(b.U):
            pos, neg, g = parts[+1][u], parts[-1][u], got['g'][u]
            assert not ((pos > 0) & (neg > 0)).any()                 # disjoint ...
            with np.errstate(divide='ignore', invalid='ignore'):
                trip = (2.0 + np.abs(np.log(np.abs(g)))) * 2.0 ** -52 * np.abs(g)
            trip = np.where(g == 0, 0.0, trip)
            assert (np.abs((pos - neg) - g) <= trip).all()           # ... and their difference is g
            share(tag, 'positive part', pos, np.maximum(twins[u]['g'], 0), allows[u]['g'] + trip)
            share(tag, 'negative part', neg, np.maximum(-twins[u]['g'], 0), allows[u]['g'] + trip)
    print('worst share of the allowance per quantity so far: %s' % WORST)
    b.close()


def test_results_of_other_passes_stay_and_two_runs_agree(eng):
    s = setup_of('dense')
    b, per_utt = make_batch(eng, s)
    b.forward_backward(fix_pi=True)
    b.viterbi()
    keys = ('alpha', 'beta', 'ksai', 'logp', 'B', 'gamma', 'pi', 'qtrace', 'npass', 'path', 'point')
    before = {k: b.get(k) for k in keys + ('lgamma',)}
    refs = b.ref_states()
    b.mbr(refs, kappa=0.1, group=3)
    first = b.mbr_get()
    assert all(same_bits(np.concatenate([np.ravel(x) for x in b.get(k)]), np.concatenate([np.ravel(x) for x in before[k]])) for k in keys + ('lgamma',))
    b.mbr_posteriors(+1)
    assert all(same_bits(np.concatenate([np.ravel(x) for x in b.get(k)]), np.concatenate([np.ravel(x) for x in before[k]])) for k in keys)
    assert not same_bits(np.concatenate([np.ravel(x) for x in b.get('lgamma')]), np.concatenate([np.ravel(x) for x in before['lgamma']]))
    b.mbr(refs, kappa=0.1, group=3)
    second = b.mbr_get()
    for k in ('logp', 'c_avg'):
        assert same_bits(first[k], second[k])
    for k in ('lgamma', 'g'):
        assert all(same_bits(x, y) for x, y in zip(first[k], second[k]))
    b.close()


def test_refusals(eng):
    from poccala_amd.engine import Batch
    s = setup_of('chain')
    eng.load_model(*s['model'])
    eng.load_frames(s['frames'])
    J = s['J']
    b = Batch(eng, s['N'], s['T'], s['begin'])
    refs = [np.zeros(t, dtype=np.int32) for t in s['T']]
    refused(STATE, lambda: b.mbr(refs))                              # no transitions
    b.set_transitions([u[0] for u in s['utts']], [u[1] for u in s['utts']])
    refused(STATE, lambda: b.mbr(refs))                              # no states
    b.set_states([u[2] for u in s['utts']])
    refused(STATE, lambda: b.mbr(refs))                              # no emissions
    b.set_emissions([u[3] for u in s['utts']])
    refused(STATE, b.mbr_get)                                        # before the pass
    refused(STATE, lambda: b.mbr_posteriors(0))
    for kw in (dict(kappa=0.0), dict(kappa=-1.0), dict(kappa=float('nan')), dict(kappa=float('inf')), dict(group=0), dict(group=-3)):
        refused(INVALID, lambda: b.mbr(refs, **kw))
    for bad in (J, -2, 2 ** 30):
        wrong = [r.copy() for r in refs]
        wrong[-1][-1] = bad
        refused(INVALID, lambda: b.mbr(wrong))
    refused(STATE, b.mbr_get)                                        # (a refused pass leaves nothing behind)
    b.mbr(refs, kappa=0.5)
    good = b.mbr_get()
    for which in (2, -2, 7):
        refused(INVALID, lambda: b.mbr_posteriors(which))
    assert all(same_bits(x, y) for x, y in zip(b.mbr_get()['g'], good['g']))
    refused(INVALID, lambda: b.mbr(refs, kappa=float('nan')))       # a refusal after a good pass: the good pass stays
    assert all(same_bits(x, y) for x, y in zip(b.mbr_get()['g'], good['g']))
    for invalidate in (lambda: b.set_emissions([u[3] for u in s['utts']]),
                       lambda: b.set_transitions([u[0] for u in s['utts']], [u[1] for u in s['utts']]),
                       lambda: b.set_states([u[2] for u in s['utts']])):
        invalidate()
        refused(STATE, b.mbr_get)
        refused(STATE, lambda: b.mbr_posteriors(+1))
        b.mbr(refs, kappa=0.5)                                       # still usable, and the same pass again
        assert all(same_bits(x, y) for x, y in zip(b.mbr_get()['g'], good['g']))
    b.close()
    from poccala_amd import PCL_F64
    s3 = setup_of('loop3')
    b3, _ = make_batch(eng, s3)
    b3.mbr([np.zeros(t, dtype=np.int32) for t in s3['T']])
    b3.score(PCL_F64)                                                # scoring invalidates the pass too
    refused(STATE, b3.mbr_get)
    b3.close()


def test_accumulate_reads_what_the_pass_left(eng):
    """accumulate(PCL_F64) after mbr_posteriors(+1) against accumulate after set_posteriors of the twin's ln max(g, 0): the same pass on
    posteriors that differ by g's allowance; the statistics are linear in the posterior with factors <= 1 (acc, alpha_acc), |x + 100|
    (mean_acc) and (x - mu)^2 (cov_acc), so beside PCL_F64's 1e-9 relative they may differ by sum_t allowance times that factor's maximum."""
    from poccala_amd import PCL_F64
    s = setup_of('loop22')
    b, per_utt = make_batch(eng, s)
    Bs = b.get('B')
    refs = refs_of(b, 'viterbi', s['J'], None)
    b.mbr(refs, kappa=0.1)
    b.mbr_posteriors(+1)
    eng.stats_zero()
    b.accumulate(PCL_F64)
    dev = eng.stats_download()
    lgs, slack = [], np.zeros(s['J'])
    for u, (la, lpi, rows) in enumerate(per_utt):
        t64 = tw.mbr(la, lpi, Bs[u], rows, refs[u], kappa=0.1)
        tld = tw.mbr(la, lpi, Bs[u], rows, refs[u], kappa=0.1, dtype=np.longdouble)
        lgs.append(tw.ln_part(t64['g'], +1))
        slack += tw.allowances(t64, tld, 0.1)['g'].sum(axis=1)[1:-1]
    b.set_posteriors(lgs)
    eng.stats_zero()
    b.accumulate(PCL_F64)
    ref = eng.stats_download()
    x, mean = s['frames'], s['model'][0]
    fx, fc = np.abs(x + ebw.BIAS).max(), ((np.abs(x).max() + np.abs(mean).max()) ** 2)
    assert ref['acc'].sum() > 0
    hold('mbr downstream', 'acc', dev['acc'], ref['acc'], F64_RTOL, slack[:, None])
    hold('mbr downstream', 'alpha_acc', dev['alpha_acc'], ref['alpha_acc'], F64_RTOL, slack)
    hold('mbr downstream', 'mean_acc', dev['mean_acc'], ref['mean_acc'], F64_RTOL, (slack * fx)[:, None, None])
    hold('mbr downstream', 'cov_acc', dev['cov_acc'], ref['cov_acc'], F64_RTOL, (slack * fc)[:, None, None])
    b.close()


def test_smbr_iterations_follow_the_host_chain(eng):
    from poccala_amd import PCL_F64
    c, cm = ebw.E2E, tw.E2E
    ref = tw.e2e_reference()
    want = ref['c_avg'].sum(axis=1)
    print('host chain: summed c_avg per iteration %s' % want)
    assert want[1] > want[0]                                         # (the twin chain's property: tests/test_mbr_twin.py)
    model, trans, frames, labels, lens, begin = ebw.e2e_setup()
    eng.load_model(*model)
    eng.load_units(trans)
    eng.load_frames(frames)
    num_b = eng.label_batch(labels, lens, begin)
    den_b = eng.loop_batch(lens, begin, trans)
    got = []
    for it in range(cm['iters'] + 1):
        num_b.score(PCL_F64)                                         # 1  the numerator alignment
        num_b.viterbi()
        refs = num_b.ref_states()
        assert all(np.array_equal(x, y) for x, y in zip(refs, ref['refs'][it]))
        den_b.score(PCL_F64)                                         # 2  the unit loop under kappa
        den_b.mbr(refs, kappa=cm['kappa'], group=cm['group'])
        got.append(den_b.mbr_get(want=('c_avg',))['c_avg'].sum())
        if it < cm['iters']:
            eng.stats_zero()                                         # 3  the positive part, held
            den_b.mbr_posteriors(+1)
            den_b.accumulate(PCL_F64)
            eng.ebw_hold()
            eng.stats_zero()                                         # 4  the negative part, and the update
            den_b.mbr_posteriors(-1)
            den_b.accumulate(PCL_F64)
            eng.mstep_ebw(E=cm['E'], tau=cm['tau'])
    got = np.array(got)
    bound = F64_RTOL * cm['kappa'] * c['T'] * ref['bsum'] * 10.0 ** np.arange(cm['iters'] + 1)
    print('device: summed c_avg per iteration %s; off the host chain by %s of the bound %s' % (got, np.abs(got - want) / bound, bound))
    assert (np.abs(got - want) <= bound).all()
    assert got[1] > got[0]
    for name, dev, host in zip(('mean', 'var', 'w'), eng.model_download(), ref['model']):
        used = (np.abs(dev - host) / (1e-7 + 1e-7 * np.abs(host))).max()
        print('final %s: %.3g of the bound' % (name, used))
        assert used <= 1.0
    num_b.close()
    den_b.close()
