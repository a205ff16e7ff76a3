"""CPU side of the log-domain forward-backward tests (tests/_fb_log_cases.py, tests/test_gpu_fb_log_edges.py): the d-set holds what it claims, the
float64 twins are measured against long double (the device bounds are multiples of THESE figures, never of what the device gives), every
batch lands on the kernel it is meant for by the launcher's own rule, and the oracle gives every case a finite ln P(O) within
PCL_MAX_PASS passes -- so that the GPU test compares every case and skips none."""
import numpy as np
import pytest

import _fb_log_cases as fc
from oracle import poccala_oracle as po

LD = np.longdouble


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps < 1e-18


# ------------------------------------------------------------------ A
def test_d_set_holds_every_node_tie_and_edge():
    d = fc.lse_d_set()
    assert d.dtype == np.float64 and (np.diff(d) > 0).all() and d[0] == 0.0 and d.size > 9000
    has = lambda v: np.isin(np.asarray(v, dtype=np.float64), d).all()
    nodes = np.arange(fc.SP_N) / 32.0
    assert has(nodes) and nodes[-1] == 40.0
    ties = fc.tie_set()
    assert ties.size == 1280 and has(ties) and has(np.nextafter(ties, 0.0)) and has(np.nextafter(ties, np.inf))
    # a tie IS one: d * 32 lies exactly between two integers, the round to even picks the even one, the Taylor step is +-1/64; and
    # k / 32 - 1 / 64 is the tie of the node before
    assert np.array_equal(ties * 32.0 - np.floor(ties * 32.0), np.full(1280, 0.5))
    k = np.rint(ties * 32.0)
    assert (k % 2 == 0).all() and np.array_equal(np.abs(ties - k / 32.0), np.full(1280, 1.0 / 64.0)) and {-1.0, 1.0} == set(np.sign(ties - k / 32.0))
    assert np.array_equal(nodes[1:] - 1.0 / 64.0, ties)
    assert np.array_equal(np.rint(np.nextafter(ties, 0.0) * 32.0), np.floor(ties * 32.0)) and np.array_equal(np.rint(np.nextafter(ties, np.inf) * 32.0), np.ceil(ties * 32.0))
    lo1 = np.nextafter(fc.SP_MAX, 0.0)
    hi1 = np.nextafter(fc.SP_MAX, np.inf)
    assert has([0.0, 5e-324, 2.0 ** -53, fc.SP_MAX, lo1, np.nextafter(lo1, 0.0), hi1, np.nextafter(hi1, np.inf), 40.0, 41.0])
    assert ((d > 0) & (d < 40) & ~np.isin(d, np.concatenate([nodes, ties, np.nextafter(ties, 0.0), np.nextafter(ties, np.inf)]))).sum() >= 4096
    hi, lo = fc.lse_operands()
    assert hi.size % 32 == 0 and hi.size // 32 <= 300                                # a few hundred utterances of 64 x 2
    pairs = set(zip(hi.tolist(), lo.tolist()))
    assert (0.0, -np.inf) in pairs and (-np.inf, -np.inf) in pairs and all((0.0, -v) in pairs for v in d.tolist())
    # the table index of every operand pair stays inside the table
    assert np.rint(np.where(d < fc.SP_MAX, d, 0.0) * 32.0).max() < fc.SP_N


def test_expected_values():
    want = fc.lse_expected([0.0, 0.0, 0.0, 0.0, -np.inf, 0.0], [0.0, -fc.SP_MAX, -np.nextafter(fc.SP_MAX, 0.0), -41.0, -np.inf, -np.inf])
    assert want[0] == np.log(LD(2)) and want[1] == 0 and 0 < want[2] < 5e-18 and want[3] == 0 and np.isneginf(want[4]) and want[5] == 0


def test_table_twin_against_long_double():
    """the figure the device bound of section A is twice of; a bound above 1e-15 could not tell the sixth-order coefficient from zero."""
    err = fc.lse_twin_error()
    flipped = fc.lse_twin_error(c6_sign=-1.0)
    print('lse2_tab twin vs long double over %d values of d: max |error| %.3e -> device bound %.3e; with the sign of c6 flipped %.3e'
          % (fc.lse_d_set().size, err, 2 * err, flipped))
    assert 0 < err and 2 * err < 1e-15
    assert flipped > 4 * err                                   # (twice the bound: the mutant is out even if the device sits at the bound's edge)
    hi, lo = fc.lse_operands()
    got, want = fc.lse2_tab_twin(hi, lo), fc.lse_expected(hi, lo)
    plain = ~np.isfinite(hi) | ~(hi - np.where(np.isfinite(lo), lo, -1e300) < fc.SP_MAX)
    assert np.array_equal(got[plain], want[plain].astype(np.float64)) and np.array_equal(got[plain], hi[plain])      # exactly the maximum, -inf included


@pytest.mark.parametrize('cross', [False, True])
@pytest.mark.parametrize('order', [0, 1])
def test_lse_batches_isolate_one_log_sum_exp(order, cross):
    """alpha_1(sink) and beta_0(source) of the built utterances are the log-sum-exp of the operand pair and nothing else (the oracle's own
    forward / backward, float64); the structure takes the branch it is built for."""
    c = fc.lse_batch(order, cross)
    a = c['a']
    assert set(np.unique(a)) == {0.0, 1.0} and (a != 0).sum(axis=0).max() == 2 and (a != 0).sum(axis=1).max() == 2
    assert fc.is_left_right(a) == (not cross)                  # hmm_fb2_body's `near` is the same rule on predecessors and successors
    assert fc.dispatch([dict(a=a)]) == 'hmm_fb2_kernel'
    i, j = np.nonzero(a)
    assert ((np.abs(i - j) <= 1).all()) == (not cross) and (not cross or (a[0, 63] == 1.0))
    hi, lo = fc.lse_operands()
    want = fc.lse_expected(hi, lo).astype(np.float64)
    assert len(c['Bs']) == 2 * (hi.size // 32) and all(B.shape == (64, 2) for B in c['Bs'])
    alpha = [po.forward(a, np.ones(64), B) for B in c['Bs']]
    with np.errstate(invalid='ignore'):
        beta = [po.backward(a, B) for B in c['Bs']]
    ga = np.array([alpha[u][s, 1] for u, s in zip(*c['alpha_read'])])
    gb = np.array([beta[u][s, 0] for u, s in zip(*c['beta_read'])])
    for got in (ga, gb):
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        fin = np.isfinite(want)
        assert np.abs(got[fin] - want[fin]).max() < 5e-16


# ------------------------------------------------------------------ B
def test_groups_cover_the_edges_they_name():
    g = fc.groups()
    small = g['small']
    seen = {(c['kind'], c['variant'], c['a'].shape[0]) for c in small}
    assert seen >= {(k, v, n) for k in fc.KINDS for v in fc.VARIANTS for n in fc.N_SMALL}
    assert {c['B'].shape[1] for c in small} == set(fc.T_SMALL) and set(fc.T_SMALL) >= set(fc.T_FB) | set(fc.T_POST)
    for k in fc.KINDS:
        assert any(c['kind'] == k and np.isneginf(c['B']).any() and not c['impossible'] for c in small), k
        assert {c['B'].shape[1] for c in g['sweep'] if c['kind'] == 'ring'} == set(fc.T_SMALL)
    assert any(abs(c['B'][np.isfinite(c['B'])]).max() > 3000 for c in small) and any(abs(c['B'][np.isfinite(c['B'])]).max() < 300 for c in small)
    for c in small:
        a, s = c['a'], c['a'].shape[0] // 2
        if c['variant'] == 'nosucc':
            assert not a[s].any()
        if c['variant'] == 'nopred':
            assert not a[:, s].any() and c['pi'][s] > 0
        if c['variant'] == 'selfonly':
            assert a[s, s] == 1.0 and (a[s] != 0).sum() == 1
    ring = next(c for c in small if c['kind'] == 'ring' and c['variant'] == 'plain' and c['a'].shape[0] == 64)
    assert ring['a'][63, 0] > 0                                # the closing edge: lane 63 -> lane 0
    wide = [c for name in fc.WIDE_GROUPS for c in g[name]]
    assert {(c['kind'], c['a'].shape[0], c['B'].shape[1]) for c in wide} >= {(k, n, t) for k in ('ring', 'skip') for n in fc.N_WIDE for t in fc.T_WIDE}
    assert {c['variant'] for c in g['wide192']} == set(fc.VARIANTS)
    assert sorted(c['a'].shape[0] for c in g['wide_gap']) == [5, 129] and g['wide_lr'][0]['a'].shape[0] == 257 and g['wide_lr'][0]['lr']
    assert max(c['a'].shape[0] * c['B'].shape[1] for cs in fc.groups_all().values() for c in cs) <= 257 * 20


def test_every_batch_lands_on_the_kernel_it_is_meant_for():
    """the predicates pcl_launch_forward_backward dispatches on, from the matrices alone."""
    g = fc.groups_all()
    for name, cs in g.items():
        for c in cs:
            a = c['a']
            assert (a != 0).sum(axis=0).max() <= 2 and (a != 0).sum(axis=1).max() <= 2, c['name']
            assert c['lr'] == fc.is_left_right(a), c['name']
            if c['kind'] == 'l2r' or a.shape[0] > 3:           # (with 2 or 3 states an altered state can leave a left-to-right HMM behind)
                assert c['lr'] == (c['kind'] == 'l2r'), c['name']
            assert np.array_equal(c['pi'] > 0, np.isin(np.arange(a.shape[0]), fc.support(a.shape[0])))
        nmax = max(c['a'].shape[0] for c in cs)
        if name in fc.SMALL_GROUPS + ('post',):
            assert nmax <= 64 and fc.dispatch(cs, linear=False) == 'hmm_fb2_kernel', name
        else:
            assert name in fc.WIDE_GROUPS and nmax > 64 and fc.dispatch(cs, linear=False) == fc.dispatch(cs, linear=True) == 'hmm_fb_kernel<2>', name
        if name not in ('lr_alone', 'wide_lr'):                # not left to right as a batch: the log-domain kernels whatever PCL_FB_LINEAR says
            assert not all(c['lr'] for c in cs) and fc.dispatch(cs, linear=True) in ('hmm_fb2_kernel', 'hmm_fb_kernel<2>'), name
    assert all(c['lr'] for c in g['lr_alone']) and fc.dispatch(g['lr_alone'], linear=True) == 'hmm_fbl_kernel'
    mixed = g['mixed']
    assert any(c['lr'] for c in mixed) and any(not c['lr'] for c in mixed)
    assert all(any(c is m for m in mixed) for c in g['lr_alone'])                    # the very same HMMs, alone and inside the mixed batch
    # rings and permutations are what the cross-lane branch is for: a state reached from / reaching a lane that is not its neighbour
    for c in g['small']:
        i, j = np.nonzero(c['a'])
        if c['kind'] in ('ring', 'perm') and c['a'].shape[0] >= 63 and c['variant'] == 'plain':
            assert (np.abs(i - j) > 1).any(), c['name']


@pytest.mark.parametrize('name', sorted(fc.groups()))
def test_oracle_finishes_every_case(name):
    """no case may be skipped on the device: finite ln P(O), at most PCL_MAX_PASS passes, and no pass decision that rounding could turn
    (fc.decisive) -- but for the cases named impossible, which keep P(O) = 0 and the reference's NaN posteriors."""
    for k, c in enumerate(fc.groups()[name]):
        for fix_pi, thr in fc.SETTINGS:
            bw = fc.oracle(name, k, fix_pi, thr)
            if c['impossible']:
                assert np.isneginf(bw['logp'][0]) and bw['n_pass'] == 1, c['name']
                l = bw['alpha'][0] + bw['beta'][0]
                assert np.isneginf(l).all() and np.isneginf(bw['ksai']).all() and np.isneginf(bw['gamma']).all(), c['name']
                assert np.array_equal(bw['pi'], c['pi']) if fix_pi else np.isnan(bw['pi']).all(), c['name']
                continue
            assert np.isfinite(bw['logp'][0]) and bw['n_pass'] <= fc.MAX_PASS, (c['name'], fix_pi, thr, bw['n_pass'])
            assert fc.decisive(bw, thr), (c['name'], fix_pi, thr, bw['q_trace'])
            assert bw['n_pass'] == 2 if fix_pi or thr == 1e9 else bw['n_pass'] >= 2, (c['name'], fix_pi, thr)
    if name in ('small', 'wide128', 'wide192', 'wide320'):     # 1e-13: pi is re-estimated and read back more than once
        assert max(fc.oracle(name, k, False, 1e-13)['n_pass'] for k in range(len(fc.groups()[name]))) >= 3


# ------------------------------------------------------------------ C
def test_exp_neg_twin():
    x = -np.concatenate([np.linspace(0.0, 745.0, 20001), [5e-324, 1e-300, 1e-17, np.log(2) / 2, 744.999]])
    got, want = fc.exp_neg_twin(x), np.exp(x.astype(LD))
    norm = x > -700                                            # (below: subnormal results, absolute precision only)
    assert (np.abs(got[norm].astype(LD) / want[norm] - 1) < 4e-16).all()
    assert np.array_equal(fc.exp_neg_twin(np.array([-745.0, -746.0, -1e4, -np.inf])), np.zeros(4)) and fc.exp_neg_twin(np.array([0.0]))[0] == 1.0


def test_post_cases_and_twin_against_long_double():
    """the figure the device bound of section C is four times of: the float64 restatement of hmm_post_body's online log-sum-exps, merged in
    wave order over 8 waves, against long double on the same alpha / beta."""
    cases = fc.post_cases()
    for k, c in enumerate(cases):
        fin = c['B'][np.isfinite(c['B'])]
        assert c['B'].shape[1] <= 17 and c['a'].shape[0] <= 64 and np.isfinite(c['B']).all()
        assert np.abs(fin).max() <= 8.0 or c['name'].endswith('driven'), c['name']
        bw = fc.oracle('post', k, True, 0.64)
        assert np.isfinite(bw['logp'][0]) and bw['n_pass'] == 2, c['name']
    drv = cases[-1]
    bw = fc.oracle('post', len(cases) - 1, True, 0.64)
    post = bw['alpha'][0] + bw['beta'][0] - bw['logp'][0]
    assert drv['name'].endswith('driven') and (post[32, 5:8] < -745.0).all() and np.isfinite(post[32]).all() and (post[32, :5] > -745.0).any()
    err = fc.post_twin_error()
    print('hmm_post_body twin vs long double over %d cases: max |error| of ln gamma / ln xi %.3e -> device bound %.3e' % (len(cases), err, 4 * err))
    assert 0 < err < 1e-13
