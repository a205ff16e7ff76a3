"""The log-domain forward-backward kernels of csrc/hmm_dp.hip that drawn HMMs never reach (tests/_fb_log_cases.py builds the cases,
tests/test_fb_log_cases.py holds the builders, the twins and the bounds on the CPU):

  A  lse2_tab read straight out of alpha_1 / beta_0 at every table node, every rounding tie and the 39.98 cut, on the wave-shift and the
     cross-lane branch of hmm_fb2_body, against long double; the bound is twice the float64 twin's own error.
  B  rings, right-to-left chains, skip chains, woven chains and permutations with their degenerate states, on hmm_fb2_kernel +
     hmm_post_kernel (N <= 64) and hmm_fb_kernel<2> (N > 64), against oracle/poccala_oracle.py baum_welch at the tolerances of
     tests/test_gpu_fuzz_hmm.py; a left-to-right HMM alone and beside a ring, bit for bit.
  C  hmm_post_kernel's exp_neg / online_lse / merge / series: posteriors that sum to one, the summed ln xi / ln gamma against long double
     at four times the float64 twin's own error.

PCL_FB_LINEAR=0 for every test: left-to-right batches then take the log-domain kernels too (it is read per call)."""
import numpy as np
import pytest

import _fb_log_cases as fc
from _parity import hold
from oracle import poccala_oracle as po

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def log_route(monkeypatch):
    monkeypatch.setenv('PCL_FB_LINEAR', '0')


def run_fb(eng, As, pis, Bs, fix_pi, threshold):
    N = np.array([a.shape[0] for a in As], dtype=np.int32)
    T = np.array([b.shape[1] for b in Bs], dtype=np.int32)
    begin = np.concatenate([[0], np.cumsum(T[:-1])]).astype(np.int64)
    eng.load_frames(np.zeros((int(T.sum()), max(eng.D, 1)), dtype=np.float32))
    b = eng.batch(N, T, begin)
    with np.errstate(divide='ignore'):
        b.set_transitions([np.log(a) for a in As], [np.log(p) for p in pis])
    b.set_emissions(Bs)
    b.forward_backward(fix_pi=fix_pi, threshold=threshold)
    out = {k: b.get(k) for k in fc.KEYS}
    b.close()
    return out


def run_cases(eng, cases, fix_pi, threshold):
    return run_fb(eng, [c['a'] for c in cases], [c['pi'] for c in cases], [c['B'] for c in cases], fix_pi, threshold)


def same(tag, what, got, want, rtol, atol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (tag, what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), '%s / %s: NaN pattern' % (tag, what)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), '%s / %s: -inf pattern' % (tag, what)
    hold(tag, what, np.where(nan, 0.0, got), np.where(nan, 0.0, want), rtol, atol)


def check_against_oracle(tag, c, out, u, bw, fix_pi):
    """one utterance against baum_welch: the comparisons of tests/test_gpu_fuzz_hmm.py plus the Q trace and the -inf patterns."""
    T = c['B'].shape[1]
    at = fc.tolerance(c)
    ctx = (c['name'], fix_pi)
    npass = int(out['npass'][u])
    assert npass == int(bw['n_pass']), ctx
    qt = np.asarray(out['qtrace'][u])
    assert qt.shape == (fc.MAX_PASS,) and np.isnan(qt[npass:]).all(), ctx
    if c['impossible']:                              # P(O) = 0: what the reference's arithmetic gives (tests/test_gpu_fb_linear.py test_impossible_utterance)
        assert np.isneginf(out['logp'][u]) and np.isneginf(qt[0]), ctx
        same(tag, 'ln alpha', out['alpha'][u], bw['alpha'][0], 1e-10, at)
        same(tag, 'ln beta', out['beta'][u], bw['beta'][0], 1e-10, at)
        assert np.isnan(out['lgamma'][u]).all() and np.isneginf(out['ksai'][u]).all() and np.isneginf(out['gamma'][u]).all(), ctx
        if fix_pi:                                   # (the library hands back exp(ln pi))
            np.testing.assert_allclose(out['pi'][u], c['pi'], rtol=max(1e-9, 100 * at), atol=1e-300, err_msg=str(ctx))
        else:
            assert np.isnan(out['pi'][u]).all(), ctx
        return
    same(tag, 'Q trace', qt[:npass], np.concatenate([bw['q_trace'][1:], [bw['q_final']]]), 1e-10, at)
    same(tag, 'ln P(O)', out['logp'][u], bw['logp'][0], 1e-10, at)
    same(tag, 'ln alpha', out['alpha'][u], bw['alpha'][0], 1e-10, at)
    same(tag, 'ln beta', out['beta'][u], bw['beta'][0], 1e-10, at)
    if T > 1:
        same(tag, 'ln xi (sum over t)', out['ksai'][u], bw['ksai'], 1e-10, at)
        same(tag, 'ln gamma (sum over t)', out['gamma'][u], bw['gamma'], 1e-10, at)
        l = bw['alpha'][0] + bw['beta'][0]
        same(tag, 'ln gamma_t(j)', out['lgamma'][u], l - po.lse(l, axis=0)[None, :], 1e-10, at)
    else:                                            # one frame: the reference raises (golden G15); the library says ln 0
        assert np.isneginf(out['ksai'][u]).all() and np.isneginf(out['lgamma'][u]).all(), ctx
    np.testing.assert_allclose(out['pi'][u], bw['pi'], rtol=max(1e-9, 100 * at), atol=1e-300, err_msg=str(ctx))


# ------------------------------------------------------------------ A
@pytest.mark.parametrize('cross', [False, True], ids=['shift', 'cross-lane'])
@pytest.mark.parametrize('order', [0, 1], ids=['larger-first', 'larger-second'])
def test_table_log_sum_exp_at_its_own_precision(eng, order, cross):
    """alpha_1(sink) = beta_0(source) = lse2_tab(hi, lo) of every operand pair of fc.lse_operands(): within twice the float64 twin's error of
    long double (measured by tests/test_fb_log_cases.py: 1.352e-16, bound 2.704e-16); exactly the larger operand from d = 39.98 on and when
    an operand is -inf."""
    c = fc.lse_batch(order, cross)
    U = len(c['Bs'])
    out = run_fb(eng, [c['a']] * U, [np.ones(64)] * U, c['Bs'], True, 1e9)
    hi, lo = fc.lse_operands()
    want = fc.lse_expected(hi, lo)
    bound = 2 * fc.lse_twin_error()
    with np.errstate(invalid='ignore'):
        exact = ~np.isfinite(hi) | ~(hi - lo < fc.SP_MAX)
    tag = 'lse2_tab vs long double (%s branch, larger operand %s)' % ('cross-lane' if cross else 'wave-shift', 'second' if order else 'first')
    for what, key, (utt, st), t in (('alpha_1', 'alpha', c['alpha_read'], 1), ('beta_0', 'beta', c['beta_read'], 0)):
        got = np.array([out[key][u][s, t] for u, s in zip(utt, st)])
        assert np.array_equal(got[exact], hi[exact]), (tag, what)                    # the maximum itself, -inf included
        err = (got[~exact].astype(LD) - want[~exact]).astype(np.float64)
        k = int(np.abs(err).argmax())
        print('%s / %s: max |error| %.3e at d = %r (bound %.3e)' % (tag, what, np.abs(err).max(), float(-lo[~exact][k]), bound))
        hold(tag, what + ' - log1p(exp(-d))', err, np.zeros_like(err), 0.0, bound)


# ------------------------------------------------------------------ B
@pytest.mark.parametrize('setting', fc.SETTINGS, ids=lambda s: 'fix_pi=%s,thr=%g' % s)
@pytest.mark.parametrize('name', [n for n in fc.SMALL_GROUPS + fc.WIDE_GROUPS if n != 'lr_alone'])
def test_degree_two_structures_against_the_oracle(eng, name, setting):
    fix_pi, thr = setting
    cases = fc.groups()[name]
    out = run_cases(eng, cases, fix_pi, thr)
    tag = 'log-domain forward-backward vs oracle (%s)' % fc.dispatch(cases)
    for u, c in enumerate(cases):
        check_against_oracle(tag, c, out, u, fc.oracle(name, u, fix_pi, thr), fix_pi)


@pytest.mark.parametrize('fix_pi', [False, True])
def test_left_to_right_hmm_alone_and_beside_a_ring_bit_for_bit(eng, fix_pi):
    """a ring in the batch sends every utterance to hmm_fb2_kernel, where the left-to-right ones take the wave-shift branch beside the
    ring's cross-lane branch in one launch: what the kernel does per utterance does not depend on the batch."""
    g = fc.groups()
    alone, mixed = run_cases(eng, g['lr_alone'], fix_pi, 1e-13), run_cases(eng, g['mixed'], fix_pi, 1e-13)
    for u, c in enumerate(g['lr_alone']):
        v = next(k for k, m in enumerate(g['mixed']) if m is c)
        for key in fc.KEYS:
            assert np.array_equal(alone[key][u], mixed[key][v], equal_nan=True), (c['name'], key)
        check_against_oracle('log-domain forward-backward vs oracle (left-to-right, alone)', c, alone, u, fc.oracle('lr_alone', u, fix_pi, 1e-13), fix_pi)


# ------------------------------------------------------------------ C
def test_posterior_kernel_arithmetic(eng):
    """|b| <= 8 and T <= 17: an ulp of ln alpha is ~1e-14, what is measured is hmm_post_kernel.  sum_i exp(ln gamma_t(i)) = 1 within an ulp
    of ln P(O) + 1e-15 (the series / wave_lse normaliser is rounded once at the size of ln P(O); exp_neg's 2e-16 relative over <= 64 terms and
    the rounding of the O(1) differences l - norm make up the rest); summed ln xi / ln gamma within 4 x the twin's error of long double."""
    cases = fc.post_cases()
    out = run_cases(eng, cases, True, 0.64)
    bound = 4 * fc.post_twin_error()
    tag = 'hmm_post_kernel vs long double'
    for u, c in enumerate(cases):
        bw = fc.oracle('post', u, True, 0.64)
        check_against_oracle('log-domain forward-backward vs oracle (O(1) emissions)', c, out, u, bw, True)
        if c['B'].shape[1] > 1:                      # (one frame has no posteriors: held to ln 0 by check_against_oracle)
            check_posteriors(tag, c, out, u, bw, bound)
    from _parity import REPORT
    print({k: '%.3e of %.3e' % (v['max_abs'], v['bound']['atol']) for k, v in REPORT[tag].items() if isinstance(v, dict)})


def check_posteriors(tag, c, out, u, bw, bound):
    lg = out['lgamma'][u]
    assert np.array_equal(np.isfinite(lg), np.isfinite(bw['alpha'][0] + bw['beta'][0])), c['name']
    s = np.exp(lg.astype(LD)).sum(axis=0)
    hold(tag, 'sum_i gamma_t(i) - 1', (s - 1).astype(np.float64), np.zeros(lg.shape[1]), 0.0, float(np.spacing(abs(bw['logp'][0]))) + 1e-15)
    gamma, ksai = fc.post_reference(c, bw['alpha'][0], bw['beta'][0])
    for what, got, want in (('ln gamma (sum over t)', out['gamma'][u], gamma), ('ln xi (sum over t)', out['ksai'][u], ksai)):
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin) and np.isneginf(got[~fin]).all(), (c['name'], what)
        err = (got[fin].astype(LD) - want[fin]).astype(np.float64)
        hold(tag, what, err, np.zeros_like(err), 0.0, bound)
