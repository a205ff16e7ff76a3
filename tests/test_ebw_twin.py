"""The extended Baum-Welch rule's own invariants, on the CPU (tests/_ebw_twin.py; the device is held to it by tests/test_gpu_ebw.py), and
proof that the cases of the GPU test can fail: every term of the rule, left out, moves a compared quantity by at least 100 allowances."""
import numpy as np
import pytest

import _ebw_twin as tw

SHAPES = [s for s in tw.SHAPES if s[0] * s[1] <= 200]
_STATS = {}


def stats(shape):
    if shape not in _STATS:
        model, frames, gnum, gden = tw.make_case(*shape)
        _STATS[shape] = model, tw.numpy_stats(model, frames, gnum), tw.numpy_stats(model, frames, gden)
    return _STATS[shape]


@pytest.mark.parametrize('shape', SHAPES)
def test_equal_sets_leave_the_model_where_it_is(shape):
    model, num, _ = stats(shape)
    t = tw.update(*model, num, num, E=2.0, tau=0.0, weight_iters=100)
    occupied = num['acc'] > 0
    assert occupied.any() and not t['keep'][occupied].any()
    assert np.array_equal(t['mean'], model[0])
    ulp = np.abs(t['var'] - model[1]) / np.spacing(model[1])
    print('equal sets %s: variances off by at most %.1f ulp' % (shape, ulp.max()))
    assert ulp.max() <= 2
    assert np.allclose(t['w'], model[2], rtol=1e-13, atol=0)
    assert np.array_equal(t['w'] == 0, model[2] == 0)


@pytest.mark.parametrize('shape', SHAPES)
def test_every_variance_is_positive_before_the_floor(shape):
    model, num, den = stats(shape)
    role = tw.roles(shape[0], shape[1])
    for tau, E, iters in tw.GRID:
        t = tw.update(*model, num, den, E=E, tau=tau, weight_iters=iters)
        upd = ~t['keep']
        assert (t['prevar'][upd] > 0).all(), (tau, E)
        assert (t['g'][upd] < 0).any() and (t['Dmin'][upd] > 0).any()            # the cases the bound is about are there
        assert (t['Dmin'][role == 2] > 0).all() and t['counts'][2] > 0 and t['keep'][role == 4].all()
        assert t['negdisc'] == 0                                                   # (c - g v)^2 + 4 v x^2: never negative here
        ws = t['w'].sum(axis=1)
        assert np.allclose(ws, 1.0, rtol=1e-12) and (t['w'] >= 0).all()
        assert t['counts'][0] + t['counts'][1] == shape[0] * shape[1]


# (one mixture per state: its weight is 1 whatever the rule, so the weight iteration is looked for where M > 1)
@pytest.mark.parametrize('shape,drop,key', [(s, d, k) for s in SHAPES for d, k in [('ismooth', 'mean'), ('factor2', 'var'), ('delta2', 'var'), ('weights', 'w')]
                                            if not (d == 'weights' and s[1] == 1)])
def test_a_dropped_term_is_seen(shape, drop, key):
    model, num, den = stats(shape)
    full = tw.update(*model, num, den)
    ld = tw.update(*model, num, den, dtype=np.longdouble)
    cut = tw.update(*model, num, den, drop=drop)
    with np.errstate(over='ignore'):                                               # (a weight that is 0 in both runs has an allowance of 5e-324)
        share = np.abs(cut[key] - full[key]) / tw.allowance(full, ld, key)
    print('%s without %s: %s moves by %.3g allowances' % (shape, drop, key, share.max()))
    assert share.max() >= 100


def test_arguments():
    model, num, den = stats(SHAPES[0])
    for kw in (dict(E=0.0), dict(E=-1.0), dict(E=np.nan), dict(tau=-1.0), dict(tau=np.inf), dict(c_covariance=-1.0), dict(weight_iters=-1)):
        with pytest.raises(ValueError):
            tw.update(*model, num, den, **kw)
