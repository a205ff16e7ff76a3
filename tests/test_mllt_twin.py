"""The MLLT twin's own invariants (tests/_mllt_twin.py; the rule: include/poccala_hip.h, row f13), on the CPU.  tests/test_gpu_mllt.py
holds the device to this twin, so what the twin computes is held here to the definition and to planted data."""
import numpy as np
import pytest

import _mllt_twin as tw


def random_posteriors(D, seed=3):
    """a random model whose means are NOT the ML means of the posteriors, two 'utterances' of frames, soft posteriors for every state;
    mixture (1, 2) gathers nothing (acc = 0), state 2 is dropped -> (model, post of all states, state_keep)"""
    rng = np.random.default_rng(seed + D)
    J, M = 4, 3
    model = (rng.standard_normal((J, M, D)) * 1.5, rng.uniform(0.3, 3.0, (J, M, D)), np.full((J, M), 1.0 / M))
    post = []
    for T in (23, 41):
        x = rng.standard_normal((T, D)) * 2.0 + rng.standard_normal(D)
        for j in range(J):
            g = rng.uniform(0, 1, (T, M)) * (rng.uniform(0, 1, (T, 1)) < 0.7)
            if j == 1:
                g[:, 2] = 0.0
            post.append((x, j, g))
    return model, post, np.array([1, 1, 0, 1])


@pytest.mark.parametrize('D', [2, 5, 13])
def test_the_expanded_form_is_the_centred_definition(D):
    """G_i = F_i - C_i from p_i(t), acc and s equals sum gamma / var_i (x - mu)(x - mu)^T within 1e-10 x the per-element sum of absolute
    terms -- with means that are not the statistics' ML means (s != n mu: the cross terms count), an empty mixture and a dropped state"""
    model, post, keep = random_posteriors(D)
    kept = [p for p in post if keep[p[1]]]
    acc, macc = tw.block_stats(model, post)                       # the block holds ALL states: the mixture side must leave state 2 out
    assert acc[1, 2] == 0 and acc[2].sum() > 0
    s = macc - tw.BIAS * acc[:, :, None]
    assert np.abs(s - acc[:, :, None] * model[0]).max() > 1.0     # far from ML
    G0, beta0 = tw.centred(model, kept)
    e = tw.expanded(model, kept, acc, macc, keep)
    worst = (np.abs(e['G'] - G0) / (1e-10 * e['Gabs'])).max()
    print('D=%d: expanded against centred, worst error / bound = %.3e; beta %.6f, occ %.6f' % (D, worst, e['beta'], e['occ']))
    assert worst <= 1.0
    assert abs(e['beta'] - beta0) <= 1e-12 * beta0 and abs(e['occ'] - beta0) <= 1e-12 * beta0
    for i in range(D):
        assert np.array_equal(e['F'][i], e['F'][i].T) or np.abs(e['F'][i] - e['F'][i].T).max() <= 1e-12 * e['Fabs'][i].max()
    # and the dropped state matters: with it the sum is another one
    assert np.abs(tw.mixture_side(model, acc, macc)['C'] - e['C']).max() > 1e-3


@pytest.mark.parametrize('D', [2, 5, 13])
def test_the_sweeps_climb_and_normalise_every_row(D):
    model, post, keep = random_posteriors(D)
    G, beta = tw.centred(model, [p for p in post if keep[p[1]]])
    e = tw.estimate(G, beta, 60, 1.0)
    q, A = e['q_trace'], e['A']
    assert e['status'] == tw.OK and len(q) == 61
    assert q[0] == -0.5 * sum(G[i, i, i] for i in range(D))
    assert (np.diff(q) >= -1e-12 * np.abs(q[1:])).all() and q[-1] > q[0]
    rows = max(abs(A[i] @ G[i] @ A[i] - beta) / beta for i in range(D))
    print('D=%d: Q %.6f -> %.6f, rows |a G a - beta| / beta <= %.2e, det A %.6f' % (D, q[0], q[-1], rows, np.linalg.det(A)))
    assert rows <= 1e-9 and np.linalg.det(A) > 0
    assert abs(e['logdet'] - np.linalg.slogdet(A)[1]) <= 1e-10
    assert abs(q[-1] - tw.aux(A, G, beta)) <= 1e-9 * abs(q[-1])
    ld = tw.estimate(G, beta, 60, 1.0, dtype=np.longdouble)
    assert np.abs(A - ld['A']).max() <= 1e-9 * np.abs(A).max()


def test_refusals():
    model, post, keep = random_posteriors(3)
    G, beta = tw.centred(model, post)
    for e, st in ((tw.estimate(G, beta, 4, beta * 2), tw.LOW_OCCUPANCY), (tw.estimate(G * np.array([1.0, 0.0, 1.0])[:, None, None], beta, 4, 1.0), tw.NOT_POSITIVE_DEFINITE),
                  (tw.estimate(G, np.inf, 4, 1.0), tw.SINGULAR)):
        assert e['status'] == st and np.array_equal(e['A'], np.eye(3)) and e['logdet'] == 0 and np.isnan(e['q_trace']).all() and len(e['q_trace']) == 5


@pytest.mark.parametrize('D,factor', [(4, 3776.5), (13, 117.6)])
def test_planted_diagonal_classes_are_decorrelated(D, factor):
    """z with per-class diagonal covariances of different shape behind x = R z (R of condition 3, not orthogonal), one Gaussian per class
    with the ML mean and diagonal variance of x, hard posteriors.  The occupancy-weighted ratio of off-diagonal to diagonal energy of
    A Sigma_c A^T falls, from A = I to the estimate after 100 sweeps, by a factor measured on this twin at the fixed seed: 3776.5 at
    D = 4 (1.0724 -> 2.8398e-4), 117.6 at D = 13 (0.98085 -> 8.3431e-3).  Asserted with a 10x margin.  And the likelihood of y = A x under
    re-estimated diagonal Gaussians, plus n ln|det A|, exceeds that of x (measured: -9451.7 -> -7750.2 at D = 4)."""
    p = tw.planted(D)
    G, beta, Sig, n = tw.hard_stats(p)
    assert 2.9 < np.linalg.cond(p['R']) < 3.1 and np.abs(p['R'] @ p['R'].T - np.eye(D)).max() > 0.1
    e = tw.estimate(G, beta, 100, 1.0)
    r0, r1 = tw.offdiag_ratio(np.eye(D), Sig, n), tw.offdiag_ratio(e['A'], Sig, n)
    ll0 = tw.diag_loglik(p['x'], p['cls'], len(n))
    ll1 = tw.diag_loglik(p['x'] @ e['A'].T, p['cls'], len(n)) + beta * float(e['logdet'])
    print('D=%d: off-diagonal / diagonal energy %.4e -> %.4e (factor %.1f, measured %.1f); log-likelihood %.1f -> %.1f' % (D, r0, r1, r0 / r1, factor, ll0, ll1))
    assert e['status'] == tw.OK and r0 / r1 >= factor / 10
    assert ll1 > ll0
