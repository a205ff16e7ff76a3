"""The NumPy statement of pcl_batch_mbr's rule (tests/_mbr_twin.py) against things that do not share its code: every path enumerated one
by one, the identities the rule implies, a central difference of c_avg, the oracle's forward / backward, and three wrong variants that
must be caught.  No GPU."""
import numpy as np
import pytest

import _mbr_twin as tw
from oracle import poccala_oracle as po

RTOL = 1e-12                 # brute force against the twin: both float64, a few hundred operations each


def small_case(N, T, seed, J=4):
    """random dense a with zeros, row 1 unreachable (N >= 3), one row with B = -inf throughout (the last), a ref with a -1 in it"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.1, 1.0, (N, N)) * (rng.uniform(size=(N, N)) > 0.3)
    a[np.arange(N), (np.arange(N) + 1) % N] += 0.2
    pi = rng.uniform(0.1, 1.0, N)
    if N >= 3:
        a[:, 1] = 0.0
        pi[1] = 0.0
    a[0, 0] += 0.1                                                  # (row 0 keeps a successor and a predecessor whatever the holes)
    a = a / a.sum(axis=1, keepdims=True)
    pi = pi / pi.sum()
    B = rng.uniform(-6.0, 0.0, (N, T))
    if N >= 3:
        B[N - 1] = -np.inf
    row_state = rng.integers(0, J, N).astype(np.int32)
    if N >= 4:
        row_state[2] = -1
    ref = np.maximum(row_state[rng.integers(0, N, T)], 0).astype(np.int32)       # states that rows do carry: some frames can be right
    if T >= 3:
        ref[1] = -1
    return a, pi, B, row_state, ref


def logs(a, pi):
    with np.errstate(divide='ignore'):
        return np.log(a), np.log(pi)


def close(got, want, tol=RTOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.all(np.abs(got - want) <= tol * np.maximum(1.0, np.abs(want)))


@pytest.mark.parametrize('N', [2, 3, 4])
@pytest.mark.parametrize('T', [1, 2, 3, 5])
@pytest.mark.parametrize('kappa,group', [(1.0, 1), (0.3, 2)])
def test_every_path_one_by_one(N, T, kappa, group):
    a, pi, B, rs, ref = small_case(N, T, seed=100 * N + T)
    la, lpi = logs(a, pi)
    t = tw.mbr(la, lpi, B, rs, ref, kappa=kappa, group=group)
    bf = tw.brute_force(a, pi, B, rs, ref, kappa=kappa, group=group)
    with np.errstate(all='ignore'):
        gamma = np.exp(t['lgamma'])
    assert close(t['logp'], bf['logp']) and close(t['c_avg'], bf['c_avg'])
    assert close(gamma, bf['gamma']) and close(t['g'], bf['g'])
    if N >= 3:
        assert (gamma[1] == 0).all() and (gamma[N - 1] == 0).all() and (t['g'][1] == 0).all()      # the unreachable row, the row that emits nothing


@pytest.mark.parametrize('N,T', [(3, 1), (4, 5), (7, 9), (70, 6)])
def test_identities(N, T):
    a, pi, B, rs, ref = small_case(N, T, seed=7 * N + T, J=5)
    la, lpi = logs(a, pi)
    for kappa in (1.0, 0.1):
        t = tw.mbr(la, lpi, B, rs, ref, kappa=kappa)
        gamma = np.exp(t['lgamma'])
        per_frame = (gamma * (t['alphap'] + t['betap'])).sum(axis=0)
        assert close(per_frame, np.full(T, t['c_avg']))             # the expected accuracy is the same number at every frame
        assert np.abs(t['g'].sum(axis=0)).max() <= RTOL * T * kappa
        assert 0.0 <= t['c_avg'] <= T
        z = tw.mbr(la, lpi, B, rs, np.full(T, -1, dtype=np.int32), kappa=kappa)
        assert z['c_avg'] == 0.0 and (z['g'] == 0.0).all()          # nothing to be accurate about: exactly


def test_g_is_the_gradient_of_c_avg():
    """Central difference with step h = 1e-4 in B[j, t].  c_avg = E[acc] under a Gibbs weight in theta = kappa B[j, t]; its third derivative
    in theta is the joint cumulant of (acc, 1_jt, 1_jt, 1_jt): 15 partitions of four variables, acc in [0, T], the indicator in [0, 1], so
    |c'''| <= 16 T kappa^3 with room; the central difference's truncation error is h^2 |c'''| / 6.  Rounding: two evaluations of c_avg,
    each good to a few ulp of T, divided by 2h: 8 eps T / h."""
    N, T, h = 4, 5, 1e-4
    a, pi, B, rs, ref = small_case(N, T, seed=3)
    B[N - 1] = np.random.default_rng(4).uniform(-6.0, 0.0, T)      # (a finite row, so that every reachable entry can be stepped)
    rs, ref = np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 2, 3, -1, 0], dtype=np.int32)   # (some frames can be right, none must be)
    la, lpi = logs(a, pi)
    for kappa in (1.0, 0.3):
        t = tw.mbr(la, lpi, B, rs, ref, kappa=kappa)
        tol = h * h * 16.0 * T * kappa ** 3 / 6.0 + 8.0 * np.finfo(np.float64).eps * T / h
        worst = 0.0
        for j in range(N):
            for f in range(T):
                up, dn = B.copy(), B.copy()
                up[j, f] += h
                dn[j, f] -= h
                d = (tw.mbr(la, lpi, up, rs, ref, kappa=kappa)['c_avg'] - tw.mbr(la, lpi, dn, rs, ref, kappa=kappa)['c_avg']) / (2 * h)
                worst = max(worst, abs(d - t['g'][j, f]))
        print('kappa %g: worst |difference quotient - g| %.3e, tolerance %.3e, largest |g| %.3e' % (kappa, worst, tol, np.abs(t['g']).max()))
        assert worst <= tol and np.abs(t['g']).max() > 1e3 * tol


def test_scale_against_the_oracle():
    """kappa = 1 is oracle.forward / oracle.backward (which add ln a, B and beta in another association: a few ulp of |alpha| per step);
    kappa with B is kappa = 1 on kappa B, bit for bit -- the product is formed once either way."""
    N, T = 6, 12
    a, pi, B, rs, ref = small_case(N, T, seed=11)
    la, lpi = logs(a, pi)
    t = tw.mbr(la, lpi, B, rs, ref, kappa=1.0)
    alpha, beta = po.forward(a, pi, B), po.backward(a, B)
    with np.errstate(all='ignore'):
        lg = alpha + beta
        lg = lg - po.lse(lg, axis=0)[None, :]
    fin = np.isfinite(lg)
    tol = 4 * T * np.spacing(np.abs(alpha[np.isfinite(alpha)]).max())
    assert np.array_equal(fin, np.isfinite(t['lgamma']))
    assert abs(t['logp'] - po.lse(alpha[:, -1])) <= tol and np.abs(t['lgamma'][fin] - lg[fin]).max() <= tol
    k = 0.37
    s, u = tw.mbr(la, lpi, B, rs, ref, kappa=k), tw.mbr(la, lpi, k * B, rs, ref, kappa=1.0)
    assert s['logp'] == u['logp'] and np.array_equal(s['lgamma'], u['lgamma'], equal_nan=True) and s['c_avg'] == u['c_avg']
    assert (np.abs(s['g'] - k * u['g']) <= 2 * np.spacing(np.abs(s['g']))).all()   # (k gamma) x against k (gamma x): one rounding each way


def test_grouping_compares_units():
    N, T, J = 8, 7, 9                                               # 3 units of 3 states
    a, pi, B, _, _ = small_case(N, T, seed=21)
    rng = np.random.default_rng(22)
    rs = np.concatenate([[-1], rng.integers(0, J, N - 2), [-2]]).astype(np.int32)
    ref = rng.integers(0, J, T).astype(np.int32)
    ref[3] = -1
    la, lpi = logs(a, pi)
    by_group = tw.mbr(la, lpi, B, rs, ref, kappa=0.5, group=3)
    by_unit = tw.mbr(la, lpi, B, np.where(rs >= 0, rs // 3, rs), np.where(ref >= 0, ref // 3, ref), kappa=0.5, group=1)
    by_state = tw.mbr(la, lpi, B, rs, ref, kappa=0.5, group=1)
    assert by_group['c_avg'] == by_unit['c_avg'] and np.array_equal(by_group['g'], by_unit['g'])
    assert by_group['c_avg'] > by_state['c_avg']                    # units agree more often than states


@pytest.mark.parametrize('depart', tw.DEPARTURES)
def test_omissions_are_caught(depart):
    """each wrong variant against the enumeration: off by at least 1e-3, nine orders above the 1e-12 the right rule is held to"""
    N, T, kappa = 4, 5, 0.3
    a, pi, B, rs, ref = small_case(N, T, seed=100 * N + T)
    la, lpi = logs(a, pi)
    bf = tw.brute_force(a, pi, B, rs, ref, kappa=kappa)
    t = tw.mbr(la, lpi, B, rs, ref, kappa=kappa, depart=depart)
    off = max(abs(t['c_avg'] - bf['c_avg']), np.abs(t['g'] - bf['g']).max())
    print('%s: off the enumeration by %.3e' % (depart, off))
    assert off > 1e-3


def test_the_smbr_chain_raises_the_expected_accuracy():
    """the end-to-end setup of tests/test_gpu_mbr.py on the CPU: the condition the GPU test leans on belongs to this chain and this seed"""
    ref = tw.e2e_reference()
    total = ref['c_avg'].sum(axis=1)
    print('summed c_avg per iteration: %s of %d frames' % (total, ref['c_avg'].shape[1] * 40))
    assert total[1] > total[0]
