"""Segmental GMM training, CPU side: the float64 twin (tests/_segment_twin.py) is pinned to the REFERENCE by golden G18 (the
reference's own Clustering.GMM.em run by tests/golden/make_golden_em.py), the way test_oracle_golden.py pins the oracle; the GPU
tests then compare the library with the golden and with this twin.  Also: the new C-ABI symbols, and the host logic around them."""
import os
import re

import numpy as np
import pytest

import _segment_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['pcl_seg_centres', 'pcl_seg_create', 'pcl_seg_destroy', 'pcl_seg_em', 'pcl_seg_get', 'pcl_seg_kmeans']


def cases(golden):
    g = golden('G18_gmm_em')
    return [{k: g['c%d_%s' % (c, k)] for k in ('data', 'mean0', 'var0', 'w0', 'c_cov', 'mean', 'var', 'w', 'q_seq')}
            for c in range(int(g['n_cases']))]


def test_golden_holds_its_own_condition(golden):
    """Every step of the reference's Q sequence is a factor two away from the 1.28 of Clustering.py:706."""
    cs = cases(golden)
    assert len(cs) >= 4
    for c in cs:
        dq = np.diff(c['q_seq'])
        assert np.all((dq >= 2.56) | (dq <= 0.64)), dq
        assert dq[-1] <= 0.64 and np.all(dq[:-1] >= 2.56)
    assert (cs[1]['var'] == cs[1]['c_cov']).any(), 'the floor binds in the final model of case 1'
    assert len(cs[3]['data']) == cs[3]['mean0'].shape[0] + 1, 'n just above M'


def test_twin_reproduces_the_reference_em(golden):
    for c in cases(golden):
        r = tw.em(c['data'], c['mean0'], c['var0'], c['w0'], c_covariance=float(c['c_cov']))
        assert r['iters'] == len(c['q_seq'])
        np.testing.assert_allclose(r['q_seq'], c['q_seq'], rtol=1e-9)
        np.testing.assert_allclose(r['mean'], c['mean'], rtol=1e-10, atol=1e-10 * np.abs(c['mean']).max())
        np.testing.assert_allclose(r['var'], c['var'], rtol=1e-10)
        np.testing.assert_allclose(r['w'], c['w'], rtol=1e-10)


def test_closed_form_q_is_the_literal_double_loop(golden):
    for c in cases(golden)[:2]:
        x = c['data']
        gamma = tw.expectation(x, c['mean0'], c['var0'], c['w0'])
        mean, var, w, s2, big = tw.maximization(x, gamma, float(c['c_cov']))
        lit = tw.q_literal(x, gamma, mean, var, w)
        assert abs(tw.q_closed(big, w, var, s2) - lit) <= 1e-11 * abs(lit)


def test_new_symbols_are_declared_exported_and_bound():
    import subprocess
    import poccala_amd._lib as L
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'poccala_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(pcl_[a-z0-9_]+)\s*\(', text))
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    lib = L.load()
    for n in NEW_SYMBOLS:
        assert n in declared, n
        assert n in exported, n
        assert n in L.PROTOTYPES and hasattr(lib, n), n


def test_generator_is_the_documented_one():
    # SplitMix64's finaliser over seed * golden-ratio + (j << 32) + k + 1, top 53 bits
    assert tw.uniform(0, 0, 0) == (0x5692161D100B05E5 >> 11) * 2.0 ** -53
    u = np.array([tw.uniform(7, j, k) for j in range(40) for k in range(50)])
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.03 and len(set(u)) == len(u)


def test_frame_state_mapping():
    from poccala_amd.engine import frame_state_of
    fu = np.array([0, 0, 2, 2, -1, 1])
    fk = np.array([0, 2, 1, 0, 0, -1])
    want = np.array([0, 2, 7, 6, -1, -1], dtype=np.int32)
    assert np.array_equal(frame_state_of(fu, fk, 3), want)
    assert np.array_equal(tw.frame_state_of(fu, fk, 3), want)


def test_twin_kmeans_protocol():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal((40, 3)) + 6 * k for k in range(4)])
    idx, margin = tw.seeds(x, 4, seed=11, j=2)
    assert len(set(idx.tolist())) == 4 and margin > 0
    assert idx[0] == min(int(tw.uniform(11, 2, 0) * len(x)), len(x) - 1)
    mean, var, w, assign, sweeps = tw.kmeans(x, 4, seed=11, j=2)
    assert abs(w.sum() - 1) < 1e-12 and (var >= 1e-4).all() and sweeps >= 2
    for k in range(4):
        np.testing.assert_allclose(mean[k], x[assign == k].mean(0), rtol=1e-12)
    # an all-equal segment: total D^2 = 0, still K seeds, no division by zero
    idx, _ = tw.seeds(np.ones((9, 3)), 3, seed=1, j=0)
    assert len(idx) == 3 and idx.min() >= 0 and idx.max() < 9


def test_skip_rule_and_return_shapes_need_no_gpu():
    """n_j < M: the reference skips the state (AcousticModel.py:549-551); the drop-in surface refuses before it touches a GPU."""
    from poccala_amd.StatisticalModel.Clustering import Clustering
    g = Clustering.GMM(dimension=3, mix_level=4, mean=np.zeros((4, 3)), variance=np.ones((4, 3)))
    with pytest.raises(NotImplementedError):
        g.em(smem=True)
    g.data = [[0., 0., 0.], [1., 1., 1.]]
    with pytest.raises(ValueError):
        g.em()
    ci = Clustering.ClusterInitialization(np.zeros((2, 3)), 4, 3)
    with pytest.raises(ValueError):
        ci.kmeans(algorithm=1)
    with pytest.raises(ValueError):
        Clustering.ClusterInitialization(np.zeros((8, 3)), 2, 3).kmeans(algorithm=2)
    g.set_model(np.zeros((2, 3)), np.ones((2, 3)), np.array([0.5, 0.5]))
    assert g.mixture == 2 and g.covariance.shape == (2, 3, 3) and g.acc.shape == (2,) and g.mean_acc.shape == (2, 3)
