"""The adaptation rules (include/poccala_hip.h: pcl_mllr_estimate, pcl_model_transform_means, pcl_mstep_map) as tests/_adapt_twin.py
states them: identity and exact recovery of a known transform, the three refusals, the limits of MAP, the conditioning of the inputs the
GPU tests use, and AcousticModel.adapt_batch's host bookkeeping on a stand-in engine.  No GPU.  tests/test_gpu_adapt.py holds the device
to the same twin."""
import numpy as np
import pytest

import _adapt_twin as tw

COND_MAX = 1e4               # a condition on the INPUTS of the GPU tests: the solve amplifies float64 rounding by cond x (D+1) x 1.1e-16


def synthetic(seed, J=6, M=40, D=13):
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((J, M, D))
    var = rng.uniform(0.5, 2.0, (J, M, D))
    acc = rng.uniform(0.5, 3.0, (J, M))
    return rng, mean, var, acc


def stats_at(acc, target):
    return acc[:, :, None] * (target + tw.BIAS)


def rel_rows(got, want):
    """largest error of a row of W relative to the row's largest element: the scale a linear solve's error bound is stated on"""
    return float((np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)).max())


@pytest.mark.parametrize('D', [13, 39, 20, 31])
def test_statistics_at_the_models_means_give_the_identity(D):
    rng, mean, var, acc = synthetic(1, M=4 * (D + 1), D=D)
    cls = np.array([0, 0, 1, 1, 1, -1])
    out = tw.mllr_estimate(mean, var, acc, stats_at(acc, mean), cls, 2, min_occ=1.0)
    assert out['status'].tolist() == [0, 0] and np.nanmax(out['cond']) < COND_MAX
    print('D = %d: |W - [0|I]| = %.2e, cond <= %.1f' % (D, np.abs(out['W'] - tw.identity(D)).max(), np.nanmax(out['cond'])))
    assert np.abs(out['W'] - tw.identity(D)).max() < 1e-10
    np.testing.assert_allclose(out['occ'], [acc[:2].sum(), acc[2:5].sum()], rtol=1e-12)


@pytest.mark.parametrize('D', [13, 39, 20, 31])
def test_a_known_transform_is_recovered(D):
    rng, mean, var, acc = synthetic(2, M=4 * (D + 1), D=D)
    acc[1, ::5] = 0.0                                                                 # dead mixtures, and junk behind them
    acc[3, 7] = np.nan
    A = np.eye(D) * 0.9 + 0.1 * rng.standard_normal((D, D))
    b = rng.standard_normal(D)
    target = mean @ A.T + b
    macc = stats_at(np.where(tw.contributes(acc), acc, 0.0), target)
    macc[1, ::5] = 1e30                                                               # acc == 0: contributes exactly nothing
    out = tw.mllr_estimate(mean, var, acc, macc, None, 1, min_occ=1.0)
    want = np.concatenate([b[:, None], A], axis=1)
    print('D = %d: row-relative error %.2e, cond <= %.1f' % (D, rel_rows(out['W'][0], want), out['cond'].max()))
    assert out['status'].tolist() == [0] and rel_rows(out['W'][0], want) < 1e-10
    new, _ = tw.transform_means(mean, out['W'])
    assert np.abs(new - target).max() < 1e-9
    assert np.isfinite(out['G']).all() and np.allclose(out['G'], np.swapaxes(out['G'], 2, 3))


def test_each_refusal_gives_the_identity_and_its_own_status():
    D = 13
    rng, mean, var, acc = synthetic(3, J=5, M=4 * (D + 1), D=D)
    acc[1] *= 1e-3                                                                    # class 1: occupancy below min_occ
    acc[2, D:] = 0.0                                                                  # class 2: D contributing mixtures, one too few
    mean[3] = 0.0                                                                     # class 3: xi = (1, 0 .. 0): the second pivot is exactly 0
    cls = np.array([0, 1, 2, 3, -1])
    target = mean * 1.1 + 0.3
    out = tw.mllr_estimate(mean, var, acc, stats_at(acc, target), cls, 5, min_occ=5.0)
    assert out['status'].tolist() == [tw.OK, tw.LOW_OCCUPANCY, tw.FEW_MIXTURES, tw.NOT_POSITIVE_DEFINITE, tw.LOW_OCCUPANCY]
    for r in (1, 2, 3, 4):
        assert np.array_equal(out['W'][r], tw.identity(D))
    assert not np.array_equal(out['W'][0], tw.identity(D)) and out['occ'][4] == 0.0
    new, _ = tw.transform_means(mean, out['W'], cls)
    assert np.array_equal(new[1:], mean[1:]) and not np.array_equal(new[0], mean[0])
    # the order of the tests: a class that is short of both occupancy and mixtures reports the occupancy
    assert tw.mllr_estimate(mean, var, acc, stats_at(acc, target), cls, 5, min_occ=1e9)['status'].tolist() == [tw.LOW_OCCUPANCY] * 5
    for bad in (dict(n_classes=0), dict(state_class=np.array([0, 0, 0, 0, 5])), dict(state_class=np.array([0, 0, 0, 0, -2])), dict(min_occ=-1.0),
                dict(min_occ=np.nan)):
        with pytest.raises(ValueError):
            tw.mllr_estimate(mean, var, acc, stats_at(acc, target), **dict(dict(state_class=None, n_classes=1, min_occ=1.0), **bad))


def test_the_limits_of_map():
    rng, mean, var, acc = synthetic(4)
    acc[2, ::4] = 0.0
    acc[4, 3] = np.inf
    data_mean = mean + rng.standard_normal(mean.shape)
    macc = stats_at(np.where(tw.contributes(acc), acc, 0.0), data_mean)
    live = tw.contributes(acc)
    ml = tw.map_means(mean, acc, macc, 0.0)
    assert np.abs(ml - data_mean)[live].max() < 1e-11                                 # tau = 0: the ML mean
    assert np.array_equal(ml[~live], mean[~live])                                     # acc == 0 (or not finite): the mean stays, bit for bit
    far = tw.map_means(mean, acc, macc, 1e18)
    assert np.abs(far - mean).max() < 1e-12                                           # a huge tau leaves the mean
    mid = tw.map_means(mean, acc, macc, 10.0)
    lo, hi = np.minimum(mean, data_mean) - 1e-9, np.maximum(mean, data_mean) + 1e-9
    assert ((mid >= lo) & (mid <= hi)).all()                                          # between the prior and the data
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            tw.map_means(mean, acc, macc, bad)


@pytest.mark.parametrize('D', [13, 26, 39, 48, 1, 2, 12, 14, 15, 20, 30, 31, 40, 46, 47])
def test_the_gpu_tests_inputs_are_well_conditioned(D):
    """cond(G[r, i]) < 1e4 for every accepted class of the models and batches tests/test_gpu_adapt.py runs on, from statistics formed here
    in NumPy (the device's differ from them by its float64 rounding); at least 4 (D + 1) contributing mixtures per accepted class.
    12 .. 47: the dimensions the device pads.  D = 1 and 2: state 5's ALIVE5 = 10 live mixtures are no longer fewer than D + 1, so class 1
    is accepted too (and must then be as well conditioned)."""
    model, frames, gamma = tw.make_case(D)
    acc, macc = tw.numpy_stats(model, frames, gamma)
    assert (acc[2, ::3] == 0).all() and (acc[5, tw.ALIVE5:] == 0).all()
    for cls, R, min_occ in ((None, 1, 1.0), (tw.CLASSES3, 3, tw.MIN_OCC3)):
        out = tw.mllr_estimate(*model[:2], acc, macc, cls, R, min_occ)
        print('D = %d, R = %d: status %s, occ %s, cond <= %s' % (D, R, out['status'], out['occ'], np.nanmax(out['cond'], axis=1)))
        assert out['status'].tolist() == ([tw.OK] if R == 1 else [tw.OK, tw.FEW_MIXTURES if D + 1 > tw.ALIVE5 else tw.OK, tw.LOW_OCCUPANCY])
        members = np.ones(tw.J, bool) if cls is None else cls == 0
        assert tw.contributes(acc[members]).sum() >= 4 * (D + 1)
        assert out['cond'][out['status'] == tw.OK].max() < COND_MAX
        for i in range(D):                                                            # the residual the GPU test asserts holds for the twin itself
            Gm, km, wv = out['G'][0, i], out['k'][0, i], out['W'][0, i]
            assert (np.abs(Gm @ wv - km) <= 1e-10 * (np.abs(Gm) @ np.abs(wv) + np.abs(km))).all()
    if D == 13:                                                                       # the closed-form case: M = 1, J = 64
        rng = np.random.default_rng(5)
        mean, var = rng.standard_normal((64, 1, D)), rng.uniform(0.5, 2.0, (64, 1, D))
        out = tw.mllr_estimate(mean, var, np.full((64, 1), 3.0), stats_at(np.full((64, 1), 3.0), mean), None, 1, 1.0)
        print('closed form: cond <= %.1f' % out['cond'].max())
        assert out['cond'].max() < COND_MAX


class TwinEngine(object):
    """The part of Engine that AcousticModel.adapt_batch touches beyond the E-step, the model adapted by the twin"""

    def __init__(self, model, acc, macc):
        self.model, self.acc, self.macc = model, acc, macc
        self.J, self.M, self.D = model[0].shape
        self.calls = []

    def mllr_estimate(self, state_class=None, n_classes=1, min_occ=1000.0):
        self.calls.append(('estimate', None if state_class is None else state_class.tolist(), n_classes, min_occ))
        self.out = tw.mllr_estimate(*self.model[:2], self.acc, self.macc, state_class, n_classes, min_occ)
        return self.out['W'], self.out['occ'], self.out['status']

    def transform_means(self, W=None, state_class=None, n_classes=1):
        assert W is None
        self.model = (tw.transform_means(self.model[0], self.out['W'], state_class)[0],) + self.model[1:]

    def mstep_map(self, tau):
        self.calls.append(('map', tau))
        self.model = (tw.map_means(self.model[0], self.acc, self.macc, tau),) + self.model[1:]

    def model_download(self):
        return tuple(a.copy() for a in self.model)


def test_adapt_batch_keeps_the_gmm_objects_and_the_engine_in_step(tmp_path, monkeypatch):
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel

    class StubBatch(object):
        def score(self, p): pass
        def forward_backward(self): pass
        def accumulate(self, p): pass
        def get(self, what): return np.array([-10.0, -20.0])
        def close(self): pass

    S, Mx, D = 5, 3, 13
    am = AcousticModel(state_num=S, mix_level=Mx, dct_num=13, delta_1=False, delta_2=False)
    names = ['a', 'b', 'c']
    unit_hmms = {u: am.init_unit(u) for u in names}
    rng = np.random.default_rng(6)
    Jn = len(names) * (S - 2)
    mean, var = rng.standard_normal((Jn, Mx, D)), rng.uniform(0.5, 2.0, (Jn, Mx, D))
    w = np.full((Jn, Mx), 1.0 / Mx)
    am._adopt_model((mean, var, w), names, unit_hmms)
    acc = rng.uniform(1.0, 2.0, (Jn, Mx))
    eng = TwinEngine((mean, var, w), acc, stats_at(acc, mean * 1.2 - 0.4))
    eng.stats_zero = lambda: None
    monkeypatch.setattr(AcousticModel, '_sentence_batch', lambda self, *a: (StubBatch(), None, names, None))
    data = [np.zeros((4, D)), np.zeros((5, D))]
    out = am.adapt_batch([['a', 'b'], ['c']], data, unit_hmms, method='mllr', unit_class={'a': 0, 'b': 0, 'c': -1}, iterations=2, min_occ=1.0, engine=eng)
    assert out['logp'] == [-30.0, -30.0] and len(out['W']) == 2 and out['status'][0].tolist() == [0]
    assert eng.calls[0] == ('estimate', [0] * 6 + [-1] * 3, 1, 1.0)
    for ui, u in enumerate(names):
        for k in range(S - 2):
            assert np.array_equal(unit_hmms[u].profunction[1 + k].model_arrays()[0], eng.model[0][ui * (S - 2) + k])
    assert np.array_equal(eng.model[0][6:], mean[6:]) and not np.array_equal(eng.model[0][:6], mean[:6])
    out = am.adapt_batch([['a', 'b'], ['c']], data, unit_hmms, method='map', tau=4.0, engine=eng)
    assert sorted(out) == ['logp'] and eng.calls[-1] == ('map', 4.0)
    assert np.array_equal(unit_hmms['c'].profunction[1].model_arrays()[0], eng.model[0][6])
    with pytest.raises(ValueError):
        am.adapt_batch([['a']], data[:1], unit_hmms, method='fmllr', engine=eng)
