"""The mix-up rule (include/poccala_hip.h, pcl_model_mixup) as tests/_mixup_twin.py states it: its invariants on random models, the
cases the rule singles out worked by hand, what it refuses, and AcousticModel.mixup_batch's host bookkeeping on a stand-in engine that
grows its model with the twin.  No GPU.  tests/test_gpu_mixup.py holds the device to the same twin on the shapes listed here."""
import numpy as np
import pytest

import _mixup_twin as tw

# (M, M_new, what the case is there for): the shapes tests/test_gpu_mixup.py runs
CASES = [(1, 2, 'one mixture'), (3, 4, 'one split'), (4, 8, 'all split'), (3, 7, 'two rounds'), (5, 6, 'two equal top weights'),
         (4, 8, 'only index 2 live'), (31, 33, 'across the 32-mixture tile edge'), (32, 64, 'a whole tile doubled'), (3, 5, 'the Mpad edge')]


def random_model(seed, J, M, D, what=''):
    """mean, var (J, M, D), weight (J, M); weights distinct within a state unless the case asks otherwise"""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((J, M, D)) * 3.0
    var = rng.uniform(0.05, 4.0, (J, M, D))
    w = rng.uniform(0.1, 1.0, (J, M))
    if what == 'two equal top weights':
        for j in range(J):
            a, b = rng.choice(M, 2, replace=False)
            w[j, a] = w[j, b] = 2.0
    if what == 'only index 2 live':
        w[:] = 0.0
        w[:, 2] = 1.0
        w[0, 0] = np.nan                                              # NaN is not live either
    w = w / np.nansum(w, axis=1, keepdims=True)
    return mean, var, w


@pytest.mark.parametrize('D', [13, 39, 20, 48])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_invariants_on_random_models(case, D):
    M, M_new, what = CASES[case]
    J = 4
    mean, var, w = random_model(10 + case, J, M, D, what)
    mu, vr, wn, origin = tw.mixup(mean, var, w, M_new, 0.2)
    assert mu.shape == vr.shape == (J, M_new, D) and wn.shape == origin.shape == (J, M_new)
    assert np.array_equal(origin[:, :M], np.broadcast_to(np.arange(M), (J, M)))
    assert origin.min() >= 0 and origin.max() < M
    live = w > 0
    for j in range(J):
        # every old mixture's descendants' weights add back to it: at most 14 additions of dyadic multiples, each within 2^-53
        back = np.array([wn[j, origin[j] == i].sum() for i in range(M)])
        np.testing.assert_allclose(back[live[j]], w[j, live[j]], rtol=1e-14, atol=0)
        assert vr[j].tobytes() == var[j, origin[j]].tobytes()         # variances are copies
        assert live[j, origin[j, M:]].all()                           # a mixture without weight is never a parent ...
        for i in np.flatnonzero(~live[j]):                            # ... and stays as it was
            assert mu[j, i].tobytes() == mean[j, i].tobytes() and (origin[j] == i).sum() == 1
            assert wn[j, i].tobytes() == w[j, i].tobytes()
    # perturb = 0: every descendant has its origin's mean, and nothing else differs
    mu0, vr0, w0, origin0 = tw.mixup(mean, var, w, M_new, 0.0)
    assert np.array_equal(origin0, origin) and w0.tobytes() == wn.tobytes() and vr0.tobytes() == vr.tobytes()
    for j in range(J):
        assert np.array_equal(mu0[j], mean[j, origin[j]])


def test_one_split_takes_the_heaviest_and_moves_both_means():
    mean = np.array([[[1.0, -2.0], [5.0, 0.5], [0.0, 3.0]]])
    var = np.array([[[4.0, 0.25], [1.0, 9.0], [0.01, 1.0]]])
    w = np.array([[0.2, 0.5, 0.3]])
    mu, vr, wn, origin = tw.mixup(mean, var, w, 4, 0.2)
    assert origin.tolist() == [[0, 1, 2, 1]]
    assert wn.tolist() == [[0.2, 0.25, 0.3, 0.25]]
    delta = np.float64(0.2) * np.sqrt(var[0, 1])
    assert np.array_equal(mu[0, 1], mean[0, 1] - delta) and np.array_equal(mu[0, 3], mean[0, 1] + delta)
    assert np.array_equal(mu[0, [0, 2]], mean[0, [0, 2]]) and np.array_equal(vr[0, 3], var[0, 1])


def test_ties_go_to_the_lower_index():
    mean, var = np.zeros((1, 5, 3)), np.ones((1, 5, 3))
    w = np.array([[0.1, 0.3, 0.1, 0.3, 0.2]])
    assert tw.mixup(mean, var, w, 6)[3][0, 5] == 1
    assert tw.mixup(mean, var, w, 7)[3][0, 5:].tolist() == [1, 3]
    w = np.full((1, 5), 0.2)
    assert tw.mixup(mean, var, w, 8)[3][0, 5:].tolist() == [0, 1, 2]


def test_more_new_mixtures_than_live_ones_takes_several_rounds():
    """3 -> 7: round one splits all three, round two the heaviest of the six -- slot 0, whose 0.25 ties with its own child in slot 3"""
    mean = np.arange(6, dtype=np.float64).reshape(1, 3, 2)
    var = np.array([[[4.0, 1.0], [0.25, 9.0], [1.0, 1.0]]])
    w = np.array([[0.5, 0.3, 0.2]])
    mu, vr, wn, origin = tw.mixup(mean, var, w, 7, 0.2)
    assert origin.tolist() == [[0, 1, 2, 0, 1, 2, 0]]
    assert wn.tolist() == [[0.125, 0.15, 0.1, 0.25, 0.15, 0.1, 0.125]]
    d0 = np.float64(0.2) * np.sqrt(var[0, 0])
    assert np.array_equal(mu[0, 0], (mean[0, 0] - d0) - d0)          # split twice
    assert np.array_equal(mu[0, 3], mean[0, 0] + d0)                 # born in round one, left alone in round two
    assert np.array_equal(mu[0, 6], (mean[0, 0] - d0) + d0)          # born in round two from the parent as round one left it
    # 1 -> 8 doubles three times: 1, 2, 4 live mixtures
    _, _, w8, o8 = tw.mixup(mean[:, :1], var[:, :1], np.ones((1, 1)), 8, 0.2)
    assert w8.tolist() == [[0.125] * 8] and o8.tolist() == [[0] * 8]


def test_a_mixture_without_weight_is_never_a_parent():
    mean, var, w = random_model(3, 3, 4, 5, 'only index 2 live')
    mu, vr, wn, origin = tw.mixup(mean, var, w, 8, 0.2)
    assert (origin[:, 4:] == 2).all()                                 # rounds of 1, 2, 1: everything descends from index 2
    assert np.array_equal(np.sort(wn[1][origin[1] == 2]), [0.125, 0.125, 0.25, 0.25, 0.25])
    assert np.isnan(wn[0, 0]) and wn[1, 0] == 0.0


def test_what_the_rule_refuses():
    mean, var, w = random_model(4, 3, 4, 5)
    for bad in (4, 3, 0, tw.M_MAX + 1):
        with pytest.raises(ValueError):
            tw.mixup(mean, var, w, bad)
    for bad in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError):
            tw.mixup(mean, var, w, 8, bad)
    for dead in (0.0, np.nan, -1.0):
        w2 = w.copy()
        w2[1] = dead
        with pytest.raises(ValueError, match='state 1'):
            tw.mixup(mean, var, w2, 8)
    tw.mixup(mean, var, w, 8)                                         # (the same arrays pass when nothing is wrong)


class TwinEngine(object):
    """The part of Engine that AcousticModel.mixup_batch touches, its model grown by the twin"""

    def __init__(self):
        self.J = self.M = self.D = 0
        self.loads = 0

    def load_model(self, mean, var, weight):
        self.model = tuple(np.array(a, dtype=np.float64) for a in (mean, var, weight))
        self.J, self.M, self.D = self.model[0].shape
        self.loads += 1

    def mixup(self, M_new, perturb=0.2, want_origin=False):
        out = tw.mixup(*self.model, M_new, perturb)
        self.model, self.M = out[:3], int(M_new)
        return out[3] if want_origin else None

    def model_download(self):
        return tuple(a.copy() for a in self.model)


def test_mixup_batch_keeps_the_gmm_objects_and_the_engine_in_step(tmp_path):
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    S, M, D = 5, 2, 13
    am = AcousticModel(None, 'XIF_tone', parameters_path=str(tmp_path), state_num=S, mix_level=M, dct_num=D, delta_1=False, delta_2=False)
    names = ['b', 'a', 'c']
    unit_hmms = {u: am.init_unit(u) for u in names}
    mean, var, w = random_model(8, len(names) * (S - 2), M, D)
    for ui, u in enumerate(sorted(names)):                            # states unit-major over the SORTED names
        for k in range(S - 2):
            unit_hmms[u].profunction[1 + k].set_model(mean[ui * 3 + k], var[ui * 3 + k], w[ui * 3 + k])
    eng = TwinEngine()
    origin = am.mixup_batch(unit_hmms, 5, perturb=0.3, engine=eng)
    want = tw.mixup(mean, var, w, 5, 0.3)
    assert eng.loads == 1 and np.array_equal(origin, want[3]) and (eng.J, eng.M, eng.D) == (9, 5, D)
    for ui, u in enumerate(sorted(names)):
        for k in range(S - 2):
            g = unit_hmms[u].profunction[1 + k]
            assert g.mixture == 5
            for got, ref in zip(g.model_arrays(), want[:3]):
                assert got.tobytes() == ref[ui * 3 + k].tobytes()
    assert am.init_unit('d').profunction[1].mixture == 5              # the object's own mix_level followed
    am.mixup_batch(unit_hmms, 8, engine=eng)                          # the engine holds the units' shape: nothing is uploaded again
    assert eng.loads == 1 and unit_hmms['a'].profunction[2].mixture == 8
    am.save_parameter('a', unit_hmms['a'])                            # ... and the grown objects can be written
    with pytest.raises(ValueError):
        am.mixup_batch(unit_hmms, 8, engine=eng)                      # not a growth: refused, the objects stay
    assert unit_hmms['a'].profunction[2].mixture == 8
