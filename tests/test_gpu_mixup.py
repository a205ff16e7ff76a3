"""Mix-up on the device (csrc/model_mixup.hip: pcl_model_mixup, Engine.mixup, AcousticModel.mixup_batch) against the NumPy twin of the
rule (tests/_mixup_twin.py, whose own invariants tests/test_mixup_twin.py holds) on the shapes listed there.

Bounds.  origin, weights and variances: exact -- integers, halvings and copies.  Means: the float64 model contract of DESIGN.md section 7
(f7), 1e-10 relative, through tests/_parity.py:hold, which records the measured worst case; the device and the twin run the same rounded
operations (no contraction, a correctly rounded sqrt), so bit equality is expected and asserted behind the bound.  ln b from the
device-made model against ln b after an upload of the downloaded arrays: bit-identical on every route.  perturb = 0 leaves the mixture density as it was: ln b under PCL_F64 within that mode's contract, 1e-9
(DESIGN.md section 2).  Every figure is printed before it is asserted.

The device keeps the model at a padded feature stride (13, 26, 39, 47, 48 or 64).  WIDE_D runs the fill kernel with a host dimension below
that stride (12, 20, 40, 50) and with an even stride (26, 48, 64; 50 -> 64), where none of its two-element stores straddles two mixtures
-- 13, 39 and 47 are odd, there one does.  50 and 64 lie beyond what the adaptation calls take: mix-up has no such limit."""
import numpy as np
import pytest

import _mixup_twin as tw
from _parity import hold
from test_mixup_twin import CASES, random_model

pytestmark = pytest.mark.gpu
RTOL = 1e-10                 # float64 restatements of the model
F64_RTOL = 1e-9              # ln b under PCL_F64
J = 4
WIDE_D = [12, 20, 26, 40, 47, 48, 50, 64]
SMALL_GROWTHS = [(3, 7), (8, 16), (2, 5)]      # 7 and 5 are no multiple of 4: a padded mixture follows the last real one, at an even stride too


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ------------------------------------------------------------------ (a), (b), (e): the grown model against the twin
@pytest.mark.parametrize('D', [13, 39])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_the_grown_model_is_the_twins(eng, case, D):
    M, M_new, what = CASES[case]
    grown_model_is_the_twins(eng, 10 + case, M, M_new, D, what)


@pytest.mark.parametrize('D', WIDE_D)
@pytest.mark.parametrize('M,M_new', SMALL_GROWTHS)
def test_the_grown_model_is_the_twins_at_every_device_stride(eng, M, M_new, D):
    grown_model_is_the_twins(eng, 100 + M, M, M_new, D, 'stride')


def grown_model_is_the_twins(eng, seed, M, M_new, D, what):
    mean, var, w = random_model(seed, J, M, D, what)
    eng.load_model(mean, var, w)
    origin = eng.mixup(M_new, perturb=0.2, want_origin=True)
    assert (eng.J, eng.M, eng.D) == (J, M_new, D)
    tm, tv, tww, to = tw.mixup(mean, var, w, M_new, 0.2)
    m, v, ww = eng.model_download()
    assert origin.dtype == np.int32 and np.array_equal(origin, to)                         # (a)
    assert same_bits(ww, tww) and same_bits(v, tv)
    r = hold('mixup %d->%d D=%d (%s)' % (M, M_new, D, what), 'mean vs twin', m, tm, RTOL)   # (b)
    print('%d -> %d, D = %d (%s): max |d mean| = %.3e, bit-equal: %s' % (M, M_new, D, what, r['max_abs'], same_bits(m, tm)))
    assert same_bits(m, tm)
    st = eng.stats_download()                                                               # (e)
    assert st['acc'].shape == (J, M_new) and st['alpha_acc'].shape == (J,) and st['mean_acc'].shape == st['cov_acc'].shape == (J, M_new, D)
    assert all(not a.any() for a in st.values())
    assert eng.mixup(M_new + 1) is None                                                     # (origin on request only)
    m2 = eng.model_download()[0]
    assert same_bits(m2, tw.mixup(tm, tv, tww, M_new + 1, 0.2)[0])                         # a grown model grows again


@pytest.mark.parametrize('M,M_new', [(500, 513), (300, 2049), (8000, 8192)])
def test_every_instance_of_the_plan_kernel(eng, M, M_new):
    """the plan kernel is built for 512, 2048 and 8192 slots per state: the first size past each threshold, and the largest model"""
    Jn, D = 3, 13
    mean, var, w = random_model(30, Jn, M, D)
    w[1, ::3] = 0.0                                                                          # a state with a third of its mixtures dead
    w[2, 7:40] = w[2, 7]                                                                     # a run of equal weights
    eng.load_model(mean, var, w)
    origin = eng.mixup(M_new, perturb=0.2, want_origin=True)
    tm, tv, tww, to = tw.mixup(mean, var, w, M_new, 0.2)
    m, v, ww = eng.model_download()
    assert np.array_equal(origin, to) and same_bits(ww, tww) and same_bits(v, tv)
    r = hold('mixup %d->%d D=%d' % (M, M_new, D), 'mean vs twin', m, tm, RTOL)
    print('%d -> %d: max |d mean| = %.3e, bit-equal: %s' % (M, M_new, r['max_abs'], same_bits(m, tm)))
    assert same_bits(m, tm)


def test_two_runs_give_the_same_bits(eng):
    mean, var, w = random_model(40, J, 31, 39)
    w[:, 5:9] = w[:, 4:5]                                                                    # runs of equal weights
    out = []
    for _ in range(2):
        eng.load_model(mean, var, w)
        o = eng.mixup(64, perturb=0.25, want_origin=True)
        out.append((o,) + eng.model_download())
    for a, b in zip(*out):
        assert same_bits(a, b)
    assert np.array_equal(out[0][0], tw.mixup(mean, var, w, 64, 0.25)[3])


# ------------------------------------------------------------------ (c), (d): scoring from the device-made model
def scoring_model(seed, M, D, split):
    """a model whose states stay on the matrix pipe; split: two tight mixtures per state far from its centre leave the pipe"""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((J, M, D)) * 0.3
    var = rng.uniform(0.5, 2.0, (J, M, D))
    w = rng.uniform(0.2, 1.0, (J, M))
    if split:
        mean[:, :2] += 4.0
        var[:, :2] = 0.5
        w[:, 0] = 2.0                                                  # one of the off-pipe mixtures is heavy enough to be split itself
    return mean, var, w / w.sum(axis=1, keepdims=True)


def lnb(eng, T, begin, precision):
    b = eng.all_state_batch(T, begin)
    b.score(precision)
    B = b.get('B')
    b.close()
    return B


@pytest.mark.parametrize('route', ['default', 'split', 'f64'])
def test_lnb_from_the_device_made_model_equals_an_upload(eng, route):
    lnb_equals_an_upload(eng, route, 8, 16, 39, np.array([37, 20, 64], dtype=np.int32), np.array([0, 40, 61], dtype=np.int64))


@pytest.mark.parametrize('D', [12, 40])
@pytest.mark.parametrize('route', ['default', 'split', 'f64'])
def test_the_padding_stays_zero(eng, route, D):
    """the device rows are 13 and 47 wide, and an upload zeroes the padded columns: a padded mean, variance or coefficient the fill left
    non-zero would move the bits of ln b; one utterance of every row of the frame matrix, 15 mixtures padded to 16"""
    lnb_equals_an_upload(eng, route, 8, 15, D, np.array([130], dtype=np.int32), np.array([0], dtype=np.int64))


def lnb_equals_an_upload(eng, route, M, M_new, D, T, begin):
    from poccala_amd import PCL_F32, PCL_F64
    P = PCL_F64 if route == 'f64' else PCL_F32
    mean, var, w = scoring_model(50, M, D, route == 'split')
    rng = np.random.default_rng(51)
    frames = (rng.standard_normal((130, D)) * 1.2).astype(np.float32)
    eng.load_frames(frames)
    eng.load_model(mean, var, w)
    eng.mixup(M_new, perturb=0.2)
    n_off, limit = eng.model_split_info()
    print('%s: off-pipe mixtures per state %s, limit %d' % (route, n_off, limit))
    if route == 'split':
        assert n_off.min() > 0 and n_off.max() <= limit              # the states ARE on the split route
    elif route == 'default':
        assert n_off.max() == 0
    B1 = lnb(eng, T, begin, P)
    m, v, ww = eng.model_download()
    eng.load_model(m, v, ww)
    B2 = lnb(eng, T, begin, P)
    for u in range(len(T)):
        assert np.isfinite(B1[u][1:-1]).all() and same_bits(B1[u], B2[u])


@pytest.mark.parametrize('M,M_new', [(3, 7), (8, 16)])
def test_without_perturbation_the_density_stays(eng, M, M_new):
    density_stays(eng, M, M_new, 13, 'mixup perturb 0, %d->%d' % (M, M_new))


@pytest.mark.parametrize('D', WIDE_D)
@pytest.mark.parametrize('M,M_new', [(3, 7), (8, 16)])
def test_without_perturbation_the_density_stays_at_every_device_stride(eng, M, M_new, D):
    density_stays(eng, M, M_new, D, 'mixup perturb 0, %d->%d D=%d' % (M, M_new, D))


def density_stays(eng, M, M_new, D, tag):
    from poccala_amd import PCL_F64
    mean, var, w = scoring_model(60, M, D, False)
    rng = np.random.default_rng(61)
    T, begin = np.array([50, 33], dtype=np.int32), np.array([0, 50], dtype=np.int64)
    eng.load_frames(rng.standard_normal((83, D)) * 1.2)
    eng.load_model(mean, var, w)
    before = lnb(eng, T, begin, PCL_F64)
    eng.mixup(M_new, perturb=0.0)
    after = lnb(eng, T, begin, PCL_F64)
    for u in range(len(T)):
        hold(tag, 'ln b (PCL_F64) before vs after', after[u][1:-1], before[u][1:-1], F64_RTOL)


# ------------------------------------------------------------------ (f): EM from the grown model, on segments made before the call
def test_em_on_earlier_segments_runs_from_the_grown_model(eng):
    from poccala_amd import PCL_F64
    M, M_new, D = 2, 5, 13
    counts = [40, 4, 25, 5]                                           # state 1 has fewer frames than M_new: skipped after the mix-up
    mean, var, w = scoring_model(70, M, D, False)
    rng = np.random.default_rng(71)
    state = np.concatenate([np.full(n, j, dtype=np.int32) for j, n in enumerate(counts)] + [np.full(3, -1, dtype=np.int32)])
    rng.shuffle(state)
    frames = mean[np.maximum(state, 0), rng.integers(0, M, len(state))] + rng.standard_normal((len(state), D))
    eng.load_frames(frames)
    eng.load_model(mean, var, w)
    seg = eng.segments(state, J=J)
    it0, _ = seg.em(precision=PCL_F64)
    assert (it0 >= 0).all()
    trained = eng.model_download()
    eng.mixup(M_new, perturb=0.2)
    assert not any(a.any() for a in eng.stats_download().values())    # the first EM's statistics are gone with the old shape
    grown = eng.model_download()
    twin = tw.mixup(*trained, M_new, 0.2)[:3]
    for a, b in zip(grown, twin):
        assert same_bits(a, b)
    it1, q1 = seg.em(precision=PCL_F64)
    print('frames per state %s: EM loop bodies %s -> %s after the mix-up' % (counts, it0, it1))
    assert np.array_equal(it1 >= 0, np.array(counts) >= M_new) and (it1[np.array(counts) < M_new] == -1).all()
    got = eng.model_download()
    eng.load_model(*twin)
    it2, q2 = seg.em(precision=PCL_F64)
    seg.close()
    assert same_bits(it1, it2) and same_bits(q1, q2)
    for a, b in zip(got, eng.model_download()):
        assert same_bits(a, b)
    assert same_bits(got[0][1], twin[0][1])                           # the skipped state kept the grown model


# ------------------------------------------------------------------ (g), (h): what is refused, and what the call gives back
def test_refused_calls_leave_the_model_and_the_pool_as_they_were(eng):
    from poccala_amd import Engine, PoccalaHipError
    with pytest.raises(PoccalaHipError) as ei:
        eng.mixup(4)                                                  # no model
    print(ei.value)
    assert ei.value.code == -3
    mean, var, w = random_model(80, J, 4, 13)
    w[2] = [0.0, np.nan, -0.5, 0.0]                                   # state 2 has no live mixture
    eng.load_model(mean, var, w)
    blocks = Engine.pool_stats()['handed_out_blocks']
    for args in ((4,), (3,), (0,), (8193,), (8, -0.1), (8, np.nan), (8, np.inf), (8, 0.2)):
        with pytest.raises(PoccalaHipError) as ei:
            eng.mixup(*args, want_origin=True)
        print(args, ei.value)
        assert ei.value.code == -1 and len(str(ei.value)) > 40
        if args == (8, 0.2):
            assert 'state 2' in str(ei.value)
        assert (eng.J, eng.M, eng.D) == (J, 4, 13)
        for a, b in zip(eng.model_download(), (mean, var, w)):
            assert same_bits(a, b)
        assert Engine.pool_stats()['handed_out_blocks'] == blocks
    w[2] = 0.25
    eng.load_model(mean, var, w)                                      # still usable
    eng.mixup(8)
    assert same_bits(eng.model_download()[0], tw.mixup(mean, var, w, 8)[0])


@pytest.mark.parametrize('M,M_new', [(3, 5), (32, 64)])
def test_the_call_gives_back_every_block_it_took(eng, M, M_new):
    from poccala_amd import Engine
    mean, var, w = random_model(90, J, M, 39)
    eng.load_model(mean, var, w)
    before = Engine.pool_stats()
    eng.mixup(M_new, want_origin=True)
    after = Engine.pool_stats()
    print('handed-out blocks %d -> %d, bytes %d -> %d' % (before['handed_out_blocks'], after['handed_out_blocks'], before['handed_out_bytes'],
                                                          after['handed_out_bytes']))
    assert after['handed_out_blocks'] == before['handed_out_blocks']   # a model of the new shape in the old one's place, nothing else
    assert after['handed_out_bytes'] > before['handed_out_bytes']


# ------------------------------------------------------------------ (i): the chain flat start / EM / mix-up / EM
def test_mixup_batch_then_training_continues_without_clustering(eng, monkeypatch):
    from poccala_amd import synth
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    from poccala_amd.engine import Segments
    units_n, M, D, U, L, T, S = 3, 2, 13, 6, 3, 90, 5
    mean, var, w, _ = synth.make_model(units_n, M, D, seed=21)
    labels = synth.make_labels(U, L, units_n, seed=24)
    assert len(set(int(i) for lab in labels for i in lab)) == units_n
    frames = synth.make_peaked_frames(labels, T, mean * 4, var, seed=23)
    names = ['u%d' % i for i in range(units_n)]
    am = AcousticModel(state_num=S, mix_level=M, dct_num=13, delta_1=False, delta_2=False)
    unit_hmms = {u: am.init_unit(u) for u in names}
    data_list = [frames[u * T:(u + 1) * T].astype(np.float64) for u in range(U)]
    name_labels = [[names[i] for i in lab] for lab in labels]
    am.init_segments_batch(name_labels, data_list, unit_hmms, engine=eng)                    # clustering + EM at M = 2
    trained = eng.model_download()
    origin = am.mixup_batch(unit_hmms, 4, engine=eng)
    tm, tv, tww, to = tw.mixup(*trained, 4, 0.2)
    assert np.array_equal(origin, to) and eng.M == 4
    for ui, u in enumerate(names):
        for k in range(S - 2):
            g = unit_hmms[u].profunction[1 + k]
            assert g.mixture == 4
            for got, want in zip(g.model_arrays(), (tm, tv, tww)):
                assert same_bits(got, want[ui * (S - 2) + k])
    calls = []
    real = Segments.kmeans
    monkeypatch.setattr(Segments, 'kmeans', lambda self, *a, **k: calls.append(a) or real(self, *a, **k))
    out = am.train_segments_batch(name_labels, data_list, unit_hmms, mix_level=None, engine=eng)
    assert calls == [] and eng.M == 4                                                         # GMM.em from the grown model, no k-means
    for u in names:
        iters, q, skipped = out[u]
        print('%s: frames per state %s, EM loop bodies %s' % (u, am.last_segment_counts[u], iters))
        assert np.array_equal(iters >= 0, am.last_segment_counts[u] >= 4) and (iters >= 0).any()
        assert all(unit_hmms[u].profunction[1 + k].mixture == 4 for k in range(S - 2))
    am.train_segments_batch(name_labels, data_list, unit_hmms, mix_level=2, engine=eng)      # (the spy sees a change of mix_level)
    assert len(calls) == 1
