"""Speaker adaptation on the device (csrc/model_adapt.hip: pcl_mllr_estimate, pcl_model_transform_means, pcl_mstep_map; Engine.mllr_estimate /
transform_means / mstep_map; AcousticModel.adapt_batch) against the NumPy twin of the rules (tests/_adapt_twin.py, whose own invariants
and the conditioning of the inputs used here tests/test_adapt_twin.py holds).

The statistics come from a real accumulate pass under PCL_F64 on a batch whose state posteriors are set with set_posteriors; the twin is
fed what stats_download() and model_download() return, so only the new code is under comparison.

Bounds.  G and k are not read back: they are held through the RESIDUAL, |G w - k| <= 1e-10 (|G| |w| + |k|) elementwise with the twin's G
and k and the device's w, which does not depend on the conditioning.  W against the twin: 1e-10 relative, element by element (RTOL of
DESIGN.md section 7 (f7)), on inputs whose cond(G) tests/test_adapt_twin.py keeps below 1e4 (measured there: below 10).  Transformed
means against the twin: the same 1e-10 relative, and bit equality behind it (the apply kernel and the twin run the same rounded
operations in the same order, no contraction).  occ: 1e-10 relative; statuses exact.  Everything the calls must not touch:
bit-identical.  MAP against the twin: 1e-10 relative, bit equality behind it.  MAP at tau = 0 against pcl_mstep where acc > 0: 1e-10
relative plus 1e-10 absolute (both routes subtract the bias of 100 from a number of its size; that rounding is 1e-14).  Closed form and
ln P(O): 1e-9, the PCL_F64 contract of DESIGN.md section 2.  Every figure is printed before it is asserted.

The padded mixtures of the device layout (M = 70 is padded to 72) and its padded feature columns (the device keeps D at 13, 26, 39, 47, 48
or 64) cannot be read through the C-ABI, whose downloads strip them.  They are held through their effect: the dimensions of PADDED_D run
every kernel with a host dimension below the device stride, and test_the_padding_stays_zero compares ln b from the model a call left with
ln b after an upload of the downloaded arrays, bit for bit -- a padded mean, variance or coefficient that a call made non-zero breaks it.
D = 1 and 2 (SMALL_D) have 10 live mixtures in state 5 >= D + 1, so class 1 is no longer short of mixtures: there the statuses are the
twin's, and at least one class must be accepted.  D > 48: the estimate and the transform are refused; pcl_mstep_map has no solve and no
limit (include/poccala_hip.h), and is held to the twin at D = 50 and 64."""
import numpy as np
import pytest

import _adapt_twin as tw
from _parity import hold

pytestmark = pytest.mark.gpu
RTOL = 1e-10                 # float64 restatements of the model
F64_RTOL = 1e-9              # PCL_F64
CHUNK = '97'                 # mixtures per K-chunk: 490 = 5 x 97 + 5, class 0 of CLASSES3 280 = 2 x 97 + 86 -- ragged last chunks, ragged k-steps


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def accumulate(eng, model, frames, gamma):
    """model and frames up, one PCL_F64 accumulate pass with the given state posteriors (F, J) -> the statistics as downloaded"""
    from poccala_amd import PCL_F64
    eng.load_model(*model)
    eng.load_frames(np.asarray(frames, dtype=np.float64))
    F = len(frames)
    b = eng.all_state_batch(np.array([F], dtype=np.int32), np.array([0], dtype=np.int64))
    b.score(PCL_F64)
    with np.errstate(divide='ignore'):
        lg = np.concatenate([np.full((1, F), -np.inf), np.log(gamma.T), np.full((1, F), -np.inf)])
    b.set_posteriors([lg])
    eng.stats_zero()
    b.accumulate(PCL_F64)
    st = eng.stats_download()
    b.close()
    return st


# Host dimensions below the device stride, and what each reaches in the split-K GEMM (16-wide tiles over D + 2 columns, k the last one):
# 12 -> 13 (one padded column, one tile), 14 -> 26 (k in column 15 of the only tile), 15 -> 26 (a second tile that holds only k),
# 20 -> 26 (interior), 30 -> 39 (k in column 15 of the second tile), 31 -> 39 (a third tile of k alone), 40 -> 47 (7 padded columns),
# 46 -> 47 (k in column 15 of the third tile), 47 -> 47 (a fourth tile of k alone)
PADDED_D = [12, 14, 15, 20, 30, 31, 40, 46, 47]
TILE_EDGE_D = [14, 15, 30, 31, 46, 47]
APPLY_D = [12, 20, 40, 47]
SMALL_D = [1, 2]             # n = 2 and 3; a 13-wide device row that is almost all padding

_CASES = {}


def case(D):
    if D not in _CASES:
        _CASES[D] = tw.make_case(D)
    return _CASES[D]


def worst_element(got, want):
    """the element with the largest relative error: (relative error, |want| there, |want|'s row maximum)"""
    with np.errstate(all='ignore'):
        rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == want, 0.0, np.inf))
    at = np.unravel_index(np.argmax(rel), rel.shape)
    return float(rel[at]), float(abs(want[at])), float(np.abs(want[at[:-1]]).max())


# ------------------------------------------------------------------ estimate and apply against the twin
@pytest.mark.parametrize('D', [13, 39])
@pytest.mark.parametrize('what', ['R1', 'R3', 'R1-default-chunk', 'R3-valu'])
def test_estimate_and_apply_are_the_twins(eng, monkeypatch, D, what):
    estimate_and_apply(eng, monkeypatch, D, what)


@pytest.mark.parametrize('D', [26, 48])
@pytest.mark.parametrize('what', ['R3', 'R3-valu'])
def test_the_other_instances_of_the_gemm_kernels(eng, monkeypatch, D, what):
    """the GEMM kernels are built for 1 to 4 tiles of 16 across D + 2: D = 13 and 39 above are 1 and 3, these are 2 and 4 (the widest: 10
    accumulator tiles, 80 KB of LDS for the wave sum)"""
    estimate_and_apply(eng, monkeypatch, D, what)


@pytest.mark.parametrize('D,what', [(D, 'R3') for D in PADDED_D] + [(D, 'R3-valu') for D in TILE_EDGE_D] + [(D, 'R1') for D in APPLY_D])
def test_estimate_and_apply_below_the_device_stride(eng, monkeypatch, D, what):
    """host dimension < device stride (PADDED_D): a stride used for a dimension or a slip at a tile edge of the GEMM shows here first"""
    estimate_and_apply(eng, monkeypatch, D, what)


@pytest.mark.parametrize('D', SMALL_D)
@pytest.mark.parametrize('what', ['R1', 'R3', 'R3-valu'])
def test_estimate_and_apply_at_the_smallest_dimensions(eng, monkeypatch, D, what):
    estimate_and_apply(eng, monkeypatch, D, what)


def estimate_and_apply(eng, monkeypatch, D, what):
    model, frames, gamma = case(D)
    R, cls, min_occ = (3, tw.CLASSES3, tw.MIN_OCC3) if what.startswith('R3') else (1, None, 1.0)
    if 'default' not in what:
        monkeypatch.setenv('PCL_MLLR_CHUNK', CHUNK)
    if 'valu' in what:
        monkeypatch.setenv('PCL_MLLR_VALU', '1')
    st = accumulate(eng, model, frames, gamma)
    before = eng.model_download()
    assert all(same_bits(a, b) for a, b in zip(before, model))                                    # the download is the upload, at every D
    assert (st['acc'][2, ::3] == 0).all() and (st['acc'][5, tw.ALIVE5:] == 0).all()              # dead mixtures: acc == 0 exactly
    W, occ, status = eng.mllr_estimate(cls, R, min_occ)
    W2, occ2, status2 = eng.mllr_estimate(cls, R, min_occ)
    assert same_bits(W, W2) and same_bits(occ, occ2) and same_bits(status, status2)               # two runs, the same bytes
    for a, b in zip(eng.model_download(), before):
        assert same_bits(a, b)                                                                    # the estimate changes nothing
    t = tw.mllr_estimate(before[0], before[1], st['acc'], st['mean_acc'], cls, R, min_occ)
    tag = 'adapt D=%d %s' % (D, what)
    print('%s: status %s (twin %s), occ %s, cond(G) <= %.1f' % (tag, status, t['status'], occ, np.nanmax(t['cond'][0])))
    assert status.dtype == np.int32 and status.tolist() == t['status'].tolist()
    if D + 1 > tw.ALIVE5:
        assert status.tolist() == ([0] if R == 1 else [tw.OK, tw.FEW_MIXTURES, tw.LOW_OCCUPANCY])
    assert status[0] == tw.OK                                                                     # (SMALL_D: the twin's statuses, one class accepted at least)
    assert np.nanmax(t['cond'][0]) < 1e4
    hold(tag, 'occ vs twin', occ, t['occ'], RTOL)
    worst = 0.0
    for i in range(D):                                                                            # the residual: G and k
        Gm, km, wv = t['G'][0, i], t['k'][0, i], W[0, i]
        res, scale = np.abs(Gm @ wv - km), np.abs(Gm) @ np.abs(wv) + np.abs(km)
        worst = max(worst, float((res / scale).max()))
    print('%s: max |G w - k| / (|G||w| + |k|) = %.3e' % (tag, worst))
    assert worst <= RTOL
    print('%s: W vs twin, worst element: relative %.3e at |w| = %.3e (row maximum %.3e)' % ((tag,) + worst_element(W, t['W'])))
    r = hold(tag, 'W vs twin', W, t['W'], RTOL)
    print('%s: max |dW| = %.3e' % (tag, r['max_abs']))
    for k in range(R):
        assert same_bits(W[k], tw.identity(D)) == (status[k] != tw.OK)                            # refused: the identity
    eng.transform_means(None, cls, R)
    m1, v1, w1 = eng.model_download()
    assert same_bits(v1, before[1]) and same_bits(w1, before[2])                                  # variances and weights: untouched
    tm = tw.transform_means(before[0], W, cls)[0]
    print('%s: transformed means bit-equal to the twin\'s: %s' % (tag, same_bits(m1, tm)))
    r = hold(tag, 'transformed means vs twin', m1, tm, RTOL)
    print('%s: max |d mean| = %.3e' % (tag, r['max_abs']))
    assert same_bits(m1, tm)
    moved = np.ones(tw.J, bool) if cls is None else np.isin(cls, np.flatnonzero(status == tw.OK))
    assert same_bits(m1[~moved], before[0][~moved])                                               # class -1 and refused classes keep their bits
    assert not same_bits(m1[moved], before[0][moved])
    eng.load_model(*before)                                                                       # (drops the resident estimate)
    eng.transform_means(W, cls, R)
    for a, b in zip(eng.model_download(), (m1, v1, w1)):
        assert same_bits(a, b)                                                                    # explicit W == the resident one


def test_a_class_whose_pivot_is_zero_is_refused(eng, monkeypatch):
    """every mean of the class is exactly 0: xi = (1, 0 .. 0), G = diag(sum c, 0 .. 0) exactly, the second pivot is 0"""
    monkeypatch.setenv('PCL_MLLR_CHUNK', CHUNK)
    D = 13
    (mean, var, w), frames, gamma = case(D)
    mean = mean.copy()
    mean[3:] = 0.0
    cls = np.array([0, 0, 0, 1, 1, 1, 1], dtype=np.int32)
    st = accumulate(eng, (mean, var, w), frames, gamma)
    W, occ, status = eng.mllr_estimate(cls, 2, 1.0)
    t = tw.mllr_estimate(mean, var, st['acc'], st['mean_acc'], cls, 2, 1.0)
    print('status %s, twin %s' % (status, t['status']))
    assert status.tolist() == t['status'].tolist() == [tw.OK, tw.NOT_POSITIVE_DEFINITE] and same_bits(W[1], tw.identity(D))
    print('W vs twin, worst element: relative %.3e at |w| = %.3e (row maximum %.3e)' % worst_element(W, t['W']))
    hold('adapt pivot', 'W vs twin', W, t['W'], RTOL)
    eng.transform_means(None, cls, 2)
    assert same_bits(eng.model_download()[0][3:], mean[3:])


# ------------------------------------------------------------------ closed form, no twin
def test_a_known_transform_comes_back_from_frames(eng):
    from poccala_amd import PCL_F64
    Jn, D, per = 64, 13, 2
    rng = np.random.default_rng(7)
    mean, var = rng.standard_normal((Jn, 1, D)), rng.uniform(0.5, 2.0, (Jn, 1, D))
    A = np.eye(D) * 0.9 + 0.1 * rng.standard_normal((D, D))
    b = rng.standard_normal(D)
    frames = np.repeat(mean[:, 0] @ A.T + b, per, axis=0)                                         # every frame of state j is A mu_j + b
    gamma = np.repeat(np.eye(Jn), per, axis=0)                                                    # one-hot posteriors
    eng.load_model(mean, var, np.ones((Jn, 1)))
    eng.load_frames(frames)
    bt = eng.all_state_batch(np.array([len(frames)], dtype=np.int32), np.array([0], dtype=np.int64))
    bt.score(PCL_F64)
    with np.errstate(divide='ignore'):
        bt.set_posteriors([np.concatenate([np.full((1, len(frames)), -np.inf), np.log(gamma.T), np.full((1, len(frames)), -np.inf)])])
    eng.stats_zero()
    bt.accumulate(PCL_F64)
    bt.close()
    W, occ, status = eng.mllr_estimate(None, 1, 1.0)
    want = np.concatenate([b[:, None], A], axis=1)[None]
    print('closed form: status %s, occ %s, max |dW| = %.3e' % (status, occ, np.abs(W - want).max()))
    assert status.tolist() == [0]
    hold('adapt closed form', 'occ', occ, [float(Jn * per)], F64_RTOL)
    print('closed form: worst element: relative %.3e at |w| = %.3e (row maximum %.3e)' % worst_element(W, want))
    hold('adapt closed form', 'W vs [b | A]', W, want, F64_RTOL)


# ------------------------------------------------------------------ the EM guarantee, through AcousticModel.adapt_batch
@pytest.mark.parametrize('method', ['mllr', 'map'])
def test_an_iteration_raises_the_likelihood(eng, method):
    from poccala_amd import PCL_F64, synth
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    units_n, M, D, U, L, T, S = 3, 4, 13, 6, 3, 90, 5
    mean, var, w, _ = synth.make_model(units_n, M, D, seed=31)
    labels = synth.make_labels(U, L, units_n, seed=34)
    assert len(set(int(i) for lab in labels for i in lab)) == units_n
    frames = synth.make_peaked_frames(labels, T, mean * 1.15 + 0.4, var, seed=33)                 # the model's means, scaled and shifted
    names = ['u%d' % i for i in range(units_n)]
    am = AcousticModel(state_num=S, mix_level=M, dct_num=13, delta_1=False, delta_2=False)
    unit_hmms = {u: am.init_unit(u) for u in names}
    am._adopt_model((mean, var, w), names, unit_hmms)
    data_list = [frames[u * T:(u + 1) * T].astype(np.float64) for u in range(U)]
    name_labels = [[names[i] for i in lab] for lab in labels]
    out = am.adapt_batch(name_labels, data_list, unit_hmms, method=method, iterations=2, min_occ=1.0, tau=10.0, precision=PCL_F64, engine=eng)
    before, after = out['logp']
    print('%s: total ln P(O) %.6f -> %.6f%s' % (method, before, after, '' if method == 'map' else ', status %s' % out['status'][0]))
    assert after >= before - F64_RTOL * abs(before) and after > before
    if method == 'mllr':
        assert out['status'][0].tolist() == [0] and out['W'][0].shape == (1, D, D + 1)
    got = eng.model_download()
    assert same_bits(got[1], var) and same_bits(got[2], w) and not same_bits(got[0], mean)
    for ui, u in enumerate(names):                                                                # the GMM objects follow the device
        for k in range(S - 2):
            for a, b in zip(unit_hmms[u].profunction[1 + k].model_arrays(), got):
                assert same_bits(a, b[ui * (S - 2) + k])


# ------------------------------------------------------------------ scoring sees the model an upload would give
def lnb(eng, T, begin, precision):
    b = eng.all_state_batch(T, begin)
    b.score(precision)
    B = b.get('B')
    b.close()
    return B


@pytest.mark.parametrize('route', ['default', 'f64'])
@pytest.mark.parametrize('how', ['mllr', 'map'])
def test_lnb_after_the_call_equals_an_upload(eng, route, how):
    from poccala_amd import PCL_F32, PCL_F64
    P = PCL_F64 if route == 'f64' else PCL_F32
    D = 39
    model, frames, gamma = case(D)
    accumulate(eng, model, frames, gamma)
    if how == 'mllr':
        assert eng.mllr_estimate(None, 1, 1.0)[2].tolist() == [0]
        eng.transform_means()
    else:
        eng.mstep_map(5.0)
    T, begin = np.array([37, 64], dtype=np.int32), np.array([0, 40], dtype=np.int64)
    eng.load_frames(np.asarray(frames[:130], dtype=np.float32))
    B1 = lnb(eng, T, begin, P)
    eng.load_model(*eng.model_download())
    B2 = lnb(eng, T, begin, P)
    for u in range(len(T)):
        assert np.isfinite(B1[u][1:-1]).any() and same_bits(B1[u], B2[u])


def split_model(D):
    mean, var, w = [a.copy() for a in case(D)[0]]
    mean[:, :3] += 3.0
    var[:, :3] = 0.02                                                                             # three tight mixtures far from the centre: off the matrix pipe
    return mean, var, w


def known_transform(D, seed=3):
    rng = np.random.default_rng(seed)
    return np.concatenate([0.3 * rng.standard_normal((D, 1)), np.eye(D) * 0.9 + 0.05 * rng.standard_normal((D, D))], axis=1)[None]


def lnb_all_rows(eng, precision):
    return lnb(eng, np.array([eng.F], dtype=np.int32), np.array([0], dtype=np.int64), precision)[0]


@pytest.mark.parametrize('how', ['mllr', 'map'])
@pytest.mark.parametrize('D', [12, 40])
def test_the_padding_stays_zero(eng, how, D):
    """ln b over every row from the model the call left == ln b after an upload of the arrays it downloads, on the default, the split and
    the PCL_F64 route: the upload zeroes every padded column, so a padded mean or coefficient the call wrote would move the bits"""
    from poccala_amd import PCL_F32, PCL_F64
    _, frames, gamma = case(D)
    for route, model in (('default', case(D)[0]), ('split', split_model(D))):
        accumulate(eng, model, frames, gamma)
        before = eng.model_download()
        if how == 'mllr':
            eng.transform_means(known_transform(D))
        else:
            eng.mstep_map(5.0)
        assert not same_bits(eng.model_download()[0], before[0])
        if route == 'split':
            assert eng.model_split_info()[0].min() > 0                                            # the states ARE on the split route
        B1 = {P: lnb_all_rows(eng, P) for P in (PCL_F32, PCL_F64)}
        eng.load_model(*eng.model_download())
        for P in (PCL_F32, PCL_F64):
            assert np.isfinite(B1[P][1:-1]).any() and same_bits(B1[P], lnb_all_rows(eng, P)), (route, P)


# ------------------------------------------------------------------ MAP
@pytest.mark.parametrize('D', [13, 39] + SMALL_D + APPLY_D + [50, 64])
def test_map_means_are_the_twins(eng, D):
    model, frames, gamma = case(D)
    st = accumulate(eng, model, frames, gamma)
    before = eng.model_download()
    eng.mstep_map(7.5)
    m, v, w = eng.model_download()
    tm = tw.map_means(before[0], st['acc'], st['mean_acc'], 7.5)
    r = hold('map D=%d' % D, 'mean vs twin', m, tm, RTOL)
    print('MAP D = %d: max |d mean| = %.3e, bit-equal: %s' % (D, r['max_abs'], same_bits(m, tm)))
    assert same_bits(m, tm)
    assert same_bits(v, before[1]) and same_bits(w, before[2])
    dead = ~tw.contributes(st['acc'])
    assert dead.any() and same_bits(m[dead], before[0][dead]) and not same_bits(m[~dead], before[0][~dead])
    accumulate(eng, model, frames, gamma)                                                         # tau = 0 against pcl_mstep, same statistics
    eng.mstep_map(0.0)
    m0 = eng.model_download()[0]
    st2 = accumulate(eng, model, frames, gamma)
    eng.mstep(1e-3)
    ml = eng.model_download()[0]
    live = tw.contributes(st2['acc'])
    r = hold('map D=%d' % D, 'tau = 0 vs pcl_mstep', m0[live], ml[live], RTOL, atol=RTOL)
    print('MAP tau = 0 vs mstep: max |d mean| = %.3e' % r['max_abs'])


# ------------------------------------------------------------------ what is refused, and what the calls give back
def test_refused_calls_leave_the_model_as_it_was(eng):
    from poccala_amd import PoccalaHipError
    D = 13
    for call in (lambda: eng.mllr_estimate(), lambda: eng.transform_means(), lambda: eng.mstep_map(1.0)):
        with pytest.raises(PoccalaHipError) as ei:
            call()                                                                                # no model, no statistics
        assert ei.value.code == -3
    model, frames, gamma = case(D)
    accumulate(eng, model, frames, gamma)
    before = eng.model_download()
    bad_cls, low_cls = tw.CLASSES3.copy(), tw.CLASSES3.copy()
    bad_cls[3], low_cls[0] = 3, -2
    ident = np.stack([tw.identity(D)] * 3)
    calls = [lambda: eng.mllr_estimate(None, 0), lambda: eng.mllr_estimate(bad_cls, 3), lambda: eng.mllr_estimate(low_cls, 3),
             lambda: eng.mllr_estimate(None, 1, -1.0), lambda: eng.mllr_estimate(None, 1, np.nan), lambda: eng.mllr_estimate(None, 1, np.inf),
             lambda: eng.transform_means(ident, bad_cls, 3), lambda: eng.transform_means(ident[:0], None, 0),
             lambda: eng.transform_means(None, None, 1),                                          # nothing estimated yet
             lambda: eng.mstep_map(-0.5), lambda: eng.mstep_map(np.nan), lambda: eng.mstep_map(np.inf)]
    for k, call in enumerate(calls):
        with pytest.raises(PoccalaHipError) as ei:
            call()
        print(k, ei.value)
        assert ei.value.code == -1 and len(str(ei.value)) > 40
        for a, b in zip(eng.model_download(), before):
            assert same_bits(a, b)
    eng.mllr_estimate(tw.CLASSES3, 3, tw.MIN_OCC3)
    with pytest.raises(PoccalaHipError) as ei:
        eng.transform_means(None, None, 1)                                                        # the resident estimate has another R
    assert ei.value.code == -1
    other = (before[0] + 1.0, before[1], before[2])
    eng.load_model(*other)
    with pytest.raises(PoccalaHipError) as ei:
        eng.transform_means(None, tw.CLASSES3, 3)                                                 # ... and it went with the model it was made for
    assert ei.value.code == -1
    for a, b in zip(eng.model_download(), other):
        assert same_bits(a, b)


@pytest.mark.parametrize('D', [49, 64])
def test_beyond_48_dimensions_the_estimate_and_the_transform_are_refused(eng, D):
    """the solve's LDS matrix and the apply kernel's tile hold D <= 48: PCL_ERR_INVALID, the model as it was (its arrays, and ln b from it)"""
    from poccala_amd import PCL_F64, PoccalaHipError
    model, frames, gamma = case(D)
    accumulate(eng, model, frames, gamma)
    before, B = eng.model_download(), lnb_all_rows(eng, PCL_F64)
    for call in (lambda: eng.mllr_estimate(None, 1, 1.0), lambda: eng.mllr_estimate(tw.CLASSES3, 3, tw.MIN_OCC3),
                 lambda: eng.transform_means(known_transform(D)), lambda: eng.transform_means(None, None, 1)):
        with pytest.raises(PoccalaHipError) as ei:
            call()
        print(D, ei.value)
        assert ei.value.code == -1 and 'dimension %d' % D in str(ei.value)
        for a, b in zip(eng.model_download(), before):
            assert same_bits(a, b)
        assert same_bits(lnb_all_rows(eng, PCL_F64), B)
    eng.mstep_map(5.0)                                                                            # (MAP has no such limit: test_map_means_are_the_twins)
    assert not same_bits(eng.model_download()[0], before[0])


def test_the_calls_give_back_every_block_they_took(eng, monkeypatch):
    from poccala_amd import Engine
    monkeypatch.setenv('PCL_MLLR_CHUNK', CHUNK)
    model, frames, gamma = case(13)
    accumulate(eng, model, frames, gamma)
    start = Engine.pool_stats()['handed_out_blocks']
    eng.mllr_estimate(tw.CLASSES3, 3, tw.MIN_OCC3)
    resident = Engine.pool_stats()['handed_out_blocks']
    eng.mllr_estimate(tw.CLASSES3, 3, tw.MIN_OCC3)
    eng.transform_means(None, tw.CLASSES3, 3)
    eng.transform_means(np.stack([tw.identity(13)] * 3), tw.CLASSES3, 3)
    eng.mstep_map(3.0)
    end = Engine.pool_stats()['handed_out_blocks']
    print('handed-out blocks: %d at the start, %d with the resident transforms, %d at the end' % (start, resident, end))
    assert resident == start + 1 and end == resident                                              # the resident W is the one block the context keeps
