"""Segmental GMM training on the device (pcl_seg_*; training scheme 1) against golden G18 -- the REFERENCE's own Clustering.GMM.em --
and against the float64 twin that G18 pins (tests/_segment_twin.py, tests/test_segment_em_twin.py).

Bounds.  PCL_F64: the bound the project holds a device M-step to, 1e-9 relative, times the number of M-steps run (errors compound
through the iteration, each step adds one M-step's worth).  PCL_F32: the project's contract, 1e-4 relative on mean (relative to
sqrt(var)), var, weight and every Q of the trace.  Both against the reference golden, never against another run of the build.  Every figure is printed
before it is asserted.
"""
import json
import os

import numpy as np
import pytest

import _segment_twin as tw

pytestmark = pytest.mark.gpu
S = 5
_RECORDS = {}


@pytest.fixture(scope='module', autouse=True)
def parity_record():
    """POCCALA_SEGMENT_PARITY=<file>: the measured deviations from golden G18 are written there (profiles/r07_segment_parity.json is
    such a file: `POCCALA_SEGMENT_PARITY=profiles/r07_segment_parity.json python -m pytest tests/test_gpu_segment_em.py -m gpu`)."""
    yield
    path = os.environ.get('POCCALA_SEGMENT_PARITY')
    if path and _RECORDS:
        out = dict(what="device EM against golden G18 (the reference's Clustering.GMM.em): worst relative deviation of mean (relative to "
                        "sqrt(var)), var, weight and of the Q trace, per entry point, precision and golden case",
                   bounds='PCL_F64: 1e-9 x M-steps run; PCL_F32: 1e-4; asserted on every figure listed',
                   made_by='tests/test_gpu_segment_em.py with POCCALA_SEGMENT_PARITY set',
                   records=[_RECORDS[k] for k in sorted(_RECORDS)])
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)


def cases(golden):
    g = golden('G18_gmm_em')
    return [{k: g['c%d_%s' % (c, k)] for k in ('data', 'mean0', 'var0', 'w0', 'c_cov', 'mean', 'var', 'w', 'q_seq')}
            for c in range(int(g['n_cases']))]


def deviations(got, want):
    """worst relative deviations (mean relative to sqrt(var))"""
    (gm, gv, gw), (wm, wv, ww) = got, want
    return dict(mean=float(np.abs((gm - wm) / np.sqrt(wv)).max()), var=float(np.abs(gv / wv - 1).max()), w=float(np.abs(gw / ww - 1).max()))


def bound_of(precision, msteps):
    from poccala_amd import PCL_F64
    return 1e-9 * msteps if precision == PCL_F64 else 1e-4


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_golden_through_gmm_em(golden, prec):
    from poccala_amd import PCL_F32, PCL_F64
    from poccala_amd.StatisticalModel.Clustering import Clustering
    for ci, c in enumerate(cases(golden)):
        g = Clustering.GMM(dimension=c['data'].shape[1], mix_level=len(c['w0']), alpha=c['w0'].copy(), mean=c['mean0'].copy(),
                           variance=c['var0'].copy(), precision=prec)
        g.data = [r for r in c['data']]
        g.em(c_covariance=float(c['c_cov']))
        dev = deviations((g.mean, g.diag_variance(), g.alpha), (c['mean'], c['var'], c['w']))
        bound = bound_of(PCL_F64 if prec == 'f64' else PCL_F32, len(c['q_seq']))
        print('GMM.em %s case %d: iters %d (reference %d)  deviations %s  bound %.1e' % (prec, ci, g.em_iterations, len(c['q_seq']), dev, bound))
        assert g.em_iterations == len(c['q_seq'])
        assert max(dev.values()) <= bound, (ci, dev, bound)
        q_ref = c['q_seq'][-2]                               # the last accepted Q
        print('GMM.em %s case %d: Q %.12g reference %.12g' % (prec, ci, g.em_q, q_ref))
        assert abs(g.em_q - q_ref) <= bound * abs(q_ref)
        _RECORDS[('Clustering.GMM.em', prec, ci)] = dict(entry='Clustering.GMM.em', precision=prec, golden_case=ci, iters=g.em_iterations,
                                                         reference_iters=len(c['q_seq']), measured=dev, last_accepted_q_rel=float(abs(g.em_q / q_ref - 1)), bound=bound)
    with pytest.raises(NotImplementedError):
        g.em(smem=True)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('group', [(0, 0), (1, 1), (2, 3)])
def test_golden_through_segments_stacked(golden, eng, prec, group):
    """Golden cases of equal (D, M, floor) as the states of ONE model, their frames interleaved in the frame matrix, plus a state
    without frames and frames nobody owns."""
    from poccala_amd import PCL_F32, PCL_F64
    precision = PCL_F64 if prec == 'f64' else PCL_F32
    cs = [cases(golden)[i] for i in group]
    J = len(cs) + 1
    rng = np.random.default_rng(3)
    owner = np.concatenate([np.full(len(c['data']), j) for j, c in enumerate(cs)] + [np.full(17, -1)])
    perm = rng.permutation(len(owner))
    pos = np.concatenate([np.sort(np.nonzero(owner[perm] == j)[0]) for j in list(range(len(cs))) + [-1]])   # order inside a state is kept
    d = cs[0]['data'].shape[1]
    frames = np.empty((len(owner), d))
    frames[pos] = np.concatenate([c['data'] for c in cs] + [rng.standard_normal((17, d)) * 50])
    state = np.empty(len(owner), dtype=np.int32)
    state[pos] = owner
    eng.load_model(np.stack([c['mean0'] for c in cs] + [cs[0]['mean0']]), np.stack([c['var0'] for c in cs] + [cs[0]['var0']]),
                   np.stack([c['w0'] for c in cs] + [cs[0]['w0']]))
    eng.load_frames(frames)
    seg = eng.segments(state)
    assert list(seg.counts) == [len(c['data']) for c in cs] + [0]
    for j, part in enumerate(seg.split(seg.order)):
        assert np.array_equal(part, np.nonzero(state == j)[0])
    iters, q, qt = seg.em(c_covariance=float(cs[0]['c_cov']), precision=precision, max_iters=64, trace=True)
    seg.close()
    mean, var, w = eng.model_download()
    assert iters[-1] == -1 and np.isnan(q[-1])
    assert np.array_equal(mean[-1], cs[0]['mean0']) and np.array_equal(var[-1], cs[0]['var0']) and np.array_equal(w[-1], cs[0]['w0'])
    for j, c in enumerate(cs):
        n = len(c['q_seq'])
        bound = bound_of(precision, n)
        dev = deviations((mean[j], var[j], w[j]), (c['mean'], c['var'], c['w']))
        dq = float(np.abs(qt[j, :n] / c['q_seq'] - 1).max())
        print('Segments.em %s cases %s state %d: iters %d (reference %d)  deviations %s  Q %.2e  bound %.1e' % (prec, group, j, iters[j], n, dev, dq, bound))
        assert iters[j] == n
        assert np.isnan(qt[j, n:]).all()
        assert max(dev.values()) <= bound, (j, dev, bound)
        assert dq <= bound
        assert q[j] == qt[j, n - 2]
        _RECORDS[('Segments.em', prec, group[j])] = dict(entry='Segments.em', precision=prec, golden_case=group[j], iters=int(iters[j]), reference_iters=n,
                                                         measured=dev, q_trace_rel=dq, bound=bound)


def lloyd_problem(margin_needed, dtype, first_seed):
    """continuous random data, re-drawn until every frame's best and second-best distance differ by the margin in every sweep"""
    for s in range(first_seed, first_seed + 50):
        rng = np.random.default_rng(s)
        xs, cs, res = [], [], []
        for j, (n, k) in enumerate([(300, 5), (77, 3), (1000, 8)]):
            x = rng.standard_normal((n, 13)) * rng.uniform(0.5, 2, 13) + rng.integers(0, k, n)[:, None] * 2.0
            c0 = x[rng.choice(n, 8, replace=False)]
            c0[k:] = 1e3 + np.arange(8 - k)[:, None]              # states with fewer clusters in use: far-away centres stay empty
            r = tw.lloyd(x, c0, 100, dtype)
            xs.append(x), cs.append(c0), res.append(r)
        if min(r[3] for r in res) > margin_needed:
            return xs, cs, res
    raise AssertionError('no draw holds the margin condition')


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_lloyd_from_given_centres_equals_the_twin(eng, prec):
    from poccala_amd import PCL_F32, PCL_F64
    f64 = prec == 'f64'
    xs, cs, res = lloyd_problem(1e-9 if f64 else 1e-4, np.float64 if f64 else np.float32, 100)
    frames = np.concatenate(xs)
    if not f64:
        frames = frames.astype(np.float32)
        xs = [x.astype(np.float32).astype(np.float64) for x in xs]
        res = [tw.lloyd(x, c, 100, np.float32) for x, c in zip(xs, cs)]
        assert min(r[3] for r in res) > 1e-4
    state = np.concatenate([np.full(len(x), j, dtype=np.int32) for j, x in enumerate(xs)])
    eng.load_frames(frames)
    seg = eng.segments(state, J=3)
    sweeps = seg.kmeans(8, max_sweeps=100, precision=PCL_F64 if f64 else PCL_F32, init_centres=np.stack(cs))
    assign, centres = seg.split(seg.assignments()), seg.centres()
    seg.close()
    mean, var, w = eng.model_download()
    for j, (a, n_sw, c, margin) in enumerate(res):
        spread = xs[j].std()
        err = float(np.abs(centres[j] - c).max())
        print('lloyd %s state %d: sweeps %d (twin %d), margin %.2e, centre error %.2e (spread %.2f)' % (prec, j, sweeps[j], n_sw, margin, err, spread))
        assert sweeps[j] == n_sw
        assert np.array_equal(assign[j], a)
        assert err <= (1e-12 if f64 else 1e-5) * spread
        m_t, v_t, w_t = tw.cluster_model(xs[j], a, c)
        np.testing.assert_allclose(mean[j], m_t, rtol=1e-12, atol=1e-12 * spread)
        np.testing.assert_allclose(var[j], v_t, rtol=1e-10)
        np.testing.assert_allclose(w[j], w_t, rtol=1e-15)


def test_seeding_equals_the_twin(eng):
    from poccala_amd import PCL_F64
    rng = np.random.default_rng(8)
    K = 6
    xs = [rng.standard_normal((n, 13)) * 3 for n in (40, 700, 6, 2500)]
    xs.append(np.ones((9, 13)) * 2.5)                                        # all equal: total D^2 = 0
    xs.append(np.repeat(rng.standard_normal((3, 13)), 5, axis=0))            # 3 distinct rows only
    xs.append(rng.standard_normal((4, 13)))                                  # fewer frames than clusters: skipped
    state = np.concatenate([np.full(len(x), j, dtype=np.int32) for j, x in enumerate(xs)])
    perm = rng.permutation(len(state))
    inv = np.argsort(perm, kind='stable')
    frames, st = np.concatenate(xs)[perm], state[perm]
    eng.load_frames(frames)
    seg = eng.segments(st, J=len(xs))
    order = seg.split(seg.order)
    seed = 12345
    sweeps = seg.kmeans(K, seed=seed, max_sweeps=1, precision=PCL_F64)
    pos = seg.seed_positions()
    seg.close()
    compared = 0
    for j in range(len(xs)):
        x = frames[order[j]]                                                 # the state's frames in segment order
        if len(x) < K:
            assert sweeps[j] == -1 and (pos[j] == -1).all()
            continue
        assert pos[j].min() >= 0 and pos[j].max() < len(x)                  # rows of its own segment
        distinct = len(np.unique(x, axis=0))
        assert len(np.unique(x[pos[j]], axis=0)) == min(K, distinct)
        want, margin = tw.seeds(x, K, seed, j)
        print('seeding state %d: n %d, twin margin %.2e, device %s twin %s' % (j, len(x), margin, pos[j].tolist(), want.tolist()))
        if margin > 1e-9:
            assert np.array_equal(pos[j], want)
            compared += 1
    assert compared >= 4


def random_problem(rng, J, M, D, n_big=4000):
    counts = rng.integers(0, 120, J)
    counts[:6] = [0, M - 1, M, M + 1, n_big, 1]
    rng.shuffle(counts)
    state = np.concatenate([np.full(c, j, dtype=np.int32) for j, c in enumerate(counts)] + [np.full(50, -1, dtype=np.int32)])
    rng.shuffle(state)
    centre = rng.standard_normal((J, 3, D)) * 3
    frames = np.where(state[:, None] >= 0, centre[np.maximum(state, 0), rng.integers(0, 3, len(state))], 0.0) + rng.standard_normal((len(state), D))
    return counts, state, frames


def run_training(eng, state, frames, J, M, precision, seed=5):
    eng.load_frames(frames)
    D = frames.shape[1]
    eng.load_model(np.zeros((J, M, D)) + np.arange(M)[None, :, None], np.full((J, M, D), 2.0), np.full((J, M), 1.0 / M))
    seg = eng.segments(state)
    sweeps = seg.kmeans(M, seed=seed, precision=precision)
    iters, q, qt = seg.em(precision=precision, max_iters=30, trace=True)
    counts = seg.counts.copy()
    seg.close()
    return (sweeps, iters, q, qt, counts) + eng.model_download()


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_properties_on_random_states(eng, prec):
    from poccala_amd import PCL_F32, PCL_F64
    precision = PCL_F64 if prec == 'f64' else PCL_F32
    J, M, D = 80, 4, 13
    rng = np.random.default_rng(17)
    counts, state, frames = random_problem(rng, J, M, D)
    if prec == 'f32':
        frames = frames.astype(np.float32)
    sweeps, iters, q, qt, got_counts, mean, var, w = run_training(eng, state, frames, J, M, precision)
    assert np.array_equal(got_counts, counts)
    small = counts < M
    assert (iters[small] == -1).all() and (sweeps[small] == -1).all() and (iters[~small] >= 1).all()
    # skipped states: bit-identical to before
    assert np.array_equal(mean[small], (np.zeros((J, M, D)) + np.arange(M)[None, :, None])[small]) and (var[small] == 2.0).all() and (w[small] == 1.0 / M).all()
    assert np.abs(w[~small].sum(1) - 1).max() < (1e-12 if prec == 'f64' else 1e-5)      # f32: the responsibilities of a frame sum to 1 in float32
    assert (var[~small] >= 1e-3).all() and np.isfinite(mean).all()
    for j in np.nonzero(~small)[0]:
        seq = qt[j, :iters[j]]
        assert np.isfinite(seq).all()
        acc = seq[:-1] if iters[j] < 30 else seq
        assert (np.diff(acc) > 1.28).all(), (j, seq)                # Q grows over the accepted iterations
        if iters[j] < 30 and iters[j] > 1:
            assert seq[-1] - seq[-2] <= 1.28
    # frames nobody owns have no influence; the same seed gives the same bits
    frames2 = frames.copy()
    frames2[state < 0] += 1000.0
    again = run_training(eng, state, frames2, J, M, precision)
    for a, b in zip((sweeps, iters, q, mean, var, w), (again[0], again[1], again[2]) + again[5:]):
        assert np.array_equal(a, b, equal_nan=True)


def test_train_segments_batch_equals_the_twin(golden, tmp_path):
    """Alignment -> regroup -> clustering -> EM in one call, against the twin fed with what regroup_batch returns."""
    from test_gpu_dropin import RecLog, build_units
    from poccala_amd import PCL_F64
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    g = golden('G6_small_fix0')
    label, hmm_list = build_units(g)
    am = AcousticModel(RecLog(), 'XIF_tone', state_num=S, mix_level=4, dct_num=13, delta_1=False, delta_2=False, parameters_path=str(tmp_path))
    unit_hmms = {u: hmm_list[label.index(u)] for u in set(label)}
    rng = np.random.default_rng(2)
    data = [g['x'] + 0.05 * rng.standard_normal(g['x'].shape) for _ in range(8)]
    labels = [label] * len(data)
    regrouped, dropped = am.regroup_batch(labels, data, unit_hmms, precision=PCL_F64)
    K, seed, e = 2, 9, S - 2
    res = am.train_segments_batch(labels, data, unit_hmms, init=True, mix_level=K, c_covariance=1e-3, seed=seed, precision=PCL_F64)
    assert am.last_dropped == dropped
    units = sorted(unit_hmms)
    compared = 0
    for ui, unit in enumerate(units):
        iters, q, skipped = res[unit]
        for k in range(e):
            x = regrouped[unit][k] if unit in regrouped else np.zeros((0, 13))
            gmm = unit_hmms[unit].profunction[1 + k]
            if len(x) < K:
                assert skipped[k] and iters[k] == -1 and gmm.mixture == 4
                continue
            assert gmm.mixture == K and not skipped[k]
            idx, smargin = tw.seeds(x, K, seed, ui * e + k)
            a, sw, c, lmargin = tw.lloyd(x, x[idx])
            r = tw.em(x, *tw.cluster_model(x, a, c), c_covariance=1e-3)
            steps = np.diff(np.concatenate([[-np.inf], r['q_seq']]))
            if smargin < 1e-9 or lmargin < 1e-9 or np.abs(steps - 1.28).min() < 1e-6 or r['w'].min() < 1e-6:
                continue                                              # the twin itself sits on a decision boundary here
            dev = deviations((gmm.mean, gmm.diag_variance(), gmm.alpha), (r['mean'], r['var'], r['w']))
            print('train_segments_batch %s/%d: n %d iters %d (twin %d) deviations %s' % (unit, k, len(x), iters[k], r['iters'], dev))
            assert iters[k] == r['iters']
            assert max(dev.values()) <= 1e-9 * r['iters']
            assert abs(q[k] - r['q']) <= 1e-9 * r['iters'] * abs(r['q'])
            compared += 1
    assert compared >= len(units) * e // 2
    # the variant from already regrouped data gives the same model
    label2, hmm_list2 = build_units(g)
    unit_hmms2 = {u: hmm_list2[label2.index(u)] for u in set(label2)}
    res2 = am.train_segments_data(regrouped, unit_hmms2, init=True, mix_level=K, c_covariance=1e-3, seed=seed, precision=PCL_F64)
    for unit in units:
        assert np.array_equal(res[unit][0], res2[unit][0])
        for k in range(e):
            assert np.array_equal(unit_hmms[unit].profunction[1 + k].mean, unit_hmms2[unit].profunction[1 + k].mean)


def test_batch_segments_equals_engine_segments(golden, tmp_path):
    """Batch.segments (regroup handed on, frames in front of / behind the batch and a dropped utterance left out) builds the lists
    Engine.segments builds from the owner array put together on the host."""
    from test_gpu_dropin import RecLog, build_units
    from poccala_amd import PCL_F64
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    from poccala_amd.engine import frame_state_of
    from poccala_amd.runtime import default_engine
    g = golden('G6_small_fix0')
    label, hmm_list = build_units(g)
    am = AcousticModel(RecLog(), 'XIF_tone', state_num=S, mix_level=4, dct_num=13, delta_1=False, delta_2=False, parameters_path=str(tmp_path))
    unit_hmms = {u: hmm_list[label.index(u)] for u in set(label)}
    eng = default_engine()
    units, idx, (mean, var, w), trans = am._model_arrays(unit_hmms)
    eng.load_model(mean, var, w)
    eng.load_units(np.stack(trans))
    x = g['x']
    T = len(x)
    frames = np.concatenate([x[:7], x, x[::-1], x + 0.01, x[:5]])           # 7 rows in front, three utterances, 5 rows behind
    eng.load_frames(frames)
    begin = np.array([7, 7 + T, 7 + 2 * T], dtype=np.int64)
    ids = [np.array([idx[u] for u in label], dtype=np.int32)] * 3
    b = eng.label_batch(ids, [T] * 3, begin)
    b.score(PCL_F64)
    b.viterbi()
    rep = np.repeat(ids[0], S - 2)
    row_unit = [np.concatenate([[rep[0]], rep, [rep[-1]]]).astype(np.int32)] * 3
    fu, fk = b.regroup(row_unit, S - 2)
    want = np.full(len(frames), -1, dtype=np.int32)
    for u in (0, 2):                                                         # utterance 1 is dropped
        want[begin[u]:begin[u] + T] = frame_state_of(fu[u], fk[u], S - 2)
    got = b.segments(row_unit, S - 2, dropped=[1])
    again = b.segments(row_unit, S - 2, dropped=[1], regrouped=(fu, fk))
    ref = eng.segments(want)
    b.close()
    assert ref.counts.sum() == 2 * T
    for sg in (got, again):
        assert np.array_equal(sg.counts, ref.counts) and np.array_equal(sg.order, ref.order)
        sg.close()
    ref.close()


def test_train_segments_edges(golden, tmp_path):
    """smem is refused before anything is aligned; no data at all: every state skipped, the model untouched."""
    from test_gpu_dropin import RecLog, build_units
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    g = golden('G6_small_fix0')
    label, hmm_list = build_units(g)
    am = AcousticModel(RecLog(), 'XIF_tone', state_num=S, mix_level=4, dct_num=13, delta_1=False, delta_2=False, parameters_path=str(tmp_path))
    unit_hmms = {u: hmm_list[label.index(u)] for u in set(label)}
    with pytest.raises(NotImplementedError):
        am.train_segments_batch([label], [g['x']], unit_hmms, smem=True)
    with pytest.raises(NotImplementedError):
        am.train_segments_data({}, unit_hmms, smem=True)
    before = {u: unit_hmms[u].profunction[1].mean.copy() for u in unit_hmms}
    res = am.train_segments_data({}, unit_hmms, init=True, mix_level=2)
    for u in unit_hmms:
        iters, q, skipped = res[u]
        assert (iters == -1).all() and np.isnan(q).all() and skipped.all()
        assert np.array_equal(unit_hmms[u].profunction[1].mean, before[u])


def test_cluster_initialization_return_shapes():
    from poccala_amd.StatisticalModel.Clustering import Clustering
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.standard_normal((50, 5)) + 8 * k for k in range(3)])
    for alg in (0, 1):
        mean, sd, alpha, clustered = Clustering.ClusterInitialization(x, 3, 5).kmeans(algorithm=alg, seed=3)
        assert mean.shape == (3, 5) and sd.shape == (3, 5) and alpha.shape == (3,) and len(clustered) == 3
        assert sum(len(c) for c in clustered) == len(x) and abs(alpha.sum() - 1) < 1e-12
        m2, cov, a2, _ = Clustering.ClusterInitialization(x, 3, 5).kmeans(algorithm=alg, cov_matrix=True, seed=3)
        assert cov.shape == (3, 5, 5) and np.array_equal(m2, mean)
        np.testing.assert_allclose(np.diagonal(cov, axis1=1, axis2=2), sd ** 2, rtol=1e-14)
        for k in range(3):
            np.testing.assert_allclose(mean[k], clustered[k].mean(0), rtol=1e-12, atol=1e-12)


def test_baseline_shaped_training_finishes(eng):
    """549 states x 64 mixtures, D = 39, 220 k frames: properties only."""
    from poccala_amd import PCL_F32
    J, M, D, F = 549, 64, 39, 220000
    rng = np.random.default_rng(1)
    state = rng.integers(0, J, F).astype(np.int32)
    state[rng.integers(0, F, 2000)] = -1
    state[state == 7] = 8                                                    # one state without frames
    frames = (rng.standard_normal((J, D))[np.maximum(state, 0)] * 3 + rng.standard_normal((F, D))).astype(np.float32)
    eng.load_frames(frames)
    seg = eng.segments(state, J=J)
    sweeps = seg.kmeans(M, seed=1, max_sweeps=5, precision=PCL_F32)
    iters, q, qt = seg.em(precision=PCL_F32, max_iters=4, trace=True)
    counts = seg.counts.copy()
    seg.close()
    mean, var, w = eng.model_download()
    ok = counts >= M
    assert counts[7] == 0 and iters[7] == -1 and sweeps[7] == -1
    assert (iters[ok] >= 1).all() and (sweeps[ok] >= 1).all()
    assert np.isfinite(mean).all() and (var[ok] >= 1e-3).all() and np.abs(w[ok].sum(1) - 1).max() < 1e-5
    for j in np.nonzero(ok)[0][:50]:
        seq = qt[j, :iters[j]]
        assert np.isfinite(seq).all() and (np.diff(seq[:-1]) > 1.28).all()
