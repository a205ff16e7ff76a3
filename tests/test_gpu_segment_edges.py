"""The kernels of csrc/gmm_segment.hip (counting sort by owner state, k-means++ seeding, Lloyd sweeps, cluster model, M-step + Q) held to the
float64 twin (tests/_segment_twin.py) at their edges, on the smallest shapes that reach them (tests/_seg_cases.py builds the cases,
tests/test_seg_cases.py proves on the CPU that each reaches its edge).  Everything goes through Engine.segments / Segments.kmeans / .em /
.assignments / .centres / .seed_positions / model_download.

Bounds are the project's own.  Sort: exact.  Lloyd: sweeps and assignments exact, centres within 1e-12 (f64) / 1e-5 (f32) of the data's
spread, model mean rtol 1e-12, variance rtol 1e-10, weight rtol 1e-15 against cluster_model (test_lloyd_from_given_centres_equals_the_twin).
Seeding: positions equal.  EM: bound_of of test_gpu_segment_em.py -- 1e-9 x M-steps under PCL_F64, 1e-4 under PCL_F32 -- on mean (relative
to sqrt(var)), var, weight and every Q of the trace, iteration counts equal.  Every k-means and EM case runs twice and must give the same
bytes (no floating-point atomics).  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _seg_cases as sc
import _segment_twin as tw
from test_gpu_segment_em import bound_of, deviations

pytestmark = pytest.mark.gpu
PRECS = ['f64', 'f32']


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def precision_of(prec):
    from poccala_amd import PCL_F32, PCL_F64
    return PCL_F64 if prec == 'f64' else PCL_F32


def same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------- sort
@pytest.mark.parametrize('ci', range(len(sc.sort_cases())), ids=[c['name'] for c in sc.sort_cases()])
def test_sort_equals_a_stable_sort(eng, ci):
    c = sc.sort_cases()[ci]
    state = c['state']
    eng.load_frames(np.arange(c['F'], dtype=np.float32)[:, None] % 97)
    seg = eng.segments(state, J=c['J'])
    counts, order = seg.counts.copy(), seg.order
    seg.close()
    want = [np.flatnonzero(state == j) for j in range(c['J'])]
    print('sort %s: %d rows, %d states, %d tiles, %d owned' % (c['name'], c['F'], c['J'], sc.sort_tiles(c['F'], c['J']), len(order)))
    assert np.array_equal(counts, [len(w) for w in want])
    assert np.array_equal(order, np.concatenate(want))


# ---------------------------------------------------------------------- Lloyd and the cluster model
def run_kmeans(eng, c, max_sweeps):
    rng = np.random.default_rng(5)
    K, D, J = c['K'], c['D'], c['J']
    before = (rng.standard_normal((J, K, D)), rng.uniform(0.5, 2, (J, K, D)), rng.dirichlet(np.ones(K), J))
    eng.load_model(*before)
    eng.load_frames(c['frames'])
    seg = eng.segments(c['state'], J=J)
    sweeps = seg.kmeans(K, max_sweeps=max_sweeps, precision=precision_of(c['prec']), init_centres=c['c0'])
    assign, centres = seg.split(seg.assignments()), seg.centres()
    seg.close()
    return (sweeps, assign[0], centres) + eng.model_download(), before


def check_kmeans(c, got, before):
    sweeps, assign, centres, mean, var, w = got
    f64 = c['prec'] == 'f64'
    x, K, D = c['x'], c['K'], c['D']
    spread = x.std()
    err = float(np.abs(centres[0] - c['centres']).max())
    m_t, v_t, w_t = tw.cluster_model(x, c['assign'], c['centres'])
    dm = float(np.abs(mean[0] - m_t).max())
    dv = float(np.abs(var[0] / v_t - 1).max())
    dw = float(np.abs(w[0] - w_t).max())
    print('lloyd %s: sweeps %d (twin %d), margin %.2e, %d of %d assignments differ, centre error %.2e (bound %.1e), mean %.2e, var rel %.2e, '
          'weight %.2e' % (c['name'], sweeps[0], c['sweeps'], c['margin'], int((assign != c['assign']).sum()), len(x), err,
                           (1e-12 if f64 else 1e-5) * spread, dm, dv, dw))
    assert centres.shape == (c['J'], K, D) and mean.shape == (c['J'], K, D) and var.shape == mean.shape and w.shape == (c['J'], K)
    assert sweeps[0] == c['sweeps']
    assert np.array_equal(assign, c['assign'])
    assert err <= (1e-12 if f64 else 1e-5) * spread
    np.testing.assert_allclose(mean[0], m_t, rtol=1e-12, atol=1e-12 * spread)
    np.testing.assert_allclose(var[0], v_t, rtol=1e-10)
    np.testing.assert_allclose(w[0], w_t, rtol=1e-15)
    empty = np.bincount(c['assign'], minlength=K) == 0
    assert (var[0][empty] == sc.VAR_FLOOR).all() and (w[0][empty] == 0).all()
    far = c.get('roles', {}).get('far', [])                     # never reached: the given centre, bit for bit
    assert np.array_equal(mean[0][far], c['c0'][0][far]) and np.array_equal(centres[0][far], c['c0'][0][far])
    if c['J'] > 1:                                              # the neighbour with fewer than K frames keeps its model bit for bit
        assert sweeps[1] == -1
        assert all(np.array_equal(a[1], b[1]) for a, b in zip((mean, var, w), before))


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('n,K,D', sc.LLOYD_SHAPES)
def test_lloyd_from_given_centres(eng, n, K, D, prec):
    c = sc.lloyd_case(n, K, D, prec)
    got, before = run_kmeans(eng, c, 100)
    check_kmeans(c, got, before)
    again, _ = run_kmeans(eng, c, 100)
    assert same_bytes(got, again)


@pytest.mark.parametrize('prec', PRECS)
def test_cluster_sizes_after_one_sweep(eng, prec):
    c = sc.cluster_size_case(prec)
    got, before = run_kmeans(eng, c, 1)
    print('cluster sizes %s: device %s' % (prec, np.bincount(got[1], minlength=c['K']).tolist()))
    check_kmeans(c, got, before)
    assert np.allclose(got[5][0] * c['n'], sc.CLUSTER_SIZES, rtol=0, atol=1e-9)
    again, _ = run_kmeans(eng, c, 1)
    assert same_bytes(got, again)


# ---------------------------------------------------------------------- seeding
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('D', sc.SEED_DIMS)
def test_seeding_positions(eng, D, prec):
    c = sc.seed_case(D, prec)
    K = c['K']
    runs = []
    for _ in range(2):
        eng.load_frames(c['frames'])
        seg = eng.segments(c['state'], J=c['J'])
        sweeps = seg.kmeans(K, seed=c['seed'], max_sweeps=1, precision=precision_of(prec))
        runs.append((sweeps, seg.seed_positions(), seg.centres()))
        seg.close()
    sweeps, pos, centres = runs[0]
    for j, x in enumerate(c['xs']):
        if len(x) < K:
            assert sweeps[j] == -1 and (pos[j] == -1).all()
            continue
        print('seeding %s state %d: n %d, twin margin %.2e, device %s twin %s' % (c['name'], j, len(x), c['margin'][j], pos[j].tolist(), c['want'][j].tolist()))
        assert pos[j].min() >= 0 and pos[j].max() < len(x)
        assert np.array_equal(pos[j], c['want'][j])
        assert len(np.unique(x[pos[j]], axis=0)) == min(K, len(np.unique(x, axis=0)))
    assert same_bytes(runs[0], runs[1])


# ---------------------------------------------------------------------- EM
def run_em(eng, c, prec, max_iters):
    eng.load_model(c['mean0'], c['var0'], c['w0'], logdet=c['logdet'])
    eng.load_frames(c['frames'] if prec == 'f64' else c['frames'].astype(np.float32))
    seg = eng.segments(c['state'], J=c['J'])
    iters, q, qt = seg.em(c_covariance=c['c_cov'], q_threshold=c['threshold'][prec], max_iters=max_iters, precision=precision_of(prec), trace=True)
    seg.close()
    return (iters, q, qt) + eng.model_download()


def check_em(c, prec, max_iters, got, dead=None):
    iters, q, qt, mean, var, w = got
    thr = c['threshold'][prec]
    assert mean.shape == c['mean0'].shape and var.shape == mean.shape and w.shape == c['w0'].shape
    for j, steps in enumerate(c['steps']):
        run = sc.run_length(steps, thr, max_iters)
        last = steps[run - 1]
        bound = bound_of(precision_of(prec), run)
        live = np.ones(c['M'], dtype=bool)
        if dead is not None:
            live[dead] = False
        dev = deviations((mean[j][live], var[j][live], w[j][live]), (last['mean'][live], last['var'][live], last['w'][live]))
        q_seq = np.array([s['q'] for s in steps[:run]])
        dq = float(np.abs(qt[j, :min(run, iters[j])] / q_seq[:min(run, iters[j])] - 1).max())
        print('em %s %s max_iters %d state %d: n %d, threshold %g, iters %d (twin %d), deviations %s, Q %.2e, bound %.1e'
              % (c['name'], prec, max_iters, j, len(c['xs'][j]), thr, iters[j], run, dev, dq, bound))
        assert iters[j] == run
        assert np.isnan(qt[j, run:]).all()
        assert max(dev.values()) <= bound, (j, dev, bound)
        assert dq <= bound
        assert q[j] == qt[j, run - 2 if run > 1 and not q_seq[-1] - q_seq[-2] > thr else run - 1]       # the last accepted Q
        if dead is not None:
            assert w[j][dead] == 0 and np.array_equal(mean[j][dead], c['mean0'][j][dead]) and np.array_equal(var[j][dead], c['var0'][j][dead])
    if c['short'] is not None:
        j = c['J'] - 1
        assert iters[j] == -1 and np.isnan(q[j]) and np.isnan(qt[j]).all()
        assert np.array_equal(mean[j], c['mean0'][j]) and np.array_equal(var[j], c['var0'][j]) and np.array_equal(w[j], c['w0'][j])


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('max_iters', sc.EM_ITERS)
@pytest.mark.parametrize('M,D', sc.EM_SHAPES)
def test_em_shapes(eng, M, D, max_iters, prec):
    c = sc.em_shape_case(M, D)
    got = run_em(eng, c, prec, max_iters)
    check_em(c, prec, max_iters, got)
    assert same_bytes(got, run_em(eng, c, prec, max_iters))


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('kind', sc.EM_SPECIAL)
def test_em_special(eng, kind, prec):
    c = sc.em_special_case(kind)
    for max_iters in ((c['max_iters'],) if kind == 'ragged' else sc.EM_ITERS):
        got = run_em(eng, c, prec, max_iters)
        check_em(c, prec, max_iters, got, dead=2 if kind == 'gamma0' else None)
        if kind == 'floor':
            assert (got[4][0] == c['c_cov']).all()
        assert same_bytes(got, run_em(eng, c, prec, max_iters))
