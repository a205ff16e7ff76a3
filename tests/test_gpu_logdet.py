"""Log-determinant models (Engine.load_model(..., logdet=True), PCL_MODEL_LOGDET) on the device against the float64 reference written
out in tests/_logdet_cases.py.  The constant -D/2 ln 2pi - 1/2 sum(ln var) is computed in seven places of the scoring and accumulate path
(DESIGN.md section 7a), each behind its own test of the flag; tests/test_gpu_segment_edges.py runs the seventh (segmental EM), the cases here
run the other six, and tests/test_logdet_cases.py proves on the CPU that a site which dropped the flag -- for all mixtures or only for the
ones it handles -- would leave its case's allowance by a factor of 100 or more.

  ladder     variances over a factor of 16 inside every state, D = 13, 20 (padded to 26), 39: scoring variants 1, 3, 7 and PCL_F64
             (state_prepass_kernel and derive_kernel: K0, the f16 pieces, params32, pm32, the lazily derived params64).
  broad      every variance ~ 1024 (an ordinary problem scaled by powers of two): sum var is ~ 5e4 above sum ln var, so K0 of the prepass
             and the k' of derive_kernel have to take the SAME constant for k' - K0 to keep its bits.
  outlier    two frames 400 sigma out, one per workgroup: the flagged tile is rescored from the master rows (gmm_score.hip).
  split      states with 0, 3, 6, 9 and 48 of 48 mixtures off the pipe, a sentence batch: score, forward-backward, accumulate under every
             variant and in PCL_F64 (the coarse pass and the compact-main kernel under 7, the subset launches of score and accumulate).
  collapsed  PCL_COARSE_SPLIT_MAX=1: states with all, all but 20 and none of 160 mixtures at variances down to 5e-7, whose constants sit
             hundreds of nats above the broad ones'; scored twice for equal bits.
  survives   the flag belongs to the resident model: after the M-step, the exchanges, mix-up, a mean transform, MAP, a flat start and
             the k-means re-upload the live batch is rescored in PCL_F64 and held to the reference OF THE DOWNLOADED PARAMETERS.

Bounds, none new, all through tests/_parity.hold: PCL_F32 ln b 5e-5 absolute on ordinary states, 5e-6 relative + 5e-5 + the f32 evaluation
bound where mixtures are off the pipe, a state is in direct form or frames are outliers (tests/test_gpu_parity.py, tests/test_gpu_score_ring.py);
PCL_F64 ln b 1e-12 relative (test_score_matches_oracle); f32 statistics 1e-4 relative + 1e-6 of the largest entry (+ cov_acc_atol)
(test_estep_variants_split_states); f64 statistics 1e-9 relative + 1e-13 of the state's largest entry (tests/test_gpu_acc_edges.py); the
M-step in PCL_F64 1e-8 on weights and means, 1e-7 on variances (tests/test_gpu_units.py test_em_loop_stays_on_device).

MEASURED on the MI355X (largest share of a bound in use, `-s` prints them per test): see DESIGN.md section 7a."""
import os

import numpy as np
import pytest

import _logdet_cases as lc
from _parity import cov_acc_atol, hold
from oracle import poccala_oracle as po

pytestmark = pytest.mark.gpu

F32_RTOL = 1e-4                     # tests/test_gpu_parity.py
WORST, HERE = {}, {}


def engine_under(**env):
    """An engine whose context read the given environment; the environment is left as it was."""
    from poccala_amd import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope='module')
def eng():
    e = engine_under()
    yield e
    e.close()


@pytest.fixture(scope='module', params=[1, 3, 7])
def eng_variant(request):
    e = engine_under(PCL_SCORE_VARIANT=request.param)
    e.score_variant = request.param
    yield e
    e.close()


@pytest.fixture(scope='module')
def eng_keep_split():
    e = engine_under(PCL_COARSE_SPLIT_MAX='1.0')                         # (tests/test_gpu_score_ring.py: states stay split whatever their share)
    yield e
    e.close()


def held(kind, tag, quantity, got, want, rtol, atol=0.0):
    m = hold(tag, quantity, got, want, rtol, atol)
    for book in (WORST, HERE):
        book[kind] = max(book.get(kind, 0.0), m['used'])
    return m['used']


def report(tag):
    """The largest share of each kind of bound this test used (and the largest of the session so far)."""
    print('LOGDET %s: %s' % (tag, ', '.join('%s %.3g of the bound (worst so far %.3g)' % (k, v, WORST[k]) for k, v in HERE.items())))
    HERE.clear()


def precision(prec):
    from poccala_amd import PCL_F32, PCL_F64
    return PCL_F32 if prec == 'f32' else PCL_F64


def score_all_states(eng, c, prec):
    """(J, T): every state on every frame of one utterance, as tests/test_gpu_parity.py score_all_states does it, under the flag."""
    J, T = c['mean'].shape[0], c['frames'].shape[0]
    eng.load_model(c['mean'], c['var'], c['w'], logdet=True)
    eng.load_frames(c['frames'])
    b = eng.batch([J + 2], [T], [0])
    b.set_states([np.concatenate([[-1], np.arange(J), [-2]]).astype(np.int32)])
    b.score(precision(prec))
    B = b.get('B')[0]
    b.close()
    assert np.all(B[0] == 0.0) and np.all(np.isneginf(B[-1]))
    return B[1:-1]


@pytest.fixture(scope='module')
def reference():
    """ln b of every (state, frame) of a case under the log-determinant constant, computed once and read-only."""
    cache = {}

    def get(c):
        if c['name'] not in cache:
            r = lc.point_states(c['frames'], c['mean'], c['var'], c['w'])
            r.setflags(write=False)
            cache[c['name']] = r
        return cache[c['name']]
    return get


def device_split_info(eng, c):
    """pcl_model_split_info of the loaded model; its counts equal the NumPy twin of model_derive.hip's rule at the device's own threshold."""
    _, cmax = eng.model_conditioning()
    n_off, limit = eng.model_split_info()
    twin = lc.off_pipe(c['mean'], c['var'], cmax)
    assert np.array_equal(n_off, twin.sum(axis=1))
    return n_off, limit, twin


# ------------------------------------------------------------------ ladder: sites 1 and 2
@pytest.mark.parametrize('D', lc.LADDER_DIMS)
def test_ladder_f32(eng_variant, reference, D):
    c = lc.ladder(D)
    got, ref = score_all_states(eng_variant, c, 'f32'), reference(c)
    n_off, _, _ = device_split_info(eng_variant, c)
    assert not n_off.any()
    assert np.isfinite(got).all()
    held('f32 ln b, ordinary states', 'logdet ladder D=%d variant %d' % (D, eng_variant.score_variant), 'ln b', got, ref, 0.0, lc.F32_LOGLIK_ATOL)
    report('ladder D=%d variant %d' % (D, eng_variant.score_variant))


def test_broad_variances_f32(eng_variant, reference):
    """sum var exceeds sum ln var by ~ 5e4 here: K0 of the prepass and the k' of derive_kernel agree only if both read the flag (variant 7
    keeps k' - K0 in f16 pieces); the case is an ordinary one scaled by exact powers of two, so the 5e-5 bound applies."""
    c = lc.broad()
    got, ref = score_all_states(eng_variant, c, 'f32'), reference(c)
    n_off, _, _ = device_split_info(eng_variant, c)
    assert not n_off.any() and np.isfinite(got).all()
    held('f32 ln b, ordinary states', 'logdet broad variant %d' % eng_variant.score_variant, 'ln b', got, ref, 0.0, lc.F32_LOGLIK_ATOL)
    report('broad variant %d' % eng_variant.score_variant)


@pytest.mark.parametrize('D', lc.LADDER_DIMS)
def test_ladder_f64(eng, reference, D):
    c = lc.ladder(D)
    held('f64 ln b', 'logdet ladder D=%d f64' % D, 'ln b', score_all_states(eng, c, 'f64'), reference(c), 1e-12)
    report('ladder D=%d f64' % D)


# ------------------------------------------------------------------ outlier: site 3, the fix-up launch
def test_outlier_frames_are_rescored_under_the_flag(eng_variant, reference):
    """Variant 7 flags the tile and rescores it from MasterModel rows; variant 3 and the direct form (1) take the frames as they come."""
    c = lc.outlier()
    got, ref = score_all_states(eng_variant, c, 'f32'), reference(c)
    assert np.isfinite(got).all() and (ref[:, list(lc.OUTLIER_FRAMES)] < -4.0e4).all()
    rtol, atol = lc.score_bounds(c, ref, np.ones(len(ref), dtype=bool))
    for j in range(len(ref)):
        held('f32 ln b, f32-class bound', 'logdet outlier variant %d' % eng_variant.score_variant, 'ln b', got[j], ref[j], rtol[j], atol[j])
    far = list(lc.OUTLIER_FRAMES)
    print('LOGDET outlier variant %d: |d ln b| on the outlier frames up to %.3e at |ln b| %.0f' % (
        eng_variant.score_variant, np.abs(got - ref)[:, far].max(), np.abs(ref[:, far]).max()))
    report('outlier variant %d' % eng_variant.score_variant)


# ------------------------------------------------------------------ split: sites 3 (subset launch), 4, 5, 6
@pytest.fixture(scope='module')
def split_estep():
    """The oracle's E-step of the split case with w' (tests/_logdet_cases.estep), once."""
    return lc.estep(lc.split())


def run_estep(eng, c, prec):
    from poccala_amd.engine import make_sentence_batch
    P = precision(prec)
    eng.load_model(c['mean'], c['var'], c['w'], logdet=True)
    info = device_split_info(eng, c)
    eng.load_frames(c['frames'])
    b, _ = make_sentence_batch(eng, c['labels'], c['lens'], c['begin'], c['trans'])
    try:
        b.score(P)
        b.forward_backward(fix_pi=False)
        eng.stats_zero()
        b.accumulate(P)
        return info, b.get('B'), b.get('logp'), eng.stats_download()
    finally:
        b.close()


def hold_sentence_rows(kind_of, tag, c, B, ref, rtol, atol):
    """Every emitting row of every utterance against ref (J, F); rtol (J,), atol (J, F) or a number; the virtual rows are 0 and -inf."""
    for u, rows in enumerate(c['rows']):
        lo, T = int(c['begin'][u]), int(c['lens'][u])
        assert np.all(B[u][0] == 0.0) and np.all(np.isneginf(B[u][-1]))
        for n, j in enumerate(rows):
            if j >= 0:
                at = atol[j, lo:lo + T] if np.ndim(atol) else atol
                held(kind_of(j), tag, 'ln b (%s)' % kind_of(j), B[u][n], ref[j, lo:lo + T], rtol[j], at)


def hold_statistics(kind, tag, c, st, ref, prec):
    J = c['mean'].shape[0]
    if prec == 'f32':                                                    # tests/test_gpu_parity.py test_estep_variants_split_states
        for key in lc.KEYS:
            scale = np.abs(ref[key]).max()
            at = cov_acc_atol(ref['acc'], c['mean'], c['var'], scale * 1e-6) if key == 'cov_acc' else scale * 1e-6
            held(kind, tag, key, st[key], ref[key], F32_RTOL, at)
    else:                                                                # tests/test_gpu_acc_edges.py (_acc_edge_cases.bounds): per state
        for key in lc.KEYS:
            for j in range(J):
                held(kind, tag, key, np.asarray(st[key][j]), np.asarray(ref[key][j]), 1e-9, 1e-13 * float(np.abs(ref[key][j]).max()))


def test_split_estep_f32(eng_variant, reference, split_estep):
    c, v = lc.split(), eng_variant.score_variant
    M = c['mean'].shape[1]
    (n_off, limit, twin), B, logp, st = run_estep(eng_variant, c, 'f32')
    assert np.array_equal(n_off, [len(t) for t in c['tight']]) and limit == int(np.float32(0.99 if v == 7 else 0.5) * np.float32(M))
    ref = reference(c)
    f32_class = twin.any(axis=1)
    rtol, atol = lc.score_bounds(c, ref, f32_class)
    kind_of = lambda j: 'f32 ln b, f32-class bound' if f32_class[j] else 'f32 ln b, ordinary states'
    tag = 'logdet split variant %d' % v
    hold_sentence_rows(kind_of, tag, c, B, ref, rtol, atol)
    held('f32 ln P(O)', tag, 'ln P(O)', logp, split_estep['logp'], F32_RTOL)
    assert (split_estep['stats']['acc'][twin] > 0).sum() > 20            # the off-pipe mixtures carry real occupancy
    hold_statistics('f32 statistics', tag, c, st, split_estep['stats'], 'f32')
    report('split variant %d' % v)


def test_split_estep_f64(eng, reference, split_estep):
    c = lc.split()
    (n_off, limit, twin), B, logp, st = run_estep(eng, c, 'f64')
    assert np.array_equal(n_off, [len(t) for t in c['tight']])
    ref = reference(c)
    hold_sentence_rows(lambda j: 'f64 ln b', 'logdet split f64', c, B, ref, np.full(len(ref), 1e-12), 0.0)
    held('f64 ln P(O)', 'logdet split f64', 'ln P(O)', logp, split_estep['logp'], 1e-9)      # (tests/test_gpu_parity.py test_estep_end_to_end)
    hold_statistics('f64 statistics', 'logdet split f64', c, st, split_estep['stats'], 'f64')
    report('split f64')


# ------------------------------------------------------------------ collapsed: sites 4 and 5 where the constants are hundreds of nats apart
def score_own_frames_twice(eng, c):
    """tests/test_gpu_score_ring.py score_twice under the flag: state j on its own frames, two launches on one batch, equal bits."""
    lens = c['lens']
    eng.load_model(c['mean'], c['var'], c['w'], logdet=True)
    eng.load_frames(c['frames'])
    b = eng.batch([3] * len(lens), lens, c['begin'].tolist())
    b.set_states([np.array([-1, j, -2], dtype=np.int32) for j in range(len(lens))])
    P = precision('f32')
    b.score(P)
    first = [np.array(u, copy=True) for u in b.get('B')]
    b.score(P)
    second = b.get('B')
    b.close()
    for j, (u, v) in enumerate(zip(first, second)):
        assert np.all(u[0] == 0.0) and np.all(np.isneginf(u[-1]))
        assert np.array_equal(u, v), 'state %d: two launches on the same batch differ' % j
    return [u[1] for u in first]


def test_collapsed_states_keep_their_constants(eng_keep_split, reference):
    c = lc.collapsed()
    M = c['mean'].shape[1]
    got = score_own_frames_twice(eng_keep_split, c)
    n_off, limit, twin = device_split_info(eng_keep_split, c)
    assert limit == M and n_off.tolist() == [M, M - lc.COLLAPSED_BROAD, 0]
    ref = reference(c)
    rtol, atol = lc.score_bounds(c, ref, twin.any(axis=1))
    for j, (lo, T) in enumerate(zip(c['begin'], c['lens'])):
        assert np.isfinite(got[j]).all()
        kind = 'f32 ln b, f32-class bound' if n_off[j] else 'f32 ln b, ordinary states'
        used = held(kind, 'logdet collapsed', 'ln b, %d of %d mixtures off the pipe' % (n_off[j], M), got[j], ref[j, lo:lo + T], rtol[j], atol[j, lo:lo + T])
        print('LOGDET collapsed state %d (%d off the pipe): %.3g of the bound, max |d ln b| %.3e, ln b in [%.1f, %.1f]' % (
            j, n_off[j], used, np.abs(got[j] - ref[j, lo:lo + T]).max(), ref[j, lo:lo + T].min(), ref[j, lo:lo + T].max()))
    # for the report only: what the coarse pass evaluated exactly and what it gave up, counted by a context of its own
    e = engine_under(PCL_COARSE_SPLIT_MAX='1.0', PCL_COARSE_STATS='1')
    try:
        e.coarse_counters()
        again = score_own_frames_twice(e, c)
        pairs, given_up = e.coarse_counters()
        off_pairs = sum(int(n) * int(T) for n, T in zip(n_off, c['lens']))
        print('LOGDET collapsed counters (two launches): %d (frame, mixture) pairs evaluated exactly of %d off-pipe pairs, %d tiles given up' % (pairs, 2 * off_pairs, given_up))
        assert all(np.array_equal(a, g) for a, g in zip(again, got))
    finally:
        e.close()


# ------------------------------------------------------------------ survives: the flag belongs to the resident model
def hold_live_batch(eng, b, c, step, logdet=True):
    """model_download, rescore the live batch in PCL_F64, B against the plain reference of the DOWNLOADED parameters (1e-12 relative); the
    other constant's reference is at least D/2 nats away on every compared element, so a dropped flag cannot pass."""
    mean, var, w = eng.model_download()
    D = mean.shape[2]
    assert np.isfinite(mean).all() and (var > 0).all() and (w >= 0).all()
    b.score(precision('f64'))
    ld, q1 = lc.point_states(c['frames'], mean, var, w), lc.point_states(c['frames'], mean, var, w, True)
    cmp = lc.compared_pairs(c)
    assert (ld - q1)[cmp].min() >= 0.5 * D
    ref = ld if logdet else q1
    hold_sentence_rows(lambda j: 'f64 ln b', 'logdet survives', c, b.get('B'), ref, np.full(len(ref), 1e-12), 0.0)
    print('LOGDET survives, after %s: (J, M, D) = %s, ln b held to the %s reference of the downloaded model; the other constant is >= %.1f nats away' % (
        step, mean.shape, 'log-determinant' if logdet else 'Q1', (ld - q1)[cmp].min()))
    return mean, var, w


def estep_f64(eng, b):
    P = precision('f64')
    b.score(P)
    b.forward_backward()
    eng.stats_zero()
    b.accumulate(P)


def hold_mstep(eng, c, before, step):
    """The downloaded model against po.gmm_update_param on the oracle's accumulators (the model `before` with w'): the bounds of
    tests/test_gpu_units.py test_em_loop_stays_on_device for the PCL_F64 route."""
    nm, nv, nw = eng.model_download()
    acc = lc.estep(c, *before)['log']
    for j in range(nm.shape[0]):
        rw, rm, rv = po.gmm_update_param(acc[j], c_covariance=1e-3)
        held('f64 M-step', 'logdet survives ' + step, 're-estimated weights', nw[j], rw, 1e-8)
        held('f64 M-step', 'logdet survives ' + step, 're-estimated means', nm[j], rm, 1e-8, 1e-8)
        held('f64 M-step', 'logdet survives ' + step, 're-estimated variances', nv[j], rv, 1e-7)


def test_the_flag_survives_every_model_update(eng):
    from poccala_amd import PCL_F64
    c = lc.survives()
    J, M, D = c['mean'].shape
    eng.load_model(c['mean'], c['var'], c['w'], logdet=True)
    eng.load_frames(c['frames'])
    eng.load_units(np.stack(c['trans']))
    b = eng.label_batch(c['labels'], c['lens'], c['begin'])
    try:
        model = hold_live_batch(eng, b, c, '1 load_model(logdet=True)')
        assert all(np.array_equal(x, y) for x, y in zip(model, (c['mean'], c['var'], c['w'])))
        estep_f64(eng, b)
        eng.mstep()
        hold_mstep(eng, c, model, 'mstep')
        model = hold_live_batch(eng, b, c, '2 mstep')
        estep_f64(eng, b)
        eng.em_exchange(update_transitions=False)
        hold_mstep(eng, c, model, 'em_exchange')
        model = hold_live_batch(eng, b, c, '3 em_exchange')
        b.score(PCL_F64)
        b.forward_backward()
        eng.stats_zero()
        b.accumulate_exchange(PCL_F64, n_chunks=2)                       # (state chunks re-derived on their own: pcl_launch_derive_range)
        after = hold_live_batch(eng, b, c, '4 accumulate_exchange(n_chunks=2)')
        assert not np.array_equal(after[0], model[0])
        eng.mixup(lc.SURV_MIXUP)
        model = hold_live_batch(eng, b, c, '5 mixup(16)')
        assert model[0].shape == (J, lc.SURV_MIXUP, D)
        eng.transform_means(c['W'])
        after = hold_live_batch(eng, b, c, '6 transform_means')
        assert np.abs(after[0] - (model[0] @ c['W'][0][:, 1:].T + c['W'][0][:, 0])).max() < 1e-12 and np.array_equal(after[1], model[1])
        estep_f64(eng, b)
        eng.mstep_map(10.0)
        model = hold_live_batch(eng, b, c, '7 mstep_map(tau=10)')
        assert not np.array_equal(model[0], after[0]) and np.array_equal(model[1], after[1])
        x = c['frames'].astype(np.float64)
        eng.flat_start_model(J, M, x.mean(axis=0), x.var(axis=0), logdet=True)
        model = hold_live_batch(eng, b, c, '8 flat_start_model(logdet=True)')
        assert model[0].shape == (J, M, D)
        seg = eng.segments(c['frame_state'], J=J)
        try:
            sweeps = seg.kmeans(lc.SURV_K, seed=3)
        finally:
            seg.close()
        assert (sweeps >= 0).all()
        model = hold_live_batch(eng, b, c, '9 Segments.kmeans(K=4)')
        assert model[0].shape == (J, lc.SURV_K, D)
    finally:
        b.close()
    report('survives')


def test_reloading_the_same_arrays_with_the_other_constant(eng):
    """The engine skips an upload whose digest it holds; the digest's key includes the flag, so the same arrays under the other constant are
    uploaded again: each load gives its own reference."""
    c = lc.survives()
    eng.load_model(c['mean'], c['var'], c['w'], logdet=True)
    eng.load_frames(c['frames'])
    eng.load_units(np.stack(c['trans']))
    b = eng.label_batch(c['labels'], c['lens'], c['begin'])
    try:
        hold_live_batch(eng, b, c, 'load_model(logdet=True)')
        eng.load_model(c['mean'], c['var'], c['w'], logdet=False)
        hold_live_batch(eng, b, c, 'load_model(logdet=False), the same arrays', logdet=False)
        eng.load_model(c['mean'], c['var'], c['w'], logdet=True)
        hold_live_batch(eng, b, c, 'load_model(logdet=True) again')
    finally:
        b.close()
