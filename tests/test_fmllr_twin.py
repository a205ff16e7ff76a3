"""The NumPy twin of the fMLLR rule (tests/_fmllr_twin.py) against what the rule must satisfy whatever implements it, and the host-side
bookkeeping of AcousticModel.fmllr_batch with a stub engine.  No GPU."""
import numpy as np
import pytest

import _fmllr_twin as tw


def mixture(D, M=4, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((M, D)) * 2.0, rng.uniform(0.5, 2.0, (M, D)), np.full(M, 1.0 / M)


def affine(D, seed=5):
    rng = np.random.default_rng(seed)
    return np.eye(D) * rng.uniform(0.8, 1.2, D) + 0.1 * rng.standard_normal((D, D)), rng.standard_normal(D)


def test_the_inversion_is_an_inversion():
    rng = np.random.default_rng(0)
    for D in (2, 7, 13):
        A = rng.standard_normal((D, D))
        A[0, 0] = 0.0                                                    # forces a row swap
        inv, ld = tw.invert(A)
        assert np.abs(inv @ A - np.eye(D)).max() < 1e-10 and abs(ld - np.linalg.slogdet(A)[1]) < 1e-12
        invl, _ = tw.invert(A.astype(np.longdouble))
        assert invl.dtype == np.longdouble and np.abs(np.asarray(invl, dtype=np.float64) - inv).max() < 1e-10
    assert tw.invert(np.zeros((3, 3)))[0] is None
    assert tw.invert(np.eye(4))[0].tobytes() == np.eye(4).tobytes()


def test_cholesky_and_solve():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((30, 6))
    G, b = X.T @ X, rng.standard_normal(6)
    L = tw.cholesky(G)
    assert np.abs(L @ L.T - G).max() < 1e-12 and np.abs(G @ tw.chol_solve(L, b) - b).max() < 1e-12
    assert tw.cholesky(np.diag([1.0, 0.0])) is None and tw.cholesky(np.diag([1.0, np.nan])) is None


def test_the_models_own_moments_give_the_identity_bit_for_bit():
    """G, k, beta of frames distributed as the model says: [0 | I] is stationary, and every update reproduces it exactly when the
    moments are those of a single frame-per-Gaussian population with A0 = I, b0 = 0 -- in exact arithmetic; in float64 the twin must stay
    within rounding and, started from [0 | I] with a p that is exactly a unit vector, return alpha p G^-1 + k G^-1 = row i of [0 | I]"""
    D = 5
    mu, var, w = mixture(D)
    G, k, beta = tw.population_stats(mu, var, w, np.eye(D), np.zeros(D))
    out = tw.estimate(G, k, beta, n_iter=3, min_occ=1.0)
    assert out['status'].tolist() == [tw.OK]
    assert np.abs(out['W'][0] - tw.identity(D)).max() < 1e-12 and abs(out['logdet'][0]) < 1e-12
    # bit for bit: 16 frames of the standard normal model -- G_i = 16 I, k_i = 0, every operation of the update is exact, and the two roots
    # +-16 tie, which goes to the + root
    G2, k2, beta2 = tw.population_stats(np.zeros((1, D)), np.ones((1, D)), np.ones(1), np.eye(D), np.zeros(D), count=16.0)
    out = tw.estimate(G2, k2, beta2, n_iter=2, min_occ=1.0)
    assert out['status'].tolist() == [tw.OK] and out['W'][0].tobytes() == tw.identity(D).tobytes() and out['logdet'][0] == 0.0


def test_exact_recovery_of_a_known_transform():
    D = 6
    mu, var, w = mixture(D, M=4)
    A0, b0 = affine(D)
    G, k, beta = tw.population_stats(mu, var, w, A0, b0)
    W0 = np.concatenate([b0[:, None], A0], axis=1)[None]
    kept = tw.estimate(G, k, beta, n_iter=2, min_occ=1.0, W0=W0)
    assert kept['status'].tolist() == [tw.OK]
    print('stationary: max |dW| = %.3e' % np.abs(kept['W'] - W0).max())
    assert np.abs(kept['W'] - W0).max() < 1e-10
    found = tw.estimate(G, k, beta, n_iter=60, min_occ=1.0)
    q0 = tw.aux(W0[0], G[0], k[0], beta[0])
    print('from the identity: Q %.9f, Q(W0) %.9f' % (found['q_trace'][0, -1], q0))
    assert abs(found['q_trace'][0, -1] - q0) <= 1e-9 * abs(q0)
    assert abs(found['logdet'][0] - np.linalg.slogdet(found['W'][0][:, 1:])[1]) < 1e-10


def test_q_never_falls_over_a_row_update_and_the_scale_of_p_is_irrelevant():
    D = 6
    mu, var, w = mixture(D, M=5, seed=9)
    A0, b0 = affine(D, seed=11)
    G, k, beta = tw.population_stats(mu, var, w, A0, b0)
    qs = []
    out = tw.estimate(G, k, beta, n_iter=4, min_occ=1.0, on_row=lambda s, W: qs.append(tw.aux(W, G[0], k[0], beta[0])))
    qs = np.array(qs)
    assert len(qs) == 4 * D and (np.diff(qs) >= -1e-9 * np.abs(qs[1:])).all()
    assert (np.diff(out['q_trace'][0]) >= -1e-9 * np.abs(out['q_trace'][0, 1:])).all()
    scaled = tw.estimate(G, k, beta, n_iter=4, min_occ=1.0, p_scale=-37.5)
    assert np.abs(scaled['W'] - out['W']).max() < 1e-10
    ld = tw.estimate(G, k, beta, n_iter=4, min_occ=1.0, dtype=np.longdouble)
    assert ld['W'].dtype == np.longdouble and np.abs(np.asarray(ld['W'], dtype=np.float64) - out['W']).max() < 1e-10


def test_the_three_refusals_in_order():
    D = 4
    mu, var, w = mixture(D)
    A0, b0 = affine(D)
    G1, k1, b1 = tw.population_stats(mu, var, w, A0, b0)
    G = np.concatenate([G1, G1, G1 * 0.0, G1, G1])
    k = np.concatenate([k1, k1, k1, k1, k1])
    beta = np.array([1000.0, 5.0, 5.0, 1000.0, 1000.0])                  # speaker 2: low occupancy AND a zero G: the occupancy is tested first
    G[3, 2] = 0.0                                                        # a zero pivot
    G[4] = G[4] * np.inf                                                 # nothing finite
    out = tw.estimate(G, k, beta, n_iter=2, min_occ=10.0)
    assert out['status'].tolist() == [tw.OK, tw.LOW_OCCUPANCY, tw.LOW_OCCUPANCY, tw.NOT_POSITIVE_DEFINITE, tw.NOT_POSITIVE_DEFINITE]
    for s in (1, 2, 3, 4):
        assert out['W'][s].tobytes() == tw.identity(D).tobytes() and out['logdet'][s] == 0 and np.isnan(out['q_trace'][s]).all()
    sing = tw.estimate(G1, k1, np.array([np.inf]), n_iter=1, min_occ=1.0)
    assert sing['status'].tolist() == [tw.SINGULAR] and sing['W'][0].tobytes() == tw.identity(D).tobytes()


def test_composition_is_application_in_turn():
    D = 5
    rng = np.random.default_rng(2)
    frames = rng.standard_normal((40, D))
    T, begin, spk = np.array([10, 12]), np.array([3, 20]), np.array([1, 0])
    W1 = np.stack([np.concatenate([affine(D, s)[1][:, None], affine(D, s)[0]], axis=1) for s in (1, 2)])
    W2 = np.stack([np.concatenate([affine(D, s)[1][:, None], affine(D, s)[0]], axis=1) for s in (3, 4)])
    ld1, ld2 = [np.array([np.linalg.slogdet(W[s][:, 1:])[1] for s in range(2)]) for W in (W1, W2)]
    twice = tw.apply(tw.apply(frames, W1, T, begin, spk)[0], W2, T, begin, spk)[0]
    Wc, ldc = tw.compose(W1, ld1, W2, ld2)
    once = tw.apply(frames, Wc, T, begin, spk)[0]
    assert np.abs(once - twice).max() < 1e-12
    assert np.abs(ldc - [np.linalg.slogdet(Wc[s][:, 1:])[1] for s in range(2)]).max() < 1e-12
    untouched = np.ones(40, bool)
    untouched[3:13] = untouched[20:32] = False
    assert once[untouched].tobytes() == frames[untouched].tobytes()
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    Wa, lda = AcousticModel.compose_fmllr(W1, ld1, W2, ld2)
    assert np.abs(Wa - Wc).max() < 1e-14 and np.abs(lda - ldc).max() == 0
    ident = np.stack([tw.identity(D)] * 2)
    y64, y32 = tw.apply(frames, ident, T, begin, spk)
    assert y64.tobytes() == frames.tobytes() and y32.dtype == np.float32


def hard_stats(D, frames=None):
    """the twin's statistics of tests/test_gpu_fmllr.py's case with every frame given to the state it was drawn along"""
    model, labels, fr, T, begin, spk, W_true = tw.make_case(D)
    frames = fr if frames is None else frames
    rows, lg, lb = [], [], []
    for u, lab in enumerate(labels):
        L = len(lab)
        rows.append(np.asarray(lab))
        own = np.minimum(np.arange(T[u]) * L // T[u], L - 1)
        with np.errstate(divide='ignore'):
            lg.append(np.log((own[None] == np.arange(L)[:, None]).astype(np.float64)))
        x = frames[begin[u]:begin[u] + T[u]]
        b = np.stack([tw.mixture_posteriors(model, x, np.zeros(T[u]), np.zeros(T[u]), j).sum(axis=1) for j in lab])
        lb.append(np.log(b))
    return tw.frame_stats(model, frames, T, begin, rows, lg, lb, spk, tw.S_SPK)


@pytest.mark.parametrize('D', [13, 26, 39, 48, 1, 2, 12, 14, 15, 20, 30, 31, 40, 46, 47])
def test_the_gpu_inputs_are_well_conditioned(D):
    """cond(G[s, i]) < 1e4 on the inputs of tests/test_gpu_fmllr.py, with every frame given to the state it was drawn along (the GPU test
    asserts the same on the twin's statistics of the real posteriors); 12 .. 47 are the dimensions the device pads, 1 and 2 the smallest"""
    st = hard_stats(D)
    assert abs(st['beta'][0] - 193.0) < 1e-9 and abs(st['beta'][1] - 129.0) < 1e-9 and st['beta'][2] < tw.MIN_OCC and st['beta'][3] == 0
    worst = max(np.linalg.cond(st['G'][s, i]) for s in (0, 1) for i in range(D))
    print('D = %d: cond(G) <= %.1f' % (D, worst))
    assert worst < 1e4
    out = tw.estimate(st['G'], st['k'], st['beta'], 2, tw.MIN_OCC)
    assert out['status'].tolist() == [tw.OK, tw.OK, tw.LOW_OCCUPANCY, tw.LOW_OCCUPANCY]


@pytest.mark.parametrize('D', [13, 20])
def test_a_speaker_of_zero_frames_is_refused_alone(D):
    """the input of test_gpu_fmllr.py::test_a_speaker_refused_in_the_middle: speaker 1's frames exactly 0 -> zeta = (1, 0 .. 0), every
    G[1, i] = diag(sum p, 0 .. 0) EXACTLY, the second pivot 0; the densities stay finite (the means are N(0, 1)), speaker 0's statistics
    and transform keep their bits"""
    model, labels, fr, T, begin, spk, W_true = tw.make_case(D)
    z = fr.copy()
    for u in np.flatnonzero(spk == 1):
        z[begin[u]:begin[u] + T[u]] = 0.0
    plain, st = hard_stats(D), hard_stats(D, z)
    assert all(np.isfinite(st[key]).all() for key in ('G', 'k', 'beta'))
    G1 = st['G'][1]
    assert (G1[:, 0, 0] > 0).all() and not G1[:, 1:, :].any() and not G1[:, :, 1:].any() and not st['k'][1][:, 1:].any()
    assert abs(st['beta'][1] - 129.0) < 1e-9                                # above MIN_OCC: the occupancy is not what refuses it
    out, ref = tw.estimate(st['G'], st['k'], st['beta'], 3, tw.MIN_OCC), tw.estimate(plain['G'], plain['k'], plain['beta'], 3, tw.MIN_OCC)
    assert out['status'].tolist() == [tw.OK, tw.NOT_POSITIVE_DEFINITE, tw.LOW_OCCUPANCY, tw.LOW_OCCUPANCY]
    assert out['W'][1].tobytes() == tw.identity(D).tobytes() and out['logdet'][1] == 0 and np.isnan(out['q_trace'][1]).all()
    assert st['G'][0].tobytes() == plain['G'][0].tobytes() and out['W'][0].tobytes() == ref['W'][0].tobytes()
    assert out['q_trace'][0].tobytes() == ref['q_trace'][0].tobytes() and not np.array_equal(out['W'][0], tw.identity(D))
    y = tw.apply(z, out['W'], T, begin, spk)[0]
    own1 = np.zeros(len(z), bool)
    for u in np.flatnonzero(spk == 1):
        own1[begin[u]:begin[u] + T[u]] = True
    assert own1.sum() == 129 and y[own1].tobytes() == z[own1].tobytes() and not y[own1].any()


# ------------------------------------------------------------------ fmllr_batch's bookkeeping
class StubBatch(object):
    def __init__(self, eng, T):
        self.eng, self.T, self.N = eng, T, np.full(len(T), 3)

    def score(self, precision):
        self.eng.log.append('score')

    def forward_backward(self):
        self.eng.log.append('fb')

    def get(self, what):
        assert what == 'logp'
        return np.full(len(self.T), -10.0 * (3 - self.eng.applied))

    def accumulate_fmllr(self, spk):
        self.eng.log.append(('acc', np.asarray(spk).tolist()))

    def close(self):
        pass


class StubEngine(object):
    def __init__(self, D, transforms):
        self.FD, self.log, self.applied, self.transforms, self.uploads = D, [], 0, transforms, 0

    def load_model(self, *a):
        pass

    def load_units(self, *a):
        pass

    def load_frames(self, f):
        self.uploads += 1
        assert f.dtype == np.float64

    def label_batch(self, unit_ids, lens, begin):
        return StubBatch(self, lens)

    def fmllr_zero(self, S):
        self.log.append(('zero', S))

    def fmllr_estimate(self, n_iter, min_occ):
        W = self.transforms[self.applied]
        ld = np.array([np.linalg.slogdet(w[:, 1:])[1] for w in W])
        return W, ld, np.zeros((len(W), n_iter)), np.zeros(len(W), dtype=np.int32)

    def transform_frames(self, T, begin, spk, W, S):
        assert W is None
        self.log.append(('apply', S))
        self.applied += 1


def test_fmllr_batch_bookkeeping():
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    D = 13
    am = AcousticModel(state_num=5, mix_level=2, dct_num=13, delta_1=False, delta_2=False)
    unit_hmms = {u: am.init_unit(u) for u in ('a', 'b')}
    Ws = [np.stack([np.concatenate([affine(D, 10 * it + s)[1][:, None], affine(D, 10 * it + s)[0]], axis=1) for s in range(2)]) for it in range(2)]
    eng = StubEngine(D, Ws)
    data = [np.zeros((7, D)), np.zeros((0, D)), np.zeros((5, D))]
    out = am.fmllr_batch([['a'], ['b'], ['b', 'a']], data, unit_hmms, [1, 0, -1], iterations=2, n_iter=4, min_occ=1.0, engine=eng)
    assert eng.uploads == 1 and eng.applied == 2                         # the frames go up once; the empty utterance is left out
    assert eng.log.count('score') == 3 and ('acc', [1, -1]) in eng.log and ('zero', 2) in eng.log
    ld = [np.array([np.linalg.slogdet(w[:, 1:])[1] for w in W]) for W in Ws]
    Wc, ldc = tw.compose(Ws[0], ld[0], Ws[1], ld[1])
    assert np.abs(out['W'] - Wc).max() < 1e-13 and np.abs(out['logdet'] - ldc).max() < 1e-13
    want = [-60.0, -40.0 + 7 * ld[0][1], -20.0 + 7 * ldc[1]]              # speaker 1 owns the 7-frame utterance; speaker -1 adds nothing
    assert np.abs(np.array(out['logp']) - want).max() < 1e-12 and len(out['status']) == 2
    res = am.fmllr_batch([['a'], ['b', 'a']], (np.array([7, 5]), np.array([0, 7])), unit_hmms, [0, 0], iterations=1, engine=StubEngine(D, [W[:1] for W in Ws]))
    assert res['W'].shape == (1, D, D + 1)
