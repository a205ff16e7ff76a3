"""fMLLR on the device (csrc/frame_adapt.hip: pcl_fmllr_zero, pcl_batch_accumulate_fmllr, pcl_fmllr_stats_download, pcl_fmllr_estimate,
pcl_frames_transform; Batch.accumulate_fmllr, Engine.fmllr_* / transform_frames, AcousticModel.fmllr_batch) against the NumPy twin of the
rule (tests/_fmllr_twin.py, whose own invariants tests/test_fmllr_twin.py holds).

Inputs (_fmllr_twin.make_case): J = 7 one-state units, M = 70 (padded to 72) with dead and zero-weight mixtures, utterances of 63, 64, 1,
130, 30, 65 and 20 frames with unowned rows before, between and behind them, speakers 0 and 1 (193 and 129 frames), speaker 2 below
min_occ, speaker 3 without an utterance, one utterance of speaker -1.  Posteriors: a real PCL_F64 score + forward-backward on label batches.

Bounds.  Statistics: every element of G, k and beta within 1e-10 x the twin's sum of the ABSOLUTE terms of that element (a float64 sum of
fewer than 1e5 terms loses at most n 2^-53 of that sum in any order; 1e-10 is the project's float64 restatement contract).  Estimate, fed
the DEVICE's statistics: statuses exact; max |W_dev - W_longdouble| <= 8 e_ref, e_ref = max |W_float64_twin - W_longdouble_twin|; Q(W_dev) >=
Q(W_twin) - 1e-9 |Q|; q_trace non-decreasing; the last row's stationarity equation within 1e-10 of its terms; beta 1e-10 relative, logdet
1e-10 against ln|det| of the device's own A.  Apply: the C-ABI has no frame download, so the transformed rows are compared through ln b,
bit for bit, with ln b after load_frames of the twin's transformed array: the default and the split route read the float32 rows, PCL_F64
the float64 copy; the all-rows batch covers the unowned rows -- and, at the dimensions of PADDED_D (host dimension below the device's row stride), the padded
frame columns: load_frames zeroes them, so a padded column the apply kernel wrote would move the bits.  Every figure is printed before it
is asserted.

Refusals.  LOW_OCCUPANCY: speakers 2 and 3 of every case.  NOT_POSITIVE_DEFINITE: test_a_speaker_refused_in_the_middle, from frames that
are exactly zero.  PCL_FMLLR_SINGULAR cannot be reached through the C-ABI from finite frames -- there is no statistics upload, and for a
positive definite G the step's a = p G^-1 p^T is > 0, its discriminant c^2 + 4 a beta too -- so it is held on the twin alone
(tests/test_fmllr_twin.py, with beta = inf) and no injection hook is built for it."""
import numpy as np
import pytest

import _fmllr_twin as tw

pytestmark = pytest.mark.gpu
RTOL = 1e-10
F64_RTOL = 1e-9
CHUNK = '50'                 # frames per K-chunk: speaker 0 has 193 = 3 x 50 + 43, speaker 1 129 = 2 x 50 + 29: ragged last chunks and k-steps
N_ITER = 20


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# Host dimensions below the device stride (tests/test_gpu_adapt.py lists what each reaches in the GEMM); 40, 46 and 47 run the
# fmllr_frames_kernel<47, 2> instance, whose second half of 24 dimensions runs over the row's constant at D = 47
PADDED_D = [12, 14, 15, 20, 30, 31, 40, 46, 47]
TILE_EDGE_D = [14, 15, 30, 31, 46, 47]
APPLY_D = [12, 20, 40, 47]
SMALL_D = [1, 2]             # n = 2 and 3, a 1 x 1 inversion at D = 1, a 13-wide device row that is almost all padding

_CASES = {}


def case(D):
    if D not in _CASES:
        _CASES[D] = tw.make_case(D)
    return _CASES[D]


def unit_trans():
    from poccala_amd import synth
    rng = np.random.default_rng(4)
    return np.stack([synth.random_left_right_transmat(rng, 3) for _ in range(tw.J)])


def estep(eng, D, frames=None):
    """model, units and frames up; a label batch scored and aligned under PCL_F64 -> (batch, rows, ln gamma, ln b)"""
    from poccala_amd import PCL_F64
    model, labels, fr, T, begin, spk, _ = case(D)
    eng.load_model(*model)
    eng.load_units(unit_trans())
    eng.load_frames(np.asarray(fr if frames is None else frames, dtype=np.float64))
    b = eng.label_batch(labels, T, begin)
    b.score(PCL_F64)
    b.forward_backward()
    rows = [np.concatenate([[-1], lab, [-2]]).astype(np.int32) for lab in labels]
    return b, rows, b.get('lgamma'), b.get('B')


def twin_stats(D, rows, lg, lb, frames=None):
    model, labels, fr, T, begin, spk, _ = case(D)
    return tw.frame_stats(model, fr if frames is None else frames, T, begin, rows, lg, lb, spk, tw.S_SPK)


def hold_stats(tag, got, t, scale=1.0):
    for name, g in zip(('G', 'k', 'beta'), got):
        err, bound = np.abs(g - scale * t[name]), RTOL * scale * t[name + 'abs']
        with np.errstate(all='ignore'):
            worst = np.nanmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)))
        print('%s: %s worst error / bound = %.3e' % (tag, name, worst))
        assert worst <= 1.0


def lnb(eng, precision):
    b = eng.all_state_batch(np.array([eng.F], dtype=np.int32), np.array([0], dtype=np.int64))
    b.score(precision)
    B = b.get('B')[0]
    b.close()
    return B


# ------------------------------------------------------------------ statistics and estimate against the twin
@pytest.mark.parametrize('D,what', [(13, 'chunk'), (13, 'default-chunk'), (13, 'valu'), (39, 'chunk'), (39, 'default-chunk'), (39, 'valu'),
                                    (26, 'chunk'), (26, 'valu'), (48, 'chunk'), (48, 'valu')]
                         + [(D, 'chunk') for D in PADDED_D + SMALL_D] + [(D, 'valu') for D in TILE_EDGE_D])
def test_statistics_and_estimate_are_the_twins(eng, monkeypatch, D, what):
    if 'default' not in what:
        monkeypatch.setenv('PCL_MLLR_CHUNK', CHUNK)
    if what == 'valu':
        monkeypatch.setenv('PCL_MLLR_VALU', '1')
    tag = 'fmllr D=%d %s' % (D, what)
    model, labels, fr, T, begin, spk, _ = case(D)
    b, rows, lg, lb = estep(eng, D)
    t = twin_stats(D, rows, lg, lb)
    cond = max(np.linalg.cond(t['G'][s, i]) for s in (0, 1) for i in range(D))
    print('%s: beta %s, cond(G) <= %.1f' % (tag, t['beta'], cond))
    assert cond < 1e4 and t['beta'][2] < tw.MIN_OCC < min(t['beta'][:2]) and t['beta'][3] == 0
    eng.fmllr_zero(tw.S_SPK)
    b.accumulate_fmllr(spk)
    G, k, beta = eng.fmllr_stats()
    hold_stats(tag, (G, k, beta), t)
    assert same_bits(G, np.swapaxes(G, 2, 3))                                                      # mirrored
    eng.fmllr_zero(tw.S_SPK)
    b.accumulate_fmllr(spk)
    again = eng.fmllr_stats()
    assert all(same_bits(x, y) for x, y in zip((G, k, beta), again))                               # two runs, the same bytes
    b.accumulate_fmllr(spk)                                                                        # a second batch of the same speakers adds
    hold_stats(tag + ' twice', eng.fmllr_stats(), t, 2.0)
    eng.fmllr_zero(tw.S_SPK)
    assert all(not x.any() for x in eng.fmllr_stats())                                             # zero clears
    b.accumulate_fmllr(spk)
    b.close()
    # the estimate, fed the device's statistics
    W, logdet, q, status = eng.fmllr_estimate(N_ITER, tw.MIN_OCC)
    W2, logdet2, q2, status2 = eng.fmllr_estimate(N_ITER, tw.MIN_OCC)
    assert same_bits(W, W2) and same_bits(logdet, logdet2) and same_bits(q, q2) and same_bits(status, status2)
    t64 = tw.estimate(G, k, beta, N_ITER, tw.MIN_OCC)
    tld = tw.estimate(G, k, beta, N_ITER, tw.MIN_OCC, dtype=np.longdouble)
    print('%s: status %s (twin %s)' % (tag, status, t64['status']))
    assert status.dtype == np.int32 and status.tolist() == t64['status'].tolist() == [0, 0, tw.LOW_OCCUPANCY, tw.LOW_OCCUPANCY]
    e_ref = float(np.abs(t64['W'] - tld['W']).max())
    e_dev = float(np.abs(W - tld['W']).max())
    print('%s: e_ref = max |W_f64 - W_longdouble| = %.3e, device max |W_dev - W_longdouble| = %.3e (ratio %.2f)' % (tag, e_ref, e_dev, e_dev / e_ref if e_ref else np.inf))
    for s in (0, 1):
        qd, qt = tw.aux(W[s], G[s], k[s], beta[s]), tw.aux(t64['W'][s], G[s], k[s], beta[s])
        print('%s: speaker %d Q(W_dev) %.9f Q(W_twin) %.9f, device trace end %.9f, logdet %.12f' % (tag, s, qd, qt, q[s, -1], logdet[s]))
        assert qd >= qt - F64_RTOL * abs(qt)
        assert (np.diff(q[s]) >= -F64_RTOL * np.abs(q[s, 1:])).all()
        assert abs(q[s, -1] - qd) <= F64_RTOL * abs(qd)
        assert abs(logdet[s] - np.linalg.slogdet(W[s][:, 1:])[1]) <= RTOL
        i = D - 1                                                                                  # the last row updated: its stationarity equation
        p = np.concatenate([[0.0], np.linalg.inv(W[s][:, 1:])[:, i]])
        w = W[s][i]
        res = beta[s] * p / (p @ w) - w @ G[s, i] + k[s, i]
        scale = np.abs(w) @ np.abs(G[s, i]) + np.abs(k[s, i]) + beta[s] * np.abs(p / (p @ w))
        print('%s: speaker %d stationarity residual / scale = %.3e' % (tag, s, (np.abs(res) / scale).max()))
        assert (np.abs(res) <= RTOL * scale).all()
    for s in (2, 3):
        assert same_bits(W[s], tw.identity(D)) and logdet[s] == 0 and np.isnan(q[s]).all()
    assert np.abs(beta - t['beta']).max() <= RTOL * np.abs(t['beta']).max()
    assert e_dev <= 8 * e_ref


# ------------------------------------------------------------------ apply
def split_model(D):
    mean, var, w = [a.copy() for a in case(D)[0]]
    mean[:, :3] += 3.0
    var[:, :3] = 0.02                                                                               # three tight mixtures far from the centre: off the matrix pipe
    return mean, var, w


@pytest.mark.parametrize('D', [13, 39] + APPLY_D + SMALL_D)
def test_transformed_frames_score_as_the_twins(eng, D):
    from poccala_amd import PCL_F32, PCL_F64, PoccalaHipError
    model, labels, fr, T, begin, spk, _ = case(D)
    b, rows, lg, lb = estep(eng, D)
    eng.fmllr_zero(tw.S_SPK)
    b.accumulate_fmllr(spk)
    b.close()
    W = eng.fmllr_estimate(N_ITER, tw.MIN_OCC)[0]
    want64 = tw.apply(fr, W, T, begin, spk)[0]
    moved = np.zeros(len(fr), bool)
    for u in (0, 1, 3, 5):
        moved[begin[u]:begin[u] + T[u]] = True
    assert same_bits(want64[~moved], fr[~moved]) and not same_bits(want64[moved], fr[moved])         # speaker 2 (refused), -1 and unowned rows stay
    before = lnb(eng, PCL_F64)
    eng.transform_frames(T, begin, spk)                                                            # the resident W
    got = {P: lnb(eng, P) for P in (PCL_F32, PCL_F64)}
    eng.load_model(*split_model(D))
    assert eng.model_split_info()[0].min() > 0
    got['split'] = lnb(eng, PCL_F32)
    eng.load_model(*model)
    eng.load_frames(want64)
    for P in (PCL_F32, PCL_F64):
        assert same_bits(got[P], lnb(eng, P))
    assert same_bits(got[PCL_F64][:, ~moved], before[:, ~moved]) and not same_bits(got[PCL_F64][:, moved], before[:, moved])
    eng.load_model(*split_model(D))
    assert same_bits(got['split'], lnb(eng, PCL_F32))
    eng.load_model(*model)
    eng.load_frames(np.asarray(fr, dtype=np.float64))
    eng.transform_frames(T, begin, spk, W)                                                         # explicit W == the resident one
    assert same_bits(got[PCL_F64], lnb(eng, PCL_F64)) and same_bits(got[PCL_F32], lnb(eng, PCL_F32))
    eng.load_frames(np.asarray(fr, dtype=np.float64))
    bad = begin.copy()
    bad[1] = begin[0] + 10                                                                          # utterance 1 now starts inside utterance 0
    with pytest.raises(PoccalaHipError) as ei:
        eng.transform_frames(T, bad, spk, W)
    assert ei.value.code == -1 and same_bits(lnb(eng, PCL_F64), before)
    eng.load_frames(np.asarray(fr, dtype=np.float32))                                              # no float64 copy: the float32 rows widened
    eng.transform_frames(T, begin, spk, W)
    got32 = lnb(eng, PCL_F32)
    eng.load_frames(tw.apply(np.asarray(fr, dtype=np.float32), W, T, begin, spk)[1])
    assert same_bits(got32, lnb(eng, PCL_F32))


# ------------------------------------------------------------------ a speaker refused between two accepted ones
def zeroed_frames(D):
    """the case's frames with every frame of speaker 1 (utterances 1 and 5) exactly 0: zeta = (1, 0 .. 0), G[1, i] = diag(sum p, 0 .. 0)"""
    model, labels, fr, T, begin, spk, _ = case(D)
    z = fr.copy()
    for u in np.flatnonzero(spk == 1):
        z[begin[u]:begin[u] + T[u]] = 0.0
    return z


@pytest.mark.parametrize('D', [13, 20])
def test_a_speaker_refused_in_the_middle(eng, monkeypatch, D):
    """speaker 1's second Cholesky pivot is exactly 0: fmllr_pivot_kernel, the refused branch of gk_solve_kernel with a factor to write,
    and the sweep kernel's refused outputs for a speaker between an accepted one and two refused for another reason"""
    from poccala_amd import PCL_F64
    monkeypatch.setenv('PCL_MLLR_CHUNK', CHUNK)
    tag = 'fmllr D=%d zero frames' % D
    model, labels, fr, T, begin, spk, _ = case(D)
    zf = zeroed_frames(D)
    run = {}
    for name, frames in (('plain', fr), ('zeroed', zf)):
        b, rows, lg, lb = estep(eng, D, frames)
        assert all(np.isfinite(x[1:-1]).all() for x in lb)                                         # the posteriors stay finite
        eng.fmllr_zero(tw.S_SPK)
        b.accumulate_fmllr(spk)
        b.close()
        run[name] = eng.fmllr_stats() + eng.fmllr_estimate(N_ITER, tw.MIN_OCC)
    G, k, beta, W, logdet, q, status = run['zeroed']
    hold_stats(tag, (G, k, beta), twin_stats(D, rows, lg, lb, zf))
    assert (G[1][:, 0, 0] > 0).all() and not G[1][:, 1:, :].any() and not G[1][:, :, 1:].any() and not k[1][:, 1:].any()
    t64 = tw.estimate(G, k, beta, N_ITER, tw.MIN_OCC)
    print('%s: status %s (twin %s), beta %s' % (tag, status, t64['status'], beta))
    assert status.tolist() == t64['status'].tolist() == [tw.OK, tw.NOT_POSITIVE_DEFINITE, tw.LOW_OCCUPANCY, tw.LOW_OCCUPANCY]
    assert same_bits(W[1], tw.identity(D)) and logdet[1] == 0 and np.isnan(q[1]).all()
    for s in (2, 3):
        assert same_bits(W[s], tw.identity(D)) and logdet[s] == 0 and np.isnan(q[s]).all()
    tld = tw.estimate(G, k, beta, N_ITER, tw.MIN_OCC, dtype=np.longdouble)
    e_ref, e_dev = float(np.abs(t64['W'] - tld['W']).max()), float(np.abs(W - tld['W']).max())
    print('%s: e_ref = %.3e, device %.3e (ratio %.2f)' % (tag, e_ref, e_dev, e_dev / e_ref if e_ref else np.inf))
    assert e_dev <= 8 * e_ref
    # one speaker's refusal does not move another's result: speaker 0's utterances, chunks and statistics are those of the plain run
    Gp, kp, betap, Wp, logdetp, qp, statusp = run['plain']
    assert statusp.tolist() == [tw.OK, tw.OK, tw.LOW_OCCUPANCY, tw.LOW_OCCUPANCY]
    assert same_bits(G[0], Gp[0]) and same_bits(k[0], kp[0]) and same_bits(beta[0], betap[0])
    assert same_bits(W[0], Wp[0]) and same_bits(logdet[0], logdetp[0]) and same_bits(q[0], qp[0])
    assert not same_bits(W[0], tw.identity(D))
    own = {s: np.zeros(len(fr), bool) for s in (0, 1)}
    for u in range(len(T)):
        if spk[u] in own:
            own[spk[u]][begin[u]:begin[u] + T[u]] = True
    before = lnb(eng, PCL_F64)
    eng.transform_frames(T, begin, spk)                                                            # the resident W
    after = lnb(eng, PCL_F64)
    assert same_bits(after[:, ~own[0]], before[:, ~own[0]]) and own[1].sum() == 129                # speaker 1's rows (and all others) keep their bits
    assert not same_bits(after[:, own[0]], before[:, own[0]])
    eng.load_frames(tw.apply(zf, W, T, begin, spk)[0])
    assert same_bits(after, lnb(eng, PCL_F64))


# ------------------------------------------------------------------ end to end
def test_fmllr_batch_raises_the_likelihood(eng):
    from poccala_amd import PCL_F64, synth
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    units_n, M, D, U, L, T, S = 3, 4, 13, 6, 3, 90, 5
    mean, var, w, _ = synth.make_model(units_n, M, D, seed=31)
    labels = synth.make_labels(U, L, units_n, seed=34)
    y = synth.make_peaked_frames(labels, T, mean, var, seed=33).astype(np.float64)
    rng = np.random.default_rng(8)
    spk = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
    frames = y.copy()
    for s in (0, 1):
        A, b = np.eye(D) * rng.uniform(0.8, 1.2, D) + 0.05 * rng.standard_normal((D, D)), 0.5 * rng.standard_normal(D)
        for u in np.flatnonzero(spk == s):
            frames[u * T:(u + 1) * T] = np.linalg.solve(A, (y[u * T:(u + 1) * T] - b).T).T
    names = ['u%d' % i for i in range(units_n)]
    am = AcousticModel(state_num=S, mix_level=M, dct_num=13, delta_1=False, delta_2=False)
    unit_hmms = {u: am.init_unit(u) for u in names}
    am._adopt_model((mean, var, w), names, unit_hmms)
    data_list = [frames[u * T:(u + 1) * T] for u in range(U)]
    name_labels = [[names[i] for i in lab] for lab in labels]
    out = am.fmllr_batch(name_labels, data_list, unit_hmms, spk, iterations=2, n_iter=N_ITER, min_occ=1.0, precision=PCL_F64, engine=eng)
    print('fmllr_batch: ln P(O) + sum T ln|det A|: %s, status %s' % (out['logp'], out['status']))
    lp = out['logp']
    assert len(lp) == 3 and all(st.tolist() == [0, 0] for st in out['status'])
    for a, b2 in zip(lp[:-1], lp[1:]):
        assert b2 >= a - F64_RTOL * abs(a) and b2 > a
    Wc, ldc = tw.compose(out['W_iter'][0][0], out['W_iter'][0][1], out['W_iter'][1][0], out['W_iter'][1][1])
    assert np.abs(out['W'] - Wc).max() <= 1e-12 * np.abs(Wc).max() and np.abs(out['logdet'] - ldc).max() <= 1e-12
    for a, b2 in zip(eng.model_download(), (mean, var, w)):
        assert same_bits(a, b2)                                                                     # the model is untouched
    lens, begin = np.full(U, T, dtype=np.int32), (np.arange(U) * T).astype(np.int64)
    eng.load_frames(frames)
    calls = []
    keep = eng.load_frames
    eng.load_frames = lambda f: calls.append(1) or keep(f)
    res = am.fmllr_batch(name_labels, (lens, begin), unit_hmms, spk, iterations=2, n_iter=N_ITER, min_occ=1.0, precision=PCL_F64, engine=eng)
    eng.load_frames = keep
    assert not calls and same_bits(res['W'], out['W']) and res['logp'] == out['logp']               # the resident route: no upload, the same bits


# ------------------------------------------------------------------ what is refused, and what the calls give back
@pytest.mark.parametrize('D', [49, 64])
def test_beyond_48_dimensions_the_calls_are_refused(eng, D):
    """the estimate's LDS matrices and the apply kernel's tile hold D <= 48: PCL_ERR_INVALID, model and frames as they were"""
    from poccala_amd import PCL_F64, PoccalaHipError
    model, labels, fr, T, begin, spk, W_true = case(D)
    eng.load_model(*model)
    eng.load_frames(np.asarray(fr, dtype=np.float64))
    before = lnb(eng, PCL_F64)
    for call in (lambda: eng.fmllr_zero(tw.S_SPK), lambda: eng.transform_frames(T, begin, spk, W_true)):
        with pytest.raises(PoccalaHipError) as ei:
            call()
        print(D, ei.value)
        assert ei.value.code == -1 and 'dimension %d' % D in str(ei.value)
        assert same_bits(lnb(eng, PCL_F64), before)
        for a, b2 in zip(eng.model_download(), model):
            assert same_bits(a, b2)
    with pytest.raises(PoccalaHipError) as ei:
        eng.fmllr_stats()                                                                           # the refused pcl_fmllr_zero made nothing
    assert ei.value.code == -3


def test_refusals_and_the_pool(eng):
    from poccala_amd import Engine, PoccalaHipError
    D = 13
    model, labels, fr, T, begin, spk, _ = case(D)

    def refused(call, code):
        with pytest.raises(PoccalaHipError) as ei:
            call()
        print(ei.value)
        assert ei.value.code == code and len(str(ei.value)) > 30

    refused(lambda: eng.fmllr_zero(2), -3)                                                          # no model
    b, rows, lg, lb = estep(eng, D)
    refused(lambda: b.accumulate_fmllr(spk), -3)                                                    # no statistics
    refused(lambda: eng.fmllr_estimate(), -3)
    refused(lambda: eng.fmllr_zero(0), -1)
    eng.fmllr_zero(2)
    refused(lambda: b.accumulate_fmllr(spk), -1)                                                    # speakers 2 and 3 of S = 2
    eng.fmllr_zero(tw.S_SPK)
    start = Engine.pool_stats()['handed_out_blocks']
    b.accumulate_fmllr(spk)
    assert Engine.pool_stats()['handed_out_blocks'] == start                                        # every temporary went back
    refused(lambda: eng.fmllr_estimate(0), -1)
    refused(lambda: eng.fmllr_estimate(5, -1.0), -1)
    refused(lambda: eng.transform_frames(T, begin, spk), -1)                                        # nothing estimated yet
    eng.fmllr_estimate(3, tw.MIN_OCC)
    resident = Engine.pool_stats()['handed_out_blocks']
    eng.fmllr_estimate(3, tw.MIN_OCC)
    eng.transform_frames(T, begin, spk)
    eng.transform_frames(T, begin, spk, np.stack([tw.identity(D)] * tw.S_SPK))
    print('handed-out blocks: %d with the statistics, %d with the resident transforms' % (start, resident))
    assert resident == start + 1 and Engine.pool_stats()['handed_out_blocks'] == resident
    refused(lambda: eng.transform_frames(T, begin, spk, None, 2), -1)                               # the resident estimate has another S
    b.close()
    eng.load_frames(np.zeros((int(begin[-1] + T[-1]), 26)))                                         # a frame matrix of another D drops the statistics
    refused(lambda: eng.fmllr_stats(), -3)
    b, rows, lg, lb = estep(eng, D)
    eng.fmllr_zero(tw.S_SPK)
    eng.load_model(model[0] + 1.0, model[1], model[2])                                              # the model was replaced since pcl_fmllr_zero
    refused(lambda: eng.fmllr_stats(), -3)
    refused(lambda: eng.fmllr_estimate(), -3)
    b.close()
    other = Engine(0)                                                                               # pcl_destroy with statistics resident
    other.load_model(*model)
    other.fmllr_zero(3)
    other.close()
