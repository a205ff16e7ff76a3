"""Starting from nothing on the device (csrc/bootstrap.hip: pcl_frames_moments, pcl_model_flat_start, pcl_flat_start,
pcl_uniform_segments) against golden G20 -- the reference's own __flat_start / __eq_segment / __get_gmmdata, executed -- and against
the NumPy twin G20 pins (tests/_bootstrap_twin.py, tests/test_bootstrap_twin.py).

Bounds.  Moments and the flat-start model: 1e-10 relative, the bound DESIGN.md section 2 uses for float64 restatements (the twin's
np.mean does not share the device's summation order, so bit equality is asked only between two device runs).  The owner map, the
segment lists and everything made from them: exact.  ln b from the device-made model against ln b from an upload of the downloaded
arrays: bit-identical.  End to end: the bounds tests/test_gpu_parity.py::test_estep_end_to_end holds an E-step to.  Comparisons go
through tests/_parity.py:hold, which records the measured worst case; every figure is printed before it is asserted."""
import numpy as np
import pytest

import _bootstrap_twin as tw
from _parity import cov_acc_atol, hold
from test_bootstrap_twin import fs_cases, fs_corpus, us_labels

pytestmark = pytest.mark.gpu
RTOL = 1e-10
F32_RTOL = 1e-4              # the north-star bound (tests/test_gpu_parity.py)
F32_LOGLIK_ATOL = 5e-5       # the project's absolute bound on a float32 ln b_j(o_t) (tests/test_gpu_parity.py)
S = 5


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def ragged_corpus(seed, U, D, tmax, dtype):
    """frames with rows nobody owns between the utterances; lengths include 0 and 1"""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, tmax + 1, size=U).astype(np.int32)
    T[rng.integers(0, U)] = 0
    T[rng.integers(0, U)] = 1
    T[0] = max(T[0], 2)
    gap = rng.integers(0, 4, size=U)
    begin = (np.cumsum(gap) + np.concatenate([[0], np.cumsum(T[:-1])])).astype(np.int64)
    F = int(begin[-1] + T[-1] + 3)
    frames = (rng.standard_normal((F, D)) * rng.uniform(0.2, 3.0, D) + rng.uniform(1.0, 4.0, D) * rng.choice([-1, 1], D)).astype(dtype)
    return frames, T, begin


# ------------------------------------------------------------------ moments
def test_moments_match_the_reference_golden(eng, golden):
    g = golden('G20_bootstrap')
    frames, lens, begin, n_utts = fs_corpus(g)
    eng.load_frames(frames)                                           # float64 upload: the float64 copy is read
    for c, case in enumerate(fs_cases(g)):
        step = int(case['step'])
        mean, var, n = eng.frames_moments(lens, begin, n_utts=n_utts, step=step)
        mean2, var2, n2 = eng.frames_moments(lens, begin, n_utts=n_utts, step=step)
        assert n == n2 == len(tw.sample_rows(lens, begin, n_utts, step))
        assert mean.tobytes() == mean2.tobytes() and var.tobytes() == var2.tobytes()
        hold('bootstrap golden fs%d' % c, 'var', var, case['var'][0, 0], RTOL)
        if not int(case['diff']):
            hold('bootstrap golden fs%d' % c, 'mean', mean, case['mean'][0, 0], RTOL)
        tm, tv, _ = tw.moments(frames, lens, begin, n_utts, step)
        hold('bootstrap golden fs%d' % c, 'mean vs twin', mean, tm, RTOL)
        hold('bootstrap golden fs%d' % c, 'var vs twin', var, tv, RTOL)
        print('fs%d floored feature: %r' % (c, var[4]))
        assert var[4] == 1e-4                                         # through (v ** 0.5) ** 2


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('seed,U,D,tmax,step', [(1, 40, 39, 200, 1), (2, 25, 13, 300, 7), (3, 60, 20, 120, 2), (4, 7, 47, 2000, 3)])
def test_moments_on_random_ragged_batches(eng, dtype, seed, U, D, tmax, step):
    frames, T, begin = ragged_corpus(seed, U, D, tmax, np.float64 if dtype == 'f64' else np.float32)
    eng.load_frames(frames)
    n_utts = max(1, int(U * 0.7))
    mean, var, n = eng.frames_moments(T, begin, n_utts=n_utts, step=step)
    mean2, var2, _ = eng.frames_moments(T, begin, n_utts=n_utts, step=step)
    assert mean.tobytes() == mean2.tobytes() and var.tobytes() == var2.tobytes()      # two device runs: equal bits
    tm, tv, tn = tw.moments(frames, T, begin, n_utts, step)                            # (the twin widens the same float32 rows)
    assert n == tn
    print('moments %s seed %d: n = %d (%d workgroups)' % (dtype, seed, n, (n + 1023) // 1024))
    hold('bootstrap moments %s' % dtype, 'mean', mean, tm, RTOL)
    hold('bootstrap moments %s' % dtype, 'var', var, tv, RTOL)


# ------------------------------------------------------------------ the flat-start model
def all_state_lnb(eng, T, begin, precision):
    b = eng.all_state_batch(T, begin)
    b.score(precision)
    B = b.get('B')
    b.close()
    return B


def test_flat_start_model_matches_the_reference_golden(eng, golden):
    g = golden('G20_bootstrap')
    frames, lens, begin, n_utts = fs_corpus(g)
    eng.load_frames(frames)
    for c, case in enumerate(fs_cases(g)):
        mean, var, _ = eng.frames_moments(lens, begin, n_utts=n_utts, step=int(case['step']))
        J, M, D = case['mean'].shape
        eng.flat_start_model(J, M, mean, var, case['coeff'] if int(case['diff']) else None)
        m, v, w = eng.model_download()
        hold('bootstrap golden fs%d' % c, 'model mean', m, case['mean'], RTOL)
        hold('bootstrap golden fs%d' % c, 'model var', v, case['var'], RTOL)
        hold('bootstrap golden fs%d' % c, 'model weight', w, case['weight'], RTOL)
        # the one-call chain: the same bits
        mean_c, var_c, _ = eng.flat_start(lens, begin, J, M, n_utts=n_utts, step=int(case['step']), coeff=case['coeff'] if int(case['diff']) else None)
        assert mean_c.tobytes() == mean.tobytes() and var_c.tobytes() == var.tobytes()
        for a, b in zip(eng.model_download(), (m, v, w)):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('prec', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['small', 'split', 'none'])
def test_lnb_from_the_device_made_model_equals_an_upload(eng, prec, kind):
    """ln b scored from pcl_model_flat_start's model is bit-identical to ln b after pcl_model_upload of the downloaded arrays;
    `split`: a few coefficients large enough to take their mixtures off the matrix pipe (the split route); `none`: coeff = NULL."""
    from oracle import poccala_oracle as po
    from poccala_amd import PCL_F32, PCL_F64
    P = PCL_F32 if prec == 'f32' else PCL_F64
    J, M, D = 6, 64, 39
    frames, T, begin = ragged_corpus(9, 12, D, 120, np.float32)
    keep = T > 0
    T, begin = T[keep], begin[keep]
    eng.load_frames(frames)
    mean, var, _ = eng.frames_moments(T, begin)
    rng = np.random.default_rng(5)
    coeff = None
    if kind != 'none':
        coeff = rng.uniform(-0.05, 0.05, M)
        if kind == 'split':
            coeff[rng.choice(M, 5, replace=False)] = rng.choice([-6.0, 6.0], 5)
    eng.flat_start_model(J, M, mean, var, coeff)
    if prec == 'f32':
        n_off, limit = eng.model_split_info()
        print('%s: off-pipe mixtures per state %s, limit %d' % (kind, n_off, limit))
        if kind == 'split':
            assert n_off.min() > 0 and n_off.max() <= limit          # the states ARE on the split route
        else:
            assert n_off.max() == 0
    B1 = all_state_lnb(eng, T, begin, P)
    m, v, w = eng.model_download()
    tm, tv, tww = tw.flat_model(mean, var, coeff, J, M)
    assert m.tobytes() == tm.tobytes() and v.tobytes() == tv.tobytes() and w.tobytes() == tww.tobytes()
    eng.load_model(m, v, w)
    B2 = all_state_lnb(eng, T, begin, P)
    for u in range(len(T)):
        assert B1[u].tobytes() == B2[u].tobytes()
    if kind == 'none':                                                # every mixture equal: the single Gaussian's value
        for u in range(len(T)):
            x = frames[begin[u]:begin[u] + T[u]].astype(np.float64)
            ref = po.gmm_point(x, mean[None, :], var[None, :], np.ones(1))
            for j in (0, J - 1):
                hold('bootstrap lnb %s' % prec, 'coeff NULL vs one Gaussian', B1[u][1 + j], ref, 0.0 if prec == 'f32' else 1e-12,
                     F32_LOGLIK_ATOL if prec == 'f32' else 0.0)


# ------------------------------------------------------------------ uniform segmentation
def test_uniform_map_equals_the_reference_golden(eng, golden):
    g = golden('G20_bootstrap')
    F = int(g['us_F'])
    eng.load_frames(np.random.default_rng(0).standard_normal((F, 13)))
    for sn in (5, 4):
        J = int(g['us_n_units']) * (sn - 2)
        seg, state = eng.uniform_segments(us_labels(g), g['us_T'], g['us_begin'], sn - 2, J, want_map=True)
        assert np.array_equal(state, g['us%d_frame_state' % sn])
        assert np.array_equal(seg.counts, np.bincount(state[state >= 0], minlength=J))
        seg.close()


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_uniform_segments_on_random_ragged_label_batches(eng, seed):
    from poccala_amd import PCL_F64
    rng = np.random.default_rng(100 + seed)
    U, D, n_units, gmm_num = 30, 13, 5, 3 + seed % 2
    frames, T, begin = ragged_corpus(50 + seed, U, D, 150, np.float64)
    labels = [rng.integers(0, n_units, size=rng.integers(1, 7)).astype(np.int32) for _ in range(U)]
    labels[3] = np.zeros(0, dtype=np.int32)                           # an utterance without a label
    short = 5
    T[short] = 1
    labels[short] = np.array([1, 2, 0], dtype=np.int32)               # T < L: nothing used
    J = n_units * gmm_num
    eng.load_frames(frames)
    seg, state = eng.uniform_segments(labels, T, begin, gmm_num, J, want_map=True)
    want = tw.uniform_map(len(frames), labels, T, begin, gmm_num)
    assert np.array_equal(state, want)
    assert (want[begin[short]:begin[short] + 1] == -1).all() and (want >= 0).any() and (want == -1).any()
    ref = eng.segments(want, J=J)
    assert np.array_equal(seg.counts, ref.counts) and np.array_equal(seg.order, ref.order)
    models = []
    for s in (seg, ref):                                              # clustering is deterministic for a seed: a difference is a difference in the segments
        sw = s.kmeans(2, seed=7, precision=PCL_F64)
        it, q = s.em(precision=PCL_F64)
        models.append((sw, it, q) + eng.model_download())
        s.close()
    for a, b in zip(*models):
        assert a.tobytes() == b.tobytes()
    assert (models[0][1] >= 0).any()


# ------------------------------------------------------------------ end to end, from no model
@pytest.mark.parametrize('prec', ['f32', 'f64'])
def test_flat_start_batch_then_estep_matches_the_oracle(eng, prec):
    from oracle import poccala_oracle as po
    from poccala_amd import PCL_F32, PCL_F64, synth
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    P = PCL_F32 if prec == 'f32' else PCL_F64
    units_n, M, D = 5, 16, 39
    frames, lens, begin = synth.make_frames(6, 60, D, seed=302, ragged=True)
    labels = synth.make_labels(6, 4, units_n, seed=303)
    names = ['u%d' % i for i in range(units_n)]
    am = AcousticModel(state_num=S, mix_level=M, dct_num=13)
    unit_hmms = {u: am.init_unit(u) for u in names}
    data_list = [frames[begin[u]:begin[u] + lens[u]].astype(np.float64) for u in range(len(lens))]
    mean, var, coeff = am.flat_start_batch(data_list, unit_hmms, proportion=0.5, step=2, coefficient=0.5, seed=3, engine=eng)
    n_utts = int(len(lens) * 0.5)
    tm, tv, _ = tw.moments(np.concatenate(data_list), lens, begin, n_utts, 2)
    hold('bootstrap e2e %s' % prec, 'mean', mean, tm, RTOL)
    hold('bootstrap e2e %s' % prec, 'var', var, tv, RTOL)
    rs = np.random.RandomState(3)
    assert np.array_equal(coeff, ((rs.random_sample((M, 1)) - rs.random_sample((M, 1))) * 0.5)[:, 0])
    J = units_n * (S - 2)
    mm, mv, mw = tw.flat_model(tm, tv, coeff, J, M)
    for got, want, what in zip(eng.model_download(), (mm, mv, mw), ('model mean', 'model var', 'model weight')):   # resident
        hold('bootstrap e2e %s' % prec, what, got, want, RTOL)
    g0 = unit_hmms['u2'].profunction[2].model_arrays()                                                                # ... and in the GMM objects
    hold('bootstrap e2e %s' % prec, 'GMM object mean', g0[0], mm[0], RTOL)
    stats, hmm_acc, logp = am.estep_batch([[names[i] for i in lab] for lab in labels], data_list, unit_hmms, precision=P, engine=eng)
    model = {u: dict(trans=synth.flat_start_transmat(S), gmms=[(mm[u * 3 + k], mv[u * 3 + k], mw[u * 3 + k]) for k in range(3)]) for u in range(units_n)}
    ref = dict(acc=np.zeros((J, M)), alpha_acc=np.zeros(J), mean_acc=np.zeros((J, M, D)), cov_acc=np.zeros((J, M, D)))
    rt = F32_RTOL if prec == 'f32' else 1e-9
    for u, lab in enumerate(labels):
        bw, accs, _ = po.estep_utterance(data_list[u], list(lab), model)
        hold('bootstrap e2e %s' % prec, 'logp', logp[u], bw['logp'][0], rt)
        for pos, unit in enumerate(lab):
            for k in range(S - 2):
                a = accs[pos].gmm[k]
                for key in ref:
                    ref[key][unit * (S - 2) + k] += np.exp(a[key])
    for key in ('acc', 'alpha_acc', 'mean_acc', 'cov_acc'):
        at = np.abs(ref[key]).max() * (1e-6 if prec == 'f32' else 1e-13)
        if key == 'cov_acc' and prec == 'f32':
            at = cov_acc_atol(ref['acc'], mm, mv, at)
        hold('bootstrap e2e %s' % prec, key, stats[key], ref[key], rt, at)


def test_init_segments_batch_then_alignment_runs(eng):
    from poccala_amd import synth
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    units_n, M, D, U, L, T = 4, 2, 13, 12, 3, 90
    mean, var, w, _ = synth.make_model(units_n, M, D, seed=21)
    labels = synth.make_labels(U, L, units_n, seed=22)
    assert len(set(int(i) for lab in labels for i in lab)) == units_n
    frames = synth.make_peaked_frames(labels, T, mean * 4, var, seed=23)
    names = ['u%d' % i for i in range(units_n)]
    am = AcousticModel(state_num=S, mix_level=M, dct_num=13, delta_1=False, delta_2=False)
    unit_hmms = {u: am.init_unit(u) for u in names}
    data_list = [frames[u * T:(u + 1) * T].astype(np.float64) for u in range(U)] + [np.zeros((0, D))]      # + one without frames
    name_labels = [[names[i] for i in lab] for lab in labels] + [[names[0]]]
    assert eng.J == 0                                                     # no model in the context
    out = am.init_segments_batch(name_labels, data_list, unit_hmms, engine=eng)
    assert sorted(out) == names
    for u in names:
        iters, q, skipped = out[u]
        counts = am.last_segment_counts[u]
        print('%s: frames per state %s, EM loop bodies %s' % (u, counts, iters))
        assert np.array_equal(iters >= 0, counts >= M) and np.array_equal(skipped, iters < 0)
        assert (counts >= M).all()
    res = am.align_batch(name_labels[:-1], data_list[:-1], unit_hmms, engine=eng)
    assert len(res) == U and all(len(names_u) == T for _, names_u in res)


# ------------------------------------------------------------------ errors
def test_errors_are_invalid_with_a_message_and_leave_the_context_usable():
    from poccala_amd import Engine, PoccalaHipError
    e = Engine(0)
    try:
        T, begin = np.array([20, 30], dtype=np.int32), np.array([0, 20], dtype=np.int64)
        lab = [np.array([0, 1], dtype=np.int32), np.array([2], dtype=np.int32)]

        def invalid(fn, *a, **k):
            with pytest.raises(PoccalaHipError) as ei:
                fn(*a, **k)
            print(ei.value)
            assert ei.value.code == -1 and len(str(ei.value)) > 40
        invalid(e.frames_moments, T, begin)                                # no frames loaded
        invalid(e.uniform_segments, lab, T, begin, 3, 9)
        invalid(e.flat_start, T, begin, 9, 4)
        frames = np.random.default_rng(0).standard_normal((50, 13)) + 2
        e.load_frames(frames)
        invalid(e.frames_moments, T, begin, n_utts=0)
        invalid(e.frames_moments, T, begin, n_utts=3)
        invalid(e.frames_moments, T, begin, step=0)
        invalid(e.frames_moments, np.array([0, 30], dtype=np.int32), begin, n_utts=1)       # empty sample
        invalid(e.frames_moments, np.array([20, 31], dtype=np.int32), begin)                 # outside the frame matrix
        invalid(e.flat_start_model, 9, 4, np.zeros(12), np.ones(12))       # D mismatch with the resident frames
        invalid(e.flat_start_model, 9, 4, np.zeros(13), np.zeros(13))      # variance not positive
        invalid(e.uniform_segments, lab, T, begin, 3, 10)                  # J not a multiple of gmm_num
        invalid(e.uniform_segments, lab, T, begin, 3, 6)                   # label id 2 >= J / gmm_num
        invalid(e.uniform_segments, lab, T, np.array([0, 10], dtype=np.int64), 3, 9)         # overlapping utterances
        mean, var, n = e.frames_moments(T, begin)                          # still usable
        tm, tv, _ = tw.moments(frames, T, begin, 2, 1)
        np.testing.assert_allclose(mean, tm, rtol=RTOL)
        np.testing.assert_allclose(var, tv, rtol=RTOL)
        seg = e.uniform_segments(lab, T, begin, 3, 9)
        assert seg.counts.sum() == 50
        seg.close()
    finally:
        e.close()
