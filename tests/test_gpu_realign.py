"""Realignment on the device (row f8): pcl_batch_align_segments / Batch.align_segments -- Viterbi paths of a label-built batch ->
owner map, dropped utterances and Segments -- against its NumPy twin (tests/_realign_twin.py, held to the oracle and golden G12 by
tests/test_realign_twin.py), against the old host route (Batch.segments), and through AcousticModel's scheme-1 helpers on resident
frames.  The twin is fed with the device's own b.get('path'), which keeps Viterbi ties out of the comparison; everything here is
integer work or the same kernels on the same inputs, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _realign_twin as rt

pytestmark = pytest.mark.gpu
D, M, N_UNITS = 13, 2, 6


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def frames_along(rng, labels, T, begin, F, mean, var, gmm_num):
    """(F, D) float64 frames: the rows of an utterance walk through the states of its label, one Gaussian of the state each; rows
    nobody owns are noise."""
    fr = rng.standard_normal((F, D)) * 3
    for lab, t, b in zip(labels, T, begin):
        st = (np.asarray(lab)[:, None] * gmm_num + np.arange(gmm_num)[None, :]).reshape(-1)
        st = st[np.arange(t) * len(st) // max(int(t), 1)]
        mix = rng.integers(0, M, size=t)
        fr[b:b + t] = mean[st, mix] + np.sqrt(var[st, mix]) * rng.standard_normal((t, D))
    return fr


def place(rng, T, front=7, behind=5, max_gap=4):
    """Row ranges for the utterances in a shuffled order (begin does not ascend), `front` rows before the first, random gaps
    between them and `behind` rows after the last."""
    T = np.asarray(T, dtype=np.int32)
    order = rng.permutation(len(T))
    if (np.diff(order) > 0).all():
        order = order[::-1]
    begin = np.empty(len(T), dtype=np.int64)
    row = front
    for i, u in enumerate(order):
        begin[u] = row
        row += int(T[u]) + (int(rng.integers(1, max_gap + 1)) if i + 1 < len(T) else 0)
    assert (np.diff(begin) < 0).any()
    return begin, row + behind


def old_row_unit(labels, gmm_num):
    out = []
    for lab in labels:
        ids = np.repeat(np.asarray(lab, dtype=np.int32), gmm_num)
        out.append(np.concatenate([[ids[0]], ids, [ids[-1]]]).astype(np.int32))
    return out


def aligned_batch(eng, S, labels, T, begin, F, seed):
    from poccala_amd import PCL_F64, synth
    rng = np.random.default_rng(1000 + seed)
    mean, var, w, _ = synth.make_model(N_UNITS, M, D, seed=seed + 40, s=S)
    mean = mean * 4
    trans = np.stack([synth.random_left_right_transmat(rng, S) for _ in range(N_UNITS)])
    eng.load_model(mean, var, w)
    eng.load_units(trans)
    eng.load_frames(frames_along(rng, labels, T, begin, F, mean, var, S - 2))
    b = eng.label_batch([np.asarray(l, dtype=np.int32) for l in labels], np.asarray(T, dtype=np.int32), begin)
    b.score(PCL_F64)
    b.viterbi()
    return b, (mean, var, w)


def check_against_twin_and_old_route(eng, S, labels, T, begin, F, seed, kept=(), surely_dropped=()):
    b, _ = aligned_batch(eng, S, labels, T, begin, F, seed)
    paths = b.get('path')
    seg, dropped, state = b.align_segments(want_map=True)
    want, want_dropped = rt.realign(paths, labels, S, T, begin, F)
    print('S = %d: %d utterances, %d dropped %s, %d of %d rows owned' % (S, len(T), len(dropped), dropped, int((want >= 0).sum()), F))
    assert state.shape == (F,) and state.dtype == np.int32
    assert np.array_equal(state, want)
    assert dropped == want_dropped and all(isinstance(u, int) for u in dropped)
    for u in kept:
        assert u not in dropped, u
    for u in surely_dropped:
        assert u in dropped, u
    owned = np.zeros(F, dtype=bool)
    for u in range(len(T)):
        owned[begin[u]:begin[u] + T[u]] = u not in dropped
    assert np.array_equal(state >= 0, owned)                              # -1 in front of, between and behind the utterances
    ref = eng.segments(want)
    assert np.array_equal(seg.counts, ref.counts) and np.array_equal(seg.order, ref.order)
    old = b.segments(old_row_unit(labels, S - 2), S - 2, dropped=want_dropped)
    assert np.array_equal(seg.counts, old.counts) and np.array_equal(seg.order, old.order)
    seg2, dropped2 = b.align_segments()                                   # without the map: the same Segments
    assert dropped2 == dropped and np.array_equal(seg2.counts, seg.counts) and np.array_equal(seg2.order, seg.order)
    for s in (seg, seg2, ref, old):
        s.close()
    b.close()
    return dropped


def edge_batch():
    a, bb, c = 0, 1, 2
    cases = [                                   # (label, T)
        ([3], 1), ([4], 2),                     # 0, 1: L = 1, chunk == 0: everything to the last state
        ([a], 3), ([bb, bb], 63), ([c, c, c], 64), ([5], 65),          # 2-5: one distinct unit
        ([a, a, bb], 130), ([a, bb, a], 65), ([a, a, bb], 3), ([a, bb, a], 200), ([bb, a, bb], 2),
        (list(np.random.default_rng(5).integers(0, N_UNITS, size=20)), 200),                   # 11: L = 20
        ([0, 1, 2, 3], 2), ([5, 4, 3, 2], 2),   # 12, 13: four distinct units on two frames
        ([0, 1], 63), ([2, 3, 4], 64), ([5, 0], 130), ([1, 2], 1), ([3, 3, 4, 4], 65),
    ]
    labels, T = [l for l, _ in cases], [t for _, t in cases]
    assert sorted(set(T)) == [1, 2, 3, 63, 64, 65, 130, 200]
    single = [u for u, l in enumerate(labels) if len(set(l)) == 1]
    assert len(single) >= 5
    return labels, T, single, [12, 13, 17]


@pytest.mark.parametrize('S', [5, 4])
def test_edges_match_the_twin_and_the_old_route(eng, S):
    labels, T, single, short = edge_batch()
    begin, F = place(np.random.default_rng(3), T)
    assert begin.min() == 7 and F == int((begin + np.asarray(T)).max()) + 5
    dropped = check_against_twin_and_old_route(eng, S, labels, T, begin, F, seed=S, kept=single, surely_dropped=short)
    assert len(dropped) < len(T) - len(single)                            # utterances with several units are kept too


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_random_batches_match_the_twin_and_the_old_route(eng, seed):
    """U = 40.  Every third utterance (u % 3 == 0) names one distinct unit: kept whatever the model.  Every seventh (u % 7 == 1; the
    two that are also a third stay single-unit) has fewer frames than distinct label units: dropped whatever the model."""
    rng = np.random.default_rng(200 + seed)
    U = 40
    labels, T = [], []
    for u in range(U):
        L = int(rng.integers(1, 9))
        if u % 3 == 0:
            lab = [int(rng.integers(0, N_UNITS))] * L
            t = int(rng.integers(1, 151))
        elif u % 7 == 1:
            k = int(rng.integers(2, N_UNITS + 1))
            lab = list(rng.permutation(N_UNITS)[:k]) + list(rng.integers(0, N_UNITS, size=max(0, min(8, L) - k)))
            lab = lab[:8]
            t = int(rng.integers(1, len(set(lab))))
        else:
            lab = list(rng.integers(0, N_UNITS, size=L))
            t = int(rng.integers(1, 151))
        labels.append([int(x) for x in lab])
        T.append(t)
    begin, F = place(rng, T, front=int(rng.integers(0, 9)), behind=int(rng.integers(0, 9)), max_gap=6)
    single = [u for u in range(U) if u % 3 == 0]
    short = [u for u in range(U) if u % 7 == 1 and u % 3 != 0]
    assert all(T[u] < len(set(labels[u])) for u in short) and len(short) >= 4
    dropped = check_against_twin_and_old_route(eng, 5, labels, T, begin, F, seed=10 + seed, kept=single, surely_dropped=short)
    assert len(dropped) < U - len(single)


def test_the_same_bits_downstream(eng):
    """k-means + EM from the device-made Segments and from Engine.segments(twin map), each from the same starting model."""
    from poccala_amd import PCL_F64
    rng = np.random.default_rng(77)
    U = 24
    labels = [[int(x) for x in rng.integers(0, N_UNITS, size=rng.integers(1, 5))] for _ in range(U)]
    T = [int(t) for t in rng.integers(30, 120, size=U)]
    begin, F = place(rng, T)
    b, model = aligned_batch(eng, 5, labels, T, begin, F, seed=7)
    paths = b.get('path')
    seg, dropped = b.align_segments()
    want, want_dropped = rt.realign(paths, labels, 5, T, begin, F)
    assert dropped == want_dropped and len(dropped) < U
    b.close()
    runs = []
    for s in (seg, None):
        eng._model_key = None
        eng.load_model(*model)                                            # the same starting model (skipped states keep it)
        s = s if s is not None else eng.segments(want)
        sweeps = s.kmeans(2, seed=11, precision=PCL_F64)
        iters, q = s.em(precision=PCL_F64)
        runs.append((sweeps, iters, q) + tuple(eng.model_download()))
        s.close()
    print('EM loop bodies per state:', runs[0][1])
    assert (runs[0][1] >= 1).any()
    for x, y in zip(*runs):
        assert np.array_equal(x, y, equal_nan=True)


def test_the_resident_chain_equals_the_uploaded_one(eng):
    """PCM -> Engine.frontend -> flat_start_batch -> init_segments_batch -> train_segments_batch on (lens, begin), no frame uploaded,
    against the same chain fed with the fetched rows as host arrays on a second set of unit objects."""
    from test_gpu_vad import speech_signal
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    rng = np.random.default_rng(31)
    sigs = [speech_signal(rng, n) for n in (16000, 9000, 12345)] + [np.zeros(8000, dtype=np.int16)] + [speech_signal(rng, n) for n in (20000, 11000, 14000)]
    names = ['u0', 'u1', 'u2']
    labels = [['u0', 'u1'], ['u1', 'u2'], ['u2', 'u0'], ['u0'], ['u0', 'u1', 'u2'], ['u1', 'u1', 'u0'], ['u2', 'u1']]

    def chain(data_of):
        am = AcousticModel(state_num=5, mix_level=2, dct_num=13)
        unit_hmms = {u: am.init_unit(u) for u in names}
        lens, begin, rows = eng.frontend(sigs, 16000, keep_f64=True, fetch=True)
        data = data_of(lens, begin, rows)
        am.flat_start_batch(data, unit_hmms, proportion=0.5, seed=3, engine=eng)
        first = am.init_segments_batch(labels, data, unit_hmms, seed=5, engine=eng)
        second = am.train_segments_batch(labels, data, unit_hmms, seed=5, engine=eng)
        third = am.train_segments_batch(labels, data, unit_hmms, seed=5, engine=eng)            # round after round
        model = [unit_hmms[u].profunction[1 + k].model_arrays() for u in names for k in range(3)]
        return lens, first, second, third, list(am.last_dropped), model

    calls = []
    upload = eng.load_frames
    eng.load_frames = lambda frames: (calls.append(len(frames)), upload(frames))[1]
    try:
        lens, first, second, third, dropped, model = chain(lambda lens, begin, rows: (lens, begin))
        assert calls == []                                                # the resident form uploads no frame
        lens2, first2, second2, third2, dropped2, model2 = chain(
            lambda lens, begin, rows: [rows[begin[u]:begin[u] + lens[u]] for u in range(len(lens))])
        assert len(calls) >= 3
    finally:
        del eng.load_frames
    print('frames per utterance %s, dropped %s, EM loop bodies %s' % (lens.tolist(), dropped, {u: second[u][0].tolist() for u in names}))
    assert lens[3] == 0 and (np.delete(lens, 3) > 0).all() and np.array_equal(lens, lens2)
    assert 3 in dropped and dropped == dropped2 and dropped == sorted(dropped)
    for got, want in ((first, first2), (second, second2), (third, third2)):
        assert sorted(got) == names
        for u in names:
            for x, y in zip(got[u], want[u]):
                assert np.array_equal(x, y, equal_nan=True)
    assert any((second[u][0] >= 1).any() for u in names)
    for x, y in zip(model, model2):
        for p, q in zip(x, y):
            assert np.array_equal(p, q)


def test_align_and_estep_helpers_take_resident_frames_too(eng):
    """_sentence_batch is shared: align_batch and estep_batch accept (lens, begin) as well, an utterance of length 0 skipped as an empty
    host array is, and give what the uploaded rows give."""
    from test_gpu_vad import speech_signal
    from poccala_amd import PCL_F64
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    rng = np.random.default_rng(32)
    sigs = [speech_signal(rng, 12000), np.zeros(8000, dtype=np.int16), speech_signal(rng, 9000)]
    labels = [['u0', 'u1'], ['u1'], ['u1', 'u0', 'u1']]
    am = AcousticModel(state_num=5, mix_level=2, dct_num=13)
    unit_hmms = {u: am.init_unit(u) for u in ('u0', 'u1')}
    lens, begin, rows = eng.frontend(sigs, 16000, keep_f64=True, fetch=True)
    assert lens[1] == 0
    am.flat_start_batch((lens, begin), unit_hmms, proportion=1.0, seed=1, engine=eng)
    calls = []
    upload = eng.load_frames
    eng.load_frames = lambda frames: (calls.append(len(frames)), upload(frames))[1]
    try:
        al = am.align_batch(labels, (lens, begin), unit_hmms, precision=PCL_F64, engine=eng)
        st, acc, lp = am.estep_batch(labels, (lens, begin), unit_hmms, precision=PCL_F64, engine=eng)
        assert calls == []
    finally:
        del eng.load_frames
    data = [rows[begin[u]:begin[u] + lens[u]] for u in range(len(lens))]
    al2 = am.align_batch(labels, data, unit_hmms, precision=PCL_F64, engine=eng)
    st2, acc2, lp2 = am.estep_batch(labels, data, unit_hmms, precision=PCL_F64, engine=eng)
    assert np.isnan(al[1][0]) and len(al[1][1]) == 0 and len(al[0][1]) == lens[0]
    for x, y in zip(al, al2):
        assert np.array_equal(x[0], y[0], equal_nan=True) and np.array_equal(x[1], y[1])
    assert np.isnan(lp[1]) and np.array_equal(lp, lp2, equal_nan=True)
    for k in st2:
        assert np.array_equal(st[k], st2[k]), k
    assert sorted(acc) == sorted(acc2)
    for u in acc2:
        assert np.array_equal(acc[u][0], acc2[u][0]) and np.array_equal(acc[u][1], acc2[u][1])


def test_errors_carry_a_message_and_leave_the_context_usable(eng):
    from poccala_amd import PCL_F64, PoccalaHipError
    INVALID, STATE = -1, -3
    labels = [[0, 1], [2], [3, 4, 5]]
    T = [20, 9, 31]
    begin, F = place(np.random.default_rng(1), T)
    good, model = aligned_batch(eng, 5, labels, T, begin, F, seed=1)

    def still_fine():
        seg, dropped, state = good.align_segments(want_map=True)
        assert state.shape == (F,) and seg.counts.sum() == (state >= 0).sum()
        seg.close()

    def fails(code, fn, *a):
        with pytest.raises(PoccalaHipError) as ei:
            fn(*a)
        print(ei.value)
        assert ei.value.code == code and len(str(ei.value)) > 20
        still_fine()

    still_fine()
    # a batch not built from labels
    plain = eng.batch(np.array([5, 5], dtype=np.int32), np.array([4, 6], dtype=np.int32), np.array([0, 4], dtype=np.int64))
    fails(STATE, plain.align_segments)
    plain.close()
    # no Viterbi yet
    fresh = eng.label_batch([np.array(l, dtype=np.int32) for l in labels], np.array(T, dtype=np.int32), begin)
    fails(STATE, fresh.align_segments)
    fresh.score(PCL_F64)
    fails(STATE, fresh.align_segments)
    fresh.close()
    # both outputs NULL
    rc = eng._lib.pcl_batch_align_segments(good._b, None, None, None)
    assert rc == INVALID and len(eng._lib.pcl_last_error(eng._ctx)) > 20
    flags = np.empty(len(T), dtype=np.int32)
    rc = eng._lib.pcl_batch_align_segments(good._b, None, flags.ctypes.data_as(C.c_void_p), None)
    assert rc == INVALID and len(eng._lib.pcl_last_error(eng._ctx)) > 20
    still_fine()
    # overlapping utterances: a frame has one owner
    over = eng.label_batch([np.array(l, dtype=np.int32) for l in labels], np.array(T, dtype=np.int32), np.array([0, 15, 40], dtype=np.int64))
    over.score(PCL_F64)
    over.viterbi()
    fails(INVALID, over.align_segments)
    over.close()
    # the model's J no longer n_units * (S - 2)
    mean, var, w = model
    eng.load_model(mean[:15], var[:15], w[:15])
    with pytest.raises(PoccalaHipError) as ei:
        good.align_segments()
    print(ei.value)
    assert ei.value.code == INVALID and len(str(ei.value)) > 20
    eng.load_model(mean, var, w)
    still_fine()
    # the batch no longer fits the current frame matrix
    eng.load_frames(np.zeros((F - 10, D)))                              # 5 rows lie behind the last utterance
    with pytest.raises(PoccalaHipError) as ei:
        good.align_segments()
    print(ei.value)
    assert ei.value.code == INVALID and len(str(ei.value)) > 20
    eng.load_frames(np.ones((F, D)))
    still_fine()
    good.close()
