"""CMVN on the device (csrc/frame_cmvn.hip: pcl_cmvn_zero, pcl_cmvn_accumulate, pcl_cmvn_stats_download, pcl_frames_cmvn,
pcl_frames_cmvn_sliding; Engine.cmvn_*, AcousticModel.cmvn_batch) against the NumPy twin of the rule (tests/_cmvn_twin.py, whose own
invariants tests/test_cmvn_twin.py holds).

Inputs (_cmvn_twin.make_case, the shape of _fmllr_twin.make_case): utterances of 63, 64, 1, 130, 30, 65, 20 and 0 frames with unowned rows
before, between and behind them, speakers 0 and 1 (193 and 129 frames; column 0 of speaker 1 is constant, so its variance is floored),
speaker 2 below min_count, speaker 3 without an utterance, one utterance of speaker -1.  Every case runs on a context that holds only
float32 rows ('f32') and on one with the float64 copy ('f64').

Bounds.  Statistics: n exact; every s_d and q_d within 1e-10 x the twin's sum of the absolute terms (the project's float64 restatement
contract, as the fMLLR statistics use it); two runs the same bits.  Apply and sliding window, fed the device's own statistics: the twin's y
bit for bit -- float64 against the float64 copy, float32(y) against the float32 rows -- and everything a call must not touch keeps its
bits; the padding columns are checked through ln b against load_frames of the twin's array, as tests/test_gpu_fmllr.py does.  Every figure
is printed before it is asserted."""
import numpy as np
import pytest

import _cmvn_twin as tw

pytestmark = pytest.mark.gpu
RTOL = 1e-10
INVALID, STATE = -1, -3
ALL_D = [1, 2, 13, 39, 40, 47, 64]          # padded strides (1, 2 -> 13; 40 -> 47), one column, the frame matrix's widest
KINDS = ['f32', 'f64']


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


_CASES = {}


def case(D):
    if D not in _CASES:
        _CASES[D] = tw.make_case(D)
    return _CASES[D]


def host_frames(frames, kind):
    return np.asarray(frames, dtype=np.float32 if kind == 'f32' else np.float64)


def held(eng, kind):
    """what the context holds: (float64 copy or None, float32 rows)"""
    return (eng.frames_download(np.float64) if kind == 'f64' else None), eng.frames_download(np.float32)


def hold_frames(tag, eng, kind, y64, rows32):
    g64, g32 = held(eng, kind)
    if kind == 'f64':
        diff = int((g64.view(np.uint64) != y64.view(np.uint64)).sum())
        print('%s: float64 copy, %d of %d elements differ from the twin' % (tag, diff, g64.size))
        assert same_bits(g64, y64)
    diff = int((g32.view(np.uint32) != rows32.view(np.uint32)).sum())
    print('%s: float32 rows, %d of %d elements differ from the twin' % (tag, diff, g32.size))
    assert same_bits(g32, rows32)


def hold_stats(tag, got, t):
    n, s, q = got
    print('%s: n %s (twin %s)' % (tag, n.tolist(), t['n'].tolist()))
    assert n.dtype == np.int64 and np.array_equal(n, t['n'])
    for name, g in (('s', s), ('q', q)):
        err, bound = np.abs(g - t[name]), RTOL * t[name + 'abs']
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


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('D', ALL_D)
def test_statistics_are_the_twins(eng, D, kind):
    tag = 'cmvn stats D=%d %s' % (D, kind)
    frames, T, begin, spk = case(D)
    fr = host_frames(frames, kind)
    eng.load_frames(fr)
    eng.cmvn_zero(tw.S_SPK)
    assert all(not x.any() for x in eng.cmvn_stats())
    eng.cmvn_accumulate(T, begin, spk)
    got = eng.cmvn_stats()
    t = tw.accumulate(tw.zero(tw.S_SPK, D), fr, T, begin, spk)
    hold_stats(tag, got, t)
    eng.cmvn_zero(tw.S_SPK)
    eng.cmvn_accumulate(T, begin, spk)
    assert all(same_bits(x, y) for x, y in zip(got, eng.cmvn_stats()))                             # two runs, the same bytes
    # two calls over a split of the utterances against the twin's two calls
    eng.cmvn_zero(tw.S_SPK)
    eng.cmvn_accumulate(T[:3], begin[:3], spk[:3])
    eng.cmvn_accumulate(T[3:], begin[3:], spk[3:])
    t2 = tw.accumulate(tw.accumulate(tw.zero(tw.S_SPK, D), fr, T[:3], begin[:3], spk[:3]), fr, T[3:], begin[3:], spk[3:])
    hold_stats(tag + ' two calls', eng.cmvn_stats(), t2)
    hold_frames(tag, eng, kind, tw.widen(fr), fr.astype(np.float32))                               # the statistics read, nothing else


@pytest.mark.parametrize('kind', KINDS)
def test_statistics_at_the_chunk_edges(eng, kind):
    D = 13
    T, begin, F = tw.layout([1023, 1024, 1025, 2049], [2, 0, 1, 3])
    rng = np.random.default_rng(9)
    fr = host_frames(rng.standard_normal((F, D)) * 2 + 1, kind)
    spk = np.array([0, 1, 2, 3], dtype=np.int32)
    eng.load_frames(fr)
    eng.cmvn_zero(4)
    eng.cmvn_accumulate(T, begin, spk)
    got = eng.cmvn_stats()
    hold_stats('cmvn chunk edges %s' % kind, got, tw.accumulate(tw.zero(4, D), fr, T, begin, spk))
    # all four as ONE speaker: several utterances of several chunks each
    one = np.zeros(4, dtype=np.int32)
    eng.cmvn_zero(1)
    eng.cmvn_accumulate(T, begin, one)
    hold_stats('cmvn chunk edges one speaker %s' % kind, eng.cmvn_stats(), tw.accumulate(tw.zero(1, D), fr, T, begin, one))


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize('norm_vars', [True, False])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('D', ALL_D)
def test_apply_is_the_twin_bit_for_bit(eng, D, kind, norm_vars):
    from poccala_amd import PCL_F32, PCL_F64, synth
    tag = 'cmvn apply D=%d %s norm_vars=%s' % (D, kind, norm_vars)
    frames, T, begin, spk = case(D)
    fr = host_frames(frames, kind)
    eng.load_frames(fr)
    eng.cmvn_zero(tw.S_SPK)
    eng.cmvn_accumulate(T, begin, spk)
    n, s, q = eng.cmvn_stats()
    status = eng.cmvn_apply(T, begin, spk, norm_vars, 1e-20, tw.MIN_COUNT)
    y64, st = tw.apply(fr, T, begin, spk, n, s, q, norm_vars, 1e-20, tw.MIN_COUNT)
    print('%s: statuses %s (twin %s)' % (tag, status.tolist(), st.tolist()))
    assert status.tolist() == st.tolist() == [tw.OK, tw.OK, tw.LOW_COUNT, tw.LOW_COUNT]
    on = tw.touched(len(fr), T, begin, [sp >= 0 and st[sp] == tw.OK for sp in spk])
    rows32 = tw.as_rows32(fr.astype(np.float32), y64, on)
    hold_frames(tag, eng, kind, y64, rows32)
    assert same_bits(y64[~on], tw.widen(fr)[~on]) and on.sum() == 193 + 129                       # refused, -1 and unowned rows: the old bits
    if norm_vars:
        rows1 = np.concatenate([np.arange(begin[u], begin[u] + T[u]) for u in np.flatnonzero(spk == 1)])
        assert not eng.frames_download(np.float32)[rows1, 0].any()                               # the constant column: floored, y = 0
    # the padding columns, through ln b: load_frames zeroes them
    mean, var, w, _ = synth.make_model(1, 2, D, seed=3)
    eng.load_model(mean, var, w)
    precisions = (PCL_F32, PCL_F64) if kind == 'f64' else (PCL_F32,)
    got = {P: lnb(eng, P) for P in precisions}
    eng.load_frames(y64 if kind == 'f64' else rows32)
    for P in precisions:
        assert same_bits(got[P], lnb(eng, P))


@pytest.mark.parametrize('kind', KINDS)
def test_one_inf_refuses_its_speaker_alone(eng, kind):
    D = 13
    frames, T, begin, spk = case(D)
    fr = host_frames(frames, kind).copy()
    fr[begin[3] + 7, 5] = np.inf                                                                   # utterance 3 is speaker 0's
    eng.load_frames(fr)
    eng.cmvn_zero(tw.S_SPK)
    eng.cmvn_accumulate(T, begin, spk)
    n, s, q = eng.cmvn_stats()
    status = eng.cmvn_apply(T, begin, spk, True, 1e-20, tw.MIN_COUNT)
    y64, st = tw.apply(fr, T, begin, spk, n, s, q, True, 1e-20, tw.MIN_COUNT)
    print('cmvn inf %s: statuses %s' % (kind, status.tolist()))
    assert status.tolist() == st.tolist() == [tw.NOT_FINITE, tw.OK, tw.LOW_COUNT, tw.LOW_COUNT]
    on = tw.touched(len(fr), T, begin, spk == 1)
    hold_frames('cmvn inf %s' % kind, eng, kind, y64, tw.as_rows32(fr.astype(np.float32), y64, on))
    assert same_bits(y64[~on], tw.widen(fr)[~on])


def test_per_utterance_is_arange(eng):
    D = 13
    frames, T, begin, _ = case(D)
    eng.load_frames(frames)
    eng.cmvn_zero(len(T))
    eng.cmvn_accumulate(T, begin)
    n, s, q = eng.cmvn_stats()
    assert n.tolist() == T.tolist()
    status = eng.cmvn_apply(T, begin, None, True, 1e-20, 2)
    y64, st = tw.apply(frames, T, begin, np.arange(len(T)), n, s, q, True, 1e-20, 2)
    assert status.tolist() == st.tolist() and status.tolist() == [0, 0, 1, 0, 0, 0, 0, 1]        # T = 1 and T = 0 are below min_count = 2
    hold_frames('cmvn per utterance', eng, 'f64', y64, y64.astype(np.float32))


# ------------------------------------------------------------------ sliding window
SLIDING_T = [63, 64, 1, 130, 30, 65, 20, 0, 6, 7, 8, 9]                                            # ... and window - 1, window, window + 1 for 7 and 8
SLIDING_GAPS = [5, 0, 3, 1, 0, 7, 2, 1, 0, 2, 0, 1]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('D', [2, 13, 40, 64])
def test_sliding_is_the_twin_bit_for_bit(eng, monkeypatch, D, kind):
    frames, T, begin, _ = tw.make_case(D, seed=1, T=SLIDING_T, gaps=SLIDING_GAPS)
    fr = host_frames(frames, kind)
    on = tw.touched(len(fr), T, begin)
    for window in (7, 8):
        for center in (True, False):
            for min_window in (1, window):
                for norm_vars in (True, False):
                    tag = 'cmvn sliding D=%d %s window=%d center=%s min_window=%d norm_vars=%s' % (D, kind, window, center, min_window, norm_vars)
                    eng.load_frames(fr)
                    eng.cmvn_sliding(T, begin, window, min_window, center, norm_vars, 1e-20)
                    y64 = tw.sliding(fr, T, begin, window, min_window, center, norm_vars, 1e-20)
                    hold_frames(tag, eng, kind, y64, tw.as_rows32(fr.astype(np.float32), y64, on))
    # the result does not depend on how the utterances are grouped for the prefix block
    monkeypatch.setenv('PCL_CMVN_GROUP_ROWS', '100')
    eng.load_frames(fr)
    eng.cmvn_sliding(T, begin, 8, 1, True, True, 1e-20)
    y64 = tw.sliding(fr, T, begin, 8, 1, True, True, 1e-20)
    hold_frames('cmvn sliding D=%d %s grouped' % (D, kind), eng, kind, y64, tw.as_rows32(fr.astype(np.float32), y64, on))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('center', [True, False])
def test_sliding_over_many_blocks_and_twice(eng, kind, center):
    """one utterance of 64 x 256 + 300 rows under a window of 600: many blocks, an interior where the window is full; then a second call on
    the normalised frames -- were a row read after a neighbour had been written, the result would not be the twin applied twice"""
    D = 13
    T, begin, F = tw.layout([64 * 256 + 300, 700], [3, 2])
    rng = np.random.default_rng(12)
    fr = host_frames(rng.standard_normal((F, D)) * rng.uniform(0.5, 3.0, D) + np.sin(np.arange(F) / 500.0)[:, None] * 4, kind)
    on = tw.touched(F, T, begin)
    eng.load_frames(fr)
    eng.cmvn_sliding(T, begin, 600, 100, center, True, 1e-20)
    y1 = tw.sliding(fr, T, begin, 600, 100, center, True, 1e-20)
    r1 = tw.as_rows32(fr.astype(np.float32), y1, on)
    hold_frames('cmvn sliding long %s center=%s' % (kind, center), eng, kind, y1, r1)
    eng.cmvn_sliding(T, begin, 600, 100, center, True, 1e-20)
    y2 = tw.sliding(y1 if kind == 'f64' else r1, T, begin, 600, 100, center, True, 1e-20)
    hold_frames('cmvn sliding long twice %s center=%s' % (kind, center), eng, kind, y2, tw.as_rows32(r1, y2, on))


# ------------------------------------------------------------------ what is refused, and what the calls give back
@pytest.mark.parametrize('kind', KINDS)
def test_refusals_and_the_pool(kind):
    from poccala_amd import Engine, PoccalaHipError
    D = 13
    frames, T, begin, spk = case(D)
    fr = host_frames(frames, kind)
    eng = Engine(0)
    try:
        def refused(call, code, stats=True):
            before = held(eng, kind) if eng.F else None
            st_before = eng.cmvn_stats() if stats else None
            blocks = Engine.pool_stats()['handed_out_blocks']
            with pytest.raises(PoccalaHipError) as ei:
                call()
            print(ei.value)
            assert ei.value.code == code and len(str(ei.value)) > 20
            assert Engine.pool_stats()['handed_out_blocks'] == blocks
            if before is not None:
                after = held(eng, kind)
                assert same_bits(after[1], before[1]) and (kind == 'f32' or same_bits(after[0], before[0]))
            if stats:
                assert all(same_bits(x, y) for x, y in zip(st_before, eng.cmvn_stats()))

        refused(lambda: eng.cmvn_zero(4), STATE, stats=False)                                      # no frames
        refused(lambda: eng.cmvn_sliding(T, begin, 8, 1), STATE, stats=False)
        eng.load_frames(fr)
        refused(lambda: eng.cmvn_accumulate(T, begin, spk), STATE, stats=False)                    # no statistics
        refused(lambda: eng.cmvn_apply(T, begin, spk, n_speakers=4), STATE, stats=False)
        refused(lambda: eng.cmvn_stats(), STATE, stats=False)
        refused(lambda: eng.cmvn_zero(0), INVALID, stats=False)
        refused(lambda: eng.cmvn_zero(65536), INVALID, stats=False)
        start = Engine.pool_stats()['handed_out_blocks']
        eng.cmvn_zero(tw.S_SPK)
        assert Engine.pool_stats()['handed_out_blocks'] == start + 2                               # n and [s | q] are resident
        eng.cmvn_accumulate(T, begin, spk)
        assert Engine.pool_stats()['handed_out_blocks'] == start + 2                               # every temporary went back
        overlap = begin.copy()
        overlap[1] = begin[0] + 10                                                                 # utterance 1 now starts inside utterance 0
        outside = begin.copy()
        outside[6] = len(fr) - 5
        bad_spk, low_spk = spk.copy(), spk.copy()
        bad_spk[0], low_spk[0] = tw.S_SPK, -2
        for b_, s_ in ((overlap, spk), (outside, spk), (begin, bad_spk), (begin, low_spk)):
            refused(lambda: eng.cmvn_accumulate(T, b_, s_), INVALID)
            refused(lambda: eng.cmvn_apply(T, b_, s_), INVALID)
        refused(lambda: eng.cmvn_accumulate(-T, begin, spk), INVALID)
        refused(lambda: eng.cmvn_apply(T, begin, spk, n_speakers=3), INVALID)                      # not the statistics' S
        for vf in (0.0, -1.0, np.nan, np.inf):
            refused(lambda: eng.cmvn_apply(T, begin, spk, True, vf), INVALID)
            refused(lambda: eng.cmvn_sliding(T, begin, 8, 1, True, True, vf), INVALID)
        refused(lambda: eng.cmvn_apply(T, begin, spk, True, 1e-20, 0), INVALID)                    # min_count < 1
        for w, mw in ((0, 1), (8, 0), (8, 9), ((1 << 20) + 1, 1)):
            refused(lambda: eng.cmvn_sliding(T, begin, w, mw), INVALID)
        refused(lambda: eng.cmvn_sliding(T, overlap, 8, 1), INVALID)
        refused(lambda: eng.cmvn_sliding(T, outside, 8, 1), INVALID)
        # the calls give back what they took
        eng.cmvn_apply(T, begin, spk, False, 0.0, tw.MIN_COUNT)                                    # the floor is not read without norm_vars
        assert Engine.pool_stats()['handed_out_blocks'] == start + 2
        eng.cmvn_sliding(T, begin, 8, 1, True, True)
        assert Engine.pool_stats()['handed_out_blocks'] == start + 2
        # a speaker may span frame matrices of the same D; another D drops the statistics until the next zero
        n0 = eng.cmvn_stats()[0]
        eng.load_frames(fr)
        eng.cmvn_accumulate(T, begin, spk)
        assert np.array_equal(eng.cmvn_stats()[0], 2 * n0)
        eng.load_frames(host_frames(np.ones((len(fr), 26)), kind))
        refused(lambda: eng.cmvn_accumulate(T, begin, spk), STATE, stats=False)
        refused(lambda: eng.cmvn_apply(T, begin, spk, n_speakers=tw.S_SPK), STATE, stats=False)
        eng.cmvn_zero(2)
        assert Engine.pool_stats()['handed_out_blocks'] == start + 2 and eng.cmvn_stats()[1].shape == (2, 26)
    finally:
        eng.close()


# ------------------------------------------------------------------ the chain: front-end -> CMVN -> LDA without a frame upload
def test_frontend_cmvn_lda_chain_uploads_no_frame(eng):
    import _lda_twin as lt
    from test_gpu_vad import speech_signal
    from poccala_amd import PCL_F64
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    rng = np.random.default_rng(32)
    sigs = [speech_signal(rng, 16000), np.zeros(8000, dtype=np.int16), speech_signal(rng, 12345), speech_signal(rng, 20000)]
    labels = [['u0', 'u1'], ['u1'], ['u1', 'u0', 'u1'], ['u0', 'u1', 'u0']]
    utt_speaker = np.array([0, 1, 0, 1], dtype=np.int32)

    def fresh():
        am = AcousticModel(state_num=5, mix_level=2, dct_num=13)
        return am, {u: am.init_unit(u) for u in ('u0', 'u1')}

    def rest(am, unit_hmms, lens, begin):
        am.flat_start_batch((lens, begin), unit_hmms, proportion=1.0, seed=1, engine=eng)
        am.init_segments_batch(labels, (lens, begin), unit_hmms, seed=5, engine=eng)               # a model whose states differ: the alignment keeps utterances
        out = am.lda_batch(labels, (lens, begin), unit_hmms, 10, left=1, right=1, precision=PCL_F64, engine=eng)
        return out, eng.frames_download()

    calls = []
    upload, raw = eng.load_frames, eng._lib.pcl_frames_upload
    eng.load_frames = lambda frames: (calls.append(len(frames)), upload(frames))[1]
    try:
        am, unit_hmms = fresh()
        lens, begin, rows = eng.frontend(sigs, 16000, keep_f64=True, fetch=True)
        assert lens[1] == 0 and rows.shape[1] == 39
        cm = am.cmvn_batch(lens, begin, utt_speaker, engine=eng)
        print('cmvn_batch: statuses %s, frames per speaker %s' % (cm['status'].tolist(), cm['n'].tolist()))
        assert cm['status'].tolist() == [0, 0] and cm['n'].sum() == lens.sum()
        normalised = eng.frames_download()
        out, y = rest(am, unit_hmms, lens, begin)
        assert calls == []                                                                         # the resident chain uploads no frame
    finally:
        del eng.load_frames
    # the twin's normalised frames, from the twin's own sums of the front-end's rows
    st = tw.accumulate(tw.zero(2, 39), rows, lens, begin, utt_speaker)
    want_norm, _ = tw.apply(rows, lens, begin, utt_speaker, st['n'], st['s'], st['q'], True, 1e-20, 1)
    err = np.abs(normalised - want_norm)
    print('chain: normalised frames, max |device - twin| = %.3e' % err.max())
    # the same chain with the twin's normalised frames uploaded
    am2, unit_hmms2 = fresh()
    eng.load_frames(want_norm)
    out2, y2 = rest(am2, unit_hmms2, lens, begin)
    want = lt.project(want_norm, lens, begin, 1, 1, out2['A'], out2['b'])
    worst = (np.abs(y2 - want[0]) / np.maximum(RTOL * want[2], 1e-300)).max()
    print('chain: uploaded twin frames, projection worst error / bound = %.3e' % worst)
    assert (np.abs(y2 - want[0]) <= RTOL * want[2]).all()
    want = lt.project(want_norm, lens, begin, 1, 1, out['A'], out['b'])
    worst = (np.abs(y - want[0]) / np.maximum(RTOL * want[2], 1e-300)).max()
    print('chain: resident frames, projection worst error / bound = %.3e; A differs from the uploaded chain\'s by %.3e' %
          (worst, np.abs(out['A'] - out2['A']).max()))
    assert (np.abs(y - want[0]) <= RTOL * want[2]).all()
    print('chain: frames per utterance %s, dropped %s, rows per class %s' % (lens.tolist(), out['dropped'], out['n'].tolist()))
    assert out['dropped'] == out2['dropped'] and np.array_equal(out['n'], out2['n']) and out['n'].sum() > 0
    assert raw is eng._lib.pcl_frames_upload
