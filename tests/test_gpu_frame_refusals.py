"""What the frame-level entry points refuse, and what a refused call leaves behind: Engine.cmvn_accumulate, cmvn_apply, cmvn_sliding,
lda_accumulate, splice_project, transform_frames and Batch.accumulate_fmllr share one check of a call's utterances (csrc/frame_spans.h:
spans_check, speakers_check) and one upload (DevSpans).

Defective inputs: two utterances that overlap by rows, an utterance that ends behind the last row, a negative length, a speaker at S and
at -2 (the calls that take speakers), and no frames loaded.  Batch.accumulate_fmllr takes its utterances from the batch, which
pcl_batch_create has validated and which cannot exist without frames: only the speaker defects reach it.

Every status below is a literal, taken from the library as it was before the checks were merged (INVALID = -1, STATE = -3).  After each
refusal the pool has handed out exactly the blocks it had before, and the resident frames (float64 copy and float32 rows) and the
resident statistics of CMVN, LDA and fMLLR keep their bits."""
import numpy as np
import pytest

import _adapt_twin as at

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -3
D, S = 13, 2
T = np.array([20, 30, 10], dtype=np.int32)
BEGIN = np.array([2, 22, 60], dtype=np.int64)                     # utterances 0 and 1 touch
SPK = np.array([0, 1, -1], dtype=np.int32)
F = 74


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


DEFECTS = {                                                       # name -> (T, begin)
    'overlap': (T, np.array([2, 21, 60], dtype=np.int64)),        # one row
    'past the last row': (T, np.array([2, 22, F - 9], dtype=np.int64)),
    'negative length': (np.array([20, -1, 10], dtype=np.int32), BEGIN),
}
BAD_SPEAKERS = {'speaker S': np.array([0, S, -1], dtype=np.int32), 'speaker -2': np.array([0, 1, -2], dtype=np.int32)}


def span_calls(eng, A, b, W, cls):
    """name -> (call(T, begin, speakers), takes speakers)"""
    return {
        'cmvn_accumulate': (lambda t, g, s: eng.cmvn_accumulate(t, g, s), True),
        'cmvn_apply': (lambda t, g, s: eng.cmvn_apply(t, g, s, n_speakers=S), True),
        'cmvn_sliding': (lambda t, g, s: eng.cmvn_sliding(t, g, 8, 1), False),
        'lda_accumulate': (lambda t, g, s: eng.lda_accumulate(t, g, cls), False),
        'splice_project': (lambda t, g, s: eng.splice_project(t, g, 1, 1, A, b), False),
        'transform_frames': (lambda t, g, s: eng.transform_frames(t, g, s, W), True),
    }


def test_refused_calls_leave_everything_as_it_was():
    from poccala_amd import PCL_F64, Engine, PoccalaHipError, synth
    rng = np.random.default_rng(11)
    frames = rng.standard_normal((F, D))
    A, b = rng.standard_normal((4, 3 * D)), rng.standard_normal(4)
    W = np.stack([np.concatenate([rng.standard_normal((D, 1)), np.eye(D) * 1.5], axis=1)] * S)
    cls = rng.integers(-1, 3, size=F).astype(np.int32)
    eng = Engine(0)
    try:
        state = {'stats': []}

        def refused(tag, call, code):
            held = (eng.frames_download(np.float64), eng.frames_download(np.float32)) if eng.F else None
            stats = [fn() for fn in state['stats']]
            blocks = Engine.pool_stats()['handed_out_blocks']
            with pytest.raises(PoccalaHipError) as ei:
                call()
            print('%s: status %d, want %d: %s' % (tag, ei.value.code, code, ei.value))
            assert ei.value.code == code and len(str(ei.value)) > 20
            assert Engine.pool_stats()['handed_out_blocks'] == blocks
            if held is not None:
                assert same_bits(eng.frames_download(np.float64), held[0]) and same_bits(eng.frames_download(np.float32), held[1])
            for fn, before in zip(state['stats'], stats):
                assert all(same_bits(x, y) for x, y in zip(fn(), before))

        # no frames loaded (the wrappers read the width they check A and W against from the engine)
        eng.FD = D
        for name, (call, _) in span_calls(eng, A, b, W, cls[:0]).items():
            refused(name + ', no frames', lambda: call(T, BEGIN, SPK), STATE)
        eng.FD = 0
        # frames, a model, an aligned batch and the resident statistics of all three rules
        model = at.make_case(D)[0]
        eng.load_model(*model)
        eng.load_units(np.stack([synth.random_left_right_transmat(np.random.default_rng(4), 3) for _ in range(at.J)]))
        eng.load_frames(frames)
        eng.cmvn_zero(S)
        eng.cmvn_accumulate(T, BEGIN, SPK)
        eng.lda_zero(3, 1, 1)
        eng.lda_accumulate(T, BEGIN, cls)
        batch = eng.label_batch([rng.integers(0, at.J, size=2).astype(np.int32) for _ in T], T, BEGIN)
        batch.score(PCL_F64)
        batch.forward_backward()
        eng.fmllr_zero(S)
        batch.accumulate_fmllr(SPK)
        state['stats'] = [eng.cmvn_stats, eng.lda_stats, eng.fmllr_stats]
        assert all(x.any() for fn in state['stats'] for x in fn())
        for name, spk in BAD_SPEAKERS.items():
            refused('accumulate_fmllr, ' + name, lambda: batch.accumulate_fmllr(spk), INVALID)
        batch.close()                                             # (splice_project is refused for another reason while a batch is open)
        for name, (call, takes_speakers) in span_calls(eng, A, b, W, cls).items():
            for what, (t, g) in DEFECTS.items():
                refused('%s, %s' % (name, what), lambda: call(t, g, SPK), INVALID)
            if takes_speakers:
                for what, spk in BAD_SPEAKERS.items():
                    refused('%s, %s' % (name, what), lambda: call(T, BEGIN, spk), INVALID)
        # ... and the same calls go through on the sound input, and give back what they took
        blocks = Engine.pool_stats()['handed_out_blocks']
        for name, (call, _) in span_calls(eng, A, b, W, cls).items():
            if name != 'splice_project':                          # (last: it changes the width the other calls' arguments were made for)
                call(T, BEGIN, SPK)
                assert Engine.pool_stats()['handed_out_blocks'] == blocks, name
        eng.splice_project(T, BEGIN, 1, 1, A, b)
        assert eng.frames_download(np.float64).shape == (F, 4)
    finally:
        eng.close()


def refusal(call):
    from poccala_amd import PoccalaHipError
    with pytest.raises(PoccalaHipError) as ei:
        call()
    print('status %d: %s' % (ei.value.code, ei.value))
    return ei.value.code, str(ei.value)


def test_a_refused_zero_keeps_the_statistics_in_place():
    """pcl_lda_zero and pcl_cmvn_zero build the fresh set beside the one in place and move it in last (pcl_tree_zero's rule): a zero
    refused at its bound -- before any allocation -- leaves the accumulated statistics resident, bit for bit."""
    from poccala_amd import Engine
    rng = np.random.default_rng(12)
    cls = rng.integers(-1, 3, size=F).astype(np.int32)
    eng = Engine(0)
    try:
        eng.load_frames(rng.standard_normal((F, D)))
        eng.lda_zero(3, 1, 1)
        eng.lda_accumulate(T, BEGIN, cls)
        eng.cmvn_zero(S)
        eng.cmvn_accumulate(T, BEGIN, SPK)
        lda, cmvn = eng.lda_stats(), eng.cmvn_stats()
        assert all(x.any() for x in lda + cmvn)
        assert refusal(lambda: eng.lda_zero(65536, 1, 1))[0] == INVALID          # the documented bound: 65535 classes
        assert all(same_bits(x, y) for x, y in zip(eng.lda_stats(), lda))
        assert refusal(lambda: eng.cmvn_zero(65536))[0] == INVALID               # ... and 65535 speakers
        assert all(same_bits(x, y) for x, y in zip(eng.cmvn_stats(), cmvn))
        eng.lda_accumulate(T, BEGIN, cls)                                        # ... and both sets go on from where they were
        eng.cmvn_accumulate(T, BEGIN, SPK)
        assert same_bits(eng.lda_stats()[0], 2 * lda[0]) and same_bits(eng.cmvn_stats()[0], 2 * cmvn[0])
    finally:
        eng.close()


def test_which_of_two_defects_is_reported():
    """The order of the entries' checks where a call has two defects (the table at LdaStats, csrc/pcl_internal.h), as the library had it
    before the checks were put behind one form: the labels of pcl_lda_accumulate are looked at before the statistics' width and before
    the utterances, those of pcl_tree_accumulate after the width and before the utterances, and pcl_cmvn_accumulate looks at the
    utterances before it asks for statistics."""
    from poccala_amd import Engine
    rng = np.random.default_rng(13)
    cls = rng.integers(-1, 3, size=F).astype(np.int32)
    bad = cls.copy()
    bad[5], bad[40] = 3, -2
    overlap = DEFECTS['overlap'][1]
    eng = Engine(0)
    try:
        eng.load_frames(rng.standard_normal((F, D)))
        code, text = refusal(lambda: eng.cmvn_accumulate(T, overlap, SPK))       # no statistics AND overlapping utterances
        assert code == INVALID and 'overlap' in text
        assert refusal(lambda: eng.cmvn_accumulate(T, BEGIN, SPK))[0] == STATE
        eng.lda_zero(3, 1, 1)
        eng.tree_zero(3)
        for name, call in (('frame_class[5] = 3', eng.lda_accumulate), ('frame_row[5] = 3', eng.tree_accumulate)):
            code, text = refusal(lambda: call(T, overlap, bad))                  # a label out of range (the first is named) AND overlapping utterances
            assert code == INVALID and name in text
            code, text = refusal(lambda: call(T, overlap, cls))
            assert code == INVALID and 'overlap' in text
        eng.load_frames(rng.standard_normal((F, D - 1)))                         # both sets were made for D dimensions
        code, text = refusal(lambda: eng.lda_accumulate(T, BEGIN, bad))          # another width AND a label out of range
        assert code == INVALID and 'frame_class[5] = 3' in text
        code, text = refusal(lambda: eng.lda_accumulate(T, BEGIN, cls))
        assert code == STATE and 'pcl_lda_zero again' in text
        code, text = refusal(lambda: eng.tree_accumulate(T, BEGIN, bad))
        assert code == STATE and 'pcl_tree_zero again' in text
    finally:
        eng.close()
