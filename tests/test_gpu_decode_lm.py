"""The decoder with a bigram language model at word ends (rule D6; the reference's stub: Decoder.py:17,146-156,200-204) on the GPU
against its CPU twin (tests/_decoder_lm_twin.py, built on oracle/decoder_oracle.py): bit-exact scores, nodes, histories, chosen
words and token counts from identical emissions, on both kernels; zero tables = the plain decoder; the upload's rejections."""
import json
import os

import numpy as np
import pytest

import _decoder_lm_twin as tw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
S, E = 5, 3


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def lex(tmp_path_factory):
    from poccala_amd.Lexicon import PinYin, PronunciationLexicon
    g = json.load(open(os.path.join(HERE, 'golden', 'G13_lexicon.json')))
    path = str(tmp_path_factory.mktemp('lex') / 'Mandarin.dat')
    with open(path, 'w') as f:
        for k, v in g['table'].items():
            f.write('%s\t%s\n' % (k, v))
    py = PinYin(path)
    lx = PronunciationLexicon()
    lx.generate_lexicon(words=g['words'], pinyin=py)
    units = sorted({u for w in g['words'] for r in py.word2pinyin(w) for x in r for u in x.split(',')})
    return lx, units, lx.compile({u: i for i, u in enumerate(units)})


def left_right(n_units, seed):
    rng = np.random.default_rng(seed)
    trans = []
    for _ in range(n_units):
        a = np.zeros((S, S))
        a[0, 1] = 1.0
        for r in range(1, S - 1):
            x = rng.uniform(0.05, 0.95)
            a[r, r], a[r, r + 1] = x, 1.0 - x
        trans.append(a)
    return np.stack(trans)


def dense(n_units, seed):                                          # test_gpu_decode.py's model_for(dense=True)
    rng = np.random.default_rng(seed + 1)
    trans = []
    for _ in range(n_units):
        a = np.zeros((S, S))
        a[0, 1:3] = [0.7, 0.3]
        a[1:-1, 1:] = rng.dirichlet(np.ones(S - 1), size=E)
        trans.append(a)
    return np.stack(trans)


def scored_batch(eng, tree, n_units, trans, M, U, T, seed, ragged=True, same_gmm=False):
    from poccala_amd import PCL_F64, synth
    mean, var, w, _ = synth.make_model(n_units, M, 13, seed=seed)
    if same_gmm:
        mean[:], var[:], w[:] = mean[0], var[0], w[0]
    frames, lens, begin = synth.make_frames(U, T, 13, seed=seed + 2, ragged=ragged)
    eng.load_model(mean, var, w)
    eng.load_units(trans)
    eng.load_lexicon(tree)
    eng.load_frames(frames)
    b = eng.all_state_batch(lens, begin)
    b.score(PCL_F64)
    return b, b.get('B')                                           # the twin decodes from the bits the device decodes from


def assert_is_the_twin(g, tree, trans, b_all, lm, counters, **kw):
    trace, info = [], {}
    fin, hist = tw.decode(tree, list(trans), b_all, lm, trace=trace, info=info, counters=counters, **kw)
    assert np.array_equal(g['n_tokens'], np.array(trace)), (g['n_tokens'][:12], trace[:12])
    assert g['history'] == [(int(p), int(n), int(w)) for p, n, w in hist]
    assert [(n, h) for n, _, h in g['final']] == [(n, h) for n, _, h in fin]
    assert [s for _, s, _ in g['final']] == [float(s) for _, s, _ in fin]                  # bit-exact float64
    assert g['overflow'] == bool(info.get('overflow'))
    return trace


def test_zero_tables_give_the_plain_decoder_bit_for_bit(eng, lex, monkeypatch):
    lx, units, tree = lex
    b, B = scored_batch(eng, tree, len(units), left_right(len(units), 72), 3, 3, 80, 71)
    zero = tw.zero_lm(tree)
    eng.load_language_model(zero)
    first = {n: int(zero['node_word_ids'][zero['node_word_ptr'][n]]) for n in range(len(tree['words'])) if tree['words'][n]}
    for general in (False, True):
        if general:
            monkeypatch.setenv('PCL_DEC_GENERAL', '1')
        for beam, cap in ((0.85, 4096), (0.6, 300)):
            plain = b.decode(beam=beam, candidate=6, max_tokens=cap)
            with_lm = b.decode(beam=beam, candidate=6, max_tokens=cap, lm=True)
            for p, q in zip(plain, with_lm):
                assert q['final'] == p['final'] and q['overflow'] == p['overflow']
                assert np.array_equal(q['n_tokens'], p['n_tokens'])
                assert [(a, n) for a, n, _ in q['history']] == p['history'] and len(p['history']) > 3
                assert all(w == first[n] for _, n, w in q['history'])                      # ties: the first homophone
    monkeypatch.delenv('PCL_DEC_GENERAL')
    b.close()


@pytest.mark.parametrize('kernel', ['left_to_right', 'general', 'dense'])
@pytest.mark.parametrize('lm_scale,word_penalty', [(1.0, 0.0), (8.0, -5.0)])
def test_random_language_model_matches_the_twin_bit_for_bit(eng, monkeypatch, kernel, lm_scale, word_penalty):
    """A tree with homophones (G13 has one node with two words: too few to meet) and random bigram counts over a third of the
    vocabulary per word; seeds chosen on the CPU so that the twin alone meets the three conditions below for every set."""
    from poccala_amd import synth
    n_units = 60
    tree, _ = synth.make_pronunciation_tree(300, n_units, seed=91)
    trans = dense(n_units, 70) if kernel == 'dense' else left_right(n_units, 71)
    b, B = scored_batch(eng, tree, n_units, trans, 3, 3, 80, 70)
    lm = tw.random_lm(tree, 73, lm_scale, word_penalty)
    eng.load_language_model(lm)
    if kernel == 'general':
        monkeypatch.setenv('PCL_DEC_GENERAL', '1')
    got = [b.decode(beam=beam, candidate=6, max_tokens=cap, lm=True) for beam, cap in ((0.85, 4096), (0.6, 300))]
    if kernel == 'general':
        monkeypatch.delenv('PCL_DEC_GENERAL')
    b.close()
    for res, (beam, cap) in zip(got, ((0.85, 4096), (0.6, 300))):
        counters = {}
        for u in range(3):
            assert_is_the_twin(res[u], tree, trans, B[u][1:-1], lm, counters, beam=beam, candidate=6, max_tokens=cap)
        print('lm decode %s scale %g penalty %g beam %g cap %d: %r' % (kernel, lm_scale, word_penalty, beam, cap, counters))
        # the set visited its subject: an explicit bigram, a backoff, a history entry at a node with homophones
        assert counters['hit'] >= 1 and counters['backoff'] >= 1 and counters['resolved'] >= 1, counters


def test_many_word_end_donors_in_one_frame_with_a_language_model(eng):
    """test_decode_many_tokens_finish_in_one_frame's shape: thousands of donors in a frame, more per wavefront than the lane-per-token
    kernel keeps in LDS -- the language-model term is added to the donors it reads back from HBM as to those in LDS."""
    from poccala_amd import synth
    n_units = 183
    tree, _ = synth.make_pronunciation_tree(3000, n_units, seed=81)
    a = np.zeros((S, S))
    a[0, 1] = 1.0
    for r in range(1, S - 1):
        a[r, r], a[r, r + 1] = 0.1, 0.9
    trans = np.stack([a] * n_units)
    b, B = scored_batch(eng, tree, n_units, trans, 2, 2, 22, 82, ragged=False, same_gmm=True)
    lm = tw.random_lm(tree, 84, 1.0, 0.0, successors=20)
    eng.load_language_model(lm)
    got = b.decode(beam=1.0, candidate=4, max_tokens=8192, lm=True)
    b.close()
    swing, counters = 0, {}
    for u in range(2):
        trace = assert_is_the_twin(got[u], tree, trans, B[u][1:-1], lm, counters, beam=1.0, candidate=4, max_tokens=8192)
        swing = max(swing, int(np.abs(np.diff(np.array(trace))).max()))
    assert swing > 2000                                           # (the frames this test is about did occur)
    assert counters['hit'] >= 1 and counters['backoff'] >= 1


def test_language_model_errors_and_the_dropin(eng, lex):
    from poccala_amd import Decoder, PCL_F32, PoccalaHipError, synth
    from poccala_amd.LanguageModel import Ngram
    lx, units, tree = lex
    mean, var, w, trans = synth.make_model(len(units), 2, 13, seed=31)
    tree2 = Decoder.load_inventory(eng, units, mean, var, w, trans, lx)
    frames, lens, begin = synth.make_frames(2, 50, 13, seed=32)
    eng.load_frames(frames)
    b = eng.all_state_batch(lens, begin)
    b.score(PCL_F32)
    with pytest.raises(PoccalaHipError, match='no language model'):
        b.decode(lm=True)                                          # nothing uploaded
    good = tw.random_lm(tree, 33)
    eng.load_language_model(good)
    assert len(b.decode(lm=True)) == 2
    eng.load_lexicon(tree)                                         # a lexicon re-upload drops the language model
    with pytest.raises(PoccalaHipError, match='no language model'):
        b.decode(lm=True)
    assert len(b.decode()) == 2
    b.close()

    def broken(**kw):
        bad = dict(good)
        for k, f in kw.items():
            bad[k] = f(good[k].copy())
        return bad

    def put(i, x):
        def f(a):
            a[i] = x
            return a
        return f
    wordless = int(np.flatnonzero(np.asarray(tree['node_word']) == 0)[0])
    worded = int(np.flatnonzero(np.asarray(tree['node_word']) != 0)[0])
    row = int(np.flatnonzero(np.diff(good['row_ptr']) >= 2)[0])
    k0 = int(good['row_ptr'][row])

    def moved(node, by):                                           # one word more (or fewer) at `node`: the pointers behind it shift
        def f(p):
            p[node + 1:] += by
            return p
        return f
    cases = [('not finite', broken(uni=put(3, np.inf))), ('not finite', broken(bow=put(2, np.nan))), ('not finite', broken(val=put(k0, -np.inf))),
             ('strictly ascending', broken(col=put(k0 + 1, good['col'][k0]))), ('outside', broken(col=put(k0, good['W']))),
             ('outside', broken(node_word_ids=put(0, 0))), ('outside', broken(node_word_ids=put(0, good['W']))),
             ('has no word', dict(broken(node_word_ptr=moved(worded, -len(tree['words'][worded]))), node_word_ids=good['node_word_ids'][len(tree['words'][worded]):])),
             ('no word ends there', dict(broken(node_word_ptr=moved(wordless, 1)), node_word_ids=np.insert(good['node_word_ids'], good['node_word_ptr'][wordless], 1)))]
    for text, bad in cases:
        with pytest.raises(PoccalaHipError, match=text):
            eng.load_language_model(bad)
    # the drop-in: strings with a language model, today's lists of homophones without
    g = Ngram(2).count([[ws[0] for ws in tree['words'] if ws][:40]] * 3, [w for ws in tree['words'] for w in ws])
    chunk = [frames[:50], frames[50:]]
    plain = Decoder.decode_batch(chunk, tree2, engine=eng, precision=PCL_F32)
    with_lm = Decoder.decode_batch(chunk, tree2, engine=eng, precision=PCL_F32, lm=g, lm_scale=4.0, word_penalty=-1.0)
    again = Decoder.decode_batch(chunk, tree2, engine=eng, precision=PCL_F32)
    assert len(with_lm) == 2
    for (words, score, detail), (pw, ps, pd) in zip(with_lm, plain):
        assert np.isfinite(score) and all(isinstance(x, str) for x in words)
        assert all(len(h) == 3 for h in detail['history'])
        assert all(isinstance(x, list) for x in pw) and all(len(h) == 2 for h in pd['history'])
    assert [(x[0], x[1], x[2]['final'], x[2]['history']) for x in again] == [(x[0], x[1], x[2]['final'], x[2]['history']) for x in plain]
    streamed = list(Decoder.decode_stream(iter([chunk]), tree2, engine=eng, precision=PCL_F32, lm=g, lm_scale=4.0, word_penalty=-1.0))
    assert [(x[0], x[1]) for x in streamed[0]] == [(x[0], x[1]) for x in with_lm]
