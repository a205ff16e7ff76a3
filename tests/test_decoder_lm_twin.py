"""The CPU twin of the decoder with a language model (tests/_decoder_lm_twin.py, rule D6; the reference's stub:
Decoder.py:17,146-156,200-204): with zero tables it IS oracle/decoder_oracle.py's decode, and a bigram that favours one homophone
makes it choose that homophone.  CPU only."""
import json
import os

import numpy as np
import pytest

import _decoder_lm_twin as tw
from oracle import decoder_oracle as do

HERE = os.path.dirname(os.path.abspath(__file__))
S, E = 5, 3


@pytest.fixture(scope='module')
def g13(tmp_path_factory):
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
    return units, lx.compile({u: i for i, u in enumerate(units)})


def random_case(n_units, T, seed):
    from poccala_amd import synth
    rng = np.random.default_rng(seed)
    trans = [synth.random_left_right_transmat(rng) for _ in range(n_units)]
    return trans, rng.normal(-20.0, 4.0, size=(n_units * E, T))


def same_as_oracle(tree, trans, b_all, **kw):
    t0, i0, t1, i1 = [], {}, [], {}
    fin0, hist0 = do.decode(tree, trans, b_all, trace=t0, info=i0, **kw)
    zero = tw.zero_lm(tree)
    fin1, hist1 = tw.decode(tree, trans, b_all, zero, trace=t1, info=i1, **kw)
    assert fin1 == fin0 and t1 == t0 and i1 == i0
    assert [(p, n) for p, n, _ in hist1] == [(p, n) for p, n in hist0]
    assert all(w == zero['node_word_ids'][zero['node_word_ptr'][n]] for _, n, w in hist1)     # ties: the first homophone
    return hist1


@pytest.mark.parametrize('beam,cap', [(0.85, None), (0.6, 300)])
def test_zero_tables_equal_the_oracle_on_the_g13_lexicon(g13, beam, cap):
    units, tree = g13
    trans, b_all = random_case(len(units), 70, 5)
    hist = same_as_oracle(tree, trans, b_all, beam=beam, candidate=6, max_tokens=cap)
    assert len(hist) > 3


def test_zero_tables_equal_the_oracle_on_the_synthetic_tree():
    from poccala_amd import synth
    tree, _ = synth.make_pronunciation_tree(3000, 183, seed=81)
    trans, b_all = random_case(183, 14, 6)
    hist = same_as_oracle(tree, trans, b_all, beam=0.85, candidate=4, max_tokens=2048)
    assert hist


def test_a_bigram_that_favours_one_homophone_makes_the_twin_choose_it():
    """Rule D6 alone: the mass after a given predecessor sits on one of a node's homophones -> that one is chosen; reversed -> the
    other.  The predecessor is the sentence start (the first history entry of the utterance)."""
    from poccala_amd import synth
    from poccala_amd.LanguageModel import Ngram
    tree, _ = synth.make_pronunciation_tree(300, 60, seed=91)
    trans, b_all = random_case(60, 40, 7)
    _, hist = tw.decode(tree, trans, b_all, tw.zero_lm(tree), candidate=3)
    twins = [(i, n) for i, (p, n, _) in enumerate(hist) if p == -1 and len(tree['words'][n]) >= 2]
    assert twins, 'no history entry after the sentence start at a node with homophones: another seed'
    entry, node = twins[0]
    first, second = tree['words'][node][:2]
    vocab = list(dict.fromkeys(w for ws in tree['words'] for w in ws))
    chosen = []
    for favoured in (first, second):
        g = Ngram(2).count([[favoured]] * 50 + [[w] for w in vocab], vocab)
        lm = g.compile(tree, lm_scale=0.01)                       # a small scale: the acoustic path stays, only the choice moves
        counters = {}
        _, h = tw.decode(tree, trans, b_all, lm, candidate=3, counters=counters)
        assert counters['hit'] > 0 and counters['resolved'] > 0
        at = [w for p, n, w in h if p == -1 and n == node]
        assert at, 'the path moved away from the node'
        chosen.append(lm['words'][at[0]])
    assert chosen == [first, second]
