"""LanguageModel.Ngram, the module the reference's decoder imports and never shipped (Decoder.py:17,146-156,200-204): counts,
Witten-Bell probabilities, the save / load round trip and the flat form for the device.  CPU only."""
import numpy as np
import pytest

from poccala_amd.LanguageModel import Ngram
from poccala_amd.LanguageModel.Ngram import best_word, lm_score

VOCAB = ['a', 'b', 'c', 'd']
CORPUS = [['a', 'b', 'a', 'b', 'c'], ['b', 'x', 'c', 'a'], ['a', 'c'], []]


def counted(n=2):
    return Ngram(n).count(CORPUS, VOCAB)


def test_counts_on_a_hand_written_corpus():
    g = counted()
    assert g.words == ['<s>', 'a', 'b', 'c', 'd']
    assert g.uni_count.tolist() == [0, 4, 3, 3, 0]                # 'x' is outside the vocabulary
    assert g.bi_count == {0: {1: 2, 2: 1}, 1: {2: 2, 3: 1}, 2: {1: 1, 3: 1}, 3: {1: 1}}
    # a pair with a member outside the vocabulary is not counted: neither (b, x) nor (x, c)
    assert sum(c for row in g.bi_count.values() for c in row.values()) == 9


def test_ngram_is_the_call_of_the_reference():
    g = counted()
    assert g.ngram('a') == {'b': 2, 'c': 1}
    assert g.ngram('<s>') == {'a': 2, 'b': 1}
    assert g.ngram('d') == {} and g.ngram('nowhere') == {}
    followers = g.ngram('b')                                       # Decoder.py:152-155: count / sum
    assert sum(followers.values()) == 2 and set(followers) == {'a', 'c'}


def test_every_witten_bell_row_sums_to_one():
    g = counted()
    pw = g.unigram_prob()
    assert pw[1:].sum() == pytest.approx(1.0, abs=1e-12)
    assert pw[1] == (4 + 1) / (10 + 4)
    for v in range(len(g.words)):                                  # '<s>' included; 'd' has no successors: bow = 1
        assert sum(g.prob(v, w) for w in range(1, len(g.words))) == pytest.approx(1.0, abs=1e-12)
    rows, bow = g.bigram_rows()
    assert bow[4] == 1.0 and bow[1] == 2 / (3 + 2)
    assert rows[1][0].tolist() == [2, 3]
    assert rows[1][1][0] == (2 + 2 * pw[2]) / (3 + 2)


def test_unigram_model_has_no_rows():
    g = counted(1)
    assert g.bi_count == {}
    rows, bow = g.bigram_rows()
    assert rows == {} and (bow == 1.0).all()
    assert g.ngram('a') == {'a': 4, 'b': 3, 'c': 3}
    with pytest.raises(ValueError):
        Ngram(3)


def test_save_and_load_round_trip(tmp_path):
    for n in (1, 2):
        g = counted(n)
        g.save_gram(str(tmp_path))
        h = Ngram(n).init_gram(str(tmp_path))
        assert h.words == g.words and h.bi_count == g.bi_count
        assert np.array_equal(h.uni_count, g.uni_count)


def tiny_tree():
    # node 0: no word; node 1: the homophones b, a (in that order); node 2: c and a word the counts never saw
    return dict(words=[[], ['b', 'a'], ['c', 'e']], node_word=np.array([0, 1, 1], dtype=np.int32))


def test_compile_sorted_columns_scale_and_penalty_as_two_operations():
    g = counted()
    tree = tiny_tree()
    scale, pen = 7.3, -2.1
    c = g.compile(tree, lm_scale=scale, word_penalty=pen)
    assert c['words'] == ['<s>', 'a', 'b', 'c', 'd', 'e'] and c['W'] == 6
    assert c['node_word_ptr'].tolist() == [0, 0, 2, 4] and c['node_word_ids'].tolist() == [2, 1, 3, 5]
    assert c['row_ptr'].dtype == np.int64 and c['col'].dtype == np.int32
    for v in range(c['W']):
        row = c['col'][c['row_ptr'][v]:c['row_ptr'][v + 1]]
        assert (np.diff(row) > 0).all()
    one = g.compile(tree)                                          # scale 1, penalty 0: the plain logarithms
    for k in ('uni', 'val'):
        want = np.float64(scale) * one[k]
        want = want + np.float64(pen)
        assert np.array_equal(c[k], want)                          # equal bits: a multiply, then an add
    assert np.array_equal(c['bow'], np.float64(scale) * one['bow'])
    assert np.isfinite(c['uni']).all() and np.isfinite(c['bow']).all() and np.isfinite(c['val']).all()
    # the plain tables are the logarithms of the probabilities over the grown vocabulary
    full = Ngram(2).count(CORPUS, VOCAB + ['e'])
    assert one['val'][c['row_ptr'][1]] == np.log(full.prob(1, 2))
    assert lm_score(one, 1, 2) == np.log(full.prob(1, 2))
    assert lm_score(one, 4, 1) == one['bow'][4] + one['uni'][1] == np.log(full.prob(4, 1))
    np.testing.assert_allclose(lm_score(one, 1, 5), np.log(full.prob(1, 5)), rtol=1e-14)   # backed off: ln bow + ln P, two roundings
    # the host's pick of a pending word: after 'a' the pair (a, b) was seen twice, (a, a) never
    assert best_word(one, 1, 1) == (2, lm_score(one, 1, 2))
    assert best_word(one, 3, 1)[0] == 1                            # after 'c' only (c, a) was seen


def test_unigram_compile_backs_off_everywhere():
    c = counted(1).compile(tiny_tree())
    assert len(c['col']) == 0 and (c['row_ptr'] == 0).all() and (c['bow'] == 0.0).all()
    assert lm_score(c, 2, 3) == c['uni'][3]
