"""The CPU twin of the word lattice (tests/_lattice_twin.py) against things that do not share its code: the existing decoder twins for the
recording loop, a brute-force enumeration of every path for the lattice rule, the decoder's own best final score for the Viterbi path.
CPU only."""
import numpy as np
import pytest

import _decoder_lm_twin as lt
import _lattice_twin as lw
from oracle import decoder_oracle as do

E = 3


def random_case(n_units, T, seed):
    from poccala_amd import synth
    rng = np.random.default_rng(seed)
    trans = [synth.random_left_right_transmat(rng) for _ in range(n_units)]
    return trans, rng.normal(-20.0, 4.0, size=(n_units * E, T))


@pytest.fixture(scope='module')
def decoded():
    """One decode with a random bigram, shared (and left unchanged) by the tests below: (tree, lm, T, final, history, records, entries)."""
    from poccala_amd import synth
    tree, _ = synth.make_pronunciation_tree(300, 60, seed=91)
    trans, b_all = random_case(60, 60, 7)
    lm = lt.random_lm(tree, 73, 2.0, -1.0)
    fin, hist, rec, ent = lw.record_decode(tree, trans, b_all, lm, beam=0.85, candidate=6, max_tokens=600)
    assert len(hist) > 3 and len(rec) > len(hist)
    return tree, lm, b_all.shape[1], fin, hist, rec, ent


@pytest.mark.parametrize('beam,cap', [(0.85, None), (0.6, 300)])
def test_recording_loop_is_the_existing_twins(beam, cap):
    from poccala_amd import synth
    for seed, n_words, n_units, T in ((3, 300, 60, 50), (4, 500, 40, 35)):
        tree, _ = synth.make_pronunciation_tree(n_words, n_units, seed=seed)
        trans, b_all = random_case(n_units, T, seed + 10)
        kw = dict(beam=beam, candidate=6, max_tokens=cap)
        lm = lt.random_lm(tree, seed + 20, 3.0, -2.0)
        t0, i0, t1, i1 = [], {}, [], {}
        fin0, hist0 = lt.decode(tree, trans, b_all, lm, trace=t0, info=i0, **kw)
        fin1, hist1, rec, ent = lw.record_decode(tree, trans, b_all, lm, trace=t1, info=i1, **kw)
        assert fin1 == fin0 and hist1 == hist0 and t1 == t0 and i1 == i0
        assert len(ent) == len(hist1) and len(rec) >= len(ent) and [f for f, _ in ent] == sorted({r[0] for r in rec})
        # the seed is the winning offer: the best s + term of the frame, and the entry names its earliest donor
        for (f, seed_), (hp, hn, hw) in zip(ent, hist1):
            offers = [(r[4] + r[5], -r[1], r) for r in rec if r[0] == f]
            top = max(offers)
            assert seed_ == top[0] and (top[2][3], top[2][2], top[2][6]) == (hp, hn, hw)
        # zero tables and no tables: decoder_oracle.decode
        t2, i2, t3, i3 = [], {}, [], {}
        fin2, hist2 = do.decode(tree, trans, b_all, trace=t2, info=i2, **kw)
        fin3, hist3, rec3, _ = lw.record_decode(tree, trans, b_all, None, trace=t3, info=i3, **kw)
        assert fin3 == fin2 and hist3 == hist2 and t3 == t2 and i3 == i2
        fin4, hist4, rec4, _ = lw.record_decode(tree, trans, b_all, lt.zero_lm(tree), **kw)
        assert fin4 == fin2 and [(p, n) for p, n, _ in hist4] == hist2
        assert [r[:5] for r in rec4] == [r[:5] for r in rec3] and all(r[5] == 0.0 and r[6] == 0 for r in rec3)


@pytest.mark.parametrize('seed', range(8))
def test_enumeration_on_tiny_lattices(seed):
    rng = np.random.default_rng(seed)
    H = int(rng.integers(0, 5))                                                 # at most 6 nodes
    per = [int(rng.integers(1, 4)) for _ in range(H)]
    while sum(per) > 10:
        per[int(np.argmax(per))] -= 1
    rec, ent, fin, T = lw.random_lattice(rng, H, lambda k: per[k], n_final=2, dead=1 if seed % 2 else 0, neg_inf=1 if seed % 3 == 0 else 0)
    lat = lw.build(rec, ent, fin, T)
    assert lat['H'] + 2 <= 6 and len(lat['frame']) <= 12
    for kappa in (1.0, 0.1):
        r = lw.posteriors(lat, kappa)
        Z, arc_post, best, best_score, node_post = lw.enumerate_paths(lat, kappa)
        assert r['status'] == 0
        assert abs(r['lnZ'] - np.log(Z)) <= 1e-12 * max(1.0, abs(np.log(Z)))
        with np.errstate(under='ignore'):
            assert np.allclose(np.exp(r['lnp']), arc_post, rtol=0, atol=1e-12)
        assert r['best'] == best and abs(r['best_score'] - best_score) <= 1e-12 * max(1.0, abs(best_score))
        for k in range(lat['H'] + 1):                                           # the arcs out of a node carry the node's posterior
            out = np.flatnonzero(lat['start'] == k)
            with np.errstate(under='ignore'):
                total = np.exp(r['lnp'][out]).sum()
            assert abs(total - node_post[k]) <= 1e-12
            with np.errstate(under='ignore'):
                gamma = np.exp(r['alpha'][k] + r['beta'][k] - r['lnZ'])
            assert abs(gamma - node_post[k]) <= 1e-12
            if node_post[k] == 0.0 and not np.isfinite(r['beta'][k]):           # a dead node: -inf, not NaN
                assert r['beta'][k] == -np.inf and np.all(r['lnp'][np.flatnonzero(lat['end'] == k)] == -np.inf)
        assert not np.any(np.isnan(r['lnp']))


def viterbi_allowance(lat):
    """The path's score is a telescoping sum of H + 1 weights, each a difference and a sum rounded at the scores' magnitude."""
    fin = np.abs(lat['score'][np.isfinite(lat['score'])])
    return 3.0 * (lat['H'] + 1) * np.spacing(fin.max())


def test_viterbi_is_the_decoders_own_answer(decoded):
    tree, lm, T, fin, hist, rec, ent = decoded
    lat = lw.build(rec, ent, fin, T)
    r = lw.posteriors(lat, 1.0, use_word=True)
    allow = viterbi_allowance(lat)
    assert abs(r['best_score'] - fin[0][1]) <= allow
    # the path: the closing arc of the best final token, then its hist_prev chain -- wherever the runner-up into a node is further away
    # than the allowance
    chain, h = [], fin[0][2]
    while h >= 0:
        chain.append(h)
        h = hist[h][0]
    chain.reverse()
    nodes_on_path = [int(lat['end'][a]) for a in r['best']]
    w = r['w']
    decided = True
    for k in nodes_on_path:
        a = np.flatnonzero(lat['end'] == k)
        y = np.sort(r['vit'][lat['start'][a]] + w[a])
        decided &= len(y) < 2 or y[-1] - y[-2] > allow
    if decided:
        assert nodes_on_path[:-1] == [h + 1 for h in chain] and nodes_on_path[-1] == lat['H'] + 1
        assert [int(lat['word'][a]) for a in r['best'][:-1]] == [hist[h][2] for h in chain]
    assert decided                                                              # (this fixture does decide: the check above ran)
    conf = np.asarray(r['conf'])
    assert np.all(conf >= 0.0) and np.all(conf <= 1.0 + 1e-9)


def test_single_chain_has_confidence_one():
    rec = [(3, 0, 5, -1, -40.0, -1.0, 2), (7, 4, 6, 0, -90.0, -2.0, 3)]
    ent = [(3, -41.0), (7, -92.0)]
    fin = [(9, -120.0, 1)]
    lat = lw.build(rec, ent, fin, 10)
    for kappa in (1.0, 0.1):
        r = lw.posteriors(lat, kappa, use_word=True)
        assert r['best'] == [0, 1, 2] and np.all(r['lnp'] == 0.0) and np.all(r['conf'] == 1.0)
        assert r['lnZ'] == r['best_score']


@pytest.mark.parametrize('omission', ['subtract_seed', 'child_score', 'closing'])
def test_each_omission_moves_the_viterbi_score(decoded, omission):
    """Without the seed subtraction the histories' scores are counted once per word; with s + term for the children the term is counted
    twice; without the closing arcs the last word's frames are missing: each moves the lattice's best score away from the decoder's by far
    more than the allowance."""
    tree, lm, T, fin, hist, rec, ent = decoded
    right = lw.build(rec, ent, fin, T)
    allow = viterbi_allowance(right)
    assert abs(lw.posteriors(right)['best_score'] - fin[0][1]) <= allow
    kw = dict(closing=True, subtract_seed=True, child_score=False)
    kw[omission] = not kw[omission]
    wrong = lw.posteriors(lw.build(rec, ent, fin, T, **kw))
    assert abs(wrong['best_score'] - fin[0][1]) > 1e6 * allow
