"""Word lattices from token passing (pcl_batch_decode_lattice / pcl_batch_lattice_get / _posteriors / _results; the LAT instantiations of both
decode kernels and csrc/lattice.hip) on the GPU: the decode's outputs bit-equal with and without the lattice, the records bit-equal to
tests/_lattice_twin.py's recording loop on both kernels, capacity, degenerate utterances, the lattice pass against the twin, refusals."""
import numpy as np
import pytest

import _decoder_lm_twin as lt
import _lattice_twin as lw
import _tied_decode_twin as tt
from test_gpu_decode_lm import left_right, scored_batch
from test_gpu_decode_tied import LENS, emission_batch, lr_units, resident, tie

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STATE = -1, -3
NEW_SYMBOLS = ('pcl_batch_decode_lattice', 'pcl_batch_lattice_get', 'pcl_batch_lattice_posteriors', 'pcl_batch_lattice_results',
               'pcl_batch_lattice_set_records')


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def test_new_symbols_load(eng):
    for name in NEW_SYMBOLS:
        assert getattr(eng._lib, name) is not None


def same_raw(x, y):
    """Every array of decode_fetch: the int32 outputs whole, the scores of the returned tokens as bits."""
    assert len(x) == len(y)
    for k in (0, 1, 3, 4, 5, 6, 7, 8) + ((10,) if len(x) > 10 else ()):
        assert np.array_equal(x[k], y[k]), k
    for u in range(len(x[0])):
        assert np.array_equal(x[2][u, :x[0][u]].view(np.int64), y[2][u, :x[0][u]].view(np.int64))


def fetch(b, **kw):
    b.decode_launch(**kw)
    return b.decode_fetch()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_records(lat, fin, rec, ent, T):
    want = lw.build(rec, ent, fin, T)
    assert lat.n_arcs_wanted == len(rec) and not lat.overflow and len(lat.frame) == len(rec) + len(fin)
    for k in ('frame', 'tok', 'node', 'hist', 'word', 'start', 'end'):
        assert np.array_equal(getattr(lat, k), want[k]), k
    assert np.array_equal(bits(lat.score), bits(want['score'])) and np.array_equal(bits(lat.term), bits(want['term']))
    assert np.array_equal(lat.hist_frame, [f for f, _ in ent]) and np.array_equal(bits(lat.hist_seed), bits([s for _, s in ent]))
    assert np.array_equal(lat.span[:, 1], want['frame']) and np.array_equal(lat.span[:, 0], want['node_frame'][want['start']] + 1)
    return want


def same_lattice(x, y):
    for k in ('frame', 'tok', 'node', 'hist', 'word', 'start', 'end', 'hist_frame'):
        assert np.array_equal(getattr(x, k), getattr(y, k)), k
    for k in ('score', 'term', 'hist_seed'):
        assert np.array_equal(bits(getattr(x, k)), bits(getattr(y, k))), k
    assert (x.n_arcs_wanted, x.overflow) == (y.n_arcs_wanted, y.overflow)


def assert_pass_is_the_twin(post, want, use_word, kappa):
    """The lattice pass of one utterance against the float64 twin within the allowance; returns the largest share of it used."""
    t64 = lw.posteriors(want, kappa, use_word)
    tld = lw.posteriors(want, kappa, use_word, dtype=np.longdouble)
    allow = lw.allowances(t64, tld, want)
    assert post['status'] == 0 and t64['status'] == 0
    share = abs(post['lnZ'] - t64['lnZ']) / allow['lnZ']
    fin = np.isfinite(t64['lnp'])
    assert np.array_equal(post['lnpost'][~fin], t64['lnp'][~fin])                              # -inf where the twin has -inf, no NaN
    share = max(share, float(np.max(np.abs(post['lnpost'][fin] - t64['lnp'][fin]) / allow['lnp'][fin], initial=0.0)))
    assert abs(post['best_score'] - t64['best_score']) <= allow['best_score']
    assert list(post['best_arcs']) == t64['best']
    conf = np.array([c for _, _, _, c in post['best']])
    share = max(share, float(np.max(np.abs(conf - t64['conf']) / allow['conf'], initial=0.0)))
    assert np.all(conf >= 0.0) and np.all(conf <= 1.0 + allow['conf'])
    # posteriors sum per node: what enters an entry leaves it, and START sends out 1
    with np.errstate(under='ignore'):
        p = np.exp(post['lnpost'])
    n_nodes = want['H'] + 2
    out = np.bincount(want['start'], weights=p, minlength=n_nodes)
    into = np.bincount(want['end'], weights=p, minlength=n_nodes)
    tol = np.max(allow['lnp']) * (len(p) + 1)
    assert abs(out[0] - 1.0) <= tol and abs(into[-1] - 1.0) <= tol and np.all(np.abs(out[1:-1] - into[1:-1]) <= tol)
    assert share <= 1.0, share
    return share


@pytest.fixture(scope='module')
def untied(eng):
    """test_gpu_decode_lm.py's random-tree fixture: 300 words over 60 units with homophones, left-to-right units, U = 4 ragged, T <= 80."""
    from poccala_amd import synth
    n_units = 60
    tree, _ = synth.make_pronunciation_tree(300, n_units, seed=91)
    trans = left_right(n_units, 71)
    b, B = scored_batch(eng, tree, n_units, trans, 3, 4, 80, 70)
    lm = lt.random_lm(tree, 73, 2.0, -1.0)
    eng.load_language_model(lm)
    yield dict(tree=tree, trans=trans, b=b, B=B, lm=lm, twin={})
    b.close()


def twin_of(fx, u, lm, beam, cap, cand=6):
    key = (u, lm, beam, cap)
    if key not in fx['twin']:                                                   # computed once, shared and left unchanged
        trace = []
        fx['twin'][key] = lw.record_decode(fx['tree'], list(fx['trans']), fx['B'][u][1:-1], fx['lm'] if lm else None, beam=beam, candidate=cand, max_tokens=cap,
                                           trace=trace) + (trace,)
    return fx['twin'][key]


@pytest.mark.parametrize('lm', [0, 1])
def test_untied_decode_is_unchanged_and_records_are_the_twin(eng, untied, monkeypatch, lm):
    b, shares = untied['b'], []
    # the second setting: max_tokens below the most tokens the first one had alive -- up to the frame that reaches it the two runs are
    # the same, so that frame drops a creation: max_tokens overflows
    settings = [(0.85, 4096)]
    for beam, cap in settings:
        kw = dict(beam=beam, candidate=6, max_tokens=cap, lm=bool(lm))
        lats = {}
        for kernel in ('fast', 'general'):
            if kernel == 'general':
                monkeypatch.setenv('PCL_DEC_GENERAL', '1')
            plain = fetch(b, **kw)
            with_lat = fetch(b, lattice=True, max_arcs=20000, **kw)
            same_raw(plain, with_lat)
            lats[kernel] = b.lattice()
            post = b.lattice_posteriors(1.0) if kernel == 'fast' else None
            if kernel == 'general':
                monkeypatch.delenv('PCL_DEC_GENERAL')
            for u in range(b.U):
                fin, hist, rec, ent, _ = twin_of(untied, u, lm, beam, cap)
                want = assert_records(lats[kernel][u], fin, rec, ent, int(b.T[u]))
                if post is not None:
                    shares.append(assert_pass_is_the_twin(post[u], want, bool(lm), 1.0))
                    assert abs(post[u]['best_score'] - fin[0][1]) <= 3.0 * (want['H'] + 1) * np.spacing(np.abs(want['score']).max())
        for x, y in zip(lats['fast'], lats['general']):
            same_lattice(x, y)
        assert any(len(x.hist_frame) > 3 for x in lats['fast'])
        if cap == 4096:
            settings.append((0.85, max(max(twin_of(untied, u, lm, beam, cap)[4]) for u in range(b.U)) - 5))
        else:
            assert any(bool(o) for o in plain[8])                               # (an utterance where max_tokens overflowed)
    print('lattice pass on decoded lattices, lm=%d: worst share of the allowance %.3f' % (lm, max(shares)))


def test_capacity(eng, untied):
    b = untied['b']
    kw = dict(beam=0.85, candidate=6, max_tokens=4096, lm=True)
    plain = fetch(b, **kw)
    counts = [len(twin_of(untied, u, 1, 0.85, 4096)[2]) for u in range(b.U)]
    big = int(np.argmax(counts))
    assert sorted(counts)[-1] > sorted(counts)[-2] > 1                          # (one utterance alone overflows at its count - 1)
    raw = fetch(b, lattice=True, max_arcs=counts[big], **kw)
    same_raw(plain, raw)
    whole = b.lattice()
    whole_post = b.lattice_posteriors(1.0)
    assert [x.n_arcs_wanted for x in whole] == counts and not any(x.overflow for x in whole) and all(p['status'] == 0 for p in whole_post)
    for max_arcs in (counts[big] - 1, 1):
        raw = fetch(b, lattice=True, max_arcs=max_arcs, **kw)
        same_raw(plain, raw)                                                    # the decode does not see the overflow
        lats, post = b.lattice(), b.lattice_posteriors(1.0)
        assert [x.n_arcs_wanted for x in lats] == counts
        for u in range(b.U):
            over = counts[u] > max_arcs
            assert lats[u].overflow == over and bool(post[u]['status'] & 1) == over
            if over:
                assert np.isnan(post[u]['lnZ']) and post[u]['best'] == [] and np.all(np.isnan(post[u]['lnpost']))
            else:                                                               # a neighbour: bit-equal to the batch without the overflow
                same_lattice(lats[u], whole[u])
                assert bits(post[u]['lnZ']) == bits(whole_post[u]['lnZ']) and np.array_equal(bits(post[u]['lnpost']), bits(whole_post[u]['lnpost']))
                assert post[u]['best'] == whole_post[u]['best']
        assert lats[big].overflow and (max_arcs == 1 or sum(x.overflow for x in lats) == 1)


def test_refusals_and_drops(eng, untied):
    from poccala_amd import PCL_F64, PoccalaHipError
    from poccala_amd.engine import ptr
    b, lib = untied['b'], eng._lib
    lp = np.log(np.array([1.0 / 5, 1.0 / 8]))
    args = (b._b, 0.85, 8, 6, 4096, float(lp[0]), float(lp[1]))
    n = np.zeros(b.U, np.int32)

    def has_lattice():
        return lib.pcl_batch_lattice_get(b._b, ptr(n), *([None] * 13))
    b.decode()                                                                  # any other decode drops the lattice
    assert has_lattice() == ERR_STATE and lib.pcl_batch_lattice_posteriors(b._b, 1.0) == ERR_STATE
    assert lib.pcl_batch_lattice_results(b._b, *([None] * 7)) == ERR_STATE
    for bad in (0, -3):
        assert lib.pcl_batch_decode_lattice(*(args + (0, 0, bad))) == ERR_INVALID
    assert lib.pcl_batch_decode_lattice(*(args + (0, 1, 1000))) == ERR_STATE    # tied = 1: the lexicon is not tied
    assert 'not tied' in lib.pcl_last_error(eng._ctx).decode()
    assert has_lattice() == ERR_STATE
    assert lib.pcl_batch_decode_lattice(*(args + (1, 0, 20000))) == 0           # a valid call after the refused ones
    assert has_lattice() == 0 and n.min() > 0
    assert lib.pcl_batch_lattice_results(b._b, *([None] * 7)) == ERR_STATE      # no posteriors yet
    for kappa in (0.0, -1.0, np.nan, np.inf):
        assert lib.pcl_batch_lattice_posteriors(b._b, float(kappa)) == ERR_INVALID
    assert lib.pcl_batch_lattice_posteriors(b._b, 1.0) == 0
    z = np.zeros(b.U)
    assert lib.pcl_batch_lattice_results(b._b, ptr(z), *([None] * 6)) == 0 and np.all(np.isfinite(z))
    eng.load_lexicon(untied['tree'])                                            # a lexicon re-upload drops the language model
    assert lib.pcl_batch_decode_lattice(*(args + (1, 0, 20000))) == ERR_STATE
    assert 'no language model' in lib.pcl_last_error(eng._ctx).decode()
    assert has_lattice() == 0                                                   # (refused before anything changed: the lattice is still there)
    assert lib.pcl_batch_decode_lattice(*(args + (0, 0, 20000))) == 0 and has_lattice() == 0
    b.score(PCL_F64)                                                            # new emissions drop it
    assert has_lattice() == ERR_STATE
    with pytest.raises(PoccalaHipError):
        b.lattice_posteriors()
    eng.load_language_model(untied['lm'])
    res = b.decode(beam=0.85, candidate=6, max_tokens=4096, lm=True, lattice=True, max_arcs=20000)
    assert has_lattice() == 0 and len(res) == b.U


@pytest.mark.parametrize('lm', [0, 1])
def test_tied_decode_is_unchanged_and_records_are_the_twin(eng, monkeypatch, lm):
    """test_gpu_decode_tied.py's fixture: T = 1, 2 and 37 -- the first two are shorter than any word: closing arcs only."""
    n_units, P = 6, 3
    lex = tt.make_lexicon(n_units, 3)
    tying = tt.random_tree(n_units, P, seed=5, odd_states=True)
    states = tt.node_states(lex, tying)
    table = lt.random_lm(lex, 8) if lm else None
    trans = lr_units(n_units, 9)
    resident(eng, lex, trans, tying.n_states, 10, lm=table)
    assert tie(eng, tying) == 0
    b, b_all = emission_batch(eng, tying.n_states, 11)
    kw = dict(beam=0.85, candidate=4, max_tokens=600, lm=bool(lm), tied=True)
    lats = {}
    for kernel in ('fast', 'general'):
        if kernel == 'general':
            monkeypatch.setenv('PCL_DEC_GENERAL', '1')
        plain = fetch(b, **kw)
        with_lat = fetch(b, lattice=True, max_arcs=4000, **kw)
        same_raw(plain, with_lat)
        lats[kernel] = b.lattice()
        post = b.lattice_posteriors(0.5)
        if kernel == 'general':
            monkeypatch.delenv('PCL_DEC_GENERAL')
        for u in range(len(LENS)):
            tree2, trans2, b2, _ = tt.expand(lex, list(trans), b_all[u], states, P)
            fin, hist, rec, ent = lw.record_decode(tree2, trans2, b2, table, beam=0.85, candidate=4, max_tokens=600, s=P + 2)
            want = assert_records(lats[kernel][u], fin, rec, ent, int(LENS[u]))
            assert_pass_is_the_twin(post[u], want, bool(lm), 0.5)
            if LENS[u] <= 2:
                assert len(rec) == 0 and np.all(lats[kernel][u].word == -1) and len(fin) > 0 and np.isfinite(post[u]['lnZ'])
        assert len(lats[kernel][2].hist_frame) > 0
    for x, y in zip(lats['fast'], lats['general']):
        same_lattice(x, y)
    b.close()


def test_many_word_end_donors_in_one_frame(eng):
    """test_gpu_decode_lm.py's many-donors construction: thousands of donors in a frame -- more word-end donors in one wave than the
    lane-per-token kernel's list holds in LDS (DLW = 128), and word-end donors in every wave."""
    from poccala_amd import synth
    n_units = 183
    tree, _ = synth.make_pronunciation_tree(3000, n_units, seed=81)
    a = np.zeros((5, 5))
    a[0, 1] = 1.0
    for r in range(1, 4):
        a[r, r], a[r, r + 1] = 0.1, 0.9
    trans = np.stack([a] * n_units)
    b, B = scored_batch(eng, tree, n_units, trans, 2, 2, 22, 82, ragged=False, same_gmm=True)
    lm = lt.random_lm(tree, 84, 1.0, 0.0, successors=20)
    eng.load_language_model(lm)
    kw = dict(beam=1.0, candidate=4, max_tokens=8192, lm=True)
    plain = fetch(b, **kw)
    with_lat = fetch(b, lattice=True, max_arcs=60000, **kw)
    same_raw(plain, with_lat)
    lats = b.lattice()
    b.close()
    per_wave_max, waves_hit = 0, 0
    for u in range(2):
        trace = []
        fin, hist, rec, ent = lw.record_decode(tree, list(trans), B[u][1:-1], lm, beam=1.0, candidate=4, max_tokens=8192, trace=trace)
        assert_records(lats[u], fin, rec, ent, 22)
        for f in sorted({r[0] for r in rec}):
            C = -(-trace[f - 1] // 512) * 64                                     # the wave's share of the frame's tokens
            cnt = np.bincount([r[1] // C for r in rec if r[0] == f], minlength=8)
            per_wave_max, waves_hit = max(per_wave_max, int(cnt.max())), max(waves_hit, int((cnt > 0).sum()))
    assert per_wave_max > 128 and waves_hit == 8, (per_wave_max, waves_hit)


def test_dropin_word_times(eng):
    """Decoder.decode_batch(word_times=True): the default return is unchanged; the detail gains the best path with times and confidences."""
    import json
    import os
    from poccala_amd import Decoder, PCL_F32, synth
    from poccala_amd.Lexicon import PinYin, PronunciationLexicon
    import tempfile
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'G13_lexicon.json')))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'Mandarin.dat')
        with open(path, 'w') as f:
            for k, v in g['table'].items():
                f.write('%s\t%s\n' % (k, v))
        py = PinYin(path)
        lx = PronunciationLexicon()
        lx.generate_lexicon(words=g['words'], pinyin=py)
        units = sorted({u for w in g['words'] for r in py.word2pinyin(w) for x in r for u in x.split(',')})
    mean, var, w, trans = synth.make_model(len(units), 2, 13, seed=31)
    tree = Decoder.load_inventory(eng, units, mean, var, w, trans, lx)
    frames, lens, begin = synth.make_frames(2, 50, 13, seed=32)
    chunk = [frames[:50], frames[50:]]
    plain = Decoder.decode_batch(chunk, tree, engine=eng, precision=PCL_F32)
    timed = Decoder.decode_batch(chunk, tree, engine=eng, precision=PCL_F32, word_times=True)
    for (pw, ps, pd), (tw_, ts, td) in zip(plain, timed):
        assert pw == tw_ and ps == ts and pd['final'] == td['final'] and pd['history'] == td['history']
        assert 'word_times' not in pd and td['lattice_status'] == 0
        wt = td['word_times']
        assert len(wt) >= 1 and wt[0][1] == 0 and wt[-1][2] == 49
        assert all(0.0 <= c <= 1.0 + 1e-9 and first <= last + 1 for _, first, last, c in wt)
        assert all(x[2] + 1 == y[1] for x, y in zip(wt, wt[1:]))                # the words tile the utterance
