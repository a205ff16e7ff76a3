"""The lattice pass (csrc/lattice.hip: the build's sort and counting sort, forward-backward, Viterbi, confidences) at its list, node and
workgroup edges, on record sets of the test's own uploaded through pcl_batch_lattice_set_records -- lists no decode of a few seconds
reaches -- against tests/_lattice_twin.py within the allowance derived there."""
import numpy as np
import pytest

import _lattice_twin as lw

pytestmark = pytest.mark.gpu
T_ALL, CAND = 140, 3
# (entries, arcs into entry k): entry counts 0, 1, 63, 64, 65; lists of 1, 64, 65, 257 and 600 arcs (the workgroup has 256 threads: one, two
# and three rounds of it, a full wave and one lane more); dead ends; arcs of -inf; an entry nothing enters
CASES = [
    dict(H=0, per=lambda k: 1),
    dict(H=1, per=lambda k: 1),
    dict(H=1, per=lambda k: 600),
    dict(H=63, per=lambda k: (1, 64, 65, 257)[k % 4], dead=5, neg_inf=9),
    dict(H=64, per=lambda k: (65, 1, 2)[k % 3], neg_inf=3),
    dict(H=65, per=lambda k: 600 if k == 40 else 3, dead=2),
    dict(H=5, per=lambda k: 2, orphan=True),
    dict(H=3, per=lambda k: 1, chain=True),
]


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def make_case(c, seed):
    rng = np.random.default_rng(seed)
    if c.get('chain'):                                                          # a single chain: every posterior and confidence is 1
        rec = [(4, 0, 1, -1, -40.0, -1.0, 2), (9, 3, 2, 0, -90.0, -2.0, 3), (30, 1, 3, 1, -300.0, -0.5, 4)]
        return rec, [(4, -41.0), (9, -92.0), (30, -300.5)], [(7, -900.0, 2)]
    rec, ent, fin, _ = lw.random_lattice(rng, c['H'], c['per'], n_final=CAND, dead=c.get('dead', 0), neg_inf=c.get('neg_inf', 0), T=T_ALL)
    if c.get('orphan'):
        ent.append((ent[-1][0] + 2, ent[-1][1] - 20.0))                         # an entry without an arc in or out
    return rec, ent, fin


@pytest.fixture(scope='module')
def uploaded(eng):
    """One batch of len(CASES) utterances of T_ALL frames with the cases' records in it, shuffled inside every frame as the waves' appends
    would leave them; the twins, computed once."""
    from poccala_amd import synth
    from poccala_amd.engine import ptr
    U = len(CASES)
    mean, var, w, trans = synth.make_model(4, 2, 13, seed=1)
    eng.load_model(mean, var, w)
    eng.load_units(trans)
    frames, lens, begin = synth.make_frames(U, T_ALL, 13, seed=2, ragged=False)
    eng.load_frames(frames)
    b = eng.all_state_batch(lens, begin)
    sets = [make_case(c, 100 + i) for i, c in enumerate(CASES)]
    max_arcs = max(len(r) for r, _, _ in sets) + 7
    rng = np.random.default_rng(5)
    i32, f64 = np.int32, np.float64
    wanted, hn, nf = np.zeros(U, i32), np.zeros(U, i32), np.zeros(U, i32)
    ai = {k: np.zeros((U, max_arcs), i32) for k in ('frame', 'tok', 'node', 'hist', 'word')}
    af = {k: np.zeros((U, max_arcs), f64) for k in ('score', 'term')}
    hf, hs = np.full((U, T_ALL), -1, i32), np.zeros((U, T_ALL), f64)
    fn, fh, fs = np.zeros((U, CAND), i32), np.zeros((U, CAND), i32), np.zeros((U, CAND), f64)
    for u, (rec, ent, fin) in enumerate(sets):
        order = sorted(range(len(rec)), key=lambda i: (rec[i][0], rng.random()))
        for x, i in enumerate(order):
            f, tk, nd, h, sc, tm, wd = rec[i]
            ai['frame'][u, x], ai['tok'][u, x], ai['node'][u, x], ai['hist'][u, x], ai['word'][u, x] = f, tk, nd, h, wd
            af['score'][u, x], af['term'][u, x] = sc, tm
        wanted[u], hn[u], nf[u] = len(rec), len(ent), len(fin)
        for k, (f, sd) in enumerate(ent):
            hf[u, k], hs[u, k] = f, sd
        for c, (n, sc, h) in enumerate(fin):
            fn[u, c], fs[u, c], fh[u, c] = n, sc, h

    def upload(wanted_, cap=max_arcs):
        cut = lambda a: np.ascontiguousarray(a[:, :cap])
        rc = eng._lib.pcl_batch_lattice_set_records(b._b, cap, CAND, 1, ptr(wanted_), ptr(cut(ai['frame'])), ptr(cut(ai['tok'])), ptr(cut(ai['node'])),
                                                    ptr(cut(ai['hist'])), ptr(cut(af['score'])), ptr(cut(af['term'])), ptr(cut(ai['word'])), ptr(hn), ptr(hf),
                                                    ptr(hs), ptr(nf), ptr(fn), ptr(fs), ptr(fh))
        assert rc == 0, eng._lib.pcl_last_error(eng._ctx).decode()
        b._lat = (cap, CAND, True)
    upload(wanted)
    lats = [lw.build(rec, ent, fin, T_ALL) for rec, ent, fin in sets]
    yield dict(b=b, sets=sets, lats=lats, upload=upload, wanted=wanted, max_arcs=max_arcs)
    b.close()


def test_build_is_the_canonical_order(uploaded):
    for lat, want in zip(uploaded['b'].lattice(), uploaded['lats']):
        for k in ('frame', 'tok', 'node', 'hist', 'word', 'start', 'end'):
            assert np.array_equal(getattr(lat, k), want[k]), k
        assert np.array_equal(lat.score.view(np.int64), want['score'].view(np.int64)) and not lat.overflow


@pytest.mark.parametrize('kappa', [1.0, 0.1])
def test_pass_against_the_twin(uploaded, kappa):
    from test_gpu_lattice import assert_pass_is_the_twin
    b = uploaded['b']
    first, again = b.lattice_posteriors(kappa), b.lattice_posteriors(kappa)
    worst = 0.0
    for u, (c, want) in enumerate(zip(CASES, uploaded['lats'])):
        share = assert_pass_is_the_twin(first[u], want, True, kappa)
        worst = max(worst, share)
        print('kappa %g case %d (H = %d, %d arcs): share of the allowance %.3f' % (kappa, u, want['H'], len(want['frame']), share))
        # determinism: two runs, bit for bit
        assert np.array_equal(first[u]['lnpost'].view(np.int64), again[u]['lnpost'].view(np.int64)) and first[u]['best'] == again[u]['best']
        assert np.float64(first[u]['lnZ']).view(np.int64) == np.float64(again[u]['lnZ']).view(np.int64)
        t64 = lw.posteriors(want, kappa, True)
        if c.get('dead') or c.get('neg_inf') or c.get('orphan'):
            assert np.any(np.isneginf(first[u]['lnpost'])) or c.get('orphan')    # dead ends and -inf arcs: -inf, never NaN
            assert not np.any(np.isnan(first[u]['lnpost']))
        if c.get('orphan'):
            assert np.isneginf(t64['alpha'][want['H']]) and np.isneginf(t64['beta'][want['H']])
        if c.get('chain'):
            assert np.all(first[u]['lnpost'] == 0.0) and [x[3] for x in first[u]['best']] == [1.0] * 4
    print('kappa %g: worst share of the allowance %.3f' % (kappa, worst))


def test_overflow_and_no_final_are_flagged(uploaded):
    b, wanted = uploaded['b'], uploaded['wanted']
    whole = b.lattice_posteriors(1.0)
    more = wanted.copy()
    more[3] += 11                                                               # as if the cap had cut 11 donors of utterance 3
    uploaded['upload'](more)
    post = b.lattice_posteriors(1.0)
    lats = b.lattice()
    assert lats[3].overflow and lats[3].n_arcs_wanted == more[3] and post[3]['status'] & 1 and np.isnan(post[3]['lnZ']) and post[3]['best'] == []
    for u in range(len(CASES)):
        if u != 3:
            assert post[u]['status'] == 0 and np.array_equal(post[u]['lnpost'].view(np.int64), whole[u]['lnpost'].view(np.int64))
    uploaded['upload'](wanted)                                                  # (as the other tests found it)
