"""Token passing over the tied states of a decision tree (pcl_lexicon_tie / _untie / _states, pcl_batch_decode_tied: the TIED
instantiations of both decode kernels) against tests/_tied_decode_twin.py -- the expansion of a tied problem onto
oracle/decoder_oracle.py -- bit for bit, through the C-ABI."""
import os
import re

import numpy as np
import pytest

import _decoder_lm_twin as lt
import _tied_decode_twin as tt
from oracle import decoder_oracle as do

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LENS = np.array([1, 2, 37], dtype=np.int32)
BEGIN = np.array([0, 1, 3], dtype=np.int64)
D = 13
ERR_INVALID, ERR_STATE = -1, -3


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def lr_units(n_units, seed):
    rng = np.random.default_rng(seed)
    trans = []
    for _ in range(n_units):
        a = np.zeros((5, 5))
        a[0, 1] = 1.0
        for r in range(1, 4):
            x = rng.uniform(0.2, 0.8)
            a[r, r], a[r, r + 1] = x, 1.0 - x
        trans.append(a)
    return np.stack(trans)


def dense_units(n_units, seed):
    """S = 4, not left to right: the entry state reaches both emitting states, every emitting state every later column."""
    rng = np.random.default_rng(seed)
    trans = []
    for _ in range(n_units):
        a = np.zeros((4, 4))
        a[0, 1:3] = [0.7, 0.3]
        a[1:-1, 1:] = rng.dirichlet(np.ones(3), size=2)
        trans.append(a)
    return np.stack(trans)


def resident(eng, lex, trans, J, seed, lm=None):
    """A (J, 2, D) model, the units, the tree, 40 frames: what every case below starts from."""
    from poccala_amd import synth
    mean, var, w, _ = synth.make_model((J + 2) // 3, 2, D, seed=seed)
    eng.load_model(mean[:J], var[:J], w[:J])
    eng.load_units(trans)
    eng.load_lexicon(lex)
    if lm is not None:
        eng.load_language_model(lm)
    frames, _, _ = synth.make_frames(1, int(LENS.sum()), D, seed=seed + 1)
    eng.load_frames(frames)


def tie(eng, tying, node_ctx=None):
    from poccala_amd.engine import as_c, ptr
    eng.load_tying(tying)
    c = as_c(tt.node_contexts(eng._lex_tree, tying.n_units) if node_ctx is None else node_ctx, np.int32)
    return eng._lib.pcl_lexicon_tie(eng._ctx, ptr(c))


def lexicon_states(eng, P):
    from poccala_amd.engine import ptr
    out = np.full((eng.n_nodes, 2 * P), -7, dtype=np.int32)
    rc = eng._lib.pcl_lexicon_states(eng._ctx, ptr(out))
    return rc, out


def emission_batch(eng, J, seed):
    """An all-state batch of J + 2 rows whose emissions are the test's own: the decoder alone is compared."""
    rng = np.random.default_rng(seed)
    b_all = [rng.standard_normal((J, int(t))) * 3.0 - 20.0 for t in LENS]
    b = eng.all_state_batch(LENS, BEGIN)
    b.set_emissions([np.concatenate([np.zeros((1, x.shape[1])), x, np.full((1, x.shape[1]), -np.inf)]) for x in b_all])
    return b, b_all


def launch(eng, b, mode, cap, P=3, cand=4, beam=0.85):
    """The raw status of one of the four entry points, and the arrays pcl_batch_decode_get (and _get_words) return."""
    lp = np.log(np.array([1.0 / (P + 2), 1.0 / (2 * P + 2)]))
    args = (b._b, float(beam), 8, cand, int(cap), float(lp[0]), float(lp[1]))
    lib = eng._lib
    rc = (lib.pcl_batch_decode(*args) if mode == 'plain' else lib.pcl_batch_decode_lm(*args) if mode == 'lm' else
          lib.pcl_batch_decode_tied(*(args + (1 if mode == 'tied_lm' else 0,))))
    if rc != 0:
        return rc, lib.pcl_last_error(eng._ctx).decode()
    b._dec_candidate, b._dec_lm = cand, mode in ('lm', 'tied_lm')
    return 0, b.decode_fetch()


def both_kernels(monkeypatch, run):
    out = {'fast': run()}
    monkeypatch.setenv('PCL_DEC_GENERAL', '1')
    out['general'] = run()
    monkeypatch.delenv('PCL_DEC_GENERAL')
    return out


def same_raw(x, y):
    nf = x[0]
    for k in (0, 1, 3, 4, 5, 6, 7, 8) + ((10,) if len(x) > 10 else ()):   # every int32 output (cleared before each decode), whole
        assert np.array_equal(x[k], y[k]), k
    for u in range(len(nf)):
        assert np.array_equal(x[2][u, :nf[u]].view(np.int64), y[2][u, :nf[u]].view(np.int64))    # the scores as bits


def against_twin(b, raw, lex, trans, b_all, states, P, lm, cap, cand=4, beam=0.85):
    got = b.decode_unpack(raw)
    for u in range(len(LENS)):
        trace, info = [], {}
        fin, hist = tt.decode(lex, list(trans), b_all[u], states, P, lm=lm, beam=beam, candidate=cand, max_tokens=cap, trace=trace, info=info)
        g = got[u]
        assert np.array_equal(g['n_tokens'], np.array(trace)), (u, g['n_tokens'], trace)
        assert g['history'] == [tuple(int(x) for x in h) for h in hist]
        assert [(n, h) for n, _, h in g['final']] == [(n, h) for n, _, h in fin]
        assert [s for _, s, _ in g['final']] == [float(s) for _, s, _ in fin]                    # bit-exact float64
        assert g['overflow'] == bool(info.get('overflow'))
    return got


@pytest.mark.parametrize('lm', [0, 1])
def test_identity_tying_is_the_untied_decoder(eng, monkeypatch, lm):
    """Every (unit, k) its own leaf, state = unit P + k: every output of pcl_batch_decode_tied equals pcl_batch_decode's (lm: _lm's,
    with hist_word) on the same batch, under the left-to-right kernel and under the general one."""
    n_units, P = 6, 3
    lex = tt.make_lexicon(n_units, 3)
    resident(eng, lex, lr_units(n_units, 4), n_units * P, 5, lm=lt.random_lm(lex, 6) if lm else None)
    assert tie(eng, tt.identity_tree(n_units, P)) == 0
    b, _ = emission_batch(eng, n_units * P, 7)
    for kernel, (want, got) in both_kernels(monkeypatch, lambda: (launch(eng, b, 'lm' if lm else 'plain', 600), launch(eng, b, 'tied_lm' if lm else 'tied', 600))).items():
        assert want[0] == 0 and got[0] == 0, (kernel, want, got)
        assert len(got[1]) == (11 if lm else 10)
        same_raw(want[1], got[1])
        assert got[1][7][2, :37].min() > 0 and got[1][4].max() > 0                               # tokens lived, words ended
    b.close()


@pytest.mark.parametrize('leg', ['given', 'scored'])
@pytest.mark.parametrize('lm', [0, 1])
@pytest.mark.parametrize('odd', [False, True])
def test_real_tree_against_the_twin_bit_for_bit(eng, monkeypatch, odd, lm, leg):
    """A tying with shared roots and edge-symbol questions; J_t + 2 odd and even (the padding of the staged rows); emissions given
    (pcl_batch_set_emissions: the decoder alone) or scored from a (J_t, 2, D) model and read back; both kernels."""
    from poccala_amd import PCL_F64
    n_units, P = 6, 3
    lex = tt.make_lexicon(n_units, 3)
    tying = tt.random_tree(n_units, P, seed=5, odd_states=odd)
    J = tying.n_states
    assert (J + 2) % 2 == int(odd)
    states = tt.node_states(lex, tying)
    assert all(tt.not_vacuous(lex, tying, states).values()), tt.not_vacuous(lex, tying, states)
    table = lt.random_lm(lex, 8) if lm else None
    trans = lr_units(n_units, 9)
    resident(eng, lex, trans, J, 10, lm=table)
    assert tie(eng, tying) == 0
    if leg == 'given':
        b, b_all = emission_batch(eng, J, 11)
    else:
        b = eng.all_state_batch(LENS, BEGIN)
        b.score(PCL_F64)
        b_all = [x[1:-1] for x in b.get('B')]
    for kernel, (rc, raw) in both_kernels(monkeypatch, lambda: launch(eng, b, 'tied_lm' if lm else 'tied', 600)).items():
        assert rc == 0, (kernel, raw)
        got = against_twin(b, raw, lex, trans, b_all, states, P, table, 600)
        assert got[2]['history'] and got[2]['n_tokens'].max() > len(lex['roots'])
    b.close()


@pytest.mark.parametrize('lm', [0, 1])
def test_general_kernel_proper_with_four_state_units(eng, lm):
    """S = 4 (P = 2), unit matrices that are not left to right: only the general kernel applies."""
    n_units, P = 5, 2
    lex = tt.make_lexicon(n_units, 13)
    tying = tt.random_tree(n_units, P, seed=14, odd_states=True)
    states = tt.node_states(lex, tying)
    table = lt.random_lm(lex, 15) if lm else None
    trans = dense_units(n_units, 16)
    resident(eng, lex, trans, tying.n_states, 17, lm=table)
    assert tie(eng, tying) == 0
    rc, got = lexicon_states(eng, P)
    assert rc == 0 and np.array_equal(got, states)
    b, b_all = emission_batch(eng, tying.n_states, 18)
    rc, raw = launch(eng, b, 'tied_lm' if lm else 'tied', 600, P=P)
    assert rc == 0, raw
    against_twin(b, raw, lex, trans, b_all, states, P, table, 600)
    b.close()


def test_capacity_paths(eng, monkeypatch):
    """max_tokens below the number of roots (overflow flagged, the twin's result), and 8 LW + 1: the left-to-right kernel's KMAX = 16
    instantiation (hmm_decode_lr_dims.inc)."""
    src = open(os.path.join(HERE, '..', 'poccala_amd', 'csrc', 'hmm_decode_lr_dims.inc')).read()
    LW = int(re.search(r'#define\s+PCL_DECLR_DW\s+(\d+)', src).group(1))
    assert re.search(r'constexpr int LW = PCL_DECLR_DW;', src)
    n_units, P = 6, 3
    lex = tt.make_lexicon(n_units, 3)
    tying = tt.random_tree(n_units, P, seed=5, odd_states=True)
    states = tt.node_states(lex, tying)
    trans = lr_units(n_units, 19)
    resident(eng, lex, trans, tying.n_states, 20)
    assert tie(eng, tying) == 0
    b, b_all = emission_batch(eng, tying.n_states, 21)
    small = len(lex['roots']) - 2
    for kernel, (rc, raw) in both_kernels(monkeypatch, lambda: launch(eng, b, 'tied', small)).items():
        assert rc == 0, (kernel, raw)
        got = against_twin(b, raw, lex, trans, b_all, states, P, None, small)
        assert all(g['overflow'] for g in got)
    rc, raw = launch(eng, b, 'tied', 8 * LW + 1)
    assert rc == 0, raw
    got = against_twin(b, raw, lex, trans, b_all, states, P, None, 8 * LW + 1)
    assert not any(g['overflow'] for g in got)
    b.close()


def test_lexicon_states_are_the_walks_and_a_snapshot(eng):
    from poccala_amd import PoccalaHipError
    n_units, P = 6, 3
    lex = tt.make_lexicon(n_units, 3)
    tying = tt.random_tree(n_units, P, seed=5, odd_states=False)
    other = tt.random_tree(n_units, P, seed=23, odd_states=True)
    resident(eng, lex, lr_units(n_units, 24), tying.n_states, 25)
    assert tie(eng, tying) == 0
    ctx = tt.node_contexts(lex, n_units)
    want = tt.node_states(lex, tying)
    rc, got = lexicon_states(eng, P)
    assert rc == 0 and np.array_equal(got, want)                   # = Tree.lookup of node_contexts
    one = lex['node_nunits'] == 1
    assert one.any() and (got[one, P:] == -1).all() and (got[~one] >= 0).all() and (got[:, :P] >= 0).all()
    slots = [(i, j) for i in range(len(one)) for j in range(int(lex['node_nunits'][i]))]
    dev = eng.tying_lookup(np.array([ctx[i, j] for i, j in slots], dtype=np.int32))
    assert np.array_equal(dev, np.array([got[i, j * P:(j + 1) * P] for i, j in slots]))          # = pcl_tying_lookup of the same contexts
    assert not np.array_equal(tt.node_states(lex, other), want)
    eng.load_tying(other)                                          # a later upload of another tree ...
    assert np.array_equal(lexicon_states(eng, P)[1], want)
    eng.drop_tying()                                               # ... and a drop do not reach the kept states
    assert np.array_equal(lexicon_states(eng, P)[1], want)
    assert np.array_equal(eng.lexicon_states(), want)
    eng.load_lexicon(lex)                                          # a new tree: gone
    rc, _ = lexicon_states(eng, P)
    assert rc == ERR_STATE and 'not tied' in eng._lib.pcl_last_error(eng._ctx).decode()
    with pytest.raises(PoccalaHipError):
        eng.lexicon_states()
    # a caller's context that differs from the default moves the states exactly as Tree.lookup says
    i = int(np.flatnonzero(~one)[0])
    mine = ctx.copy()
    mine[i, 1, 2] = 2
    mine[i, 0, 0] = 4
    assert tie(eng, tying, mine) == 0
    moved = tt.node_states(lex, tying, mine)
    assert np.array_equal(lexicon_states(eng, P)[1], moved)
    eng.tie_lexicon()                                              # the engine's default rule is node_contexts
    assert np.array_equal(eng.lexicon_states(), want)
    eng.untie_lexicon()
    eng.untie_lexicon()                                            # (no refusal when there is none)
    assert lexicon_states(eng, P)[0] == ERR_STATE


def test_every_refusal_leaves_the_resident_state_usable(eng):
    """The refusals of pcl_lexicon_tie / pcl_lexicon_states / pcl_batch_decode_tied, each followed by a decode that gives the result
    from before.  (A tying whose P is not the inventory's S - 2 cannot be made resident -- pcl_tying_upload refuses it and an
    inventory of another shape drops the tying -- so that check of pcl_lexicon_tie is unreachable through the C-ABI.)"""
    from poccala_amd import synth
    n_units, P = 6, 3
    lex = tt.make_lexicon(n_units, 3)
    tying = tt.random_tree(n_units, P, seed=5, odd_states=False)
    J = tying.n_states
    trans = lr_units(n_units, 26)
    err = lambda: eng._lib.pcl_last_error(eng._ctx).decode()

    def fresh():
        resident(eng, lex, trans, J, 27)
        assert tie(eng, tying) == 0
        return emission_batch(eng, J, 28)[0]

    def ok(b):
        rc, raw = launch(eng, b, 'tied', 600)
        assert rc == 0, raw
        return raw
    b = fresh()
    ref = ok(b)
    ctx = tt.node_contexts(lex, n_units)
    two = int(np.flatnonzero(lex['node_nunits'] == 2)[0])
    bad = ctx.copy()
    bad[two, 1, 1] = (bad[two, 1, 1] + 1) % n_units                 # a centre that is not the node's unit
    assert tie(eng, tying, bad) == ERR_INVALID and 'node %d slot 1' % two in err()
    same_raw(ref, ok(b))
    for pos, val in ((0, n_units + 1), (2, -1)):                   # a neighbour outside [0, n_units]
        bad = ctx.copy()
        bad[two, 0, pos] = val
        assert tie(eng, tying, bad) == ERR_INVALID and 'node %d slot 0' % two in err()
        same_raw(ref, ok(b))
    bad = ctx.copy()
    bad[int(np.flatnonzero(lex['node_nunits'] == 1)[0]), 1] = -5    # slot 1 of a one-unit node is not looked at
    assert tie(eng, tying, bad) == 0
    same_raw(ref, ok(b))
    rc, msg = launch(eng, b, 'tied_lm', 600)                       # lm != 0 without a language model
    assert rc == ERR_STATE and 'language model' in msg
    same_raw(ref, ok(b))
    mean, var, w, _ = synth.make_model((J + 2) // 3, 2, D, seed=27)
    eng.load_model(mean[:J - 1], var[:J - 1], w[:J - 1])
    rc, msg = launch(eng, b, 'tied', 600)                          # the resident model's J is not J_t
    assert rc == ERR_STATE and 'J_t' in msg
    small = eng.all_state_batch(LENS, BEGIN)                       # not J_t + 2 rows: the all-state batch of that smaller model
    small.set_emissions([np.zeros((J + 1, int(t))) for t in LENS])
    eng.load_model(mean[:J], var[:J], w[:J])
    rc, msg = launch(eng, small, 'tied', 600)
    assert rc == ERR_INVALID and 'J_t + 2' in msg
    small.close()
    same_raw(ref, ok(b))
    eng.untie_lexicon()                                            # the lexicon is not tied
    rc, msg = launch(eng, b, 'tied', 600)
    assert rc == ERR_STATE and 'not tied' in msg
    assert lexicon_states(eng, P)[0] == ERR_STATE
    eng.drop_tying()                                               # no tying resident
    from poccala_amd.engine import as_c, ptr
    c = as_c(ctx, np.int32)
    assert eng._lib.pcl_lexicon_tie(eng._ctx, ptr(c)) == ERR_STATE and 'tying' in err()
    assert tie(eng, tying) == 0
    same_raw(ref, ok(b))
    b.close()
    eng.load_units(lr_units(n_units + 1, 29))                      # an inventory of another shape: no lexicon (and no tying) resident
    eng.load_units(trans)
    assert eng._lib.pcl_lexicon_tie(eng._ctx, ptr(c)) == ERR_STATE and 'no resident lexicon' in err()
    b = fresh()
    same_raw(ref, ok(b))
    b.close()


def test_python_surface_batch_and_stream(eng):
    """Decoder.load_inventory(tying=) / decode_batch / decode_stream(tied=True): words and scores of the twin, chunked = unchunked."""
    from poccala_amd import Decoder, PCL_F32, synth
    n_units, P = 6, 3
    lex = tt.make_lexicon(n_units, 3)
    tying = tt.random_tree(n_units, P, seed=5, odd_states=True)
    J = tying.n_states
    states = tt.node_states(lex, tying)
    trans = lr_units(n_units, 30)
    mean, var, w, _ = synth.make_model((J + 2) // 3, 2, D, seed=31)

    class Lexicon(object):
        def compile(self, unit_index):
            assert unit_index == {'u%d' % i: i for i in range(n_units)}
            return lex
    tree = Decoder.load_inventory(eng, ['u%d' % i for i in range(n_units)], mean[:J], var[:J], w[:J], trans, Lexicon(), tying=tying)
    assert tree is lex and np.array_equal(eng.lexicon_states(), states)
    rng = np.random.default_rng(32)
    data = [rng.standard_normal((int(t), D)).astype(np.float32) for t in (37, 2, 1, 20)]
    whole = Decoder.decode_batch(data, tree, engine=eng, precision=PCL_F32, candidate=4, max_tokens=600, tied=True)
    lens = np.array([len(x) for x in data], dtype=np.int32)
    b = eng.all_state_batch(lens, np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64))     # (decode_batch left its frames resident)
    b.score(PCL_F32)
    B = b.get('B')
    b.close()
    for u, (words, score, detail) in enumerate(whole):
        fin, hist = tt.decode(lex, list(trans), B[u][1:-1], states, P, candidate=4, max_tokens=600)
        assert words == do.words_of(fin[0], hist, lex) and score == float(fin[0][1])
        assert detail['history'] == [(int(p), int(n)) for p, n in hist]
    assert any(words for words, _, _ in whole)
    chunks = [data[:2], data[2:3], data[3:]]
    parts = [Decoder.decode_batch(ch, tree, engine=eng, precision=PCL_F32, candidate=4, max_tokens=600, tied=True) for ch in chunks]
    streamed = list(Decoder.decode_stream(iter(chunks), tree, engine=eng, precision=PCL_F32, candidate=4, max_tokens=600, tied=True))
    flat = lambda res: [(wds, s, d['final'], d['history']) for ch in res for wds, s, d in ch]
    assert flat(streamed) == flat(parts) == flat([whole])
