"""The walks of csrc/tying.hip (tying_walk under tying_lookup_kernel, tied_label_states_kernel and lexicon_tie_kernel) where a question
takes more than one word of the bit table, at the exact fit of the LDS staging (96 units x 1024 questions = 4096 words), through the
global-memory instances (96 x 1025 = 4100 words) and in the second trip of the lookup's grid-stride loop -- against Tree.lookup
(tests/_tied_twin.py).  tests/test_tied_twin.py and tests/test_tied_decode_twin.py prove on the CPU that the trees, the context sample
and the lexicons used here read the table at those edges, and that a walk with a wrong word index, a wrong stride or a short staging
copy differs from Tree.lookup on them.  Integer work: every comparison is for equality."""
import numpy as np
import pytest

import _tied_decode_twin as dt
import _tied_twin as tt
import test_gpu_decode_tied as gd
import test_gpu_tied_batches as gb
from test_gpu_tied_batches import same_bits

pytestmark = pytest.mark.gpu
D = 13


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def unit_trans(n_units, S, seed=3):
    from poccala_amd import synth
    rng = np.random.default_rng(seed)
    return np.stack([synth.random_left_right_transmat(rng, S) for _ in range(n_units)])


# ------------------------------------------------------------------ 1. lookup
@pytest.mark.parametrize('n_units,Q', tt.DEVICE_CASES)
@pytest.mark.parametrize('P', [1, 3])
def test_lookup_over_wide_tables(eng, P, n_units, Q):
    tree, sample, want = tt.device_case(n_units, Q, P)
    eng.load_units(unit_trans(n_units, P + 2))
    eng.load_tying(tree)
    got = eng.tying_lookup(sample)
    print('lookup (%d, %d) P=%d: %d table words, %d contexts, %d entries differ' % (n_units, Q, P, Q * tt.words(n_units), len(sample), int((got != want).sum())))
    assert got.dtype == np.int32 and got.shape == (len(sample), P) and np.array_equal(got, want)
    if n_units != 96:
        return
    # LDS and global tables in turn within one context: nothing of the table before stays behind
    ro = tt.roots_only(P, n_units)
    mono = sample[:, 1:2] * P + np.arange(P)[None, :]
    small = tt.chain(P, n_units=n_units)                           # (Q = 24: 96 words)
    small_want = tt.lookup_all(small, sample[:600])
    for other, other_want, n in ((ro, n_units * P - 1 - mono, len(sample)), (small, small_want, 600)):
        eng.load_tying(other)
        assert np.array_equal(eng.tying_lookup(sample[:n]), other_want)
        eng.load_tying(tree)
        assert same_bits(eng.tying_lookup(sample), got)


# ------------------------------------------------------------------ 2. the second trip of the grid-stride loop
@pytest.mark.parametrize('n_units,Q,P', [(96, 1025, 1), (95, 24, 3)])
def test_lookup_second_trip_of_the_grid_stride_loop(eng, n_units, Q, P):
    """pcl_tying_lookup launches min(ceil(n P / 256), 1024) workgroups of 256 threads: items 0 .. 262143 run in the loop's first trip.
    n = 262144 // P + 1 contexts are 262144 + 1 (P = 1) or 262144 + 2 (P = 3) items, so item 262144 -- context 262144 at P = 1, position
    k = 1 of context 87381 at P = 3 -- is the first of the second trip, run by thread 0 of workgroup 0, and the last context of the call
    lies in it."""
    tree, sample, want = tt.device_case(n_units, Q, P)
    n = 262144 // P + 1
    assert (n - 1) * P <= 262144 < n * P and -(-n * P // 256) > 1024
    at = (np.arange(n, dtype=np.int64) * 7 + 3) % len(sample)
    eng.load_units(unit_trans(n_units, P + 2))
    eng.load_tying(tree)
    got = eng.tying_lookup(np.take(sample, at, axis=0))
    twin = np.take(want, at, axis=0)
    print('second trip (%d, %d) P=%d: %d contexts, %d items, %d entries differ, %d of them in the second trip' % (
        n_units, Q, P, n, n * P, int((got != twin).sum()), int((got.reshape(-1)[262144:] != twin.reshape(-1)[262144:]).sum())))
    assert got.shape == (n, P) and np.array_equal(got, twin)


# ------------------------------------------------------------------ 3. the tied label batch
@pytest.mark.parametrize('n_units,Q,S', [(96, 1025, 5), (32, 24, 3)])
def test_tied_batch_over_a_wide_table(eng, n_units, Q, S):
    from poccala_amd.engine import make_sentence_batch
    P = S - 2
    tree = tt.device_case(n_units, Q, P)[0]
    assert tree.n_states <= 72 * P + P
    labels, T, begin, F = tt.edge_corpus(seed=S, n_units=n_units)
    lens = [len(l) for l in labels]
    assert lens[0] == 1 and max(lens) == 130 and max(max(l) for l in labels) >= min(n_units - 1, 64)
    trans = unit_trans(n_units, S)
    mean, var, w = tt.model_for(tree.n_states, 1, D, seed=10 + S)
    pos = tt.pos_states(tree, labels)
    want_rows = tt.row_states(tree, labels)
    eng.load_units(trans)
    eng.load_model(mean, var, w)
    eng.load_frames(gb.frames_along(np.random.default_rng(11 + S), F, labels, T, begin, pos, mean, var))
    eng.load_tying(tree)
    ref, n = make_sentence_batch(eng, labels, T, begin, trans, S, unit_state_ids=[tree.unit_state_ids(l) for l in labels])
    b = eng.label_batch([np.asarray(l, dtype=np.int32) for l in labels], T, begin, tied=True)
    rows = b.row_states()
    print('tied batch (%d, %d) S=%d: %d utterances, %d rows, %d differ from the twin' % (
        n_units, Q, S, len(labels), int(b.N.sum()), sum(int((r != q).sum()) for r, q in zip(rows, want_rows))))
    assert np.array_equal(b.N, n) and np.array_equal(b.N, P * np.array(lens) + 2)
    assert all(same_bits(r, q) for r, q in zip(rows, want_rows))
    assert all(same_bits(p, q) for p, q in zip(b.pos_states(), pos))
    assert all(same_bits(r, q) for r, q in zip(rows, ref.row_states()))
    if Q * tt.words(n_units) > tt.LDS_WORDS:
        x, y = gb.run_estep(eng, b), gb.run_estep(eng, ref)
        assert np.isfinite(x['logp']).sum() >= len(labels) // 2
        gb.hold_equal('wide', x, y)
    b.close()
    ref.close()


# ------------------------------------------------------------------ 4. the lexicon's states
@pytest.mark.parametrize('n_units', [96, 33])
def test_lexicon_states_under_wide_tyings(eng, n_units):
    P = 3
    if n_units == 96:
        tying = tt.device_case(96, 1025, P)[0]
        lex = dt.make_lexicon(96, 3, pin=(95, 64, 32, 31))
    else:
        lex, tying = dt.wide_fixture(P)
    want = dt.node_states(lex, tying)
    eng.load_units(gd.lr_units(n_units, 24))
    eng.load_lexicon(lex)
    eng.load_tying(tying)
    eng.tie_lexicon()
    got = eng.lexicon_states()
    one = lex['node_nunits'] == 1
    print('lexicon states, %d units: %d nodes, %d entries differ' % (n_units, len(one), int((got != want).sum())))
    assert got.dtype == np.int32 and np.array_equal(got, want)     # = Tree.lookup of node_contexts
    assert one.any() and (got[one, P:] == -1).all() and (got[~one] >= 0).all() and (got[:, :P] >= 0).all()


# ------------------------------------------------------------------ 5. the decoder over a wide tying
def test_decode_under_the_wide_tying(eng, monkeypatch):
    """33 units: two words a question, the edge symbol -- the right context of every node's last unit -- in the second.  Both decode
    kernels against the expansion twin, bit for bit, without a language model."""
    n_units, P = 33, 3
    lex, tying = dt.wide_fixture(P)
    J = tying.n_states
    states = dt.node_states(lex, tying)
    assert all(dt.not_vacuous(lex, tying, states).values()), dt.not_vacuous(lex, tying, states)
    trans = gd.lr_units(n_units, 9)
    gd.resident(eng, lex, trans, J, 10)
    assert gd.tie(eng, tying) == 0
    rc, got = gd.lexicon_states(eng, P)
    assert rc == 0 and np.array_equal(got, states)
    b, b_all = gd.emission_batch(eng, J, 11)
    for kernel, (rc, raw) in gd.both_kernels(monkeypatch, lambda: gd.launch(eng, b, 'tied', 600)).items():
        assert rc == 0, (kernel, raw)
        out = gd.against_twin(b, raw, lex, trans, b_all, states, P, None, 600)
        assert out[2]['history'] and out[2]['n_tokens'].max() > len(lex['roots'])
    b.close()
