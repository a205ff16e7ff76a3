"""The default context rule of a tied lexicon (PronunciationLexicon.node_contexts) and the CPU twin of the tied decoder
(tests/_tied_decode_twin.py: an expansion onto oracle/decoder_oracle.py), without a GPU."""
import numpy as np
import pytest

import _tied_decode_twin as tt
from oracle import decoder_oracle as do
from poccala_amd.Lexicon import PronunciationLexicon
from poccala_amd.Lexicon.PronunciationLexicon import node_contexts

P, S = 3, 5


def hand_tree():
    """node 0: root [2]; node 1: its child, two units [0, 4]; node 2: a lone-final child of node 1 [5]; node 3: child of node 2 [1, 3]
    (a depth-3 chain); node 4: a second root [3, 1] with a lone-final child 5 = [5]."""
    units = [[2, -1], [0, 4], [5, -1], [1, 3], [3, 1], [5, -1]]
    kids = [[1], [2], [3], [], [5], []]
    cp = np.cumsum([0] + [len(k) for k in kids]).astype(np.int32)
    return dict(node_units=np.array(units, dtype=np.int32), node_nunits=np.array([1, 2, 1, 2, 2, 1], dtype=np.int32),
                node_parent=np.array([-1, 0, 1, 2, -1, 4], dtype=np.int32), child_ptr=cp, child_idx=np.array([c for k in kids for c in k], dtype=np.int32),
                node_word=np.array([0, 1, 0, 1, 0, 1], dtype=np.int32), roots=np.array([0, 4], dtype=np.int32),
                names=list('abcdef'), words=[[], ['x'], [], ['y'], [], ['z']], dropped=[])


def test_node_contexts_on_a_hand_written_tree():
    n_units, E = 6, 6                                             # E: the edge symbol
    ctx = node_contexts(hand_tree(), n_units)
    assert ctx.shape == (6, 2, 3) and ctx.dtype == np.int32
    assert ctx[0, 0].tolist() == [E, 2, E]                         # a root, one unit: edge on both sides
    assert ctx[1].tolist() == [[2, 0, 4], [0, 4, E]]               # two units under the root: parent's last unit | the other unit | edge
    assert ctx[2, 0].tolist() == [4, 5, E]                         # a lone final: left = the LAST unit of its two-unit parent
    assert ctx[3].tolist() == [[5, 1, 3], [1, 3, E]]               # depth 3
    assert ctx[4].tolist() == [[E, 3, 1], [3, 1, E]]               # a two-unit root
    assert ctx[5, 0].tolist() == [1, 5, E]                         # the same spelling as node 2 under another parent: another left context
    for i in (0, 2, 5):
        assert ctx[i, 1].tolist() == [E, -1, E]                    # slot 1 of a one-unit node: no centre
    assert np.array_equal(PronunciationLexicon.node_contexts(hand_tree(), n_units), ctx)


def problem(seed, n_units=6, T=25):
    rng = np.random.default_rng(seed)
    lex = tt.make_lexicon(n_units, seed)
    trans = []
    for _ in range(n_units):
        a = np.zeros((S, S))
        a[0, 1] = 1.0
        for r in range(1, S - 1):
            x = rng.uniform(0.2, 0.8)
            a[r, r], a[r, r + 1] = x, 1.0 - x
        trans.append(a)
    return lex, trans, rng


def test_fixture_lexicon_has_the_shape_the_gpu_tests_state():
    lex = tt.make_lexicon(6, 3)
    n = len(lex['node_nunits'])
    assert 35 <= n <= 45 and set(lex['node_nunits'].tolist()) == {1, 2}
    depth = np.zeros(n, dtype=int)
    for i in range(n):
        depth[i] = 0 if lex['node_parent'][i] < 0 else depth[lex['node_parent'][i]] + 1   # (parents come first)
    assert depth.max() >= 3
    seen = np.zeros(n, dtype=int)
    seen[lex['child_idx']] += 1
    assert np.array_equal(seen == 0, lex['node_parent'] < 0) and seen.max() == 1 and sorted(lex['roots']) == np.flatnonzero(seen == 0).tolist()


def test_identity_tying_expansion_reproduces_the_oracle_exactly():
    lex, trans, rng = problem(3)
    b_all = rng.standard_normal((6 * P, 25)) * 3.0 - 20.0
    ident = tt.identity_tree(6, P)
    states = tt.node_states(lex, ident)
    for i, nn in enumerate(lex['node_nunits']):                    # state = centre P + k
        want = [int(lex['node_units'][i][j]) * P + k for j in range(nn) for k in range(P)] + [-1] * (P * (2 - nn))
        assert states[i].tolist() == want
    for cap in (None, 7):
        t0, t1, i0, i1 = [], [], {}, {}
        want = do.decode(lex, trans, b_all, candidate=4, max_tokens=cap, trace=t0, info=i0)
        got = tt.decode(lex, trans, b_all, states, P, candidate=4, max_tokens=cap, trace=t1, info=i1)
        assert got == want and t0 == t1 and i0 == i1               # (float scores compared with ==: the same bits)


def test_wide_tying_and_lexicons_reach_the_second_word():
    """What tests/test_gpu_tying_wide.py ties and decodes: a 33-unit tying whose questions have members on both sides of unit 32 and
    whose edge symbol is bit 1 of word 1, under a lexicon that spells units 31 and 32; a 96-unit lexicon with units in every word.
    Each walk that misreads the table (tests/_tied_twin.py BROKEN) gives some node of the lexicon another state."""
    import _tied_twin as tw
    n_units = 33
    lex, tying = tt.wide_fixture(P)
    assert tying.n_units == n_units and tying.n_states % 2 == 1 and tw.words(n_units) == 2 and (n_units >> 5, n_units & 31) == (1, 1)
    qm = tying.q_member
    assert qm.shape == (4, 34) and all(qm[q, :32].any() and qm[q, 32:].any() and not qm[q].all() for q in range(4))
    assert qm[0, 31] != qm[0, 32] and qm[3, 5] == qm[3, n_units] == 1 and qm[3].sum() == 2
    narrow = tt.random_tree(n_units, P, seed=5, odd_states=True)
    assert np.array_equal(narrow.node_cand, tying.node_cand) and not narrow.q_member[0, 32:].any()    # the same tree; only the questions' members differ
    assert lex['node_units'][:5, 0].tolist() == [32, 31, 5, 0, 1] and np.array_equal(tt.make_lexicon(6, 3, pin=())['node_units'], tt.make_lexicon(6, 3)['node_units'])
    states = tt.node_states(lex, tying)
    assert all(tt.not_vacuous(lex, tying, states).values()), tt.not_vacuous(lex, tying, states)
    ctx = node_contexts(lex, n_units)
    slots = np.array([ctx[i, j] for i in range(len(ctx)) for j in range(int(lex['node_nunits'][i]))], dtype=np.int32)
    assert (slots[:, 2] == n_units).any() and (slots[:, :2] == 32).any()
    want = tw.lookup_all(tying, slots)
    assert np.array_equal(tw.table_walk_all(tying, slots), want)
    for m in (1, 2, 3):
        n = int((tw.table_walk_all(tying, slots, m) != want).any(axis=1).sum())
        print('33-unit tying, broken walk %d: %d of %d lexicon slots get another state' % (m, n, len(slots)))
        assert n >= 1
    # the 96-unit lexicon of the lexicon test
    big = tt.make_lexicon(96, 3, pin=(95, 64, 32, 31))
    used = big['node_units'][big['node_units'] >= 0]
    n = len(big['node_nunits'])
    assert 35 <= n <= 45 and set(big['node_nunits'].tolist()) == {1, 2}
    assert {0, 1, 2} <= set((used >> 5).tolist()) and 95 in used and used.max() == 95
    tree = tw.device_case(96, 1025, P)[0]
    slots = np.array([c for i, cc in enumerate(node_contexts(big, 96)) for c in cc[:int(big['node_nunits'][i])]], dtype=np.int32)
    want = tw.lookup_all(tree, slots)
    for m in (1, 2, 3):
        k = int((tw.table_walk_all(tree, slots, m) != want).any(axis=1).sum())
        print('96-unit lexicon under the (96, 1025) chain, broken walk %d: %d of %d slots get another state' % (m, k, len(slots)))
        assert k >= 1


@pytest.mark.parametrize('odd', [False, True])
def test_expansion_is_the_stated_gather_and_the_fixture_is_not_vacuous(odd):
    lex, trans, rng = problem(3)
    tying = tt.random_tree(6, P, seed=5, odd_states=odd)
    assert tying.n_states % 2 == int(odd)
    b_all = rng.standard_normal((tying.n_states, 9))
    states = tt.node_states(lex, tying)
    tree2, trans2, b2, pseudo = tt.expand(lex, trans, b_all, states, P)
    assert len(set(pseudo)) == len(pseudo) and b2.shape == (len(pseudo) * P, 9)
    for pu, (centre, st) in enumerate(pseudo):
        assert trans2[pu] is trans[centre] or np.array_equal(trans2[pu], trans[centre])
        for k in range(P):
            assert np.array_equal(b2[pu * P + k], b_all[st[k]])
    for i, nn in enumerate(lex['node_nunits']):
        for j in range(2):
            pu = int(tree2['node_units'][i][j])
            if j >= nn:
                assert pu == -1
            else:
                assert pseudo[pu] == (int(lex['node_units'][i][j]), tuple(states[i, j * P:(j + 1) * P].tolist()))
    assert tree2['child_idx'] is lex['child_idx'] and tree2['roots'] is lex['roots']       # node ids and structure are the tree's own
    assert all(tt.not_vacuous(lex, tying, states).values()), tt.not_vacuous(lex, tying, states)
    # a caller's context that differs from the default moves exactly the states Tree.lookup says
    ctx = node_contexts(lex, 6)
    i = int(np.flatnonzero(lex['node_nunits'] == 2)[0])
    ctx[i, 1, 2] = 2                                               # "the right neighbour is unit 2", not the edge
    moved = tt.node_states(lex, tying, ctx)
    assert np.array_equal(np.delete(moved, i, axis=0), np.delete(states, i, axis=0))
    assert moved[i, P:].tolist() == [tying.lookup(ctx[i, 1, 0], ctx[i, 1, 1], 2, k) for k in range(P)]
