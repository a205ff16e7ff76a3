"""CPU twin of the decoder over tied states (pcl_batch_decode_tied), by EXPANSION onto oracle/decoder_oracle.py.  TEST INFRASTRUCTURE.

A tied problem -- a pronunciation tree whose node i, unit slot j, state position k emits with tied state states[i][j P + k] of a
(J_t, T) emission matrix, and moves with the matrix of the slot's centre unit -- is a monophone problem with one PSEUDO-UNIT per
distinct (centre unit, its P states):
    unit_trans'[pseudo]       = unit_trans[centre]
    b_all'[pseudo * P + k]    = b_all[state_k]
    node_units'               = the pseudo-units
The oracle's decode (and tests/_decoder_lm_twin.py's, with a language model) runs on the expansion unchanged; nothing is mapped back,
because node ids and history are the tree's own.  The states come from ContextTree.Tree.lookup of PronunciationLexicon.node_contexts
(or of the caller's contexts): the walk is the product's host walk, the device's is held to it separately (pcl_lexicon_states).

Also here: the small hand-made fixtures the tied-decode tests share (a pronunciation tree of about 40 nodes, decision trees with
shared roots and edge-symbol questions), and the check that such a fixture is not vacuous.
"""
import numpy as np

from oracle import decoder_oracle as do
from poccala_amd.AcousticModel.ContextTree import Tree
from poccala_amd.Lexicon.PronunciationLexicon import node_contexts


def make_tree(P, n_units, q_member, node_cand, node_child, node_state, root_of):
    """A ContextTree.Tree from the arrays a walk reads (the build's statistics fields are empty)."""
    z = np.zeros(0)
    return Tree(P, n_units, node_cand=np.asarray(node_cand, dtype=np.int32), node_child=np.asarray(node_child, dtype=np.int32).reshape(-1, 2),
                node_state=np.asarray(node_state, dtype=np.int32), node_n=np.zeros(len(node_cand), dtype=np.int64), split_gain=z, row_state=z.astype(np.int32),
                event_ctx=np.zeros((0, 3), dtype=np.int32), q_member=np.asarray(q_member, dtype=np.uint8), root_of=np.asarray(root_of, dtype=np.int32),
                leaf_n=z, leaf_s=z, leaf_q=z)


def identity_tree(n_units, P):
    """Every (unit, k) its own root and leaf, state = unit P + k: the tied decoder must then be the untied one."""
    n = n_units * P
    return make_tree(P, n_units, np.zeros((1, n_units + 1), dtype=np.uint8), np.full(n, -1), np.full((n, 2), -1), np.arange(n), np.arange(n))


def random_tree(n_units, P, seed, odd_states, wide=False):
    """A hand-grown tying: units 0 and 1 share their roots (a state shared across units), questions on the left, centre and right
    neighbour up to three levels deep, two of the four questions hold the edge symbol n_units.  odd_states: the parity of J_t.
    wide (n_units >= 33: two words of the bit table per question, the edge symbol in word 1): every question has members on both
    sides of unit 32 -- units 31 and 32 answer the first differently from each other, and unit 5 answers the last as the edge does, which
    is what a walk that reads word 0 for the edge symbol's bit would see."""
    rng = np.random.default_rng(seed)
    q = np.zeros((4, n_units + 1), dtype=np.uint8)
    q[0, [0, 1, 2]] = 1
    q[1, [3, 4, n_units]] = 1
    q[2, list(range(1, n_units, 2))] = 1
    q[3, n_units] = 1
    if wide:
        assert n_units >= 33
        q[0, 32] = 1
        q[1, 32] = 1
        q[2, 32:n_units] = 1 - q[2, 32:n_units]                    # odd units below 32, even ones from 32 on
        q[3, 5] = 1
    Q = 4
    root_of = np.zeros(n_units * P, dtype=np.int32)
    for u in range(n_units):
        for k in range(P):
            root_of[u * P + k] = (max(u, 1) - 1) * P + k           # units 0 and 1 -> the same root
    R0 = (n_units - 1) * P
    cand, child, depth = [-1] * R0, [[-1, -1] for _ in range(R0)], [0] * R0

    def split(i, c):
        cand[i] = c
        child[i] = [len(cand), len(cand) + 1]
        for _ in range(2):
            cand.append(-1)
            child.append([-1, -1])
            depth.append(depth[i] + 1)
    i = 0
    while i < len(cand):                                           # (children lie behind their parent: ids only grow)
        if depth[i] < 3 and rng.random() < (0.9, 0.6, 0.4)[depth[i]]:
            split(i, int(rng.choice([0, 0, 2, 2, 1])) * Q + int(rng.integers(Q)))
        i += 1
    if (sum(1 for c in cand if c < 0) % 2 == 1) != bool(odd_states):
        split(max(j for j, c in enumerate(cand) if c < 0), 2 * Q + 3)          # one more leaf: "is the right neighbour the edge?"
    state, nxt = [], 0
    for c in cand:
        state.append(nxt if c < 0 else -1)
        nxt += c < 0
    return make_tree(P, n_units, q, cand, child, state, root_of)


def make_lexicon(n_units, seed, n_nodes=40, pin=()):
    """A flat pronunciation tree in PronunciationLexicon.compile's form: about n_nodes nodes of one and two units, depth >= 3, words at
    every leaf and some inner nodes (a few with two homophones), and pairs of nodes that spell the same units under parents whose last
    units differ.  pin: up to five units; the i-th is the first unit of root i, whatever the draws give."""
    rng = np.random.default_rng(seed)
    units, parent, kids, depth = [], [], [], []

    def add(par, us):
        units.append(list(us) + [-1] * (2 - len(us)))
        parent.append(par)
        kids.append([])
        depth.append(0 if par < 0 else depth[par] + 1)
        if par >= 0:
            kids[par].append(len(units) - 1)
        return len(units) - 1

    def spell():
        return [int(x) for x in rng.integers(n_units, size=int(rng.integers(1, 3)))]
    for i in range(5):
        add(-1, spell())
        if i < len(pin):
            units[i][0] = int(pin[i])
    chain = 0
    for _ in range(3):                                             # a depth-3 chain, whatever the draws below do
        chain = add(chain, spell())
    while len(units) < n_nodes - 6:
        par = int(rng.integers(len(units)))
        if depth[par] < 4:
            add(par, spell())
    last = lambda i: units[i][1] if units[i][1] >= 0 else units[i][0]
    done = 0
    for a in range(len(units)):                                    # the same spelling under parents whose last units differ
        for b in range(a + 1, len(units)):
            if done < 3 and last(a) != last(b):
                us = spell()
                add(a, us)
                add(b, us)
                done += 1
                break
    n = len(units)
    child_ptr = np.zeros(n + 1, dtype=np.int32)
    for i in range(n):
        child_ptr[i + 1] = child_ptr[i] + len(kids[i])
    word = [1 if (not kids[i] or rng.random() < 0.3) else 0 for i in range(n)]
    words = [([] if not word[i] else ['w%d' % i] if i % 4 else ['w%da' % i, 'w%db' % i]) for i in range(n)]
    nu = np.array([1 if u[1] < 0 else 2 for u in units], dtype=np.int32)
    return dict(node_units=np.array(units, dtype=np.int32), node_nunits=nu, node_parent=np.array(parent, dtype=np.int32), child_ptr=child_ptr,
                child_idx=np.array([c for k in kids for c in k], dtype=np.int32), node_word=np.array(word, dtype=np.int32),
                roots=np.array([i for i in range(n) if parent[i] < 0], dtype=np.int32), names=['n%d' % i for i in range(n)], words=words, dropped=[])


def wide_fixture(P=3):
    """(lexicon, tying) over 33 units: roots that begin with units 32 and 31 (the two sides of the word boundary), 5 (which answers the
    last question as the edge symbol does) and 0 and 1 (the units that share their roots)."""
    return make_lexicon(33, 3, pin=(32, 31, 5, 0, 1)), random_tree(33, P, seed=5, odd_states=True, wide=True)


def node_states(lex, tying, node_ctx=None):
    """(n_nodes, 2 P) int32: Tree.lookup of every (node, slot, k), -1 in slot 1 of a one-unit node -- what pcl_lexicon_states returns."""
    ctx = node_contexts(lex, tying.n_units) if node_ctx is None else np.asarray(node_ctx)
    P = tying.P
    out = np.full((len(lex['node_nunits']), 2 * P), -1, dtype=np.int32)
    for i, nn in enumerate(lex['node_nunits']):
        for j in range(int(nn)):
            for k in range(P):
                out[i, j * P + k] = tying.lookup(ctx[i, j, 0], ctx[i, j, 1], ctx[i, j, 2], k)
    return out


def expand(lex, unit_trans, b_all, states, P):
    """The monophone problem of the module docstring: (tree', unit_trans' list, b_all' (n_pseudo P, T), pseudo = [(centre, states)])."""
    index, pseudo = {}, []
    nu2 = np.full_like(np.asarray(lex['node_units']), -1)
    for i, nn in enumerate(lex['node_nunits']):
        for j in range(int(nn)):
            key = (int(lex['node_units'][i][j]),) + tuple(int(s) for s in states[i, j * P:(j + 1) * P])
            if key not in index:
                index[key] = len(pseudo)
                pseudo.append((key[0], key[1:]))
            nu2[i, j] = index[key]
    tree2 = dict(lex)
    tree2['node_units'] = nu2
    trans2 = [np.asarray(unit_trans[c]) for c, _ in pseudo]
    rows = np.array([s for _, st in pseudo for s in st], dtype=np.int64)
    return tree2, trans2, np.asarray(b_all)[rows], pseudo


def decode(lex, unit_trans, b_all, states, P, lm=None, **kw):
    """The tied decode of one utterance: decoder_oracle.decode (lm None) or _decoder_lm_twin.decode on the expansion."""
    tree2, trans2, b2, _ = expand(lex, unit_trans, b_all, states, P)
    if lm is None:
        return do.decode(tree2, trans2, b2, s=P + 2, **kw)
    import _decoder_lm_twin as lt
    return lt.decode(tree2, trans2, b2, lm, s=P + 2, **kw)


def edge_decides(tying, ctx3, k):
    """Does a question that holds the edge symbol answer yes BECAUSE the asked neighbour is the edge, somewhere on this walk?"""
    node = int(tying.root_of[int(ctx3[1]) * tying.P + k])
    hit = False
    while tying.node_cand[node] >= 0:
        pos, qi = divmod(int(tying.node_cand[node]), tying.Q)
        yes = bool(tying.q_member[qi, ctx3[pos]])
        hit |= yes and int(ctx3[pos]) == tying.n_units
        node = int(tying.node_child[node, 1 if yes else 0])
    return hit


def not_vacuous(lex, tying, states, node_ctx=None):
    """The three properties a tied-decode fixture must have to test anything (each a bool)."""
    ctx = node_contexts(lex, tying.n_units) if node_ctx is None else np.asarray(node_ctx)
    P, n = tying.P, len(lex['node_nunits'])
    spell = [tuple(int(u) for u in lex['node_units'][i][:lex['node_nunits'][i]]) for i in range(n)]
    same_units_other_states = any(spell[a] == spell[b] and lex['node_parent'][a] != lex['node_parent'][b] and not np.array_equal(states[a], states[b])
                                  for a in range(n) for b in range(a + 1, n))
    ro = np.asarray(tying.root_of).reshape(tying.n_units, P)
    shared_root = any(ro[a, k] == ro[b, k] for a in range(tying.n_units) for b in range(a + 1, tying.n_units) for k in range(P))
    by_state = {}
    for i in range(n):
        for j in range(int(lex['node_nunits'][i])):
            for k in range(P):
                by_state.setdefault(int(states[i, j * P + k]), set()).add(int(lex['node_units'][i][j]))
    shared_state = shared_root and any(len(us) > 1 for us in by_state.values())
    edge = any(edge_decides(tying, ctx[i, j], k) for i in range(n) for j in range(int(lex['node_nunits'][i])) for k in range(P))
    return dict(same_units_other_states=same_units_other_states, shared_state=shared_state, edge_decides=edge)
