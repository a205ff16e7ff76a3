"""NumPy twin of the resident tying and of label-built batches over tied states (row f17; csrc/tying.hip), and the trees and corpora the
tests share.  Built from ContextTree.Tree.lookup (the walk), tests/_realign_twin.py (row -> position, runs, slices, the drop rule) and
tests/_tree_twin.py (the statistics).  Integer work only: every comparison against it is for equality.  tests/test_tied_twin.py proves on
the CPU that every tree and corpus below reaches the edge it claims; tests/test_gpu_tied_batches.py runs them on the device."""
import numpy as np

import _realign_twin as rt
import _tree_cases as tc
import _tree_twin as tw

ENTRY, EXIT = -1, -2
N_UNITS = 5


def _tree(P, n_units, q_member, cand, child, state, root_of):
    from poccala_amd.AcousticModel.ContextTree import Tree
    N, Jt = len(cand), int((np.asarray(state) >= 0).sum())
    return Tree(P, n_units, node_cand=np.asarray(cand, dtype=np.int32), node_child=np.asarray(child, dtype=np.int32).reshape(N, 2),
                node_state=np.asarray(state, dtype=np.int32), node_n=np.zeros(N, dtype=np.int64), split_gain=np.zeros(0),
                row_state=np.zeros(0, dtype=np.int32), event_ctx=np.zeros((0, 3), dtype=np.int32), q_member=np.asarray(q_member, dtype=np.uint8),
                root_of=np.asarray(root_of, dtype=np.int32), leaf_n=np.zeros(Jt, dtype=np.int64), leaf_s=np.zeros((Jt, 1)), leaf_q=np.zeros((Jt, 1)))


# ------------------------------------------------------------------ trees
def roots_only(P, n_units=N_UNITS, reverse=True):
    """No split: one root per (centre, k), every root a leaf.  The states run AGAINST the node ids, so that the map is not unit * P + k
    (reverse=False: it is -- the monophone model as a tying)."""
    N = n_units * P
    return _tree(P, n_units, tc.member([{0}], n_units), [-1] * N, [[-1, -1]] * N, list(range(N - 1, -1, -1)) if reverse else list(range(N)), np.arange(N))


CHAIN_Q = 24


def chain_follower(k, n_units=N_UNITS):
    """The context that stays on chain k to its last level: the first has both neighbours at the utterance edge (an L = 1 label)."""
    return [(n_units, 2, n_units), (1, 3, n_units), (n_units, 0, 4)][k % 3]


def chain(P, n_units=N_UNITS, Q=CHAIN_Q, seed=7):
    """One root per state position, shared by all centres; below root k a chain of depth 3 Q = 72: level l asks candidate perm_k[l] (every
    (position, question) pair once), one child is a leaf, the other the next level -- the child chain_follower(k) goes to, so that this
    context walks all 72 levels, more than a wavefront is wide, and the others leave at every depth.  The edge symbol is a member of
    about half of the questions.  Children are created behind their parent, as a build does."""
    rng = np.random.default_rng(seed)
    sets = []
    while len(sets) < Q:
        m = rng.integers(0, 2, size=n_units + 1)
        if 0 < m.sum() <= n_units:
            sets.append(set(np.flatnonzero(m).tolist()))
    qm = tc.member(sets, n_units)
    edge_in = int(qm[:, n_units].sum())
    assert 0 < edge_in < Q
    cand, child, state = [-1] * P, [[-1, -1] for _ in range(P)], [-1] * P
    nstate = 0
    for k in range(P):
        node, ctx = k, chain_follower(k, n_units)
        perm = rng.permutation(3 * Q)
        for lvl, c in enumerate(perm):
            pos, qi = divmod(int(c), Q)
            go = int(qm[qi, ctx[pos]])                             # the child the follower takes
            a, b = len(cand), len(cand) + 1                        # a: the leaf, b: the next level (the last level: a second leaf)
            cand += [-1, -1]
            child += [[-1, -1], [-1, -1]]
            state += [nstate, -1]
            nstate += 1
            cand[node] = int(c)
            child[node] = [a, b] if go == 1 else [b, a]
            node = b
        state[node] = nstate
        nstate += 1
    return _tree(P, n_units, qm, cand, child, state, np.tile(np.arange(P), n_units))


def build_case(P, seed=41):
    """A _tree_cases build case for the 5-unit inventory: every context seen, one root per state position shared by all centres, eleven
    splits below them (questions about the centre among them)."""
    return tc.make(seed + P, n_units=N_UNITS, P=P, D=3, shared_root=True, centre_shift=2.0, max_leaves=P + 11)


def built_twin(P):
    c = build_case(P)
    t = tw.build(c['n'], c['s'], c['q'], c['event_ctx'], c['P'], c['n_units'], c['q_member'], c['R0'], c['root_of'], c['min_count'], c['min_gain'],
                 c['max_leaves'], c['var_floor'])
    return tw.as_tree(t, P, N_UNITS, c['event_ctx'], c['q_member'], c['root_of'])


def all_contexts(n_units=N_UNITS):
    """Every (left, centre, right): (n_units + 1)^2 n_units of them"""
    return np.array([(l, c, r) for l in range(n_units + 1) for c in range(n_units) for r in range(n_units + 1)], dtype=np.int32)


def lookup_all(tree, ctx3):
    """(n, P) int32 by Tree.lookup"""
    return np.array([[tree.lookup(l, c, r, k) for k in range(tree.P)] for l, c, r in np.asarray(ctx3).tolist()], dtype=np.int32).reshape(-1, tree.P)


def walk_depth(tree, left, centre, right, k):
    """Inner nodes a walk passes"""
    ctx, node, depth = (left, centre, right), int(tree.root_of[centre * tree.P + k]), 0
    while tree.node_cand[node] >= 0:
        pos, qi = divmod(int(tree.node_cand[node]), tree.Q)
        node = int(tree.node_child[node, 1 if tree.q_member[qi, ctx[pos]] else 0])
        depth += 1
    return depth


# ------------------------------------------------------------------ the batch
def contexts_of(label, n_units=N_UNITS):
    lab = [int(x) for x in label]
    return [(lab[i - 1] if i > 0 else n_units, c, lab[i + 1] if i + 1 < len(lab) else n_units) for i, c in enumerate(lab)]


def pos_states(tree, labels):
    """Per utterance the (L, P) tied states of its label positions, by Tree.lookup on contexts formed as triphone_events forms them"""
    return [lookup_all(tree, contexts_of(lab, tree.n_units)) for lab in labels]


def row_states(tree, labels):
    return [np.concatenate([[ENTRY], ps.reshape(-1), [EXIT]]).astype(np.int32) for ps in pos_states(tree, labels)]


def owner_map(tree, paths, labels, S, T, begin, F):
    """(frame_state (F,) int32 over tied states, dropped, frame_pos (F,), frame_k (F,)): the monophone owner map's drop rule and slices, the
    label position of every path row, and pos_state[i][k] in place of unit * P + k."""
    P = S - 2
    mono, dropped = rt.realign(paths, labels, S, T, begin, F)
    state = np.full(F, -1, dtype=np.int32)
    pos, kk = np.full(F, -1, dtype=np.int64), np.full(F, -1, dtype=np.int64)
    for u, (path, lab, ps) in enumerate(zip(paths, labels, pos_states(tree, labels))):
        if u in dropped:
            continue
        sl = slice(int(begin[u]), int(begin[u]) + int(T[u]))
        i, k = rt.row_positions(path, len(lab), P), mono[sl].astype(np.int64) % P
        assert (mono[sl] // P == np.asarray(lab)[i]).all()
        state[sl], pos[sl], kk[sl] = ps[i, k], i, k
    return state, dropped, pos, kk


def tree_rows(label_event, labels, P, T, begin, F, frame_pos, frame_k):
    """The statistics row of every frame row for pcl_tree_accumulate: label_event[i] P + k, -1 where not kept or the event is -1"""
    off = np.concatenate([[0], np.cumsum([len(l) for l in labels])])
    rows = np.full(F, -1, dtype=np.int32)
    for u in range(len(labels)):
        for f in range(int(begin[u]), int(begin[u]) + int(T[u])):
            if frame_pos[f] >= 0:
                ev = int(label_event[off[u] + frame_pos[f]])
                if ev >= 0:
                    rows[f] = ev * P + frame_k[f]
    return rows


# ------------------------------------------------------------------ corpora
def edge_corpus(seed=0, U=70, n_units=N_UNITS):
    """U = 70 labels of mixed lengths: L = 1 (both neighbours the edge), L = 2, adjacent equal units, one of L = 130 (the 64 lanes of its
    workgroup stride it three times), T of 5 to 40 frames each, placed with gaps and rows in front and behind."""
    rng = np.random.default_rng(900 + seed)
    labels = [[2], [0, 4], [1, 1, 3], [3, 3, 3], [int(x) for x in rng.integers(0, n_units, size=130)]]
    while len(labels) < U:
        labels.append([int(x) for x in rng.integers(0, n_units, size=int(rng.integers(1, 9)))])
    labels = labels[:U]
    # (three frames a label unit where 40 frames allow it, so that most utterances have a path at S = 5 too)
    T = np.array([min(40, max(5, 3 * len(l) + int(rng.integers(0, 9)))) for l in labels], dtype=np.int32)
    begin = np.empty(len(labels), dtype=np.int64)
    row = 3
    for u in rng.permutation(len(labels)):
        begin[u] = row
        row += int(T[u]) + int(rng.integers(0, 3))
    return labels, T, begin, row + 4


def align_corpus():
    """For the owner map: adjacent equal units, an utterance the drop rule takes (two frames for four units), gaps between the utterances
    and rows outside all of them."""
    labels = [[0, 1, 2], [3, 3, 1], [0, 1, 2, 3], [4, 0, 2], [2], [1, 1, 1, 4]]
    T = np.array([40, 25, 2, 33, 5, 38], dtype=np.int32)
    begin = np.array([75, 5, 42, 120, 160, 170], dtype=np.int64)
    return labels, T, begin, 215


def model_for(J, M, D, seed):
    """A (J, M, D) model whose states lie apart"""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((J, M, D)) * 3
    var = 0.5 + rng.random((J, M, D))
    w = rng.random((J, M)) + 0.2
    return mean, var, w / w.sum(axis=1, keepdims=True)
