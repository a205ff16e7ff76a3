"""NumPy twin of the resident tying and of label-built batches over tied states (row f17; csrc/tying.hip), and the trees and corpora the
tests share.  Built from ContextTree.Tree.lookup (the walk), tests/_realign_twin.py (row -> position, runs, slices, the drop rule) and
tests/_tree_twin.py (the statistics).  Integer work only: every comparison against it is for equality.  tests/test_tied_twin.py proves on
the CPU that every tree and corpus below reaches the edge it claims; tests/test_gpu_tied_batches.py runs them on the device, and
tests/test_gpu_tying_wide.py the inventories of 31 to 96 units, whose questions take up to four words of the bit table."""
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


# ------------------------------------------------------------------ wide inventories: more than one table word per question
def words(n_units):
    """tying_words of tying_check.h, restated: 32-bit words per question, bit u of a row for u in [0, n_units]"""
    return (n_units + 1 + 31) // 32


def wide_follower(k, n_units):
    """chain_follower for an inventory of 65 .. 127 units (W = 3 or 4).  The first stands between two utterance edges (the last word of a
    row), the second has its left neighbour at bit 31 of word 1, the third at bit 0 of word 2; between them their neighbours and centres
    lie in every word (at 96 units: words 3 1 3, 1 0 0, 2 2 2)."""
    assert 65 <= n_units <= 127
    return [(n_units, 40, n_units), (63, 5, 31), (64, min(70, n_units - 1), min(95, n_units - 1))][k % 3]


def followers(tree):
    """The chain followers of a chain() or wide_chain() tree, one per state position"""
    f = wide_follower if getattr(tree, 'wide', False) else chain_follower
    return [f(k, tree.n_units) for k in range(tree.P)]


def wide_chain(P, n_units=96, Q=1024, n_levels=72, seed=11):
    """The chain tree over a large question set: one root per state position, n_levels levels below each.  The candidates of a chain are
    drawn without replacement from all 3 Q and always hold 3 Q - 1, question Q - 1 (the last table row) and question 0 at each of the
    three positions (those six in the last six levels).  wide_follower(k) stays on chain k to its last level, so the first follower reads
    the table's last word there, as a neighbour at the utterance edge.  The rows are random bits, so a unit and its aliases u +- 32 k
    disagree on about half of the questions, with two exceptions: the edge symbol is a member of question Q - 1 (the table's last word
    is not zero), and for every level a unit is made to agree with the follower on the levels above that ask the same position and to
    disagree on this one -- the follower with that unit in that position leaves the chain exactly there, so every leaf has a context
    (about 300 of the Q (n_units + 1) bits per chain and position are set for it)."""
    rng = np.random.default_rng(seed)
    qm = rng.integers(0, 2, size=(Q, n_units + 1)).astype(np.uint8)
    qm[Q - 1, n_units] = 1
    fol = [wide_follower(k, n_units) for k in range(P)]
    keep = sorted({u for f in fol for u in f})                     # the followers' own bits are never touched
    must = [pos * Q + qi for pos in range(3) for qi in (0, Q - 1)]
    assert 3 * Q - 1 in must
    rest = np.setdiff1d(np.arange(3 * Q), must)
    fixed = {}
    perms = []
    for k in range(P):
        # (the six candidates every chain shares come last: above them they would tie the made units of all chains to each other)
        perm = np.concatenate([rng.choice(rest, size=n_levels - len(must), replace=False), rng.permutation(must)])
        perms.append(perm)
        for pos in range(3):
            qs = [int(c) % Q for c in perm if int(c) // Q == pos]  # the questions this chain asks about this position, in level order
            f = fol[k][pos]
            free = [int(u) for u in rng.permutation(n_units + (pos != 1)) if u not in keep]
            for j, qj in enumerate(qs):
                want = [(q, int(qm[q, f])) for q in qs[:j]] + [(qj, 1 - int(qm[qj, f]))]
                u = next(u for u in free if all(fixed.get((q, u), v) == v for q, v in want))
                free.remove(u)
                for q, v in want:
                    qm[q, u] = v
                    fixed[(q, u)] = v
    assert ((qm.sum(axis=1) > 0) & (qm.sum(axis=1) <= n_units)).all()
    cand, child, state = [-1] * P, [[-1, -1] for _ in range(P)], [-1] * P
    nstate = 0
    for k in range(P):
        node = k
        for c in perms[k]:
            pos, qi = divmod(int(c), Q)
            go = int(qm[qi, fol[k][pos]])
            a, b = len(cand), len(cand) + 1
            cand += [-1, -1]
            child += [[-1, -1], [-1, -1]]
            state += [nstate, -1]
            nstate += 1
            cand[node] = int(c)
            child[node] = [a, b] if go == 1 else [b, a]
            node = b
        state[node] = nstate
        nstate += 1
    tree = _tree(P, n_units, qm, cand, child, state, np.tile(np.arange(P), n_units))
    tree.wide = True
    return tree


def walk_all(tree, k, ctx3=None):
    """The leaf NODE of every context's walk from position k's root, all walks at once (the contexts still walking shrink level by
    level).  Used to FIND contexts, never as the reference: that is Tree.lookup."""
    ctx = all_contexts_array(tree.n_units) if ctx3 is None else np.asarray(ctx3)
    node = tree.root_of[ctx[:, 1] * tree.P + k].astype(np.int64)
    live = np.flatnonzero(tree.node_cand[node] >= 0)
    while len(live):
        c = tree.node_cand[node[live]]
        yes = tree.q_member[c % tree.Q, ctx[live, c // tree.Q]]
        node[live] = tree.node_child[node[live], yes]
        live = live[tree.node_cand[node[live]] >= 0]
    return node


def all_contexts_array(n_units):
    """all_contexts, without the Python loop"""
    l, c, r = np.meshgrid(np.arange(n_units + 1), np.arange(n_units), np.arange(n_units + 1), indexing='ij')
    return np.stack([l.reshape(-1), c.reshape(-1), r.reshape(-1)], axis=1).astype(np.int32)


def leaf_witnesses(tree):
    """One context for every (state position, leaf) that any context of the inventory reaches"""
    ctx = all_contexts_array(tree.n_units)
    out = []
    for k in range(tree.P):
        _, first = np.unique(walk_all(tree, k, ctx), return_index=True)
        out.append(ctx[first])
    return np.concatenate(out)


BOUNDARY_UNITS = (0, 31, 32, 63, 64, 95, 96)


def context_sample(tree, n=4000, seed=5):
    """(about n, 3) int32: the followers, every unit once in each of the three positions, every pair of BOUNDARY_UNITS and the edge
    symbol as (left, right), a witness of every reachable leaf, and random contexts up to n."""
    rng = np.random.default_rng(seed)
    nu = tree.n_units
    rows = [tuple(f) for f in followers(tree)]
    for u in range(nu + 1):
        rows.append((u, int(rng.integers(nu)), int(rng.integers(nu + 1))))
        rows.append((int(rng.integers(nu + 1)), int(rng.integers(nu)), u))
        if u < nu:
            rows.append((int(rng.integers(nu + 1)), u, int(rng.integers(nu + 1))))
    edge = sorted({u for u in BOUNDARY_UNITS + (nu,) if u <= nu})
    rows += [(l, int(rng.integers(nu)), r) for l in edge for r in edge]
    rows += [tuple(int(x) for x in w) for w in leaf_witnesses(tree)]
    while len(rows) < n:
        rows.append((int(rng.integers(nu + 1)), int(rng.integers(nu)), int(rng.integers(nu + 1))))
    return np.array(rows, dtype=np.int32)


def packed(tree):
    """tying_pack's bit table, restated: Q W words as Python ints, bit u & 31 of word qi W + (u >> 5) = q_member[qi, u]"""
    W = words(tree.n_units)
    qb = [0] * (tree.Q * W)
    for qi, u in zip(*np.nonzero(tree.q_member)):
        qb[int(qi) * W + (int(u) >> 5)] |= 1 << (int(u) & 31)
    return qb


BROKEN = {1: 'the word index dropped: word qi W, bit u & 31', 2: 'stride W - 1, as if W = ceil(n_units / 32)', 3: 'stride 1',
          4: 'words at index >= 4096 read as 0: a staging copy that stops at the LDS limit', 5: 'the last word Q W - 1 reads as 0: a copy one short'}
LDS_WORDS = 4096                                                   # TY_QBITS_LDS / 4 of csrc/tying.hip


def table_walk(tree, qb, left, centre, right, k, mistake=0, reads=None):
    """tying_walk over the packed table in plain Python; mistake 1 .. 5: one of BROKEN, 0: none (then it is Tree.lookup).  reads: a set
    that takes (qi, u, answer) of every step."""
    W, Q = words(tree.n_units), tree.Q
    ctx, node = (left, centre, right), int(tree.root_of[centre * tree.P + k])
    while tree.node_cand[node] >= 0:
        pos, qi = divmod(int(tree.node_cand[node]), Q)
        u = ctx[pos]
        at = qi * W if mistake == 1 else qi * (W - 1) + (u >> 5) if mistake == 2 else qi + (u >> 5) if mistake == 3 else qi * W + (u >> 5)
        word = 0 if (mistake == 4 and at >= LDS_WORDS) or (mistake == 5 and at == Q * W - 1) else qb[at]
        yes = (word >> (u & 31)) & 1
        if reads is not None:
            reads.add((qi, u, yes))
        node = int(tree.node_child[node, yes])
    return int(tree.node_state[node])


def table_walk_all(tree, ctx3, mistake=0, reads=None):
    qb = packed(tree)
    return np.array([[table_walk(tree, qb, l, c, r, k, mistake, reads) for k in range(tree.P)] for l, c, r in np.asarray(ctx3).tolist()],
                    dtype=np.int32).reshape(-1, tree.P)


def applicable_mistakes(n_units, Q):
    """The BROKEN walks that read another bit than tying_walk somewhere in a (n_units, Q) table"""
    W = words(n_units)
    return ([1, 2, 3] if W >= 2 else []) + ([4] if Q * W > LDS_WORDS else []) + ([5] if Q * W == LDS_WORDS else [])


DEVICE_CASES = [(31, 24), (32, 24), (63, 24), (64, 24), (95, 24), (96, 1024), (96, 1025)]
_cases = {}


def device_case(n_units, Q, P):
    """(tree, sample, states of the sample by Tree.lookup) of one case the device runs; made once, shared, not to be written to"""
    key = (n_units, Q, P)
    if key not in _cases:
        tree = chain(P, n_units=n_units) if Q == CHAIN_Q else wide_chain(P, n_units=n_units, Q=Q)
        sample = context_sample(tree)
        want = lookup_all(tree, sample)
        sample.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (tree, sample, want)
    return _cases[key]


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
