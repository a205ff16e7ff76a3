"""Phonetic decision trees (row f16): the host side of Engine.tree_build.

triphone_events   the labels of a corpus -> the distinct contexts (event_ctx) and the event of every label position (label_event)
questions         unit sets -> the membership table q_member
Tree              the node arrays of a build: lookup of any context (seen in training or not), the (L, P) tied-state ids of a
                  label for make_sentence_batch(unit_state_ids=...), save / load as one .npz of arrays

The rule (rows, questions, roots, greedy growth) is stated in include/poccala_hip.h; candidate c = pos * Q + qi with pos 0 left,
1 centre, 2 right, and the value n_units stands for "no neighbour" (utterance edge)."""
import numpy as np


def triphone_events(unit_ids, n_units):
    """unit_ids: one sequence of unit indices per utterance.  Returns (event_ctx (E, 3) int32, the distinct (left, centre, right)
    in lexicographic order, label_event (sum L_u,) int32: the row of event_ctx of every label position, utterance after utterance).
    The neighbour of an utterance's first / last unit is the edge symbol n_units."""
    n_units = int(n_units)
    ctx = []
    for lab in unit_ids:
        lab = np.asarray(lab, dtype=np.int64).reshape(-1)
        if lab.size and (lab.min() < 0 or lab.max() >= n_units):
            raise ValueError('a label names a unit outside [0, %d)' % n_units)
        left = np.concatenate([[n_units], lab[:-1]])
        right = np.concatenate([lab[1:], [n_units]])
        ctx.append(np.stack([left, lab, right], axis=1))
    ctx = np.concatenate(ctx, axis=0) if ctx else np.zeros((0, 3), dtype=np.int64)
    if ctx.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32)
    event_ctx, label_event = np.unique(ctx, axis=0, return_inverse=True)
    return np.ascontiguousarray(event_ctx, dtype=np.int32), np.ascontiguousarray(label_event.reshape(-1), dtype=np.int32)


def questions(sets, n_units):
    """sets: one collection of unit ids per question (the edge symbol n_units may be a member).  Returns q_member (Q, n_units + 1) uint8."""
    n_units = int(n_units)
    q = np.zeros((len(sets), n_units + 1), dtype=np.uint8)
    for i, s in enumerate(sets):
        s = np.asarray(sorted(set(int(x) for x in s)), dtype=np.int64)
        if s.size and (s.min() < 0 or s.max() > n_units):
            raise ValueError('question %d names a unit outside [0, %d]' % (i, n_units))
        q[i, s] = 1
    return q


class Tree(object):
    """The node arrays of a build.  node_cand (N,) candidate or -1 at leaves, node_child (N, 2) = (no, yes) or -1, node_state (N,) tied id
    or -1, node_n (N,) int64, split_gain in split order, row_state (E P,) the tied id of every statistics row, event_ctx (E, 3),
    q_member (Q, n_units + 1), root_of (n_units P,), leaf_n / leaf_s / leaf_q the leaves' sums."""
    FIELDS = ('node_cand', 'node_child', 'node_state', 'node_n', 'split_gain', 'row_state', 'event_ctx', 'q_member', 'root_of', 'leaf_n',
              'leaf_s', 'leaf_q')

    def __init__(self, P, n_units, **arrays):
        self.P, self.n_units = int(P), int(n_units)
        for f in self.FIELDS:
            setattr(self, f, np.asarray(arrays[f]))
        self.Q = int(self.q_member.shape[0])
        self.n_nodes = int(self.node_cand.shape[0])
        self.n_states = int((self.node_state >= 0).sum())

    def lookup(self, left, centre, right, k):
        """The tied state of position k of `centre` between `left` and `right` (n_units = utterance edge): a walk from the root."""
        ctx = (int(left), int(centre), int(right))
        if not (0 <= ctx[1] < self.n_units and 0 <= ctx[0] <= self.n_units and 0 <= ctx[2] <= self.n_units and 0 <= int(k) < self.P):
            raise ValueError('context %s, position %d: outside the inventory' % (ctx, k))
        node = int(self.root_of[ctx[1] * self.P + int(k)])
        while self.node_cand[node] >= 0:
            pos, qi = divmod(int(self.node_cand[node]), self.Q)
            node = int(self.node_child[node, 1 if self.q_member[qi, ctx[pos]] else 0])
        return int(self.node_state[node])

    def unit_state_ids(self, unit_ids):
        """(L, P) int32 tied-state ids of one utterance's label, what embedded_row_states / make_sentence_batch(unit_state_ids=) take."""
        lab = [int(x) for x in np.asarray(unit_ids).reshape(-1)]
        out = np.empty((len(lab), self.P), dtype=np.int32)
        for i, c in enumerate(lab):
            left = lab[i - 1] if i > 0 else self.n_units
            right = lab[i + 1] if i + 1 < len(lab) else self.n_units
            for k in range(self.P):
                out[i, k] = self.lookup(left, c, right, k)
        return out

    @property
    def n_roots(self):
        """R0: the nodes 0 .. R0 - 1 are the roots (every root has a (centre, k) that maps to it)."""
        return int(self.root_of.max()) + 1

    def tying_arrays(self):
        """What Engine.load_tying hands to pcl_tying_upload, C-contiguous: (q_member uint8 (Q, n_units + 1), node_cand, node_child (N, 2),
        node_state, root_of int32)."""
        return (np.ascontiguousarray(self.q_member, dtype=np.uint8), np.ascontiguousarray(self.node_cand, dtype=np.int32),
                np.ascontiguousarray(self.node_child, dtype=np.int32).reshape(-1, 2), np.ascontiguousarray(self.node_state, dtype=np.int32),
                np.ascontiguousarray(self.root_of, dtype=np.int32).reshape(-1))

    def save(self, path):
        """One .npz holding arrays only."""
        np.savez(path, P=np.int64(self.P), n_units=np.int64(self.n_units), **{f: getattr(self, f) for f in self.FIELDS})

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(int(z['P']), int(z['n_units']), **{f: z[f] for f in cls.FIELDS})
