"""The NumPy twin of the device realignment (tests/_realign_twin.py) against the oracle's regroup_frame_states / discriminate /
eq_segment_g, which golden G12 pins to the reference's own discriminate / __eq_segment / __get_gmmdata (tests/test_regroup_oracle.py);
the drop rule on hand-made paths; and the new entry point's presence in the built library.  No GPU."""
import os

import numpy as np

import _realign_twin as rt
from oracle import poccala_oracle as po

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'G12_regroup.npz'))


def sentence_of(seq):
    """A label and a Viterbi path that give the unit sequence `seq`: one label position per run, the path on the position's first row."""
    names = sorted(set(seq))
    ids = np.array([names.index(x) for x in seq])
    starts = np.concatenate([[0], np.flatnonzero(ids[1:] != ids[:-1]) + 1])
    label = ids[starts]
    pos = np.cumsum(np.concatenate([[0], (ids[1:] != ids[:-1]).astype(int)]))
    return names, ids, label, pos


def test_slices_match_the_oracle_on_the_golden_sequences():
    for ci in range(int(G['n_cases'])):
        seq = G['d_seq_%d' % ci]
        assert np.array_equal(rt.frame_slices(seq, 3), po.regroup_frame_states(seq, 3))
        for gmm_num in (1, 2, 3, 4):
            assert np.array_equal(rt.frame_slices(seq, gmm_num), po.regroup_frame_states(seq, gmm_num))


def test_slices_match_the_oracle_on_random_sequences():
    rng = np.random.default_rng(0)
    for _ in range(200):
        runs = rng.integers(1, 12, size=rng.integers(1, 9))
        seq = np.repeat(rng.integers(0, 4, size=len(runs)), runs)          # equal neighbours merge into one run
        gmm_num = int(rng.integers(1, 5))
        assert np.array_equal(rt.frame_slices(seq, gmm_num), po.regroup_frame_states(seq, gmm_num))


def test_realign_matches_discriminate_and_eq_segment_on_the_golden_sequences():
    for S in (5, 4):
        gmm_num = S - 2
        for ci in range(int(G['n_cases'])):
            seq = G['d_seq_%d' % ci]
            names, ids, label, pos = sentence_of(seq)
            T = len(seq)
            for first_row in range(gmm_num):                                # whichever row of the position the path sits on
                path = 1 + pos * gmm_num + first_row
                path[0] = 0                                                 # the entry row belongs to position 0 ...
                if pos[-1] == len(label) - 1:
                    path[-1] = gmm_num * len(label) + 1                     # ... and the exit row to the last
                state, dropped = rt.realign([path], [label], S, [T], [4], T + 9)
                assert dropped == []
                assert (state[:4] == -1).all() and (state[4 + T:] == -1).all()
                own = state[4:4 + T]
                assert np.array_equal(own // gmm_num, ids)
                for unit in names:
                    for loc in po.discriminate(unit, seq):
                        sizes = [len(s) for s in po.eq_segment_g(loc, gmm_num)]
                        assert np.array_equal(own[loc] % gmm_num, np.repeat(np.arange(gmm_num), sizes))


def test_row_positions():
    assert rt.row_positions([0, 1, 2, 3, 4, 5, 6, 7], 2, 3).tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert rt.row_positions([0, 1, 2, 3, 4, 5], 2, 2).tolist() == [0, 0, 0, 1, 1, 1]
    assert rt.row_positions([0, 4], 1, 3).tolist() == [0, 0]


def test_drop_rule_on_hand_made_paths():
    S, g = 5, 3
    row = lambda p, k=0: 1 + p * g + k
    # one label unit missed: label a b c, the path never enters c
    lab = [0, 1, 2]
    st, dr = rt.realign([[row(0), row(0, 1), row(1), row(1, 2)]], [lab], S, [4], [0], 4)
    assert dr == [0] and (st == -1).all()
    st, dr = rt.realign([[row(0), row(1), row(2), row(2, 1)]], [lab], S, [4], [0], 4)
    assert dr == [] and (st // g).tolist() == [0, 1, 2, 2]
    # adjacent repeat a a b: two distinct units; the second a need not be visited, and a a is ONE run when it is
    lab = [5, 5, 1]
    st, dr = rt.realign([[row(0), row(0, 1), row(2), row(2)]], [lab], S, [4], [0], 4)
    assert dr == [] and (st // g).tolist() == [5, 5, 1, 1]
    path = [row(0), row(0), row(0), row(1), row(1), row(1), row(2)]
    st, dr = rt.realign([path], [lab], S, [7], [0], 7)
    assert dr == [] and st.tolist() == [15, 15, 16, 16, 17, 17, 1 * g + 2]          # one run of 6: chunk 2; a run of 1: last state
    st, dr = rt.realign([[row(0), row(1)]], [lab], S, [2], [0], 2)                  # b missed
    assert dr == [0]
    # non-adjacent repeat a b a: two distinct units, two runs of a
    lab = [3, 4, 3]
    path = [row(0), row(0), row(0), row(1), row(2), row(2), row(2)]
    st, dr = rt.realign([path], [lab], S, [7], [0], 7)
    assert dr == [] and st.tolist() == [9, 10, 11, 4 * g + 2, 9, 10, 11]
    st, dr = rt.realign([[row(0), row(1)]], [lab], S, [2], [0], 2)                  # the last a not visited: a was, nothing is missed
    assert dr == [] and st.tolist() == [3 * g + 2, 4 * g + 2]
    st, dr = rt.realign([[row(0), row(2)]], [lab], S, [2], [0], 2)                  # positions 0 and 2 are ONE run of a; b missed
    assert dr == [0]
    # several utterances: the indices of the dropped ones, sorted; the others keep their rows
    st, dr = rt.realign([[row(0)], [row(0), row(1)], [row(0)]], [[0, 1], [0, 1], [2, 1]], S, [1, 2, 1], [5, 0, 3], 7)
    assert dr == [0, 2] and st.tolist() == [2, 1 * g + 2, -1, -1, -1, -1, -1]


def test_the_entry_point_is_declared_and_exported():
    import poccala_amd._lib as L
    assert 'pcl_batch_align_segments' in L.PROTOTYPES
    assert hasattr(L.load(), 'pcl_batch_align_segments')
