"""NumPy twin of pcl_batch_align_segments (csrc/hmm_dp.hip: hmm_align_segments_kernel): Viterbi paths of label-built sentence HMMs ->
the owner map pcl_seg_create sorts by, and the dropped utterances (multi_process_data(init=False), AcousticModel.py:736-764).
Written from the rules, one utterance at a time; tests/test_realign_twin.py holds it to the oracle's regroup_frame_states /
discriminate on golden G12.  Integer work only: every comparison against it is exact."""
import numpy as np


def row_positions(path, L, gmm_num):
    """Label position of every HMM row on the path: row 0 (entry) -> 0, rows 1 .. gmm_num L -> (row - 1) // gmm_num, row N - 1 (exit) -> L - 1."""
    path = np.asarray(path, dtype=np.int64)
    N = gmm_num * L + 2
    assert path.size == 0 or (path.min() >= 0 and path.max() < N)
    return np.where(path == 0, 0, np.where(path == N - 1, L - 1, (path - 1) // gmm_num))


def frame_slices(unit_seq, gmm_num):
    """k[t]: a run = a maximal block of equal unit; a run of n frames is cut with chunk = n // gmm_num; chunk == 0 gives everything
    to the last state, otherwise k = min(pos // chunk, gmm_num - 1)."""
    unit_seq = np.asarray(unit_seq)
    k = np.empty(len(unit_seq), dtype=np.int64)
    edges = np.concatenate([[0], np.flatnonzero(unit_seq[1:] != unit_seq[:-1]) + 1, [len(unit_seq)]]) if len(unit_seq) else np.zeros(1, dtype=np.int64)
    for a, b in zip(edges[:-1], edges[1:]):
        n = b - a
        chunk = n // gmm_num
        k[a:b] = gmm_num - 1 if chunk == 0 else np.minimum(np.arange(n) // chunk, gmm_num - 1)
    return k


def is_dropped(path_units, label):
    """AcousticModel.py:751-757: fewer distinct units on the path than in the label."""
    return len(set(int(x) for x in path_units)) < len(set(int(x) for x in label))


def realign(paths, labels, S, T, begin, F):
    """(frame_state (F,) int32, dropped): frame_state[begin[u] + t] = unit * gmm_num + k for the frames of the kept utterances, -1
    for every other row; dropped = sorted utterance indices."""
    gmm_num = S - 2
    state = np.full(F, -1, dtype=np.int32)
    dropped = []
    for u, (path, lab) in enumerate(zip(paths, labels)):
        lab = np.asarray(lab, dtype=np.int64)
        path = np.asarray(path)
        assert len(path) == T[u]
        units = lab[row_positions(path, len(lab), gmm_num)]
        if is_dropped(units, lab):
            dropped.append(u)
            continue
        state[begin[u]:begin[u] + T[u]] = units * gmm_num + frame_slices(units, gmm_num)
    return state, dropped
