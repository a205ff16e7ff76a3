"""NumPy twin of csrc/bootstrap.hip: the two model-free steps the reference's training schemes begin with, restated from
AcousticModel.py:479-517 (flat start) and :605-644 (uniform segmentation), pinned to the reference itself by golden G20
(tests/golden/make_golden_bootstrap.py).  The GPU tests compare the device with these functions on random ragged batches."""
import numpy as np

VAR_FLOOR = 1e-4            # cal_variance, Clustering.py:829-830


def sample_rows(T, begin, n_utts, step):
    """Rows of the frame matrix that data[::step] of the first n_utts utterances selects, concatenated (:492-498)."""
    rows = [np.arange(0, int(T[u]), int(step), dtype=np.int64) + int(begin[u]) for u in range(int(n_utts))]
    return np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)


def moments(frames, T, begin, n_utts, step):
    """(mean, var, n) of the sample: the k = 1 result of ClusterInitialization.kmeans(algorithm=1, cov_matrix=True) (:499-501)."""
    x = np.asarray(frames)[sample_rows(T, begin, n_utts, step)].astype(np.float64)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    var = np.sqrt(np.maximum(var, VAR_FLOOR)) ** 2
    return mean, var, len(x)


def flat_model(mean, var, coeff, J, M):
    """(mean (J,M,D), var (J,M,D), weight (J,M)) of the flat-start model (:504-516); coeff (M,) or None."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    c = np.zeros((M, 1)) if coeff is None else np.asarray(coeff, dtype=np.float64).reshape(M, 1)
    g_mean = mean[None, :].repeat(M, axis=0) + c * var
    g_var = var[None, :].repeat(M, axis=0)
    return (np.ascontiguousarray(np.broadcast_to(g_mean, (J,) + g_mean.shape)), np.ascontiguousarray(np.broadcast_to(g_var, (J,) + g_var.shape)),
            np.full((J, M), 1.0 / M))


def uniform_map(F, labels, T, begin, gmm_num):
    """frame_state (F,) int32 of uniform segmentation: labels[u] = unit ids of utterance u.  __eq_segment mode 'e' (:605-612) then
    mode 'g' inside every chunk (:613-625)."""
    state = np.full(int(F), -1, dtype=np.int32)
    for u, lab in enumerate(labels):
        if len(lab) == 0:
            continue
        chunk = int(T[u]) // len(lab)
        c2 = chunk // gmm_num
        for i, unit in enumerate(lab):
            lo = int(begin[u]) + i * chunk
            for k in range(gmm_num):
                a = k * c2
                b = (k + 1) * c2 if k < gmm_num - 1 else chunk
                state[lo + a:lo + b] = int(unit) * gmm_num + k
    return state
