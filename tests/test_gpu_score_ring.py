"""The split-f16 scoring kernel stages its parameters through a ring of R LDS stages of MTS m-tiles each (PCL_SPLIT16_RING,
PCL_SPLIT16_MTS in gmm_score_split.hip; shipped: 2 x 2): a stage is refilled R - 1 stages ahead of its use, a wave waits for the
oldest stage (with a counted vmcnt where R > 2), and there is one workgroup barrier per stage.  Scoring through the batch API in f32 mode against
oracle.poccala_oracle.gmm_point at the shapes where a ring breaks:

  m-tiles per state   1, 2, 3, R MTS - 1, R MTS, R MTS + 1, 2 R MTS + 1 for the shipped layout and for every other layout the
                      knobs reach within three workgroups per CU (LAYOUTS): fewer tiles than the ring has stages (no DMA for a
                      stage that does not exist), exactly one round, one tile into the second round (the first refill of a buffer),
                      two rounds and one; even counts have a padded last tile.
  frames per state    1, 63, 64, 65, 255, 256, 257: a partial wave, inactive waves (which still issue their share of every stage
                      and meet every barrier), a full workgroup, and a second workgroup with one frame.
  D                   13, 26, 39 (4, 8, 10 chunks per m-tile: the waves' shares of a stage are equal or differ by one, which is
                      what the counted wait depends on) and 47 (the double buffer kept); 39 also with two workgroups per CU.
  split states        on-pipe tile counts 0, 1 and R MTS + 1 side by side in one launch.
  a flagged tile      a frame 400 sigma from every mean: the flag of the features is stored behind the FIRST barrier of the ring,
                      and the direct-form fix-up that reads it must still rescore the tile.

Every case scores twice on the same batch and holds the two results bit for bit: a stage refilled before every wave was done
with it, or read before it landed, depends on timing and shows as a difference between launches.  The bounds are those of
tests/test_gpu_parity.py for ln b, through tests/_parity.hold: 5e-5 absolute; 5e-6 relative beside it where |ln b| is huge
(the outlier frame) or mixtures are scored off the pipe (plus their f32 evaluation bound)."""
import os

import numpy as np
import pytest

from _parity import hold
from oracle import poccala_oracle as po

pytestmark = pytest.mark.gpu

F32_LOGLIK_ATOL = 5e-5          # tests/test_gpu_parity.py
RING, MTS = 2, 2                # the shipped layout
LAYOUTS = [(RING, MTS), (2, 1), (3, 1), (4, 1), (5, 1)]
TILE_COUNTS = sorted({1, 2, 3} | {n for r, m in LAYOUTS for n in (r * m - 1, r * m, r * m + 1, 2 * r * m + 1)})
LENS = [1, 63, 64, 65, 255, 256, 257]


def mixtures(n_tiles):
    """n_tiles m-tiles: full ones for odd counts, a padded last tile for even ones"""
    return 32 * n_tiles - (7 if n_tiles % 2 == 0 else 0)


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def random_states(rng, J, M, D):
    mean = rng.standard_normal((J, M, D)) * 0.5
    var = rng.uniform(0.5, 2.0, (J, M, D))
    w = rng.uniform(0.5, 1.5, (J, M))
    return mean, var, w / w.sum(axis=1, keepdims=True)


def score_twice(eng, mean, var, w, x, lens):
    """state j scored for its own lens[j] frames, twice on one batch: the rows of the first launch, after holding the second to them"""
    from poccala_amd import PCL_F32
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    eng.load_model(mean, var, w)
    eng.load_frames(x)
    b = eng.batch([3] * len(lens), lens, begin.tolist())
    b.set_states([np.array([-1, j, -2], dtype=np.int32) for j in range(len(lens))])
    b.score(PCL_F32)
    first = [np.array(u, copy=True) for u in b.get('B')]
    b.score(PCL_F32)
    second = b.get('B')
    b.close()
    for j, (u, v) in enumerate(zip(first, second)):
        assert np.all(u[0] == 0.0) and np.all(np.isneginf(u[-1]))
        assert np.array_equal(u, v), 'state %d: two launches on the same batch differ' % j
    return [u[1] for u in first], begin


@pytest.mark.parametrize('D', [39, 13, 26, 47])
@pytest.mark.parametrize('n_tiles', TILE_COUNTS)
def test_ring_tile_counts_and_lengths(eng, n_tiles, D):
    rng = np.random.default_rng(2200 + 100 * n_tiles + D)
    M = mixtures(n_tiles)
    mean, var, w = random_states(rng, len(LENS), M, D)
    x = (rng.standard_normal((sum(LENS), D)) * 0.6).astype(np.float32)
    got, begin = score_twice(eng, mean, var, w, x, LENS)
    for j, T in enumerate(LENS):
        ref = po.gmm_point(x[begin[j]:begin[j] + T].astype(np.float64), mean[j], var[j], w[j])
        hold('score ring %d m-tiles D=%d' % (n_tiles, D), 'ln b (%d frames)' % T, got[j], ref, 0.0, F32_LOGLIK_ATOL)


@pytest.mark.parametrize('n_tiles', [RING * MTS + 1, 2 * RING * MTS + 1])
def test_ring_with_two_workgroups_per_cu(eng, n_tiles):
    """pcl_score_occupancy(ctx, 2) pads a workgroup's LDS to 56 KB beside the ring"""
    rng = np.random.default_rng(2290 + n_tiles)
    M, D = mixtures(n_tiles), 39
    mean, var, w = random_states(rng, len(LENS), M, D)
    x = (rng.standard_normal((sum(LENS), D)) * 0.6).astype(np.float32)
    eng.score_occupancy(2)
    try:
        got, begin = score_twice(eng, mean, var, w, x, LENS)
    finally:
        eng.score_occupancy(0)
    for j, T in enumerate(LENS):
        ref = po.gmm_point(x[begin[j]:begin[j] + T].astype(np.float64), mean[j], var[j], w[j])
        hold('score ring two workgroups per CU, %d m-tiles' % n_tiles, 'ln b (%d frames)' % T, got[j], ref, 0.0, F32_LOGLIK_ATOL)


def test_ring_split_states_with_0_1_and_a_round_plus_one_tiles():
    """On-pipe tile counts 0, R MTS + 1, 1, 0, R MTS + 1 in one launch: states 0 and 3 have every mixture tight enough to leave the
    matrix pipe (PCL_COARSE_SPLIT_MAX=1 keeps them split, as tests/test_gpu_score_schedule.py does), state 2 all but 20, states 1
    and 4 none.  Bound: 5e-5 for the ordinary states; with mixtures off the pipe 5e-5 + the f32 evaluation bound of the direct
    form, 5e-6 relative (tests/test_gpu_parity.py, tests/test_gpu_coarse.py)."""
    from poccala_amd import Engine
    from _oracle_pool import f32_evaluation_bound_rows
    rng = np.random.default_rng(2207)
    n_full = RING * MTS + 1
    M, D = 32 * n_full, 39
    lens = [65, 257, 255, 64, 1]
    tight = [M, 0, M - 20, M, 0]
    mean, var, w = random_states(rng, len(lens), M, D)
    for j, n in enumerate(tight):
        idx = rng.choice(M, n, replace=False)
        var[j, idx] = (10.0 ** rng.uniform(-6, -3, n))[:, None] * rng.uniform(0.5, 2.0, (n, D))
    xs = []
    for j, T in enumerate(lens):                     # frames of the state's own mixtures, so that ln b is finite and sizeable
        comp = rng.integers(0, M, T)
        xs.append(mean[j, comp] + np.sqrt(var[j, comp]) * rng.standard_normal((T, D)))
    x = np.concatenate(xs).astype(np.float32)
    old = os.environ.get('PCL_COARSE_SPLIT_MAX')
    os.environ['PCL_COARSE_SPLIT_MAX'] = '1.0'
    try:
        e = Engine(0)
    finally:
        if old is None:
            del os.environ['PCL_COARSE_SPLIT_MAX']
        else:
            os.environ['PCL_COARSE_SPLIT_MAX'] = old
    try:
        got, begin = score_twice(e, mean, var, w, x, lens)
        n_off, limit = e.model_split_info()
        assert limit == M and np.array_equal(n_off, tight)                 # on-pipe tiles: 0, n_full, 1, 0, n_full
        for j, T in enumerate(lens):
            xj = x[begin[j]:begin[j] + T]
            ref = po.gmm_point(xj.astype(np.float64), mean[j], var[j], w[j])
            if tight[j] == 0:
                hold('score ring split states', 'ln b, every mixture on the pipe', got[j], ref, 0.0, F32_LOGLIK_ATOL)
            else:
                bound = f32_evaluation_bound_rows([(mean[j], var[j], w[j])], xj)[0]
                hold('score ring split states', 'ln b, %d of %d mixtures off the pipe' % (tight[j], M), got[j], ref, 5e-6, F32_LOGLIK_ATOL + bound)
    finally:
        e.close()


def test_ring_flagged_tile_is_rescored(eng):
    """Frames 17 (first workgroup) and 256 (second) of state 0 lie 400 sigma from every mean: their scaled features leave the f16 range,
    the kernel clamps them and flags the tile, and the direct-form fix-up rescored it in the same call -- a lost flag leaves the clamped
    value standing, some 1e4 nats off.  State 1 beside it has no such frame.  Bound of the outlier test of tests/test_gpu_parity.py."""
    rng = np.random.default_rng(2213)
    M, D = mixtures(RING * MTS + 1), 39
    lens = [257, 65]
    mean, var, w = random_states(rng, 2, M, D)
    x = (rng.standard_normal((sum(lens), D)) * 0.6).astype(np.float32)
    far = 400.0 * np.sqrt(var[0].max())
    for t in (17, 256):
        x[t] = 0.0
        x[t, 3] = far + np.abs(mean[0, :, 3]).max()
    got, begin = score_twice(eng, mean, var, w, x, lens)
    for j, T in enumerate(lens):
        ref = po.gmm_point(x[begin[j]:begin[j] + T].astype(np.float64), mean[j], var[j], w[j])
        if j == 0:
            assert np.isfinite(got[j]).all() and ref[17] < -4.0e4 and ref[256] < -4.0e4
        hold('score ring flagged tile', 'ln b (state %d)' % j, got[j], ref, 5e-6 if j == 0 else 0.0, F32_LOGLIK_ATOL)
