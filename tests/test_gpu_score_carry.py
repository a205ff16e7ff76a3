"""The split-f16 scoring kernel runs one frame tile's MFMA chain at a time and carries the log-sum-exp of the LAST frame tile of an m-tile
under the first chain of the next m-tile (PCL_SPLIT16_CARRY in gmm_score_split.hip, the D <= 39 kernels): tile 1's accumulator lives across
the m-tile boundary -- and across the ring's wait and barrier at a stage boundary -- its sum and reference are settled between the next
m-tile's two chains, and the last m-tile's tile 1 is finished behind the loop.  Scoring through the batch API in f32 mode against
oracle.poccala_oracle.gmm_point at the shapes where that order can go wrong:

  m-tiles per state   1 (nothing to carry), 2 (a carry inside a stage of two m-tiles, also as 33 mixtures: a padded second tile), 3 (a carry
                      across the stage barrier, the last stage one m-tile), 5 (both, twice).
  frames per state    1 (a wave with only tile 0 valid), 33 (tile 1 with one frame), 64, 65 (a second wave), 129 (inactive waves, which run
                      no chain and no tail), 257 (a second workgroup).
  D                   13, 26, 39 (6, 12, 15 MFMA gaps per chain for the 32 operations), 47 (the order unchanged).
  a late first value  the first 32, 64 or 128 mixtures of a state have weight 0, log zero for every frame: tile 1's reference, and the write
                      of the frame operand's spare slot that the NEXT chain of tile 1 subtracts, arrive in m-tile 1, 2 or 4 -- inside a
                      stage, behind a barrier, or in the last m-tile, which only the tail behind the loop settles.
  an overflowing sum  frames 32..63 of a state are tile 1: the construction of tests/test_gpu_parity.py (best mixture in the third tile,
                      more than 88.7 nats above the first, a runner-up summed before it) and weights rising by e^100 per m-tile (a rescale
                      at every carried settle).
  split states        on-pipe tile counts 0 (the early return), 1 and 3 below the layout's full count, side by side in one launch.

Every case scores twice on one batch and holds the two results bit for bit.  Bounds: tests/test_gpu_parity.py's for ln b through
tests/_parity.hold: 5e-5 absolute; beside it 5e-6 relative and the f32 evaluation bound where frames lie far out or mixtures leave the pipe."""
import os

import numpy as np
import pytest

from _parity import hold
from oracle import poccala_oracle as po

pytestmark = pytest.mark.gpu

F32_LOGLIK_ATOL = 5e-5          # tests/test_gpu_parity.py
LENS = [1, 33, 64, 65, 129, 257]
MIXTURES = [32, 33, 64, 96, 160]            # 1, 2 (padded), 2, 3, 5 m-tiles


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


def oracle_rows(x, begin, lens, mean, var, w):
    with np.errstate(divide='ignore'):
        return [po.gmm_point(x[begin[j]:begin[j] + T].astype(np.float64), mean[j], var[j], w[j]) for j, T in enumerate(lens)]


@pytest.mark.parametrize('D', [39, 13, 26, 47])
@pytest.mark.parametrize('M', MIXTURES)
def test_carry_tile_counts_and_lengths(eng, M, D):
    rng = np.random.default_rng(2800 + 10 * M + D)
    mean, var, w = random_states(rng, len(LENS), M, D)
    x = (rng.standard_normal((sum(LENS), D)) * 0.6).astype(np.float32)
    got, begin = score_twice(eng, mean, var, w, x, LENS)
    for j, ref in enumerate(oracle_rows(x, begin, LENS, mean, var, w)):
        hold('score carry M=%d D=%d' % (M, D), 'ln b (%d frames)' % LENS[j], got[j], ref, 0.0, F32_LOGLIK_ATOL)


@pytest.mark.parametrize('D', [39, 13])
@pytest.mark.parametrize('M,n_zero', [(64, 32), (96, 32), (96, 64), (160, 64), (160, 128)])
def test_carry_first_value_arrives_late(eng, M, n_zero, D):
    """The first n_zero mixtures carry weight 0: no frame has a reference before m-tile n_zero / 32, where tile 1 takes its own between the
    two chains of the m-tile after (M = 96, 32 and M = 160, 64: that settle follows a stage barrier) or, when that m-tile is the last
    (64, 32; 96, 64; 160, 128), in the tail behind the loop.  State 1 beside it has every weight."""
    rng = np.random.default_rng(2850 + M + n_zero + D)
    lens = [65, 257, 33]
    mean, var, w = random_states(rng, len(lens), M, D)
    w[0, :n_zero] = 0.0
    w[2, :n_zero] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    x = (rng.standard_normal((sum(lens), D)) * 0.6).astype(np.float32)
    got, begin = score_twice(eng, mean, var, w, x, lens)
    for j, ref in enumerate(oracle_rows(x, begin, lens, mean, var, w)):
        assert np.isfinite(got[j]).all()
        hold('score carry late first value M=%d zero=%d D=%d' % (M, n_zero, D), 'ln b (state %d)' % j, got[j], ref, 0.0, F32_LOGLIK_ATOL)


def far_frame_problem(gap, runner_up, R=30.0, M=96, D=39, T=70, seed=0):
    """tests/test_gpu_parity.py's: mixtures near the state's centre, frames R sigma out along one direction, so that the first tile lies `gap`
    nats below the best mixture (third tile) and a runner-up `runner_up` below it (second tile).  70 frames: 32..63 are the wave's tile 1."""
    rng = np.random.default_rng(seed)
    e = np.zeros(D)
    e[0] = 1.0
    C, p_best = 3.2, 3.0
    p = np.full(M, p_best - (gap + 40.0) / R)
    p[:32] = p_best - gap / R - rng.uniform(0, 0.3, 32) / R
    p[40] = p_best - runner_up / R
    p[77] = p_best
    u = rng.standard_normal((M, D))
    u[:, 0] = 0.0
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    mean = (p[:, None] * e[None, :] + np.sqrt(C * C - p * p)[:, None] * u)[None]
    var = np.ones((1, M, D))
    w = np.full((1, M), 1.0 / M)
    x = (R * e[None, :] + 0.003 * rng.standard_normal((T, D))).astype(np.float32)
    return mean, var, w, x


@pytest.mark.parametrize('gap,runner_up', [(89.2, 1.0), (90.0, 2.0), (130.0, 1.0)])
def test_carry_sum_overflows_in_tile_1(eng, gap, runner_up):
    """The sum of tile 1 overflows f32 in the third and last m-tile of three: the vote on the carried sum, the move of the reference and the
    rescale in two half-steps all run in the tail behind the loop.  Bound of the test this construction comes from: 5e-6 relative + 5e-5 +
    the f32 evaluation bound."""
    from _oracle_pool import f32_evaluation_bound_rows
    mean, var, w, x = far_frame_problem(gap, runner_up)
    got, begin = score_twice(eng, mean, var, w, x, [len(x)])
    ref = oracle_rows(x, begin, [len(x)], mean, var, w)[0]
    bound = f32_evaluation_bound_rows([(mean[0], var[0], w[0])], x)[0]
    hold('score carry overflow in tile 1, gap %g' % gap, 'ln b', got[0], ref, 5e-6, F32_LOGLIK_ATOL + bound)


@pytest.mark.parametrize('M', [64, 96, 160])
def test_carry_rescale_at_every_settle(eng, M):
    """Weights e^100 apart from one m-tile to the next (tests/test_gpu_score_schedule.py's 'rising' kind): every settle of a carried sum
    takes the slow path, moves the reference and rewrites the spare slot that the next chain of that frame tile reads."""
    rng = np.random.default_rng(2870 + M)
    D, lens = 39, [33, 65, 129]
    mean, var, w = random_states(rng, len(lens), M, D)
    tile = np.arange(M) // 32
    lw = np.log(w) - 100.0 * (tile.max() - tile)[None]
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    x = (rng.standard_normal((sum(lens), D)) * 0.6).astype(np.float32)
    got, begin = score_twice(eng, mean, var, w, x, lens)
    for j, ref in enumerate(oracle_rows(x, begin, lens, mean, var, w)):
        hold('score carry rising weights M=%d' % M, 'ln b (%d frames)' % lens[j], got[j], ref, 0.0, F32_LOGLIK_ATOL)


def test_carry_split_states_with_0_1_and_3_tiles_on_the_pipe():
    """On-pipe tile counts 0, 5, 1, 3, 5 in one launch of a five-tile layout: state 0 has every mixture tight enough to leave the matrix pipe
    (the early return: no chain, no tail), state 2 all but 20, state 3 all but 70 (PCL_COARSE_SPLIT_MAX=1 keeps them split, as
    tests/test_gpu_score_ring.py does), states 1 and 4 none.  Bound: 5e-5 for the ordinary states; with mixtures off the pipe 5e-5 + the
    f32 evaluation bound of the direct form, 5e-6 relative."""
    from poccala_amd import Engine
    from _oracle_pool import f32_evaluation_bound_rows
    rng = np.random.default_rng(2880)
    M, D = 160, 39
    lens = [65, 257, 129, 64, 33]
    tight = [M, 0, M - 20, M - 70, 0]
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
        assert limit == M and np.array_equal(n_off, tight)                 # on-pipe tiles: 0, 5, 1, 3, 5
        for j, ref in enumerate(oracle_rows(x, begin, lens, mean, var, w)):
            if tight[j] == 0:
                hold('score carry split states', 'ln b, every mixture on the pipe', got[j], ref, 0.0, F32_LOGLIK_ATOL)
            else:
                bound = f32_evaluation_bound_rows([(mean[j], var[j], w[j])], x[begin[j]:begin[j] + lens[j]])[0]
                hold('score carry split states', 'ln b, %d of %d mixtures off the pipe' % (tight[j], M), got[j], ref, 5e-6, F32_LOGLIK_ATOL + bound)
    finally:
        e.close()
