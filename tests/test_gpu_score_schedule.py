"""The split-f16 scoring kernel's m-tile loop is scheduled by hand (fragment reads ahead of use, one frame tile's log-sum-exp
beside the next one's MFMAs): scoring through the batch API in f32 mode against oracle.poccala_oracle.gmm_point at the shapes
where a rotated loop breaks.

Mixtures 32 / 64 / 96 / 160 are 1 / 2 / 3 / 5 m-tiles (odd and even stage counts of the double buffer, and the one-tile case),
40 has a padded last tile.  Frames per state 1 / 63 / 64 / 65 / 255 / 256 / 257: a partial wave, inactive waves, full workgroups
and a second workgroup with one frame.  State kinds: random; the mixtures of the LAST m-tile e^100 above
the rest (the reference is re-taken late, and the running sum overflows f32 against the first one: the two-half-step rescale);
those of the FIRST m-tile above the rest (the slow path never runs after tile 0); 'rising', every m-tile e^100 above the one
before (a rescale at every tile; a weight staircase stands in for tight variances, which would leave the regime of the bound).
Every kind meets every length.  One state has no mixture on the pipe at all (the kernel's n_mtiles == 0 exit).
The tile flags are not reachable through the public interface, and the fix-up kernel that reads them is launched whether one
is set or not, so "no new flag" is held only through the results: bit-equal outputs to the previous kernel were checked when
the schedule was written (profiles/r19_score_schedule.txt).  The bound is the one of
tests/test_gpu_parity.py for ln b (5e-5 absolute), through tests/_parity.hold."""
import numpy as np
import pytest

from _parity import hold
from oracle import poccala_oracle as po

pytestmark = pytest.mark.gpu

F32_LOGLIK_ATOL = 5e-5          # tests/test_gpu_parity.py
LENS = [1, 63, 64, 65, 255, 256, 257]
KINDS = ['random', 'best_last', 'best_first', 'rising']     # every kind at every length: the product, one state each


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def make_state(rng, kind, M, D):
    """Means and variances as the random kind has them throughout (the 5e-5 bound is 3x the worst case measured at such models,
    |ln b| ~ 85; it does not hold where a state's expansion about its centre is ill conditioned, which is not what is tested
    here): the kinds differ in the WEIGHTS, by m-tile, in steps of e^100 -- past the e^88.7 at which an f32 sum against the
    earlier reference overflows."""
    mean = rng.standard_normal((M, D)) * 0.5
    var = rng.uniform(0.5, 2.0, (M, D))
    tile = np.arange(M) // 32
    last = (M - 1) // 32
    lw = np.log(rng.uniform(0.5, 1.5, M))
    if kind == 'best_last':
        lw -= 100.0 * (tile < last)
    elif kind == 'best_first':
        lw -= 100.0 * (tile > 0)
    elif kind == 'rising':                           # every m-tile e^100 above the one before: a rescale at every tile
        lw -= 100.0 * (last - tile)
    w = np.exp(lw - lw.max())
    return mean, var, w / w.sum()


@pytest.mark.parametrize('D', [39, 13])
@pytest.mark.parametrize('M', [32, 64, 96, 160, 40])
def test_score_schedule_shapes(eng, M, D):
    from poccala_amd import PCL_F32
    rng = np.random.default_rng(1000 + 10 * M + D)
    cases = [(k, T) for k in KINDS for T in LENS]
    states = [make_state(rng, k, M, D) for k, _ in cases]
    mean, var, w = (np.stack([s[i] for s in states]) for i in range(3))
    lens = [T for _, T in cases]
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    x = (rng.standard_normal((sum(lens), D)) * 0.6).astype(np.float32)
    eng.load_model(mean, var, w)
    eng.load_frames(x)
    b = eng.batch([3] * len(lens), lens, begin.tolist())
    b.set_states([np.array([-1, j, -2], dtype=np.int32) for j in range(len(lens))])
    b.score(PCL_F32)
    B = b.get('B')
    for j, (kind, T) in enumerate(cases):
        ref = po.gmm_point(x[begin[j]:begin[j] + T].astype(np.float64), mean[j], var[j], w[j])
        assert np.all(B[j][0] == 0.0) and np.all(np.isneginf(B[j][-1]))
        hold('score schedule M=%d D=%d' % (M, D), 'ln b (%s, %d frames)' % (kind, T), B[j][1], ref, 0.0, F32_LOGLIK_ATOL)
    b.close()


def test_score_state_without_mixture_on_the_pipe():
    """Every mixture of states 0 and 2 is tight enough to be taken off the matrix pipe (variances 1e-6 .. 1e-3), and
    PCL_COARSE_SPLIT_MAX=1 keeps such a state split instead of sending it whole to the direct-form kernel, as
    tests/test_gpu_coarse.py does: the scoring kernel finds n_mtiles == 0, writes ln 0 and raises no flag, and the coarse pass
    adds the exact terms.  State 1 is an ordinary one in the same launch.  Lengths 65 and 257: a partial wave, and a second
    workgroup with one frame.  Bound: the one of tests/test_gpu_coarse.py for such states (5e-5 + the f32 evaluation bound of
    the direct form, 5e-6 relative); the ordinary state is held to 5e-5 alone."""
    import os
    from poccala_amd import Engine, PCL_F32
    from _oracle_pool import f32_evaluation_bound_rows
    rng = np.random.default_rng(77)
    M, D = 64, 39
    lens = [65, 257, 65]
    mean = rng.standard_normal((3, M, D)) * 0.5
    var = rng.uniform(0.5, 2.0, (3, M, D))
    for j in (0, 2):
        var[j] = (10.0 ** rng.uniform(-6, -3, M))[:, None] * rng.uniform(0.5, 2.0, (M, D))
    w = rng.uniform(0.5, 1.5, (3, M))
    w /= w.sum(axis=1, keepdims=True)
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    xs = []
    for j, T in enumerate(lens):                     # frames of the state's own mixtures, so that ln b is finite and sizeable
        comp = rng.integers(0, M, T)
        xs.append(mean[j, comp] + np.sqrt(var[j, comp]) * rng.standard_normal((T, D)))
    x = np.concatenate(xs).astype(np.float32)
    old = os.environ.get('PCL_COARSE_SPLIT_MAX')
    os.environ['PCL_COARSE_SPLIT_MAX'] = '1.0'
    try:
        eng = Engine(0)
    finally:
        if old is None:
            del os.environ['PCL_COARSE_SPLIT_MAX']
        else:
            os.environ['PCL_COARSE_SPLIT_MAX'] = old
    try:
        eng.load_model(mean, var, w)
        eng.load_frames(x)
        b = eng.batch([3] * 3, lens, begin.tolist())
        b.set_states([np.array([-1, j, -2], dtype=np.int32) for j in range(3)])
        b.score(PCL_F32)
        B = b.get('B')
        n_off, limit = eng.model_split_info()
        assert limit == M and n_off[0] == M and n_off[1] == 0 and n_off[2] == M       # states 0 and 2: nothing left on the pipe
        for j, T in enumerate(lens):
            xj = x[begin[j]:begin[j] + T]
            ref = po.gmm_point(xj.astype(np.float64), mean[j], var[j], w[j])
            assert np.all(B[j][0] == 0.0) and np.all(np.isneginf(B[j][-1]))
            if j == 1:
                hold('score schedule empty state', 'ln b of the ordinary state beside it', B[j][1], ref, 0.0, F32_LOGLIK_ATOL)
            else:
                bound = f32_evaluation_bound_rows([(mean[j], var[j], w[j])], xj)[0]
                hold('score schedule empty state', 'ln b of a state with no on-pipe mixture', B[j][1], ref, 5e-6, F32_LOGLIK_ATOL + bound)
        b.close()
    finally:
        eng.close()
