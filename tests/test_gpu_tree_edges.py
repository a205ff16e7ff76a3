"""The decision tree at its kernels' edges (csrc/tree_cluster.hip; the counting sort of csrc/gmm_segment.hip that it uses), against
tests/_tree_twin.py.  tests/test_gpu_tree.py holds the feature; this file holds what that one cannot see: the summation ORDER the header
states, the sort across tiles, every device width with the last frame row kept, an utterance longer than the key kernel's grid, the
build at D = 1 .. 64 and at the candidate-group edges, leaves that tie exactly, counts beyond 32 bits, and the install where the device
pads the feature dimension.  tests/test_tree_twin.py shows on the CPU that every case reaches the edge it is named after.

Every comparison is byte equality, except the split gains, which keep tests/test_gpu_tree.py's bound 64 * 2^-52 * B (only ln may differ
by an ulp a term).  Every count of differing entries is printed before it is asserted."""
import numpy as np
import pytest

import _tree_cases as tc
import _tree_twin as tw
from test_gpu_tree import drive, exact, hold_tree, same_bits

pytestmark = pytest.mark.gpu
EDGE = tc.edge_cases()
_BUILT, _ORDERED = {}, {}
CHUNK_DEFAULT = 256                                               # csrc/tree_cluster.hip, TREE_CHUNK_DEFAULT


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def built(name):
    if name not in _BUILT:
        c = EDGE[name]
        _BUILT[name] = tw.build(c['n'], c['s'], c['q'], c['event_ctx'], c['P'], c['n_units'], c['q_member'], c['R0'], c['root_of'], c['min_count'],
                                c['min_gain'], c['max_leaves'], c['var_floor'])
    return _BUILT[name]


# ------------------------------------------------------------------ statistics
def ordered(kind, chunk):
    """The order case in the header's order at this chunk length: (one call over both utterances, the first utterance alone, the second
    onto the first), computed once."""
    if (kind, chunk) not in _ORDERED:
        frames, T, begin, frame_row, R = tc.order_case()
        fr = frames.astype(np.float32) if kind == 'f32' else frames
        z = tw.zero(R, fr.shape[1])
        first = tw.accumulate_ordered(z, fr, T[:1], begin[:1], frame_row, chunk)
        _ORDERED[(kind, chunk)] = (tw.accumulate_ordered(z, fr, T, begin, frame_row, chunk), first,
                                   tw.accumulate_ordered(first, fr, T[1:], begin[1:], frame_row, chunk))
    return _ORDERED[(kind, chunk)]


@pytest.mark.parametrize('chunk', ['1', '7', None])
@pytest.mark.parametrize('kind', ['f32', 'f64'])
def test_statistics_in_the_stated_order(eng, monkeypatch, kind, chunk):
    """n, s and q equal tests/_tree_twin.accumulate_ordered -- the order of include/poccala_hip.h (ACCUMULATE, "Order:") taken literally --
    byte for byte, on Gaussian frames whose sums depend on the order: a stable sort over three tiles (the rows on either side of a tile
    edge share a statistics row), chunks in ascending frame row, each summed from 0 in ascending order with x x rounded before it is
    added (the build's -ffp-contract=off), the chunks' sums added onto the resident value in chunk order; in one call and in two.
    A float64 upload leaves the context with both copies (the float32 one is derived on the device); the header says the float64 copy
    is read when the context holds one, so the twin sums the float64 frames there and the float32 frames, widened, otherwise.
    tests/test_tree_twin.py::test_order_case_tells_the_orders_apart shows that this input can tell: of the 117 entries of q, at chunk 7
    and float64 / float32 input, 77 / 83 differ when the chunks' sums are added last first, 44 / 11 when a chunk is summed in descending
    order, 83 / 68 when a row's frames are swapped pair by pair, 19 / none when q + x x is rounded once (a float32 value's square is
    exact in float64: only the float64 run can see a contracted multiply-add).  Tried once on the device: tree_cluster.hip compiled with
    -ffp-contract=fast fails the float64 cases at chunk 7 and at the default, q differing in those same 19 entries (at chunk 1 a
    chunk's q is 0 + x x either way)."""
    if chunk:
        monkeypatch.setenv('PCL_TREE_CHUNK', chunk)
    else:
        monkeypatch.delenv('PCL_TREE_CHUNK', raising=False)
    frames, T, begin, frame_row, R = tc.order_case()
    fr = frames.astype(np.float32) if kind == 'f32' else frames
    whole, first, both = ordered(kind, int(chunk) if chunk else CHUNK_DEFAULT)
    tag = 'tree order %s chunk=%s' % (kind, chunk)
    eng.load_frames(fr)
    eng.tree_zero(R)
    eng.tree_accumulate(T, begin, frame_row)
    exact(tag, eng.tree_stats(), whole)
    eng.tree_zero(R)
    eng.tree_accumulate(T[:1], begin[:1], frame_row)
    exact(tag + ', the first utterance', eng.tree_stats(), first)
    eng.tree_accumulate(T[1:], begin[1:], frame_row)
    exact(tag + ', the second onto it', eng.tree_stats(), both)


@pytest.mark.parametrize('kind', ['f32', 'f64'])
@pytest.mark.parametrize('D', tc.WIDTH_DIMS)
def test_statistics_at_every_device_width_with_the_last_row_kept(eng, monkeypatch, D, kind):
    """Grid frames (exact in any order), one utterance over all F = 64 frame rows, the last two in different statistics rows.  A lane
    loads the G columns from d0 = G g (d0 < D) of frame row f in ONE 16-byte piece iff f FD + d0 + G <= F FD and element by element
    otherwise; only the last row can fail that, where it reads d0 + G <= FD, FD the device width (13, 26, 39, 47, 48, 64).  float32,
    G = 4: FD = 13 has d0 = 12 (D = 13), FD = 26 d0 = 24 (D = 25, 26), FD = 39 d0 = 36 (D = 37 .. 39), FD = 47 d0 = 44 (D = 45 .. 47).
    float64, G = 2: d0 = FD - 1 at the odd widths, D = 13, 39, 47.  So of the widths run here the element-by-element branch is entered
    at D = 13, 26, 37, 39, 45, 47 in float32 and at D = 13, 39, 47 in float64 (tests/_tree_cases.tail_load_dims; tests/test_tree_twin.py
    asserts the lists); no other statistics test keeps frame row F - 1."""
    monkeypatch.setenv('PCL_TREE_CHUNK', '4')
    frames, T, begin, frame_row, R = tc.width_case(D)
    eng.load_frames(np.asarray(frames, dtype=np.float32 if kind == 'f32' else np.float64))
    eng.tree_zero(R)
    eng.tree_accumulate(T, begin, frame_row)
    t = tw.accumulate(tw.zero(R, D), frames, T, begin, frame_row)
    assert t['n'][frame_row[-1]] > 0
    exact('tree width D=%d %s (tail branch: %s)' % (D, kind, D in tc.tail_load_dims(4 if kind == 'f32' else 2)), eng.tree_stats(), t)


def test_statistics_of_a_long_utterance(eng):
    """The key kernel covers an utterance with at most 64 x 256 threads that stride: T = 16384 fills the grid exactly, 16385 sends one
    thread round again, 40000 every thread twice and some a third time (and the sort over 20 tiles)."""
    for T in (16384, 16385, 40000):
        frames, Tu, begin, frame_row, R = tc.long_case(T)
        eng.load_frames(frames)
        eng.tree_zero(R)
        eng.tree_accumulate(Tu, begin, frame_row)
        exact('tree long utterance T=%d' % T, eng.tree_stats(), tw.accumulate(tw.zero(R, 2), frames, Tu, begin, frame_row))


# ------------------------------------------------------------------ build
@pytest.mark.parametrize('name', sorted(EDGE))
def test_edge_build_is_the_twins(eng, name):
    c, t = EDGE[name], built(name)
    tree = drive(eng, c)
    hold_tree('tree edge build %s' % name, tree, t)
    if name == 'big_counts':
        print('tree edge build big_counts: node_n %s' % (tree.node_n.tolist(),))
        assert tree.node_n.max() > 2 ** 32
        assert tree.node_n.dtype == np.int64 and np.array_equal(tree.node_n, t['node_n']) and np.array_equal(tree.leaf_n, t['leaf_n'])


# ------------------------------------------------------------------ install
@pytest.mark.parametrize('logdet', [False, True])
@pytest.mark.parametrize('name', ['wide64', 'd39', 'd14', 'd40', 'd49'])
def test_install_at_padded_widths(eng, name, logdet):
    """The install writes a state's (Mpad, Dd) block of the device layout: D = 39 and 64 fill their device width, D = 14, 40 and 49 are
    padded to 26, 47 and 64.  The model is the twin's byte for byte, and scores as an upload of the twin's arrays does -- with the
    reference's constant and with the log-determinant one, passed the way flat start passes it."""
    from poccala_amd import PCL_F64
    c, t = EDGE[name], built(name)
    D = c['D']
    tree = drive(eng, c, install=True, logdet=logdet)
    hold_tree('tree edge install %s' % name, tree, t)
    mean, var, w = tw.seed_model(t, c['var_floor'])
    got = eng.model_download()
    print('tree edge install %s logdet=%s: model (%d, %d, %d), differs from the twin in %d / %d / %d entries' % (
        name, logdet, eng.J, eng.M, eng.D, (got[0] != mean).sum(), (got[1] != var).sum(), (got[2] != w).sum()))
    assert (eng.J, eng.M, eng.D) == (tree.n_states, 1, D) == (len(t['leaf_n']), 1, D)
    assert same_bits(got[0], mean) and same_bits(got[1], var) and same_bits(got[2], w)
    frames = np.random.default_rng(D).standard_normal((8, D)) * 2

    def lnb():
        b = eng.all_state_batch(np.array([8], dtype=np.int32), np.array([0], dtype=np.int64))
        b.score(PCL_F64)
        out = np.array(b.get('B')[0])
        b.close()
        return out
    eng.load_frames(frames)
    b_installed = lnb()
    eng.load_model(mean, var, w, logdet=logdet)
    b_loaded = lnb()
    inner = b_installed[1:-1]                                     # (the rows between the entry and the exit row: the states)
    print('tree edge install %s logdet=%s: ln b (%d, %d), differs from the upload in %d entries' % (
        name, logdet, b_installed.shape[0], b_installed.shape[1], (b_installed.view(np.int64) != b_loaded.view(np.int64)).sum()))
    assert b_installed.shape == (tree.n_states + 2, 8) and np.isfinite(inner).all()
    assert same_bits(b_installed, b_loaded)
    if logdet:                                                    # the flag arrived: the other constant gives other scores
        eng.load_model(mean, var, w, logdet=False)
        assert not same_bits(inner, lnb()[1:-1])
