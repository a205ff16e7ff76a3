"""LDA on the device (row f12; csrc/frame_lda.hip) at every configuration its code has, against the NumPy twin (tests/_lda_twin.py): the
eight tile counts NT = 1 .. 8 of lda_mfma_kernel and lda_valu_kernel with the orders that are a multiple of 16, one above a multiple and
the cap 128; chunks of 1 .. 97 rows (a wave's second MFMA k-step, a second step of 32 rows, the early break); more than LDA_ROUND = 1024
chunks (the launch rounds and the reduction's clipping); an utterance longer than one pass of the key kernel's grid; the projection at the
output widths that pad differently, and a second projection of projected frames.  tests/test_lda_twin.py holds, on the CPU, that every
input here reaches the edge it is for; the tests assert the same counts again from the device's n.

Bounds: those of tests/test_gpu_lda.py, whose hold_stats / same_bits are used -- every element of S and s within 1e-10 x the twin's sum
of the absolute terms of that element, n exact, S mirrored and two runs equal to the bit, the two forms and any two chunkings within the
same bound of each other; projected float64 rows within 1e-10 (|b_i| + sum_p |A_ip x_p|), the float32 rows EQUAL np.float32 of them, rows
of no utterance zero.  The chained projection adds what its first stage may be off by, carried through the second matrix:
1e-10 (mag_2 + |A_2| splice(mag_1)).  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _lda_twin as tw
from _parity import hold
from test_gpu_lda import RTOL, device_stats, eng, hold_stats, same_bits  # noqa: F401 (eng: the fixture)

pytestmark = pytest.mark.gpu
DEVICE_DIMS = tw.DEVICE_DIMS


def hold_pair(tag, a, b, t):
    """two device results of one input within the twin's bound of each other"""
    assert np.array_equal(a[0], b[0])
    for name, x, y in (('s', a[1], b[1]), ('S', a[2], b[2])):
        err, bound = np.abs(x - y), RTOL * t[name + 'abs']
        worst = float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)).max())
        print('%s: %s worst difference / bound = %.3e' % (tag, name, worst))
        assert worst <= 1.0


def set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv('PCL_LDA_CHUNK', raising=False)
    else:
        monkeypatch.setenv('PCL_LDA_CHUNK', str(chunk))


def both_forms(eng, monkeypatch, tag, T, begin, cls, left, right, R, t):
    """(mfma, valu): each held to the twin, the MFMA form mirrored and run twice to the same bits, the two within the bound of each other"""
    monkeypatch.delenv('PCL_LDA_VALU', raising=False)
    got = device_stats(eng, T, begin, cls, left, right, R)
    Ds = t['s'].shape[1]
    assert got[0].shape == (R,) and got[1].shape == (R, Ds) and got[2].shape == (R, Ds, Ds)
    hold_stats(tag + ' mfma', got, t)
    assert same_bits(got[2], np.swapaxes(got[2], 1, 2))
    assert all(same_bits(x, y) for x, y in zip(got, device_stats(eng, T, begin, cls, left, right, R)))
    monkeypatch.setenv('PCL_LDA_VALU', '1')
    valu = device_stats(eng, T, begin, cls, left, right, R)
    monkeypatch.delenv('PCL_LDA_VALU')
    hold_stats(tag + ' valu', valu, t)
    assert same_bits(valu[2], np.swapaxes(valu[2], 1, 2))
    hold_pair(tag + ' mfma - valu', got, valu, t)
    return got, valu


def runs(rows):
    """[5, 5, 5, 2] -> '3 x 5, 2'"""
    out = []
    for r in rows:
        if out and out[-1][1] == r:
            out[-1][0] += 1
        else:
            out.append([1, r])
    return ', '.join('%d x %d' % (k, r) if k > 1 else '%d' % r for k, r in out)


_CASES = {}


def cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


# ------------------------------------------------------------------ every tile count, every order edge
@pytest.mark.parametrize('D,left,right,n,NT', tw.EDGE_SHAPES)
def test_every_tile_count_and_order_edge(eng, monkeypatch, D, left, right, n, NT):
    fr, T, begin, cls = cached(('stat', D), lambda: tw.make_case(D))
    R, Ds = tw.R_CASE, D * (left + right + 1)
    assert Ds + 1 == n and (n + 15) // 16 == NT
    twin = {dt: cached(('stat', D, left, right, dt), lambda: tw.stats(np.asarray(fr, dtype=dt), T, begin, cls, R, left, right)) for dt in (np.float64, np.float32)}
    for chunk in (16, None):
        set_chunk(monkeypatch, chunk)
        for dt in (np.float64, np.float32):
            tag = 'lda edges NT=%d n=%d D=%d (%d, %d) chunk %s %s' % (NT, n, D, left, right, chunk, np.dtype(dt).name)
            t = twin[dt]
            eng.load_frames(np.asarray(fr, dtype=dt))
            got, valu = both_forms(eng, monkeypatch, tag, T, begin, cls, left, right, R, t)
            assert got[0][3] == 0 and got[0][2] > 32 and (cls == -1).any() and got[0].sum() < (cls >= 0).sum()       # the case reached the device
            plan = tw.chunk_plan(got[0], chunk)
            assert plan['chunks'] > R - 1 if chunk else plan['chunks'] == R - 1
            eng.lda_zero(R, left, right)                                                              # two calls over a split of the utterances against one
            eng.lda_accumulate(T[:4], begin[:4], cls)
            eng.lda_accumulate(T[4:], begin[4:], cls)
            split = eng.lda_stats()
            hold_stats(tag + ' split', split, t)
            hold_pair(tag + ' split - one call', split, got, t)
            eng.lda_accumulate(T, begin, cls)                                                         # ... and onto statistics that are not zero
            hold_stats(tag + ' twice', eng.lda_stats(), t, 2.0)


# ------------------------------------------------------------------ K edges
@pytest.mark.parametrize('chunk', [1, 5, 33, None])
@pytest.mark.parametrize('D,left,right', [(3, 1, 1), (16, 2, 1)])
def test_k_edges(eng, monkeypatch, D, left, right, chunk):
    counts = np.array(tw.KEDGE_COUNTS, dtype=np.float64)
    R = len(counts)
    fr, T, begin, cls = cached(('k', D), lambda: tw.plant_case(D, tw.KEDGE_LENGTHS, tw.KEDGE_COUNTS))
    t = cached(('k', D, left, right), lambda: tw.stats(fr, T, begin, cls, R, left, right))
    assert np.array_equal(t['n'], counts)
    tag = 'lda K edges D=%d (%d, %d) chunk %s' % (D, left, right, chunk)
    set_chunk(monkeypatch, chunk)
    eng.load_frames(fr)
    got, valu = both_forms(eng, monkeypatch, tag, T, begin, cls, left, right, R, t)
    assert np.array_equal(got[0], counts) and np.array_equal(valu[0], counts)                     # one class per row count, two empty
    plan = tw.chunk_plan(got[0], chunk)
    lo = plan['cls_chunk0']
    print('%s: %d chunks in %d round; the class of 65 rows in chunks of %s rows, the class of 97 in %s' % (
        tag, plan['chunks'], plan['rounds'], runs(plan['rows'][lo[13]:lo[14]]), runs(plan['rows'][lo[14]:lo[15]])))
    if chunk is None:
        steps = [tw.chunk_steps(c) for c in plan['rows']]
        assert plan['chunks'] == 14 and max(s['steps'] for s in steps) == 4 and sum(s['second'] for s in steps) == 8 and sum(s['early'] for s in steps) == 10
    eng.load_frames(np.asarray(fr, dtype=np.float32))                                              # float32-only rows through the same chunks
    hold_stats(tag + ' f32 rows', device_stats(eng, T, begin, cls, left, right, R), cached(('k32', D, left, right), lambda: tw.stats(
        np.asarray(fr, dtype=np.float32), T, begin, cls, R, left, right)))


# ------------------------------------------------------------------ more chunks than one launch round takes
@pytest.mark.parametrize('D,left,right,lengths,counts', [(3, 0, 0, tw.ROUND_LENGTHS, tw.ROUND_COUNTS), (13, 1, 1, tw.ROUND40_LENGTHS, tw.ROUND40_COUNTS)])
def test_rounds(eng, monkeypatch, D, left, right, lengths, counts):
    R = len(counts)
    fr, T, begin, cls = tw.plant_case(D, lengths, counts)
    t = tw.stats(fr, T, begin, cls, R, left, right)
    tag = 'lda rounds D=%d (%d, %d) order %d' % (D, left, right, t['s'].shape[1] + 1)
    eng.load_frames(fr)
    set_chunk(monkeypatch, 1)
    got, valu = both_forms(eng, monkeypatch, tag + ' chunk 1', T, begin, cls, left, right, R, t)
    assert np.array_equal(got[0], counts) and np.array_equal(valu[0], counts)
    plan = tw.chunk_plan(got[0], 1)
    print('%s chunk 1: %d chunks in %d rounds, class boundaries at chunks %s, classes over two rounds %s' % (
        tag, plan['chunks'], plan['rounds'], plan['cls_chunk0'].tolist(), plan['split']))
    assert plan['chunks'] == sum(counts) > tw.ROUND and plan['rounds'] == -(-sum(counts) // tw.ROUND) and plan['split'] == [2]
    eng.lda_accumulate(T, begin, cls)                                                              # the rounds add onto running statistics
    hold_stats(tag + ' chunk 1 twice', eng.lda_stats(), t, 2.0)
    set_chunk(monkeypatch, None)
    whole = device_stats(eng, T, begin, cls, left, right, R)
    one = tw.chunk_plan(whole[0], None)
    print('%s default chunk: %d chunks in %d round' % (tag, one['chunks'], one['rounds']))
    assert one['rounds'] == 1
    hold_stats(tag + ' default chunk', whole, t)
    hold_pair(tag + ' chunk 1 - default chunk', got, whole, t)


# ------------------------------------------------------------------ one long utterance
def test_long_utterance(eng, monkeypatch):
    D, left, right, R = 2, 1, 1, tw.LONG_R
    set_chunk(monkeypatch, None)
    fr, T, begin, cls = tw.long_case(D)
    t = tw.stats(fr, T, begin, cls, R, left, right)
    eng.load_frames(fr)
    got, valu = both_forms(eng, monkeypatch, 'lda long utterance', T, begin, cls, left, right, R, t)
    plan = tw.chunk_plan(got[0], None)
    print('lda long utterance: %d rows, rows per class %s, %d chunks' % (T[1], got[0], plan['chunks']))
    assert T[1] == tw.LONG_ROWS > 64 * 256 and (got[0] > 2 * tw.CHUNK_DEFAULT).all() and plan['chunks'] == 3 * R
    rng = np.random.default_rng(77)
    A, b = rng.standard_normal((2, 3 * D)) / 100.0, rng.standard_normal(2)
    y64, y32, mag = tw.project(fr, T, begin, left, right, A, b)
    owned = tw.splice(fr, T, begin, left, right)[1]
    eng.splice_project(T, begin, left, right, A, b)
    g64, g32 = eng.frames_download(np.float64), eng.frames_download(np.float32)
    assert g64.shape == (len(fr), 2) and eng.FD == 2
    ratio = np.zeros_like(g64)
    ratio[owned] = np.abs(g64 - y64)[owned] / (RTOL * mag[owned])
    b1 = int(begin[1])
    edges = [b1, b1 + 1, b1 + T[1] - 2, b1 + T[1] - 1]
    print('lda long utterance: projection worst error / bound = %.3e over %d rows; first and last rows %.3e; behind row 64 x 256: %.3e' % (
        ratio.max(), owned.sum(), ratio[edges].max(), ratio[b1 + 64 * 256:b1 + T[1]].max()))
    assert owned.sum() == T.sum() and ratio.max() <= 1.0
    assert same_bits(g32, g64.astype(np.float32)) and np.abs(g64[owned]).min() > 0
    assert not g64[~owned].any() and not g32[~owned].any() and (~owned).sum() > 5


# ------------------------------------------------------------------ the projection's output widths
WIDTHS = [(1, 0, 0, 1), (5, 1, 1, 1), (5, 1, 1, 14), (16, 0, 0, 14), (7, 4, 4, 40), (7, 4, 4, 47), (7, 4, 4, 48), (16, 2, 1, 1), (16, 2, 1, 14),
          (16, 2, 1, 47), (16, 2, 1, 64), (1, 63, 63, 1), (1, 63, 63, 14), (1, 63, 63, 40), (1, 63, 63, 48), (1, 63, 63, 64)]


def width_case(D, left, right, D_out):
    rng = np.random.default_rng(7000 + 1000 * D + 10 * left + D_out)
    Ds = D * (left + right + 1)
    return rng.standard_normal((D_out, Ds)) / 100.0, rng.standard_normal(D_out)


def hold_projection(tag, g64, y64, mag, owned, extra=None):
    bound = RTOL * (mag if extra is None else mag + extra)
    assert (bound[owned] > 0).all()
    worst = float((np.abs(g64 - y64)[owned] / bound[owned]).max())
    print('%s: worst error / bound = %.3e' % (tag, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('D,left,right,D_out', WIDTHS)
def test_projection_widths(eng, D, left, right, D_out):
    import _bootstrap_twin as bt
    from poccala_amd import PCL_F32, synth
    assert (D, left, right) in [s[:3] for s in tw.EDGE_SHAPES] and D_out <= D * (left + right + 1)
    stride = next(o for o in DEVICE_DIMS if D_out <= o)
    tag = 'lda widths D=%d (%d, %d) Ds=%d -> %d (held at %d)' % (D, left, right, D * (left + right + 1), D_out, stride)
    fr, T, begin, cls = cached(('stat', D), lambda: tw.make_case(D))
    A, b = width_case(D, left, right, D_out)
    y64, y32, mag = tw.project(fr, T, begin, left, right, A, b)
    owned = tw.splice(fr, T, begin, left, right)[1]
    eng.load_frames(np.asarray(fr, dtype=np.float64))
    eng.splice_project(T, begin, left, right, A, b)
    assert eng.FD == D_out and eng.F == len(fr)
    g64, g32 = eng.frames_download(np.float64), eng.frames_download(np.float32)
    assert g64.shape == g32.shape == (len(fr), D_out) and g32.dtype == np.float32
    hold_projection(tag, g64, y64, mag, owned)
    assert same_bits(g32, g64.astype(np.float32))                                                 # float32(y), exactly
    assert not g64[~owned].any() and not g32[~owned].any() and (~owned).sum() > 5                 # rows of no utterance: zero
    mean, var, n = eng.frames_moments(T, begin)                                                    # the width bookkeeping holds for later stages
    tm, tv, tn = bt.moments(y64, T, begin, len(T), 1)
    assert n == tn
    hold(tag, 'moments mean', mean, tm, RTOL)
    hold(tag, 'moments var', var, tv, RTOL)
    if stride > D_out:                                                                             # padding columns: what an upload of the same rows leaves (zeros)
        eng.load_model(*synth.make_model(2, 4, D_out, seed=3)[:3])

        def lnb():
            bb = eng.all_state_batch(np.array([eng.F], dtype=np.int32), np.array([0], dtype=np.int64))
            bb.score(PCL_F32)
            out = bb.get('B')[0]
            bb.close()
            return out
        resident = lnb()
        eng.load_frames(g32)
        assert same_bits(resident, lnb()) and np.isfinite(resident[1:-1]).all()
    # float32-only frames: no float64 copy is made, the rows are the float32 of the same sums over the widened rows
    f32 = np.asarray(fr, dtype=np.float32)
    eng.load_frames(f32)
    eng.splice_project(T, begin, left, right, A, b)
    z64, z32, zmag = tw.project(f32, T, begin, left, right, A, b)
    r32 = eng.frames_download(np.float32)
    assert eng.FD == D_out and r32.shape == (len(fr), D_out)
    assert (np.abs(r32.astype(np.float64) - z64) <= RTOL * zmag + 2.0 ** -24 * np.abs(z64)).all() and not r32[~owned].any()
    mean, var, n = eng.frames_moments(T, begin)
    tm, tv, tn = bt.moments(r32.astype(np.float64), T, begin, len(T), 1)
    assert n == tn
    hold(tag + ' f32', 'moments mean', mean, tm, RTOL)
    hold(tag + ' f32', 'moments var', var, tv, RTOL)


def test_projection_of_projected_frames(eng):
    """tw.CHAIN: (13, 2, 1) -> 40, held at a stride of 47, then (1, 0) over the projected frames -> 64: the second splice reads a matrix
    the device built, at its padded stride.  (A first stage of context (1, 1) has 39 spliced dimensions and cannot give 40: D_out <= Ds.)"""
    (D, l1, r1, o1), (D2, l2, r2, o2) = tw.CHAIN
    fr, T, begin, cls = cached(('stat', D), lambda: tw.make_case(D))
    A1, b1 = width_case(D, l1, r1, o1)
    A2, b2 = width_case(D2, l2, r2, o2)
    owned = tw.splice(fr, T, begin, l1, r1)[1]
    y1, _, mag1 = tw.project(fr, T, begin, l1, r1, A1, b1)
    y2, _, mag2 = tw.project(y1, T, begin, l2, r2, A2, b2)
    carried = tw.project(mag1, T, begin, l2, r2, np.abs(A2), np.zeros(o2))[0]                      # |A_2| splice(mag_1): the first stage's bound through A_2
    eng.load_frames(np.asarray(fr, dtype=np.float64))
    eng.splice_project(T, begin, l1, r1, A1, b1)
    assert eng.FD == o1 == D2
    g1 = eng.frames_download(np.float64)
    hold_projection('lda chained, stage 1 -> %d' % o1, g1, y1, mag1, owned)
    eng.splice_project(T, begin, l2, r2, A2, b2)
    assert eng.FD == o2 and eng.F == len(fr)
    g2, g2_32 = eng.frames_download(np.float64), eng.frames_download(np.float32)
    hold_projection('lda chained, stage 2 -> %d, the twin applied twice' % o2, g2, y2, mag2, owned, carried)
    again = tw.project(g1, T, begin, l2, r2, A2, b2)                                               # ... and the second stage alone, from the rows the device held
    hold_projection('lda chained, stage 2 from the device\'s stage 1', g2, again[0], again[2], owned)
    assert same_bits(g2_32, g2.astype(np.float32)) and not g2[~owned].any() and not g2_32[~owned].any()
    # float32-only: the second stage reads the float32 rows of the first
    eng.load_frames(np.asarray(fr, dtype=np.float32))
    eng.splice_project(T, begin, l1, r1, A1, b1)
    r1_32 = eng.frames_download(np.float32)
    eng.splice_project(T, begin, l2, r2, A2, b2)
    r2_32 = eng.frames_download(np.float32)
    z64, _, zmag = tw.project(r1_32.astype(np.float64), T, begin, l2, r2, A2, b2)
    assert r2_32.shape == (len(fr), o2) and not r2_32[~owned].any()
    assert (np.abs(r2_32.astype(np.float64) - z64) <= RTOL * zmag + 2.0 ** -24 * np.abs(z64)).all()
