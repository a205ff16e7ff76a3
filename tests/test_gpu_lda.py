"""LDA on the device (row f12; csrc/frame_lda.hip: pcl_lda_zero, pcl_lda_accumulate, pcl_batch_accumulate_lda, pcl_lda_stats_download,
pcl_frames_splice_project, pcl_frames_download; Engine.lda_* / splice_project / frames_download, Batch.accumulate_lda,
AcousticModel.lda_batch) against the NumPy twin of the rule (tests/_lda_twin.py, whose own invariants tests/test_lda_twin.py holds).

Inputs (_lda_twin.make_case): 7 utterances of 1, 2, 3, 9, 40, 64 and 65 rows -- the first three shorter than the context, so both clamps
act on one row -- with gaps between them, neighbouring utterances offset by +-1000 so that a read across a boundary cannot hide, R = 5
with class 3 empty and some rows -1, PCL_LDA_CHUNK=16 so that classes span several chunks and chunks end at class boundaries.

Bounds.  Statistics: every element of S and s within 1e-10 x the twin's sum of the ABSOLUTE terms of that element (the project's float64
contract; two orderings of a float64 sum of n terms differ by at most n 2^-52 of that sum, about 1.5e-14 at the largest class here); n is
exact.  Projection: float64 rows within 1e-10 (|b_i| + sum_p |A_ip x_p|) of the twin, the float32 rows EQUAL np.float32 of the float64
rows.  End to end the eigenvalues of the estimate fed the device's statistics against the twin's: measured once on an MI355X at the fixed
seed (E2E_EIG_REL below), asserted with a 10x margin -- the bound depends on the conditioning of W and cannot be derived here.  Every
figure is printed before it is asserted."""
import numpy as np
import pytest

import _lda_twin as tw
from _parity import hold

pytestmark = pytest.mark.gpu
RTOL = 1e-10
CHUNK = '16'
SHAPES = [(13, 4, 4), (5, 1, 2), (3, 0, 0)]         # order 118: eight tiles, the last partial; order 21: two tiles, asymmetric; order 4: one tile
# max |lambda_dev - lambda_twin| / lambda_twin over the three eigenvalues of the planted case, measured on an MI355X at the fixed seed:
# 1.433e-14 (python -m pytest tests/test_gpu_lda.py -m gpu -s -k end_to_end).  Asserted with a 10x margin.
E2E_EIG_REL = 1.433e-14


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


_CASES = {}


def case(D):
    if D not in _CASES:
        _CASES[D] = tw.make_case(D)
    return _CASES[D]


_TWIN = {}


def twin_stats(D, left, right, dtype):
    key = (D, left, right, dtype)
    if key not in _TWIN:
        fr, T, begin, cls = case(D)
        _TWIN[key] = tw.stats(np.asarray(fr, dtype=dtype), T, begin, cls, tw.R_CASE, left, right)
    return _TWIN[key]


def hold_stats(tag, got, t, scale=1.0):
    n, s, S = got
    print('%s: n %s (twin %s)' % (tag, n, scale * t['n']))
    assert np.array_equal(n, scale * t['n'])
    for name, g in (('s', s), ('S', S)):
        err, bound = np.abs(g - scale * t[name]), RTOL * scale * t[name + 'abs']
        with np.errstate(all='ignore'):
            worst = np.nanmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)))
        print('%s: %s worst error / bound = %.3e' % (tag, name, worst))
        assert worst <= 1.0


def device_stats(eng, T, begin, cls, left, right, R=tw.R_CASE):
    eng.lda_zero(R, left, right)
    eng.lda_accumulate(T, begin, cls)
    return eng.lda_stats()


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize('D,left,right', SHAPES)
def test_statistics_are_the_twins(eng, monkeypatch, D, left, right):
    monkeypatch.setenv('PCL_LDA_CHUNK', CHUNK)
    tag = 'lda D=%d (%d, %d)' % (D, left, right)
    fr, T, begin, cls = case(D)
    t = twin_stats(D, left, right, np.float64)
    assert t['n'][3] == 0 and t['n'][2] > 32 and (cls == -1).any()
    eng.load_frames(np.asarray(fr, dtype=np.float64))
    got = device_stats(eng, T, begin, cls, left, right)
    Ds = D * (left + right + 1)
    assert got[0].shape == (5,) and got[1].shape == (5, Ds) and got[2].shape == (5, Ds, Ds)
    hold_stats(tag + ' mfma', got, t)
    assert same_bits(got[2], np.swapaxes(got[2], 1, 2))                                            # mirrored
    again = device_stats(eng, T, begin, cls, left, right)
    assert all(same_bits(x, y) for x, y in zip(got, again))                                       # two runs, the same bits
    eng.lda_accumulate(T, begin, cls)                                                              # the statistics add over calls
    hold_stats(tag + ' twice', eng.lda_stats(), t, 2.0)
    # one call over all utterances == two calls over a split of them, within the bound
    eng.lda_zero(tw.R_CASE, left, right)
    eng.lda_accumulate(T[:4], begin[:4], cls)
    eng.lda_accumulate(T[4:], begin[4:], cls)
    split = eng.lda_stats()
    hold_stats(tag + ' split', split, t)
    assert (np.abs(split[2] - got[2]) <= RTOL * t['Sabs']).all() and (np.abs(split[1] - got[1]) <= RTOL * t['sabs']).all()
    # the VALU form
    monkeypatch.setenv('PCL_LDA_VALU', '1')
    valu = device_stats(eng, T, begin, cls, left, right)
    hold_stats(tag + ' valu', valu, t)
    assert all(same_bits(x, y) for x, y in zip(valu, device_stats(eng, T, begin, cls, left, right)))
    assert (np.abs(valu[2] - got[2]) <= RTOL * t['Sabs']).all() and (np.abs(valu[1] - got[1]) <= RTOL * t['sabs']).all()
    monkeypatch.delenv('PCL_LDA_VALU')
    # float32-only frames: the float32 rows widened
    eng.load_frames(np.asarray(fr, dtype=np.float32))
    hold_stats(tag + ' f32 rows', device_stats(eng, T, begin, cls, left, right), twin_stats(D, left, right, np.float32))
    # the default chunk: one chunk per class
    monkeypatch.delenv('PCL_LDA_CHUNK')
    eng.load_frames(np.asarray(fr, dtype=np.float64))
    hold_stats(tag + ' default chunk', device_stats(eng, T, begin, cls, left, right), t)


# ------------------------------------------------------------------ from a batch's Viterbi paths
@pytest.mark.parametrize('fold', [False, True])
def test_batch_statistics_equal_the_downloaded_owner_map(eng, monkeypatch, fold):
    from test_gpu_realign import aligned_batch, edge_batch, place
    monkeypatch.setenv('PCL_LDA_CHUNK', CHUNK)
    labels, T, single, short = edge_batch()
    begin, F = place(np.random.default_rng(3), T)
    b, _ = aligned_batch(eng, 5, labels, T, begin, F, seed=5)
    J = eng.J
    sc, R = None, J
    if fold:
        sc = (np.arange(J) // 3).astype(np.int32)                                                   # the three states of a unit tied
        sc[J - 1] = -1
        R = J // 3
    eng.lda_zero(R, 1, 1)
    b.accumulate_lda(sc)
    got = eng.lda_stats()
    seg, dropped, state = b.align_segments(want_map=True)
    seg.close()
    assert len(dropped) > 0 and (state >= 0).any()
    want_cls = tw.fold(state, sc)
    Tn = np.asarray(T, dtype=np.int32)
    eng.lda_zero(R, 1, 1)
    eng.lda_accumulate(Tn, begin, want_cls)
    ref = eng.lda_stats()
    print('batch lda fold=%s: rows per class %s, %d utterances dropped' % (fold, got[0], len(dropped)))
    assert got[0].sum() == (want_cls >= 0).sum() > 0
    assert all(same_bits(x, y) for x, y in zip(got, ref))
    fr = eng.frames_download()
    t = tw.stats(fr, Tn, begin, want_cls, R, 1, 1)
    hold_stats('batch lda fold=%s' % fold, got, t)
    b.close()


# ------------------------------------------------------------------ projection
def projection_case(D, left, right, D_out):
    rng = np.random.default_rng(1000 * D + D_out)
    Ds = D * (left + right + 1)
    return rng.standard_normal((D_out, Ds)) / 100.0, rng.standard_normal(D_out)


@pytest.mark.parametrize('D,left,right,D_out', [(D, l, r, o) for D, l, r in SHAPES for o in (39, 13, 2) if o <= D * (l + r + 1)])
def test_projected_frames_are_the_twins(eng, D, left, right, D_out):
    import _bootstrap_twin as bt
    from poccala_amd import PCL_F32, synth
    tag = 'lda project D=%d (%d, %d) -> %d' % (D, left, right, D_out)
    fr, T, begin, cls = case(D)
    A, b = projection_case(D, left, right, D_out)
    y64, y32, mag = tw.project(fr, T, begin, left, right, A, b)
    owned = tw.splice(fr, T, begin, left, right)[1]
    eng.load_frames(np.asarray(fr, dtype=np.float64))
    eng.splice_project(T, begin, left, right, A, b)
    assert eng.FD == D_out and eng.F == len(fr)
    g64, g32 = eng.frames_download(np.float64), eng.frames_download(np.float32)
    assert g64.shape == g32.shape == (len(fr), D_out) and g32.dtype == np.float32
    worst = (np.abs(g64 - y64)[owned] / (RTOL * mag[owned])).max()
    print('%s: worst error / bound = %.3e' % (tag, worst))
    assert worst <= 1.0
    assert same_bits(g32, g64.astype(np.float32))                                                 # float32(y), exactly
    assert not g64[~owned].any() and not g32[~owned].any() and (~owned).sum() > 5                 # rows of no utterance: zero
    mean, var, n = eng.frames_moments(T, begin)                                                    # the width bookkeeping holds for later stages
    tm, tv, tn = bt.moments(y64, T, begin, len(T), 1)
    assert n == tn
    hold(tag, 'moments mean', mean, tm, RTOL)
    hold(tag, 'moments var', var, tv, RTOL)
    if D_out == 39:                                                                                # the matrix-pipe route on the projected frames
        model = synth.make_model(2, 4, 39, seed=3)[:3]
        eng.load_model(*model)

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
    assert (np.abs(r32.astype(np.float64) - z64) <= RTOL * zmag + 2.0 ** -24 * np.abs(z64)).all() and not r32[~owned].any()


# ------------------------------------------------------------------ end to end
def test_planted_subspace_end_to_end(eng):
    fr, T, begin, cls, basis = tw.planted_case()
    R, left, right, D_out = 4, 1, 1, 3
    eng.load_frames(fr)
    got = device_stats(eng, T, begin, cls, left, right, R)
    A, b, lam = eng.lda_estimate(D_out)
    t = tw.stats(fr, T, begin, cls, R, left, right)
    At, bt_, lamt = tw.estimate(t['n'], t['s'], t['S'], D_out)
    rel = float((np.abs(lam - lamt) / np.abs(lamt)).max())
    print('lda e2e: eigenvalues %s (twin %s), max relative difference %.3e (bound %.1e)' % (lam, lamt, rel, 10 * E2E_EIG_REL))
    angle = tw.principal_angle(A[:2], basis)
    print('lda e2e: principal angle of the two leading rows %.4f rad' % angle)
    eng.splice_project(T, begin, left, right, A, b)
    y = eng.frames_download()
    yt = tw.project(fr, T, begin, left, right, At, bt_)[0]
    err, errt = tw.nearest_mean_error(y, cls, R), tw.nearest_mean_error(yt, cls, R)
    print('lda e2e: nearest-class-mean error rate %.4f (twin %.4f)' % (err, errt))
    W, B, m = tw.class_covariances(y, cls, R)
    print('lda e2e: |W - I| %.2e, |B - diag(lambda)| %.2e' % (np.abs(W - np.eye(D_out)).max(), np.abs(B - np.diag(lam)).max()))
    assert rel <= 10 * E2E_EIG_REL
    assert err <= errt
    assert np.abs(W - np.eye(D_out)).max() <= 1e-8 and np.abs(B - np.diag(lam)).max() <= 1e-8


def test_lda_batch_projects_the_resident_frames(eng):
    from poccala_amd import PCL_F64, synth
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    units_n, M, D, U, L, T, S = 3, 2, 13, 6, 3, 60, 5
    mean, var, w, _ = synth.make_model(units_n, M, D, seed=31)
    labels = synth.make_labels(U, L, units_n, seed=34)
    frames = synth.make_peaked_frames(labels, T, mean * 3, var, seed=33).astype(np.float64)
    names = ['u%d' % i for i in range(units_n)]
    am = AcousticModel(state_num=S, mix_level=M, dct_num=13, delta_1=False, delta_2=False)
    unit_hmms = {u: am.init_unit(u) for u in names}
    am._adopt_model((mean * 3, var, w), names, unit_hmms)
    data = [frames[u * T:(u + 1) * T] for u in range(U)]
    out = am.lda_batch([[names[i] for i in lab] for lab in labels], data, unit_hmms, 8, left=1, right=1, precision=PCL_F64, engine=eng)
    print('lda_batch: rows per class %s, eigenvalues %s, dropped %s' % (out['n'], out['eigenvalues'], out['dropped']))
    assert out['A'].shape == (8, 39) and eng.FD == 8 and eng.F == U * T
    assert out['n'].sum() == T * (U - len(out['dropped'])) > 0 and (np.diff(out['eigenvalues']) <= 0).all()
    y = eng.frames_download()
    want = tw.project(frames, out['lens'], out['begin'], 1, 1, out['A'], out['b'])
    assert (np.abs(y - want[0]) <= RTOL * want[2]).all()


# ------------------------------------------------------------------ what is refused, and what the calls give back
def test_refusals_and_the_pool(eng):
    from poccala_amd import Engine, PoccalaHipError
    INVALID, STATE = -1, -3
    D, left, right = 5, 1, 2
    fr, T, begin, cls = case(D)
    Ds = D * (left + right + 1)
    A, b = projection_case(D, left, right, 2)

    def refused(call, code):
        before = Engine.pool_stats()['handed_out_blocks']
        with pytest.raises(PoccalaHipError) as ei:
            call()
        print(ei.value)
        assert ei.value.code == code and len(str(ei.value)) > 30
        assert Engine.pool_stats()['handed_out_blocks'] == before                                  # a refused call keeps nothing

    refused(lambda: eng.lda_zero(5, left, right), STATE)                                           # no frames
    eng.load_frames(np.asarray(fr, dtype=np.float32))
    refused(lambda: eng.lda_accumulate(T, begin, cls), STATE)                                      # before lda_zero
    refused(lambda: eng.lda_stats(), STATE)
    refused(lambda: eng.frames_download(np.float64), STATE)                                        # no float64 copy
    assert same_bits(eng.frames_download(np.float32), np.asarray(fr, dtype=np.float32))
    refused(lambda: eng.lda_zero(5, 12, 13), INVALID)                                              # Ds + 1 = 131 > 128
    refused(lambda: eng.lda_zero(0, left, right), INVALID)
    refused(lambda: eng.splice_project(T, begin, 12, 13, np.zeros((2, 130)), np.zeros(2)), INVALID)
    refused(lambda: eng.splice_project(T, begin, left, right, np.zeros((Ds + 1, Ds)), np.zeros(Ds + 1)), INVALID)     # D_out > Ds
    eng.lda_zero(tw.R_CASE, left, right)
    bad = cls.copy()
    bad[begin[3] + 1] = tw.R_CASE
    refused(lambda: eng.lda_accumulate(T, begin, bad), INVALID)                                    # a class id >= R
    over = begin.copy()
    over[5] = begin[4] + 10
    refused(lambda: eng.lda_accumulate(T, over, cls), INVALID)                                     # overlapping utterances
    start = Engine.pool_stats()['handed_out_blocks']
    eng.lda_accumulate(T, begin, cls)
    assert Engine.pool_stats()['handed_out_blocks'] == start                                        # every temporary went back
    assert np.array_equal(eng.lda_stats()[0], twin_stats(D, left, right, np.float32)['n'])
    eng.lda_zero(tw.R_CASE, left, right)                                                            # the next lda_zero frees the last one's block
    assert Engine.pool_stats()['handed_out_blocks'] == start
    live = eng.batch(np.array([3], dtype=np.int32), np.array([4], dtype=np.int32), np.array([0], dtype=np.int64))
    refused(lambda: eng.splice_project(T, begin, left, right, A, b), STATE)                         # a live batch
    live.close()
    eng.sync()
    seg = eng.segments(np.where(cls >= 0, 0, -1).astype(np.int32), J=1)
    refused(lambda: eng.splice_project(T, begin, left, right, A, b), STATE)                         # a live Segments
    seg.close()
    eng.load_frames(np.asarray(fr[:, :3], dtype=np.float32))                                        # another width since lda_zero: (left, right) no longer matches
    refused(lambda: eng.lda_accumulate(T, begin, cls), STATE)
    eng.load_frames(np.asarray(fr, dtype=np.float32))
    eng.lda_accumulate(T, begin, cls)                                                               # the context is usable
    assert np.array_equal(eng.lda_stats()[0], twin_stats(D, left, right, np.float32)['n'])
    eng.splice_project(T, begin, left, right, A, b)
    assert eng.frames_download(np.float32).shape == (len(fr), 2)
    refused(lambda: eng.lda_accumulate(T, begin, cls), STATE)                                      # the projected frames have another width too
    other = Engine(0)                                                                               # pcl_destroy with statistics resident
    other.load_frames(np.asarray(fr, dtype=np.float64))
    other.lda_zero(3, 1, 1)
    other.close()
