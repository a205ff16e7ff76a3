"""The pitch kernels (poccala_amd/csrc/pitch.hip) at their geometry edges, against tests/_pitch_twin.py.  The cases come from
tests/_pitch_cases.py; tests/test_pitch_cases.py proves on the CPU that each one carries its edge and that a planted defect leaves the
bound.  Bounds and helpers are those of tests/test_gpu_pitch.py, unchanged: correlations bit for bit, lags and voicing exact, ln f0 within
4 ulp, delta bit-equal to the twin's rule on the device's ln f0 and within 4 ulp of ln f0 of the twin's delta.  Samples are always finite:
rule P1-P5 does not define anything else.

Which line each case is there for:
  rows beyond 256   test_rows_beyond_256_*: 581 rows in one call, so blockIdx.x = 1 and 2 of pitch_out_kernel and pitch_delta_kernel run;
                    utterance 24 holds rows 238 .. 297 and utterance 41 rows 480 .. 539, so `at(t +- 1)`, `at(t +- 2)` of pitch_delta_kernel
                    clamp to the utterance's own rows on both sides of a workgroup boundary and read ln f0 that another workgroup's lanes
                    of pitch_out_kernel wrote.  From samples at L = 65, and through PCL_PITCH_NCCF_IN.
  lag grid          test_lag_grid_ends: L = 2 (one wave with 62 idle lanes; `li > 0 && li < L - 1` of pitch_out_kernel never true), 63
                    (one lane short of a wave), 1023 and 1024 = PITCH_MAX_LAGS (16 waves, 3 L doubles of LDS in pitch_track_kernel, the
                    `li = tid; li < L; li += blockDim.x` loop of pitch_nccf_kernel one trip with the last lane off and on).
  LDS limit         test_the_largest_window_*: (size + Lmax + 64) * 8 = 65536 bytes of dynamic LDS in pitch_nccf_kernel, the last window
                    pitch_geometry_check accepts; one sample more is refused as an invalid argument with nothing allocated.
  frame geometry    test_frame_geometry: overlap = 1 (step = size), an odd size, steps that do not divide n - size (`k < n ? s[k] : 0` of
                    pitch_nccf_kernel inside `a`).  test_the_lag_tail_*: a last frame whose own samples are the signal's last, so zeros
                    enter b and not a; followed by full-scale samples that `k < n` must keep out.
  P2                test_p2_branches: `den == 0.0` with p != 0 (underflow), den = inf (overflow: p / sqrt(inf) = 0, not NaN),
                    `db == 0.0` (ballast 0 on silence), ballast 0 on a signal (bal IS raw), int16 at -32768 / 32767, and a DC offset of
                    3e7 on float64 samples (the 64 partial sums of P1's mean).
  P5                test_p5_branches: `li == 0` and `li == L - 1` (no interpolation), `den >= 0` (flat and convex), the shift clamped at
                    +0.5 and at -0.5, a shift of exactly 0.5, and the unclamped vertex, li = 1 and L - 2 among them; nccf_bal picks the
                    lag and nccf_raw is what P5 reads, handed independently.
  track             test_track_*: T = 600 at L = 65 and T = 300 at L = 281 (the double-buffered `best` column, one barrier per frame);
                    T = 1, 2, 3, 257 in one launch (one workgroup each, `T > 1` and `t + 1 < T` of the prefetch); pf = 0 (every lane's
                    argmin is the previous column's first minimum); soft_min_f0 = 200 (fac from 0.5 down to -1.1).  Values on a coarse
                    grid, so ties are everywhere; two calls give the same bits.
  fused front-end   test_frontend_pitch_columns_beyond_256_rows: 479 rows through pcl_frontend_pitch_pcm16, detector on and off."""
import numpy as np
import pytest

import _pitch_cases as pc
import _pitch_twin as pt
from test_gpu_pitch import against_the_twin, check_outputs, speech

pytestmark = pytest.mark.gpu


def from_samples(c):
    """the case through pitch_batch from its samples, every utterance held to its own twin (against_the_twin) and to the case's expectation"""
    with np.errstate(all='ignore'):                      # (the twin on the overflow case)
        rows, info = against_the_twin(c['sigs'], c['rate'], c['name'], **c['kw'])
    size, step, lmin, lmax = pc.geometry(c)
    assert (info['lag_min'], info['lag_max']) == (lmin, lmax)
    assert [len(r) for r in rows] == pc.frames(c)
    for u, ref in enumerate(pc.expect(c)):
        assert np.array_equal(info['lag'][u], ref['lag']) and np.array_equal(info['nccf_raw'][u], ref['raw']), (c['name'], u)
    return rows, info


def from_given(c):
    """the case through PCL_PITCH_NCCF_IN: lags exactly the twin's, the columns by check_outputs; a second call gives the same bits"""
    from poccala_amd.StatisticalModel.AudioProcessing import pitch_batch
    rows, info = pitch_batch(c['sigs'], c['rate'], details=True, nccf=c['nccf'], **c['kw'])
    lmin = pc.geometry(c)[2]
    assert [len(r) for r in rows] == pc.frames(c)
    for u, ref in enumerate(pc.expect(c)):
        assert np.array_equal(info['lag'][u], ref['lag']), (c['name'], u, np.flatnonzero(info['lag'][u] != ref['lag'])[:8])
        check_outputs(rows[u], ref['raw'], ref['lag'], c['rate'], lmin, '%s utterance %d' % (c['name'], u))
    again, info2 = pitch_batch(c['sigs'], c['rate'], details=True, nccf=c['nccf'], **c['kw'])
    assert np.array_equal(np.concatenate(again), np.concatenate(rows)) and np.array_equal(np.concatenate(info2['lag']), np.concatenate(info['lag']))
    return rows, info


# ------------------------------------------------------------------ the lag grid's ends
@pytest.mark.parametrize('L', sorted(pc.LAG_GRID))
def test_lag_grid_ends(L):
    c = pc.lag_grid(L)
    rows, info = from_samples(c)
    assert info['nccf_bal'][0].shape[1] == L == info['lag_max'] - info['lag_min'] + 1
    assert np.isfinite(np.concatenate(rows)).all()


# ------------------------------------------------------------------ the LDS limit
def test_the_largest_window_runs_and_one_sample_more_is_refused():
    from poccala_amd import PoccalaHipError
    from poccala_amd.engine import Engine
    from poccala_amd.StatisticalModel.AudioProcessing import pitch_batch
    c = pc.lds(0)
    assert pc.lds_bytes(c) == 65536
    rows, info = from_samples(c)
    assert len(rows[0]) == 3 and rows[0][:, 0].max() > 0.5
    blocks = Engine.pool_stats()['handed_out_blocks']
    c = pc.lds(1)
    assert pc.lds_bytes(c) == 65544
    with pytest.raises(PoccalaHipError) as e:
        pitch_batch(c['sigs'], c['rate'], **c['kw'])
    print(str(e.value))
    assert e.value.code == -1 and '7809 + 320 samples needs 65544 bytes of LDS, at most 65536' in str(e.value)
    assert Engine.pool_stats()['handed_out_blocks'] == blocks
    again, _ = from_samples(pc.lds(0))                   # and the call before it is still what it was
    assert np.array_equal(again[0], rows[0]) and Engine.pool_stats()['handed_out_blocks'] == blocks


# ------------------------------------------------------------------ frame geometry
@pytest.mark.parametrize('make', [pc.overlap_one, pc.odd_size], ids=['overlap-1', 'odd-size'])
def test_frame_geometry(make):
    rows, info = from_samples(make())
    assert np.isfinite(np.concatenate(rows)).all()


def test_the_lag_tail_past_the_signal_is_zeros_whatever_follows():
    rows, info = from_samples(pc.ragged_tail())
    alone, ialone = from_samples(pc.ragged_tail(alone=True))
    assert np.array_equal(rows[0], alone[0]) and np.array_equal(info['lag'][0], ialone['lag'][0])
    assert np.array_equal(info['nccf_bal'][0], ialone['nccf_bal'][0]) and np.array_equal(info['nccf_raw'][0], ialone['nccf_raw'][0])
    assert np.abs(info['nccf_raw'][1]).max() > 0.9       # (the full-scale square wave itself is voiced)


# ------------------------------------------------------------------ more than 256 rows
def test_rows_beyond_256_from_samples():
    c = pc.straddle()
    rows, info = from_samples(c)
    off = pc.row_off(c)
    assert off[-1] == sum(len(r) for r in rows) > 512 and {k for _, k in pc.straddling(c)} == {1, 2}
    for u, ref in enumerate(pc.expect(c)):               # against_the_twin held each delta column by check_outputs; and once more in plain words
        assert np.array_equal(rows[u][:, 2], pt.delta(rows[u][:, 1])), u


def test_rows_beyond_256_from_given_correlations():
    c = pc.straddle(given=True)
    rows, info = from_given(c)
    assert sum(len(r) for r in rows) > 512


# ------------------------------------------------------------------ P2's branches
@pytest.mark.parametrize('which', pc.P2_CASES)
def test_p2_branches(which):
    c = pc.p2(which)
    rows, info = from_samples(c)
    for u in range(len(rows)):                           # finite samples: nothing is NaN or inf
        assert np.isfinite(rows[u]).all() and np.isfinite(info['nccf_bal'][u]).all() and np.isfinite(info['nccf_raw'][u]).all(), (which, u)
    bal, raw = np.concatenate(info['nccf_bal']), np.concatenate(info['nccf_raw'])
    if which == 'underflow':
        assert np.all(raw == 0.0) and np.any(bal != 0.0)
    if which == 'overflow':
        assert np.all(raw == 0.0) and np.all(bal == 0.0)
    if which == 'ballast0-silence':
        assert np.all(raw == 0.0) and np.all(bal == 0.0) and np.all(np.concatenate(info['lag']) == info['lag_min'])
    if which == 'ballast0':
        assert np.array_equal(bal.view(np.int64), raw.view(np.int64))


# ------------------------------------------------------------------ P5's branches
def test_p5_branches():
    c = pc.p5()
    rows, info = from_given(c)
    lmin = info['lag_min']
    total = {}
    for u, ref in enumerate(pc.expect(c)):               # the device took the branches the case was built for: its lags are the twin's
        assert np.array_equal(rows[u][:, 0], ref['out'][:, 0])
        for k, v in pc.p5_branches(c['nccf'][1][u], info['lag'][u] - lmin).items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert all(v > 0 for v in total.values()) and len(total) == 6


# ------------------------------------------------------------------ the track over many frames
@pytest.mark.parametrize('which', pc.TRACK_CASES)
def test_track_from_given_correlations(which):
    c = pc.track(which)
    rows, info = from_given(c)
    assert np.isfinite(np.concatenate(rows)).all()


# ------------------------------------------------------------------ the fused front-end
LONG = [speech(16000, n, 60 + k) for k, n in enumerate((30000, 41234, 25000))]


@pytest.mark.parametrize('vad', [True, False])
def test_frontend_pitch_columns_beyond_256_rows(vad):
    """the comparison of test_frontend_with_pitch_columns on 149 + 206 + 124 rows: the last three columns are pcl_pitch's rows at the kept
    indices (float64 in the fetched rows, rounded to float32 in the resident matrix), and pcl_pitch's rows are the twin's"""
    from poccala_amd.runtime import default_engine
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch, pitch_batch, vad_batch
    eng = default_engine()
    D = 39
    lens, begin, rows = eng.frontend(LONG, 16000, fetch=True, pitch=True, vad=vad)
    res = eng.frames_download(np.float32).copy()
    assert (eng.F, eng.FD) == (int(lens.sum()), D + 3) and rows.shape == res.shape == (eng.F, D + 3)
    mats = mfcc_batch(LONG, 16000, d1=True, d2=True)
    assert [m.shape for m in mats] == [(149, D), (206, D), (124, D)]
    kept = vad_batch(mats, details=True)[1]['kept'] if vad else [np.arange(len(m)) for m in mats]
    assert [len(k) for k in kept] == lens.tolist() and 0 < lens.sum() and (not vad or lens.sum() < 479)
    pit = pitch_batch(LONG, 16000)
    want = np.concatenate([p[k] for p, k in zip(pit, kept)])
    assert np.array_equal(rows[:, :D], np.concatenate([m[k] for m, k in zip(mats, kept)]))
    assert np.array_equal(rows[:, D:], want)
    assert np.array_equal(res[:, D:], np.float32(want))
    assert want[:, 0].max() > 0.9
    if vad:                                              # once: the stand-alone rows themselves, 479 of them at L = 281, are the twin's
        held, _ = against_the_twin(LONG, 16000, 'front-end signals')
        assert all(np.array_equal(a, b) for a, b in zip(held, pit))
