"""Pitch and voicing features on the GPU (csrc/pitch.hip) against their NumPy definition (tests/_pitch_twin.py).

What is compared how:
  nccf_bal / nccf_raw   BIT FOR BIT: the twin mirrors the kernel's summation order exactly (one lane per lag, ascending sample index, one
                        rounded multiplication and addition at a time; sqrt and division are correctly rounded on both sides).
  lags, voicing         exactly equal, from the device's own correlations and (PCL_PITCH_NCCF_IN) from the twin's or constructed ones.
  ln f0                 within 4 ulp: the device's log is the one operation that is not the twin's.
  delta ln f0           bit-equal to the twin's delta rule applied to the DEVICE's ln f0 column (the rule itself is exact), and within
                        4 ulp of ln f0 of the twin's delta: the delta is ((x[t+1] - x[t-1]) + 2 (x[t+2] - x[t-2])) / 10, so input errors of
                        e = 4 ulp(ln f0) reach it as at most (2 e + 4 e) / 10 = 0.6 e, plus three roundings of values no larger than 2 |ln f0|
                        -- below 4 ulp(ln f0) in all.  (A bound in ulps of the delta itself would be meaningless: it is a difference of
                        nearly equal logs, exactly 0 on a steady tone.)
Shapes: the smallest at which each kernel can go wrong -- L = 141 (three waves, the last partial), 281 (five waves, past 256 lanes), 64
and 65 (a full wave, one lane more); utterances of fewer samples than a frame, exactly one frame, one sample more, silence, a glide."""
import numpy as np
import pytest

import _pitch_twin as pt
from _parity import hold
from test_pitch_twin import KINDS, TONES, tone, tone_result

pytestmark = pytest.mark.gpu

F32_LOGLIK_ATOL = 5e-5          # tests/test_gpu_parity.py


def glide(rate, seconds=0.3, f_lo=120.0, f_hi=180.0, seed=1, noise=200.0, amp=6000.0):
    n = int(rate * seconds)
    f = np.linspace(f_lo, f_hi, n)
    ph = 2 * np.pi * np.cumsum(f) / rate
    s = sum((amp / k) * np.sin(k * ph) for k in range(1, 4)) + noise * np.random.default_rng(seed).standard_normal(n)
    return np.round(s).astype(np.int16)


def ragged(rate):
    """U = 5: shorter than a frame (T = 1), exactly one frame, one sample more (T = 2, the second frame almost all padding), silence, a glide"""
    size = int(rate * 0.025)
    g = glide(rate)
    return [g[:size - 63].copy(), g[100:100 + size].copy(), g[50:50 + size + 1].copy(), np.zeros(3 * size, dtype=np.int16), g]


def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def check_outputs(out, raw, lag, rate, lmin, what):
    """the three columns of one utterance from ITS lags and raw correlations: v and the lag exact, ln f0 and delta within 4 ulp (docstring)"""
    want = pt.outputs(raw, lag - lmin, rate, lmin)
    assert np.array_equal(out[:, 0], want[:, 0]), what
    u = ulps(out[:, 1], want[:, 1]).max()
    scale = np.spacing(np.abs(want[:, 1]).max())
    d = np.abs(out[:, 2] - want[:, 2]).max() / scale
    print(what, 'ln f0: %.2f ulp, delta: %.2f ulp of ln f0' % (u, d))
    assert u <= 4.0, what
    assert d <= 4.0, what
    assert np.array_equal(out[:, 2], pt.delta(out[:, 1])), what


def against_the_twin(sigs, rate, what, **kw):
    from poccala_amd.StatisticalModel.AudioProcessing import pitch_batch
    rows, info = pitch_batch(sigs, rate, details=True, **kw)
    tw = {k: kw[k] for k in ('sampletime', 'overlap', 'f_min', 'f_max', 'ballast', 'soft_min_f0', 'pf') if k in kw}
    for u, x in enumerate(sigs):
        ref = pt.pitch(x, rate, **tw)
        tag = '%s utterance %d' % (what, u)
        assert rows[u].shape == ref['out'].shape and info['nccf_bal'][u].shape == ref['bal'].shape, tag
        assert np.array_equal(info['nccf_bal'][u], ref['bal']), tag              # bit for bit
        assert np.array_equal(info['nccf_raw'][u], ref['raw']), tag
        assert np.array_equal(info['lag'][u], ref['lag']), tag
        check_outputs(rows[u], ref['raw'], ref['lag'], rate, info['lag_min'], tag)
    return rows, info


# ------------------------------------------------------------------ 1. the correlations and everything behind them, from samples
@pytest.mark.parametrize('rate,L', [(8000, 141), (16000, 281)])
def test_ragged_batch_is_the_twins_bits(rate, L):
    sigs = ragged(rate)
    rows, info = against_the_twin(sigs, rate, 'ragged %d Hz' % rate)
    assert info['lag_max'] - info['lag_min'] + 1 == L
    assert [len(r) for r in rows][:4] == [1, 1, 2, 5]
    lmin = info['lag_min']
    # silence: unvoiced, the shortest lag, a flat track
    assert np.all(rows[3][:, 0] == 0.0) and np.all(info['lag'][3] == lmin) and np.all(rows[3][:, 2] == 0.0)
    # the glide is voiced and rises from 120 to 180 Hz
    assert rows[4][2:-3, 0].min() > 0.8 and np.all(np.abs(np.exp(rows[4][1:-3, 1]) - np.linspace(120, 180, len(rows[4]))[1:-3]) < 12.0)
    assert rows[4][3:-5, 2].min() > 0.0


@pytest.mark.parametrize('f_min,L', [(96.0, 64), (95.0, 65)])
def test_one_full_wave_of_lags_and_one_lane_more(f_min, L):
    """8 kHz, lags 20 .. 83 / 84; float64 samples that are no integers, so the mean's summation order shows too"""
    rate = 8000
    sigs = [0.37 * s.astype(np.float64) + 0.123 for s in ragged(rate)]
    rows, info = against_the_twin(sigs, rate, 'L = %d' % L, f_min=f_min, ballast=900.0)
    assert info['nccf_bal'][4].shape[1] == L == info['lag_max'] - info['lag_min'] + 1


def test_int16_and_float64_samples_give_the_same_bits():
    from poccala_amd.StatisticalModel.AudioProcessing import pitch_batch
    sigs = ragged(16000)
    a, ia = pitch_batch(sigs, 16000, details=True)
    b, ib = pitch_batch([s.astype(np.float64) for s in sigs], 16000, details=True)
    c, ic = pitch_batch(sigs, 16000, details=True)                               # and two calls: no atomics anywhere
    for u in range(len(sigs)):
        for x, y, z in ((a[u], b[u], c[u]), (ia['lag'][u], ib['lag'][u], ic['lag'][u]), (ia['nccf_bal'][u], ib['nccf_bal'][u], ic['nccf_bal'][u]),
                        (ia['nccf_raw'][u], ib['nccf_raw'][u], ic['nccf_raw'][u])):
            assert np.array_equal(x, y) and np.array_equal(x, z)
    assert np.array_equal(pitch_batch(sigs, 16000)[4], a[4])                     # without the optional outputs: the same rows


# ------------------------------------------------------------------ 2. the track alone, from given correlations
def test_track_from_given_correlations_is_exact():
    """PCL_PITCH_NCCF_IN with the twin's arrays, random ones on a coarse grid (ties everywhere), a constant (every minimum a tie) and two
    equal peaks: lags exactly equal, T = 1 and T = 2 among them"""
    from poccala_amd.StatisticalModel.AudioProcessing import pitch_batch
    rate = 16000
    size, step, lmin, lmax = pt.geometry(rate)
    L = lmax - lmin + 1
    g = pt.log_lags(lmin, lmax)
    rng = np.random.default_rng(5)
    sigs = ragged(rate)
    tw = [pt.nccf(x, rate) for x in sigs]
    lens = [1, 2, 7, 40, 3]
    bal = [t[0] for t in tw] + [np.round(rng.uniform(-1, 1, (T, L)), 1) for T in lens]
    raw = [t[1] for t in tw] + [np.round(rng.uniform(-1, 1, (T, L)), 2) for T in lens]
    peaks = np.zeros((6, L))
    peaks[:, 30] = peaks[:, 200] = 0.5
    bal += [np.full((9, L), 0.25), peaks]
    raw += [np.full((9, L), 0.25), peaks]
    # signals of the right lengths only: the samples are not read
    dummy = [np.zeros(len(x), dtype=np.int16) for x in sigs] + [np.zeros(size + (len(b) - 1) * step, dtype=np.int16) for b in bal[len(sigs):]]
    for soft in (pt.SOFT_MIN_F0, 0.0):                  # soft_min_f0 = 0: the local cost of the constant case is the same at every lag
        rows, info = pitch_batch(dummy, rate, soft_min_f0=soft, details=True, nccf=(bal, raw))
        for u in range(len(bal)):
            want = pt.track(bal[u], rate, lmin, g, soft_min_f0=soft) + lmin
            assert np.array_equal(info['lag'][u], want), (soft, u)
            check_outputs(rows[u], raw[u], want, rate, lmin, 'given correlations %d (soft %g)' % (u, soft))
        if soft == 0.0:
            assert np.all(info['lag'][-2] == lmin) and np.all(info['lag'][-1] == lmin + 30)


# ------------------------------------------------------------------ 3. end to end on tones whose period is known
@pytest.mark.parametrize('rate', [8000, 16000])
def test_tones_end_to_end(rate):
    from poccala_amd.StatisticalModel.AudioProcessing import pitch_batch
    cases = [(f0, kind) for r, f0 in TONES if r == rate for kind in KINDS]
    rows, info = pitch_batch([tone(rate, f0, kind) for f0, kind in cases], rate, details=True)
    for (f0, kind), out, lag in zip(cases, rows, info['lag']):
        ref = tone_result(rate, f0, kind)
        assert np.all(np.abs(lag[:-3] - rate / f0) <= 1.0), (f0, kind)           # what tests/test_pitch_twin.py asserts of the twin
        assert np.all(out[:-3, 0] >= 0.98), (f0, kind)
        assert np.array_equal(lag, ref['lag']) and np.array_equal(out[:, 0], ref['out'][:, 0]), (f0, kind)
        assert ulps(out[:, 1], ref['out'][:, 1]).max() <= 4.0


def test_the_class_and_the_timer_groups():
    from poccala_amd.runtime import default_engine
    from poccala_amd.StatisticalModel.AudioProcessing import AudioProcessing, pitch_batch
    x = tone(16000, 220, 'harmonics8000')
    p = AudioProcessing.Pitch()
    p.set_signal(x, 16000)
    eng = default_engine()
    eng.enable_timing(True)
    try:
        eng.kernel_time('pitch_nccf'), eng.kernel_time('pitch_track')
        got = p.pitch()
        ms_n, n_n = eng.kernel_time('pitch_nccf')
        ms_t, n_t = eng.kernel_time('pitch_track')
    finally:
        eng.enable_timing(False)
    assert (n_n, n_t) == (1, 1) and ms_n > 0 and ms_t > 0
    assert np.array_equal(got, pitch_batch([x], 16000)[0])
    q = AudioProcessing.Pitch(f_min=100.0, f_max=300.0)
    q.set_signal(x, 16000)
    assert np.array_equal(q.pitch(), pitch_batch([x], 16000, f_min=100.0, f_max=300.0)[0])


# ------------------------------------------------------------------ 4. the fused front-end
def speech(rate, n, seed):
    """int16 PCM: a noise floor, a voiced stretch with a moving pitch in the middle"""
    rng = np.random.default_rng(seed)
    s = 60 * rng.standard_normal(n)
    a, b = int(0.3 * n), int(0.75 * n)
    f = np.linspace(140, 210, b - a) + 10 * np.sin(np.arange(b - a) / 900.0)
    ph = 2 * np.pi * np.cumsum(f) / rate
    s[a:b] += np.hanning(b - a) ** 0.5 * (3000 * np.sin(ph) + 1800 * np.sin(2 * ph + 0.4) + 900 * np.sin(7 * ph))
    s = np.round(s).astype(np.int16)
    s[s == 0] = 1
    return s


SIGS = [speech(16000, n, 40 + k) for k, n in enumerate((9000, 12345, 6400))]


@pytest.mark.parametrize('deltas', [True, False])
@pytest.mark.parametrize('vad', [True, False])
def test_frontend_with_pitch_columns(vad, deltas):
    """D = 13 * 3 + 3 = 42 and 13 + 3 = 16: lens, begin and the MFCC columns are pcl_frontend's bit for bit, the kept set is pcl_vad's on
    the MFCC alone, the last three columns are pcl_pitch's rows at the kept indices rounded to float32"""
    from poccala_amd.runtime import default_engine
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch, pitch_batch, vad_batch
    eng = default_engine()
    D = 39 if deltas else 13
    kw = dict(d1=deltas, d2=deltas, vad=vad)
    lens0, begin0, rows0 = eng.frontend(SIGS, 16000, fetch=True, **kw)
    res0 = eng.frames_download(np.float32).copy()
    lens0b, begin0b, rows0b = eng.frontend(SIGS, 16000, fetch=True, pitch=False, **kw)      # pitch=False IS the plain call
    assert np.array_equal(lens0, lens0b) and np.array_equal(begin0, begin0b) and np.array_equal(rows0, rows0b)
    assert np.array_equal(eng.frames_download(np.float32), res0) and (eng.F, eng.FD) == (rows0.shape[0], D)
    lens, begin, rows = eng.frontend(SIGS, 16000, fetch=True, pitch=True, **kw)
    res = eng.frames_download(np.float32).copy()
    assert (eng.F, eng.FD) == (int(lens.sum()), D + 3) and rows.shape == (eng.F, D + 3) and res.shape == (eng.F, D + 3)
    assert lens.dtype == np.int32 and begin.dtype == np.int64
    assert np.array_equal(lens, lens0) and np.array_equal(begin, begin0)
    assert np.array_equal(res[:, :D], res0) and np.array_equal(rows[:, :D], rows0)
    mats = mfcc_batch(SIGS, 16000, d1=deltas, d2=deltas)
    kept = vad_batch(mats, details=True)[1]['kept'] if vad else [np.arange(len(m)) for m in mats]
    assert [len(k) for k in kept] == lens.tolist() and 0 < lens.sum() and (not vad or lens.sum() < sum(len(m) for m in mats))
    pit = pitch_batch(SIGS, 16000)
    want = np.concatenate([p[k] for p, k in zip(pit, kept)])
    assert np.array_equal(rows[:, D:], want)
    assert np.array_equal(res[:, D:], np.float32(want))
    assert want[:, 0].max() > 0.9                                                # voiced frames did survive
    # float64 samples take the other entry point: the same bits
    lens2, begin2, rows2 = eng.frontend([s.astype(np.float64) for s in SIGS], 16000, fetch=True, pitch=True, **kw)
    assert np.array_equal(lens2, lens) and np.array_equal(begin2, begin) and np.array_equal(rows2, rows)
    assert np.array_equal(eng.frames_download(np.float32), res)
    # keep_f64: the float64 copy holds the survivors themselves
    eng.frontend(SIGS, 16000, pitch=True, keep_f64=True, **kw)
    assert np.array_equal(eng.frames_download(np.float64), rows)


def test_a_batch_on_the_wide_frames_scores_against_a_wide_model():
    """J = 4, M = 8, D = 42: ln b of every state on the resident 42-column rows within the project's float32 bound of the oracle"""
    from oracle import poccala_oracle as po
    from poccala_amd import PCL_F32
    from poccala_amd.runtime import default_engine
    eng = default_engine()
    lens, begin, rows = eng.frontend(SIGS, 16000, fetch=True, pitch=True)
    x = eng.frames_download(np.float32).astype(np.float64)
    assert x.shape[1] == 42
    rng = np.random.default_rng(9)
    J, M = 4, 8
    sd = x.std(axis=0) + 1e-3
    mean = x[rng.choice(len(x), J * M, replace=False)].reshape(J, M, 42) + 0.3 * sd * rng.standard_normal((J, M, 42))
    var = (sd ** 2) * rng.uniform(0.5, 2.0, (J, M, 42))
    w = rng.dirichlet(np.ones(M) * 3, J)
    eng.load_model(mean, var, w)
    keep = lens > 0
    b = eng.all_state_batch(lens[keep], begin[keep])
    b.score(PCL_F32)
    B = [m.copy() for m in b.get('B')]
    b.close()
    for u, (T, f0) in enumerate(zip(lens[keep], begin[keep])):
        for j in range(J):
            ref = po.gmm_point(x[f0:f0 + T], mean[j], var[j], w[j])
            assert np.isfinite(ref).all()
            hold('pitch columns D=42', 'ln b on the resident rows', B[u][1 + j], ref, 0.0, F32_LOGLIK_ATOL)


# ------------------------------------------------------------------ 5. refusals, and what a refused call leaves behind
def test_refusals_leave_everything_as_it_was():
    from poccala_amd import PoccalaHipError
    from poccala_amd.engine import Engine
    from poccala_amd.runtime import default_engine
    from poccala_amd.StatisticalModel.AudioProcessing import pitch_batch
    eng = default_engine()
    x = tone(8000, 150.3, 'sine')
    pitch_batch([x], 8000)                                                       # (anything the context keeps is there from here on)
    blocks = Engine.pool_stats()['handed_out_blocks']
    with pytest.raises(PoccalaHipError) as e:
        pitch_batch([x], 8000, f_max=4000.5)
    assert e.value.code == -1 and 'half the sample rate' in str(e.value)
    with pytest.raises(PoccalaHipError) as e:
        pitch_batch([tone(16000, 150.3, 'sine')], 16000, f_min=10.0)
    assert e.value.code == -1 and '1561 lags, at most 1024' in str(e.value)
    with pytest.raises(PoccalaHipError) as e:
        pitch_batch([x], 8000, f_min=399.0, f_max=400.0)
    assert e.value.code == -1 and 'at least 2' in str(e.value)
    a = pitch_batch([x, x[:37]], 8000)
    assert Engine.pool_stats()['handed_out_blocks'] == blocks                    # every pooled block of a call goes back, refused or not
    # the front-end: a good call, then refused ones, which leave its frame matrix, F and D in place
    lens, begin, rows = eng.frontend(SIGS, 16000, fetch=True, pitch=True)
    res = eng.frames_download(np.float32).copy()
    F, FD = eng.F, eng.FD
    blocks = Engine.pool_stats()['handed_out_blocks']
    for kw, text in ((dict(f_max=8000.5), 'half the sample rate'), (dict(f_min=10.0), 'at most 1024'),
                     (dict(vec_num=21), 'feature dimension 66 > 64'), (dict(simple_size=64), 'fewer than simple_size')):
        with pytest.raises(PoccalaHipError) as e:
            eng.frontend(SIGS, 16000, pitch=True, **kw)
        assert e.value.code == -1 and text in str(e.value), str(e.value)
        assert (eng.F, eng.FD) == (F, FD) == (res.shape[0], 42)
        assert np.array_equal(eng.frames_download(np.float32), res)
        assert Engine.pool_stats()['handed_out_blocks'] == blocks
    lens63, _ = eng.frontend(SIGS, 16000, vec_num=21)                            # 63 columns without the pitch are fine
    assert eng.FD == 63 and lens63.sum() > 0
    # determinism, and the pool's count after a second good call
    lens2, begin2, rows2 = eng.frontend(SIGS, 16000, fetch=True, pitch=True)
    assert np.array_equal(lens2, lens) and np.array_equal(begin2, begin) and np.array_equal(rows2, rows)
    assert np.array_equal(eng.frames_download(np.float32), res)
    assert Engine.pool_stats()['handed_out_blocks'] == blocks
    assert np.array_equal(pitch_batch([x, x[:37]], 8000)[1], a[1])
