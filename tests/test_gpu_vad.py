"""The voice-activity detector on the GPU (row f6): against the reference's own outputs (golden G19), against its NumPy twin on random
ragged batches (bit for bit from the device's own distances), and the fused PCM -> resident frames path of Engine.frontend."""
import wave

import numpy as np
import pytest

import _vad_twin as vt
from test_vad_twin import CASES, load_case

pytestmark = pytest.mark.gpu

DIST_RTOL = 1e-12     # the two differ in the order of a sum over D <= 64 terms: about D 2^-53


def speech_signal(rng, n, rate=16000, lead=0.3, tail=0.25, level=3000):
    """int16 PCM: a noise floor, with a voiced stretch in the middle."""
    t = np.arange(n) / rate
    s = 60 * rng.standard_normal(n)
    a, b = int(lead * n), int((1 - tail) * n)
    env = np.zeros(n)
    env[a:b] = np.hanning(b - a) ** 0.5
    s += env * (level * np.sin(2 * np.pi * 180 * t) + 0.6 * level * np.sin(2 * np.pi * 360 * t + 0.4) + 0.3 * level * np.sin(2 * np.pi * 1500 * t))
    s = np.round(s).astype(np.int16)
    s[s == 0] = 1                      # MFCC.init_audio deletes zero samples
    return s


# ------------------------------------------------------------------ 3. the device against the reference (G19)
@pytest.mark.parametrize('tag', CASES)
def test_vad_class_matches_the_reference(golden, tag):
    from poccala_amd.StatisticalModel.AudioProcessing import AudioProcessing
    c = load_case(golden('G19_vad'), tag)
    v = AudioProcessing.VAD(c['s'])
    v.init_mfcc(c['x'])
    dist = v.mel_distance(alpha=c['alpha'])
    print(tag, 'max relative distance error', np.max(np.abs(dist - c['dist']) / c['dist']))
    np.testing.assert_allclose(dist, c['dist'], rtol=DIST_RTOL, atol=0)
    sm = v.osf(c['dist'], beta=c['beta'])                         # from the reference's distances: its bits
    assert np.array_equal(sm, c['osf'])
    assert np.array_equal(v.detect(c['osf']), c['x'][c['kept']])
    assert np.array_equal(v.detect(v.osf(dist, beta=c['beta'])), c['x'][c['kept']])       # the three methods chained
    if (c['alpha'], c['beta']) == (0.5, 0.93):
        assert np.array_equal(v.mfcc(), c['x'][c['kept']])


def test_vad_batch_matches_the_reference(golden):
    from poccala_amd.StatisticalModel.AudioProcessing import vad_batch
    g = golden('G19_vad')
    for D in (13, 39):
        cs = [load_case(g, t) for t in CASES]
        cs = [c for c in cs if c['x'].shape[1] == D and (c['s'], c['alpha'], c['beta']) == (16, 0.5, 0.93)]
        assert len(cs) >= 1
        rows, info = vad_batch([c['x'] for c in cs], details=True)
        for c, r, k, d, o, t in zip(cs, rows, info['kept'], info['dist'], info['osf'], info['thr']):
            assert np.array_equal(k, c['kept'])
            assert np.array_equal(r, c['x'][c['kept']])
            np.testing.assert_allclose(d, c['dist'], rtol=DIST_RTOL, atol=0)
            own = vt.from_distances(d, 16, 0.93)                  # behind the distances everything is exact
            assert np.array_equal(o, own['osf']) and t == own['thr']
    c = load_case(g, 's8')
    rows = vad_batch([c['x'], c['x']], simple_size=8, beta=c['beta'])
    assert np.array_equal(rows[0], c['x'][c['kept']]) and np.array_equal(rows[1], rows[0])


def test_plotting_is_not_supported():
    from poccala_amd.StatisticalModel.AudioProcessing import AudioProcessing
    v = AudioProcessing.VAD()
    v.init_mfcc(np.zeros((20, 13)))
    with pytest.raises(NotImplementedError):
        v.mfcc(show_pic=True)
    with pytest.raises(NotImplementedError):
        v.detect(np.zeros(20), show_pic=True)


def test_short_input_raises_like_the_reference():
    from poccala_amd import PoccalaHipError
    from poccala_amd.StatisticalModel.AudioProcessing import AudioProcessing, vad_batch
    v = AudioProcessing.VAD()
    v.init_mfcc(np.random.default_rng(0).standard_normal((15, 13)))
    with pytest.raises(IndexError):
        v.mfcc()
    with pytest.raises(IndexError):
        v.mel_distance()
    rng = np.random.default_rng(1)
    with pytest.raises(PoccalaHipError) as e:
        vad_batch([rng.standard_normal((40, 13)), rng.standard_normal((15, 13)), rng.standard_normal((16, 13))])
    assert e.value.code == -1 and 'utterance 1' in str(e.value)
    with pytest.raises(PoccalaHipError) as e:                     # h + 1 = 16 = 2 s: the reference indexes out of range
        vad_batch([rng.standard_normal((40, 13))], simple_size=8)
    assert e.value.code == -1
    with pytest.raises(PoccalaHipError) as e:                     # D beyond the device dimension limit, as pcl_frames_upload
        vad_batch([rng.standard_normal((40, 65))])
    assert e.value.code == -1 and '> 64' in str(e.value)


# ------------------------------------------------------------------ random ragged batches against the twin
def random_batch(seed):
    rng = np.random.default_rng(7000 + seed)
    s = int(rng.choice([4, 8, 16, 33]))
    D = int(rng.choice([13, 26, 39, 40]))
    U = int(rng.choice([1, 2, 40, int(rng.integers(1, 41))]))
    beta = float(rng.uniform(0.05, (2 * s - 1) / (2 * s + 1) - 0.01))
    assert 0 <= vt.osf_h(s, beta) and vt.osf_h(s, beta) + 1 < 2 * s
    alpha = float(rng.uniform(0.1, 0.9))
    mats = []
    for u in range(U):
        T = int(rng.choice([s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, 2000, int(rng.integers(s, 2001))]))
        x = rng.standard_normal((T, D)) * np.abs(np.sin(np.arange(T) * rng.uniform(0.01, 0.2)) * 3 + 0.3)[:, None]
        for _ in range(int(rng.integers(0, 4))):                  # constant stretches: equal distances exercise the tie rule
            a = int(rng.integers(0, T))
            b = min(T, a + int(rng.integers(2, 3 * s + 3)))
            x[a:b] = x[a]
        if rng.random() < 0.3:                                    # a coarse grid: many equal distances all over
            x = np.round(x)
        mats.append(x)
    return s, alpha, beta, mats


@pytest.mark.parametrize('seed', range(10))
def test_random_ragged_batches_match_the_twin(seed):
    from poccala_amd.StatisticalModel.AudioProcessing import vad_batch
    s, alpha, beta, mats = random_batch(seed)
    if seed == 3:
        # one batch carries a -inf row: past the noise sample, and in the last s frames, which the filter leaves alone (inside its range
        # a lone infinite distance is the largest of every window that holds it and is smoothed away unless h + 1 = 2 s - 1)
        u = len(mats) // 2
        if len(mats[u]) <= s:
            mats[u] = np.concatenate([mats[u], mats[u]])
        mats[u][-1] = -np.inf
    rows, info = vad_batch(mats, simple_size=s, alpha=alpha, beta=beta, details=True)
    worst = 0.0
    for u, x in enumerate(mats):
        ref = vt.vad(x, s, alpha, beta)
        d = info['dist'][u]
        fin = np.isfinite(ref['dist']) & (ref['dist'] > 0)
        if fin.any():
            worst = max(worst, float(np.max(np.abs(d[fin] - ref['dist'][fin]) / ref['dist'][fin])))
        np.testing.assert_allclose(d, ref['dist'], rtol=DIST_RTOL, atol=0)
        # second leg: everything behind the distances is exact -- no tolerance, no exclusions
        own = vt.from_distances(d, s, beta)
        assert np.array_equal(info['osf'][u], own['osf'], equal_nan=True), (seed, u)
        assert np.array_equal(np.float64(info['thr'][u]), np.float64(own['thr']), equal_nan=True), (seed, u)
        assert np.array_equal(info['kept'][u], own['kept']), (seed, u)
        assert np.array_equal(rows[u], x[own['kept']], equal_nan=True), (seed, u)
        if seed == 3 and u == len(mats) // 2:
            assert len(rows[u]) == 0 and np.isnan(info['thr'][u])
    print('seed', seed, 's', s, 'U', len(mats), 'worst relative distance error', worst)


def test_raw_counts_offsets_and_padding_of_pcl_vad():
    """kept_len / kept_idx as the C-ABI lays them out: utterance u's indices at row_off[u], -1 behind them; two runs, the same bits."""
    from poccala_amd.StatisticalModel.AudioProcessing import _vad_call
    from poccala_amd.runtime import default_engine
    s, alpha, beta, mats = random_batch(100)
    a = _vad_call(default_engine(), mats, s, alpha, beta, 0, ('dist', 'osf', 'kept'))
    b = _vad_call(default_engine(), mats, s, alpha, beta, 0, ('dist', 'osf', 'kept'))
    for k in ('dist', 'osf', 'kept_len', 'kept_idx', 'thr'):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    off = a['row_off']
    for u, x in enumerate(mats):
        own = vt.from_distances(a['dist'][off[u]:off[u + 1]], s, beta)
        n = a['kept_len'][u]
        assert n == len(own['kept'])
        seg = a['kept_idx'][off[u]:off[u + 1]]
        assert np.array_equal(seg[:n], own['kept']) and np.all(seg[n:] == -1)


# ------------------------------------------------------------------ 4. the fused path
def small_model(D, seed=3):
    from poccala_amd import synth
    mean, var, w, _ = synth.make_model(2, 4, D, seed=seed)
    return mean * 4.0, var * 8.0 + 4.0, w


def score_resident(eng, lens, begin, precision):
    keep = lens > 0
    b = eng.all_state_batch(lens[keep], begin[keep])
    b.score(precision)
    B = [m.copy() for m in b.get('B')]
    b.close()
    return B


def mfcc_then_twin(sigs, rate, **kw):
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch
    mats = mfcc_batch(sigs, rate, d1=True, d2=True)
    return (mats,) + vt.vad_batch(mats, **kw)


def ragged_signals():
    rng = np.random.default_rng(77)
    return [speech_signal(rng, n) for n in (16000, 9000, 12345, 4000, 30000)]


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_frontend_on_the_mfcc_golden_signals(golden, tag):
    from poccala_amd.runtime import default_engine
    g = golden('G10_mfcc')
    sig, rate = g['signal_' + tag], int(g['rate_' + tag])
    lens, begin, rows = default_engine().frontend([sig], rate, fetch=True)
    _, rl, rb, rr = mfcc_then_twin([sig], rate)
    assert np.array_equal(lens, rl) and np.array_equal(begin, rb)
    np.testing.assert_allclose(rows, rr, rtol=1e-8, atol=1e-8)
    # and against the reference's own MFCC of the signal, through the twin
    ref = vt.vad(g['mfcc39_' + tag])
    assert lens[0] == len(ref['kept'])
    np.testing.assert_allclose(rows, g['mfcc39_' + tag][ref['kept']], rtol=1e-8, atol=1e-8)


def test_frontend_ragged_batch_and_resident_layout():
    from poccala_amd import PCL_F32, PCL_F64
    from poccala_amd.runtime import default_engine
    eng = default_engine()
    sigs = ragged_signals()
    lens, begin, rows = eng.frontend(sigs, 16000, fetch=True)
    _, rl, rb, rr = mfcc_then_twin(sigs, 16000)
    assert np.array_equal(lens, rl) and np.array_equal(begin, rb)
    assert lens.dtype == np.int32 and begin.dtype == np.int64 and 0 < lens.sum() < sum(len(m) for m in _)
    np.testing.assert_allclose(rows, rr, rtol=1e-8, atol=1e-8)
    assert (eng.F, eng.FD) == (rows.shape[0], 39)
    # ln b scored on the resident frames == ln b after uploading the fetched rows: layout, padding and cast are the upload path's
    eng.load_model(*small_model(39))
    for prec in (PCL_F32, PCL_F64):
        lens2, begin2 = eng.frontend(sigs, 16000)
        assert np.array_equal(lens2, lens) and np.array_equal(begin2, begin)
        B_res = score_resident(eng, lens, begin, prec)
        eng.load_frames(np.float32(rows))
        B_up = score_resident(eng, lens, begin, prec)
        assert all(np.isfinite(b[1:-1]).all() for b in B_up)
        for a, b in zip(B_res, B_up):
            assert np.array_equal(a, b)
    # keep_f64: parity mode reads the float64 survivors themselves, as after a float64 upload
    eng.frontend(sigs, 16000, keep_f64=True)
    B_res = score_resident(eng, lens, begin, PCL_F64)
    eng.load_frames(rows)
    B_up = score_resident(eng, lens, begin, PCL_F64)
    for a, b in zip(B_res, B_up):
        assert np.array_equal(a, b)


def test_frontend_with_a_padded_dimension():
    """vec_num = 12 with both deltas gives D = 36, which has no kernel instance of its own: rows are padded to 39 as pcl_frames_upload pads."""
    from poccala_amd import PCL_F32
    from poccala_amd.runtime import default_engine
    eng = default_engine()
    sigs = ragged_signals()[:3]
    lens, begin, rows = eng.frontend(sigs, 16000, vec_num=12, fetch=True)
    assert rows.shape[1] == 36
    eng.load_model(*small_model(36))
    B_res = score_resident(eng, lens, begin, PCL_F32)
    eng.load_frames(np.float32(rows))
    B_up = score_resident(eng, lens, begin, PCL_F32)
    for a, b in zip(B_res, B_up):
        assert np.array_equal(a, b)


def test_frontend_without_the_detector_is_mfcc_plus_upload():
    from poccala_amd import PCL_F32
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch
    from poccala_amd.runtime import default_engine
    eng = default_engine()
    sigs = ragged_signals()
    mats = mfcc_batch(sigs, 16000, d1=True, d2=True)
    lens, begin, rows = eng.frontend(sigs, 16000, vad=False, fetch=True)
    assert lens.tolist() == [len(m) for m in mats]
    assert begin.tolist() == np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    assert np.array_equal(rows, np.concatenate(mats))
    eng.load_model(*small_model(39))
    B_res = score_resident(eng, lens, begin, PCL_F32)
    eng.load_frames(np.float32(np.concatenate(mats)))
    B_up = score_resident(eng, lens, begin, PCL_F32)
    for a, b in zip(B_res, B_up):
        assert np.array_equal(a, b)


def test_frontend_short_utterance_fails_and_keeps_the_frames():
    from poccala_amd import PCL_F32, PoccalaHipError
    from poccala_amd.runtime import default_engine
    eng = default_engine()
    rng = np.random.default_rng(5)
    sigs = ragged_signals()[:2]
    eng.load_model(*small_model(39))
    lens, begin = eng.frontend(sigs, 16000)
    before = score_resident(eng, lens, begin, PCL_F32)
    F = eng.F
    short = speech_signal(rng, 400 + 200 * 14)                    # 15 frames
    with pytest.raises(PoccalaHipError) as e:
        eng.frontend([sigs[0], short], 16000)
    assert e.value.code == -1 and 'utterance 1' in str(e.value)
    assert eng.F == F
    after = score_resident(eng, lens, begin, PCL_F32)             # the previous frame matrix is still the current one
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    lens3, _ = eng.frontend([sigs[0], short], 16000, vad=False)   # without the detector 15 frames are fine
    assert lens3[1] == 15


def test_frontend_reports_an_empty_utterance_with_length_zero():
    """Digital silence: ln 0 = -inf in the MFCC, every distance of that utterance is NaN, so is its threshold, and nothing of it is kept;
    its neighbours are untouched."""
    from poccala_amd.runtime import default_engine
    eng = default_engine()
    sigs = ragged_signals()[:2]
    flat = np.zeros(8000, dtype=np.int16)
    lens, begin, rows = eng.frontend([sigs[0], flat, sigs[1]], 16000, fetch=True)
    mats, rl, rb, rr = mfcc_then_twin([sigs[0], flat, sigs[1]], 16000)
    assert np.array_equal(lens, rl) and np.array_equal(begin, rb)
    assert lens[1] == 0 and lens[0] > 0 and lens[2] > 0
    assert begin[2] == begin[1] == lens[0]
    np.testing.assert_allclose(rows, rr, rtol=1e-8, atol=1e-8)


# ------------------------------------------------------------------ 5. AcousticModel.load_audio
def write_wav(path, sig, rate=16000):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(sig.tobytes())


def test_load_audio_is_mfcc_then_vad(tmp_path):
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    from poccala_amd.StatisticalModel.AudioProcessing import AudioProcessing
    rng = np.random.default_rng(11)
    sig = speech_signal(rng, 14000)
    write_wav(tmp_path / 'a.wav', sig)
    for kw, D in ((dict(), 39), (dict(delta_2=False), 26), (dict(delta_1=False, delta_2=False), 13)):
        got = AcousticModel(**kw).load_audio(str(tmp_path / 'a.wav'))
        m = AudioProcessing.MFCC(13)
        m.init_audio(path=str(tmp_path / 'a.wav'))
        feats = m.mfcc(nfft=512, d1=kw.get('delta_1', True), d2=kw.get('delta_2', True))
        v = AudioProcessing.VAD()
        v.init_mfcc(feats)
        want = v.mfcc()
        assert got.shape[1] == D and 0 < len(got) < len(feats)
        assert np.array_equal(got, want)
        assert np.array_equal(got, feats[vt.vad(feats)['kept']])


def test_load_audio_batch_equals_the_single_calls(tmp_path):
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    from poccala_amd.runtime import default_engine
    rng = np.random.default_rng(12)
    paths = []
    for k, n in enumerate((14000, 9000, 21000)):
        write_wav(tmp_path / ('%d.wav' % k), speech_signal(rng, n))
        paths.append(str(tmp_path / ('%d.wav' % k)))
    am = AcousticModel()
    single = [am.load_audio(p) for p in paths]
    lens, begin, data = am.load_audio_batch(paths)
    assert lens.tolist() == [len(x) for x in single]
    assert begin.tolist() == [0, len(single[0]), len(single[0]) + len(single[1])]
    for a, b in zip(single, data):
        assert np.array_equal(a, b)
    assert default_engine().F == sum(len(x) for x in single)
    lens2, begin2, none = am.load_audio_batch(paths, fetch=False)
    assert none is None and np.array_equal(lens2, lens) and np.array_equal(begin2, begin)


# ------------------------------------------------------------------ the selection itself: non-finite distances inside the filter's range, wide windows
@pytest.mark.parametrize('seed', range(8))
def test_filter_on_given_distances_is_the_twins_bits(seed):
    """pcl_vad from the caller's distances (PCL_VAD_DIST_IN): +inf, NaN and runs of equal values INSIDE the filtered range, so that they
    enter the rank counting (NaN sorts last, as np.sort has it); simple_size up to 100 (a window of 200 values, 7 KB of LDS)."""
    from poccala_amd._lib import PCL_VAD_DIST_IN
    from poccala_amd.StatisticalModel.AudioProcessing import _vad_call
    from poccala_amd.runtime import default_engine
    rng = np.random.default_rng(8100 + seed)
    s = [4, 16, 33, 64, 100, 16, 64, 100][seed]
    h_top = 2 * s - 2                                             # the largest admissible h: w[h + 1] is the window's maximum
    beta = [0.93 if s == 16 else (h_top + 0.5) / (2 * s + 1), float(rng.uniform(0.05, (2 * s - 1) / (2 * s + 1) - 0.01))][seed % 2]
    assert 0 <= vt.osf_h(s, beta) and vt.osf_h(s, beta) + 1 < 2 * s
    dists = []
    for u in range(int(rng.integers(3, 12))):
        T = int(rng.choice([2 * s + 1, 3 * s, 700, int(rng.integers(2 * s + 1, 1500))]))
        d = np.abs(rng.standard_normal(T)) * 3
        if rng.random() < 0.5:
            d = np.round(d, 1)                                    # many ties
        kind = u % 4
        mid = int(rng.integers(s, T - s))                         # inside the filtered range
        if kind == 1:
            d[mid] = np.inf
        elif kind == 2:
            d[mid] = np.nan
        elif kind == 3:
            d[mid:mid + 3] = [np.nan, np.inf, np.nan][:len(d[mid:mid + 3])]
        dists.append(d)
    r = _vad_call(default_engine(), None, s, 0.5, beta, PCL_VAD_DIST_IN, ('osf', 'kept'), dist=dists)
    off = r['row_off']
    some_nonfinite = False
    for u, d in enumerate(dists):
        own = vt.from_distances(d, s, beta)
        got = r['osf'][off[u]:off[u + 1]]
        assert np.array_equal(got, own['osf'], equal_nan=True), (seed, u)
        assert np.array_equal(np.float64(r['thr'][u]), np.float64(own['thr']), equal_nan=True), (seed, u)
        n = r['kept_len'][u]
        assert n == len(own['kept']) and np.array_equal(r['kept_idx'][off[u]:off[u] + n], own['kept']), (seed, u)
        some_nonfinite |= bool((~np.isfinite(own['osf'])).any())
    if seed % 2 == 0:                                             # h + 1 = 2 s - 1: the window's maximum is selected
        assert some_nonfinite                                     # an infinite / NaN distance did come out of the selection


@pytest.mark.parametrize('s', [64, 100])
def test_wide_windows_from_features(s):
    from poccala_amd.StatisticalModel.AudioProcessing import vad_batch
    rng = np.random.default_rng(s)
    mats = [rng.standard_normal((T, 39)) * np.linspace(0.3, 3, T)[:, None] for T in (s, 2 * s, 2 * s + 1, 5 * s + 7, 1000)]
    beta = 0.9
    rows, info = vad_batch(mats, simple_size=s, beta=beta, details=True)
    for u, x in enumerate(mats):
        np.testing.assert_allclose(info['dist'][u], vt.mel_distance(x, s), rtol=DIST_RTOL, atol=0)
        own = vt.from_distances(info['dist'][u], s, beta)
        assert np.array_equal(info['osf'][u], own['osf']) and np.array_equal(info['kept'][u], own['kept'])
        assert np.array_equal(rows[u], x[own['kept']])


def test_order_statistic_is_checked_only_where_a_frame_is_filtered():
    """simple_size = 8 at the default beta: h + 1 = 16 lies outside the window, which the reference notices only when a frame is filtered
    (T > 2 s).  With every T <= 16 the class and the batch call return rows as the reference does; one longer utterance is the error."""
    from poccala_amd import PoccalaHipError
    from poccala_amd.StatisticalModel.AudioProcessing import AudioProcessing, vad_batch
    rng = np.random.default_rng(21)
    mats = [rng.standard_normal((T, 13)) * np.linspace(0.5, 3, T)[:, None] for T in (8, 12, 16)]
    rows = vad_batch(mats, simple_size=8)
    for x, r in zip(mats, rows):
        ref = vt.vad(x, 8)                                        # the twin, like the reference, never indexes the window here
        assert np.array_equal(r, x[ref['kept']])
        v = AudioProcessing.VAD(8)
        v.init_mfcc(x)
        assert np.array_equal(v.mfcc(), r)
        np.testing.assert_allclose(v.osf(v.mel_distance()), ref['dist'], rtol=DIST_RTOL, atol=0)     # nothing to filter
    with pytest.raises(PoccalaHipError):
        vad_batch(mats + [rng.standard_normal((17, 13))], simple_size=8)
    v = AudioProcessing.VAD(8)
    v.init_mfcc(rng.standard_normal((17, 13)))
    with pytest.raises(PoccalaHipError):
        v.mfcc()


def test_frontend_when_nothing_survives_anywhere():
    """The same convention as for one empty utterance among others: every length 0, and the frame matrix is empty."""
    from poccala_amd import PoccalaHipError
    from poccala_amd.runtime import default_engine
    eng = default_engine()
    silent = [np.zeros(8000, dtype=np.int16), np.zeros(5000, dtype=np.int16)]
    lens, begin, rows = eng.frontend(silent, 16000, fetch=True)
    assert lens.tolist() == [0, 0] and begin.tolist() == [0, 0]
    assert rows.shape == (0, 39) and eng.F == 0
    eng.load_model(*small_model(39))
    with pytest.raises(PoccalaHipError):                          # no batch can be made on an empty frame matrix
        eng.all_state_batch(np.array([1], dtype=np.int32), np.array([0], dtype=np.int64))
    lens, begin = eng.frontend(ragged_signals()[:1], 16000)       # and the engine goes on
    assert lens[0] > 0 and eng.F == lens[0]


# ------------------------------------------------------------------ empty utterances through AcousticModel's batch helpers
def test_batch_helpers_skip_an_utterance_without_frames(golden):
    from test_gpu_dropin import RecLog, S, build_units
    from poccala_amd import PCL_F64
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    g = golden('G6_small_fix0')
    label, hmm_list = build_units(g)
    am = AcousticModel(RecLog(), 'XIF_tone', state_num=S, mix_level=4)
    unit_hmms = {u: hmm_list[label.index(u)] for u in set(label)}
    x = np.asarray(g['x'])
    empty = np.zeros((0, x.shape[1]))
    labels3, data3 = [label, label, label], [x, empty, x[:len(x) - 1]]
    labels2, data2 = [label, label], [x, x[:len(x) - 1]]
    st3, acc3, lp3 = am.estep_batch(labels3, data3, unit_hmms, fix_code=0, precision=PCL_F64)
    st2, acc2, lp2 = am.estep_batch(labels2, data2, unit_hmms, fix_code=0, precision=PCL_F64)
    assert np.isnan(lp3[1]) and np.array_equal(lp3[[0, 2]], lp2)
    # the same two utterances in the same order on the device: at most the order of a sum over < 200 frames differs (n 2^-53 = 2e-14)
    for k in st2:
        np.testing.assert_allclose(st3[k], st2[k], rtol=1e-12, atol=0, err_msg=k)
    assert sorted(acc3) == sorted(acc2)
    for u in acc2:
        np.testing.assert_allclose(acc3[u][0], acc2[u][0], rtol=1e-12, atol=0)
        np.testing.assert_allclose(acc3[u][1], acc2[u][1], rtol=1e-12, atol=0)
    al3 = am.align_batch(labels3, data3, unit_hmms)
    al2 = am.align_batch(labels2, data2, unit_hmms)
    assert np.isnan(al3[1][0]) and len(al3[1][1]) == 0
    for a, b in zip([al3[0], al3[2]], al2):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    seg3, drop3 = am.segment_batch(labels3, data3, unit_hmms)
    seg2, drop2 = am.segment_batch(labels2, data2, unit_hmms)
    assert drop3 == sorted([1] + [[0, 2][u] for u in drop2])
    assert sorted(seg3) == sorted(seg2) and all(len(seg3[u]) == len(seg2[u]) for u in seg2)
    rg3, rdrop3 = am.regroup_batch(labels3, data3, unit_hmms)
    rg2, rdrop2 = am.regroup_batch(labels2, data2, unit_hmms)
    assert rdrop3 == sorted([1] + [[0, 2][u] for u in rdrop2])
    for u in rg2:
        for a, b in zip(rg3[u], rg2[u]):
            assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        am.estep_batch([label], [empty], unit_hmms)
