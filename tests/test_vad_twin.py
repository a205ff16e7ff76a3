"""The NumPy twin of the voice-activity detector (tests/_vad_twin.py) against the reference's own outputs (golden G19).  CPU only."""
import numpy as np
import pytest

import _vad_twin as vt

CASES = ['speech39', 'speech13', 't16', 't17', 't31', 't32', 't33', 't40', 's8', 'piecewise']


def load_case(g, tag):
    s, alpha, beta = g[tag + '_params']
    return dict(x=g[tag + '_x'], dist=g[tag + '_dist'], osf=g[tag + '_osf'], kept=g[tag + '_kept'], thr=float(g[tag + '_thr']),
                s=int(s), alpha=float(alpha), beta=float(beta))


def test_the_golden_lists_the_cases(golden):
    assert sorted(golden('G19_vad')['cases'].tolist()) == sorted(CASES)


@pytest.mark.parametrize('tag', CASES)
def test_twin_matches_the_reference(golden, tag):
    c = load_case(golden('G19_vad'), tag)
    r = vt.vad(c['x'], c['s'], c['alpha'], c['beta'])
    assert np.array_equal(r['kept'], c['kept'])
    # the two differ in the order of the sum over D <= 64 terms only: about D 2^-53
    np.testing.assert_allclose(r['dist'], c['dist'], rtol=1e-12, atol=0)


@pytest.mark.parametrize('tag', CASES)
def test_twin_is_bit_equal_from_the_reference_distances(golden, tag):
    """Selection is exact and the blend / the threshold are single rounded operations: fed the reference's distances, the twin
    reproduces its smoothed distances, threshold and kept set bit for bit."""
    c = load_case(golden('G19_vad'), tag)
    r = vt.from_distances(c['dist'], c['s'], c['beta'])
    assert np.array_equal(r['osf'], c['osf'])
    assert r['thr'] == c['thr']
    assert np.array_equal(r['kept'], c['kept'])


def test_golden_covers_what_it_should(golden):
    g = golden('G19_vad')
    shapes = {t: g[t + '_x'].shape for t in CASES}
    assert shapes['speech39'][1] == 39 and shapes['speech13'][1] == 13
    assert [shapes['t%d' % T][0] for T in (16, 17, 31, 32, 33, 40)] == [16, 17, 31, 32, 33, 40]
    assert int(g['s8_params'][0]) == 8
    assert (float(g['piecewise_params'][1]), float(g['piecewise_params'][2])) == (0.3, 0.8)
    for t in CASES:                                              # the gap that lets every test demand the exact kept set
        gap = np.abs(g[t + '_osf'] - g[t + '_thr']) / abs(g[t + '_thr'])
        assert gap.min() >= 1e-6, (t, gap.min())
        assert 0 < len(g[t + '_kept']) <= shapes[t][0]


def test_short_input_raises():
    with pytest.raises(IndexError):
        vt.vad(np.zeros((15, 13)))
    with pytest.raises(IndexError):
        vt.vad(np.ones((7, 5)), s=8)
    assert len(vt.vad(np.random.default_rng(0).standard_normal((16, 13)))['dist']) == 16


def test_filter_range_and_window():
    """s <= T <= 2s: no frame is filtered; at T = 2s + 1 exactly frame s is, from the 2s values d[0:2s] (not 2s + 1)."""
    rng = np.random.default_rng(3)
    for T in (16, 31, 32):
        d = rng.random(T)
        assert np.array_equal(vt.osf(d), d)
    d = rng.random(33)
    out = vt.osf(d)
    w = np.sort(d[0:32])
    assert out[16] == (1 - 0.93) * w[30] + 0.93 * w[31]
    assert np.array_equal(np.delete(out, 16), np.delete(d, 16))


def test_order_statistic_outside_the_window_raises():
    with pytest.raises(IndexError):
        vt.osf(np.arange(40.), s=8)                             # h + 1 = 16 = 2s, as the reference fails


def test_non_finite_distances_follow_the_arithmetic():
    d = np.abs(np.random.default_rng(4).standard_normal(50)) + 1
    d[20] = np.inf
    r = vt.from_distances(d)
    assert np.isnan(r['thr']) and len(r['kept']) == 0          # (inf - min) / inf
    d[20] = np.nan
    r = vt.from_distances(d)
    assert np.isnan(r['thr']) and len(r['kept']) == 0


def test_batch_helper_reports_empty_utterances():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((40, 13)) * np.linspace(0.5, 3, 40)[:, None]
    b = a.copy()
    b[30] = -np.inf
    lens, begin, rows = vt.vad_batch([a, b, a])
    assert lens[1] == 0 and lens[0] == lens[2] > 0
    assert begin.tolist() == [0, lens[0], lens[0]]
    assert rows.shape == (2 * lens[0], 13)


def test_the_detector_is_wired_through_every_layer():
    """No GPU needed: the C-ABI exports and binds the two entry points, and the drop-in surface of the reference's class is there."""
    import poccala_amd._lib as L
    from poccala_amd import Engine
    from poccala_amd.AcousticModel.AcousticModel import AcousticModel
    from poccala_amd.StatisticalModel.AudioProcessing import AudioProcessing, vad_batch
    lib = L.load()
    for name in ('pcl_vad', 'pcl_frontend'):
        assert name in L.PROTOTYPES and hasattr(lib, name)
    for method in ('init_mfcc', 'mel_distance', 'osf', 'detect', 'mfcc'):
        assert callable(getattr(AudioProcessing.VAD, method))
    assert callable(vad_batch) and callable(Engine.frontend)
    assert callable(AcousticModel.load_audio) and callable(AcousticModel.load_audio_batch)
    v = AudioProcessing.VAD()
    v.init_mfcc(np.zeros((15, 13)))
    with pytest.raises(IndexError):                              # V5 is decided before the device is asked
        v.mfcc()
    with pytest.raises(NotImplementedError):
        v.detect(np.zeros(15), show_pic=True)
