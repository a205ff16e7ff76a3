"""The NumPy twin of csrc/bootstrap.hip (tests/_bootstrap_twin.py) against golden G20 -- the reference's own __flat_start,
__eq_segment(mode='e') and __get_gmmdata, executed (tests/golden/make_golden_bootstrap.py).  The owner map must match exactly; mean,
variance and the model at 1e-10 relative, the bound DESIGN.md section 2 uses for float64 restatements.  No GPU."""
import numpy as np

import _bootstrap_twin as tw

RTOL = 1e-10


def fs_cases(g):
    return [{k: g['fs%d_%s' % (c, k)] for k in ('step', 'diff', 'coeff', 'mean', 'var', 'weight')} for c in range(int(g['fs_n_cases']))]


def fs_corpus(g):
    lens = g['fs_lens'].astype(np.int32)
    begin = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
    return g['fs_frames'], lens, begin, int(len(lens) * float(g['fs_proportion']))


def us_labels(g):
    off = np.concatenate([[0], np.cumsum(g['us_label_len'])])
    return [g['us_labels'][off[u]:off[u + 1]] for u in range(len(g['us_label_len']))]


def test_golden_covers_what_it_should(golden):
    g = golden('G20_bootstrap')
    frames, lens, begin, n_utts = fs_corpus(g)
    assert n_utts == 5 and len(lens) * float(g['fs_proportion']) != n_utts          # int() truncated
    assert sorted(set(int(c['step']) for c in fs_cases(g))) == [1, 3]
    assert sorted(set(int(c['diff']) for c in fs_cases(g))) == [0, 1]
    assert lens[:n_utts].min() < 3                                                  # an utterance shorter than the step
    assert frames[:lens[:n_utts].sum(), 4].var() < 1e-4                             # a feature under the variance floor
    T, ll = g['us_T'], g['us_label_len']
    chunk = T // ll
    assert (T % ll != 0).any() and (T < ll).any() and ((chunk > 0) & (chunk < 3)).any() and (chunk % 3 != 0).any()
    assert any(len(set(l.tolist())) < len(l) for l in us_labels(g))                 # a repeated unit


def test_twin_moments_and_model_match_the_reference(golden):
    g = golden('G20_bootstrap')
    frames, lens, begin, n_utts = fs_corpus(g)
    for c, case in enumerate(fs_cases(g)):
        mean, var, n = tw.moments(frames, lens, begin, n_utts, int(case['step']))
        assert n == len(tw.sample_rows(lens, begin, n_utts, int(case['step'])))
        J, M, D = case['mean'].shape
        coeff = case['coeff'] if int(case['diff']) else None
        m, v, w = tw.flat_model(mean, var, coeff, J, M)
        print('fs%d: n = %d  max rel dev mean %.2e var %.2e' % (c, n, np.abs(m / case['mean'] - 1).max(), np.abs(v / case['var'] - 1).max()))
        np.testing.assert_allclose(m, case['mean'], rtol=RTOL, atol=0)
        np.testing.assert_allclose(v, case['var'], rtol=RTOL, atol=0)
        np.testing.assert_allclose(w, case['weight'], rtol=RTOL, atol=0)
        assert var[4] == 1e-4 and np.all(case['var'][..., 4] == 1e-4)               # the floor, through (v ** 0.5) ** 2
        if not int(case['diff']):
            assert np.all(m == m[:, :1])


def test_twin_uniform_map_equals_the_reference(golden):
    g = golden('G20_bootstrap')
    for sn in (5, 4):
        got = tw.uniform_map(int(g['us_F']), us_labels(g), g['us_T'], g['us_begin'], sn - 2)
        assert np.array_equal(got, g['us%d_frame_state' % sn])
    assert (g['us5_frame_state'] == -1).any() and g['us5_frame_state'].max() < int(g['us_n_units']) * 3


def test_sample_rows_edges():
    T, begin = np.array([5, 0, 2, 7]), np.array([0, 5, 5, 7])
    assert tw.sample_rows(T, begin, 4, 3).tolist() == [0, 3, 5, 7, 10, 13]
    assert tw.sample_rows(T, begin, 2, 1).tolist() == [0, 1, 2, 3, 4]
    assert tw.sample_rows(T, begin, 0, 1).size == 0
