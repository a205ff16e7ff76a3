"""CPU companion of tests/test_gpu_mfcc_edges.py: every case of tests/_mfcc_cases.py reaches the edge it is there for.  The edges are
stated against `kernel_geometry` / `kernel_frames`, a restatement of the index arithmetic of csrc/mfcc.hip, and the conditions the
device tests rest on (no zero bin behind the identity tables, no empty filter and a finite oracle behind the real ones) are asserted
here, where no device is needed."""
import numpy as np
import pytest

import _mfcc_cases as mc
from oracle import mfcc_oracle as mo

IDS = [mc.case_id(c) for c in mc.SPECTRUM_CASES]


def geometries():
    return [mc.kernel_geometry(r, st, 0.5, nfft, nfft // 2 + 1) for r, st, nfft in mc.SPECTRUM_CASES]


def test_spectrum_cases_order_size_and_nfft_all_three_ways_on_both_paths():
    seen = {(np.sign(g['size'] - g['nfft']), g['use_fft']) for g in geometries()}
    assert seen == {(s, p) for s in (-1, 0, 1) for p in (True, False)} - {(-1, False)}    # (nfft 500 > size: test_gpu_mfcc.py)
    for g in geometries():
        assert g['len'] == min(g['size'], g['nfft']) and g['step'] == g['size'] // 2


def test_spectrum_cases_reach_every_stage_count_and_both_sides_of_256_bins():
    radix2 = [g for g in geometries() if g['use_fft']]
    tables = [mc.kernel_geometry(r, st, 0.5, nfft, fb) for r, st, nfft, fb in mc.TABLE_CASES]
    assert {g['logn'] for g in radix2} == set(range(4, 12)) - {7}
    assert {g['logn'] for g in radix2 + tables if g['use_fft']} == set(range(4, 12))     # (nfft 128 runs with real tables)
    assert all(1 << g['logn'] == g['nfft'] for g in radix2)
    assert min(g['nfft'] // 2 for g in radix2) < 64 < 256 < max(g['nfft'] // 2 for g in radix2)   # butterflies: under a wavefront, over a block
    trips = {mc.strided_trips(g['nbin']) for g in geometries()}
    assert trips == {1, 2, 3, 5}                                  # the loops over nbin, nfilt and rank (all nbin behind identity tables)
    assert {mc.strided_trips(g['nfft'] // 2) for g in radix2} == {1, 2, 4}     # butterflies per thread and stage (x 256 threads: 8 at 2048)
    assert max(g['lds'] for g in geometries()) == 58832 <= 64 * 1024           # identity tables at nfft 2048 fit without a selection of bins


@pytest.mark.parametrize('case', mc.SPECTRUM_CASES, ids=IDS)
def test_spectrum_case_has_ragged_frames_and_no_zero_bin(case):
    rate, st, nfft = case
    g = mc.kernel_geometry(rate, st, 0.5, nfft, nfft // 2 + 1)
    sigs = mc.spectrum_signals(*case)
    frames = [mc.kernel_frames(len(s), g['size'], g['step']) for s in sigs]
    assert frames == [2, 3, 4, 7] and frames == [mo.frame_geometry(len(s), rate, st)[2] for s in sigs]
    pad = [(f - 1) * g['step'] + g['size'] - len(s) for f, s in zip(frames, sigs)]
    assert pad == [0, g['step'] - 1, 1, 0]                        # exact fit | all but one sample of padding | one sample | exact
    assert (len(sigs[0]) + len(sigs[1])) % 2 == 1                 # utterance 2 starts at an odd sample of the concatenation
    for s in sigs:
        mag, A = mc.spectrum_reference(s, rate, st, nfft)
        assert mag.shape == (mc.kernel_frames(len(s), g['size'], g['step']), g['nbin'])
        assert np.isfinite(mag).all() and mag.min() > 0 and A.min() > 0
        assert (mc.spectrum_bound(mag, A, g) < 1e-6 * mag.max()).all()           # the bound is a rounding bound, not a loose one


@pytest.mark.parametrize('case', mc.TABLE_CASES, ids=[mc.case_id(c) for c in mc.TABLE_CASES])
def test_table_case_has_no_empty_filter_and_a_finite_oracle(case):
    rate, st, nfft, fb = case
    assert (mo.mel_response(rate, nfft, fb).sum(axis=1) > 0).all()
    assert not (mo.mel_response(rate, nfft, fb + 1).sum(axis=1) > 0).all()        # ... and fb is the largest such count
    assert (mo.mel_response(rate, nfft, fb)[:, nfft // 2] == 0).all()             # the Nyquist bin weighs nothing: only c0 sees it
    sigs = mc.table_signals(rate, st, nfft)
    g = mc.kernel_geometry(rate, st, 0.5, nfft, fb)
    assert [mc.kernel_frames(len(s), g['size'], g['step']) for s in sigs] == [2, 4, 8]
    runs = mc.table_runs(fb)
    assert {v for v, _, _, _ in runs} == {1, 13, fb} and {e for _, e, _, _ in runs} == {True, False}
    for v, e, d1, d2 in runs:
        for s in sigs:
            assert np.isfinite(mo.mfcc(s, rate, vec_num=v, sampletime=st, nfft=nfft, filterbanks=fb, cal_energy=e, d1=d1, d2=d2)).all()


def test_table_cases_cover_the_listed_geometries():
    assert {(r, n) for r, _, n, _ in mc.TABLE_CASES} == {(16000, 512), (16000, 256), (16000, 300), (16000, 128), (8000, 64), (8000, 32),
                                                          (44100, 2048), (48000, 2048), (16000, 1024)}
    assert max(mc.kernel_geometry(r, st, 0.5, n, fb)['lds'] for r, st, n, fb in mc.TABLE_CASES) <= 64 * 1024


def test_empty_filter_case_takes_the_second_trip_of_the_filter_loop():
    c = mc.EMPTY_FILTER_CASE
    assert mc.strided_trips(c['filterbanks']) == 2 and mc.strided_trips(c['vec_num']) == 1
    resp = mo.mel_response(c['rate'], c['nfft'], c['filterbanks'])
    empty = resp.sum(axis=1) == 0
    assert empty.any() and not empty.all() and len(empty[256:]) == 44
    with np.errstate(all='ignore'):
        ref = mo.mfcc(mc.table_signals(c['rate'], 0.025, c['nfft'])[2], c['rate'], vec_num=c['vec_num'], nfft=c['nfft'],
                      filterbanks=c['filterbanks'])
    assert np.isfinite(ref[:, 0]).all() and not np.isfinite(ref[:, 1:]).any()     # c0 = ln(energy) is all that is finite


def test_frame_count_case_has_every_count_from_one_to_six():
    size, step = 400, 200
    got = [mc.kernel_frames(n, size, step) for n in mc.FRAME_COUNT_LENGTHS]
    assert tuple(got) == mc.FRAME_COUNTS and set(got) == set(range(1, 7))
    assert got == [mo.frame_geometry(n, mc.EDGE_RATE)[2] for n in mc.FRAME_COUNT_LENGTHS]
    sigs = mc.frame_count_signals()
    assert [len(s) for s in sigs] == list(mc.FRAME_COUNT_LENGTHS)
    with np.errstate(all='ignore'):
        refs = [mo.mfcc(s, mc.EDGE_RATE, d1=True, d2=True) for s in sigs]
    assert np.isnan(refs[0]).all() and all(np.isfinite(r).all() for r in refs[1:])
    # with 5 frames or fewer every delta row clamps at an end; the 6-frame utterance has none that clamps at both
    for t in got:
        clamped = [f for f in range(t) if f - 2 < 0 or f + 2 > t - 1]
        assert len(clamped) == min(t, 4)


@pytest.mark.parametrize('overlap,step,frames', [(1.0, 400, [2, 3, 3, 5]), (1.5, 600, [2, 3, 3, 4, 3]), (0.005, 2, [11])])
def test_step_cases(overlap, step, frames):
    g = mc.kernel_geometry(mc.EDGE_RATE, 0.025, overlap, 512, 26)
    assert (g['size'], g['step']) == (400, step)
    sigs = mc.step_signals(overlap)
    assert [mc.kernel_frames(len(s), 400, step) for s in sigs] == frames
    assert frames == [mo.frame_geometry(len(s), mc.EDGE_RATE, 0.025, overlap)[2] for s in sigs]
    # a last frame with no sample of the signal in it (or only the last one, which pre-emphasis zeroes): ln 0 in the oracle
    silent = [(f - 1) * step >= len(s) - 1 for f, s in zip(frames, sigs)]
    assert silent == {1.0: [False, True, False, False], 1.5: [False, True, False, True, True], 0.005: [False]}[overlap]
    with np.errstate(all='ignore'):
        for s, dead in zip(sigs, silent):
            ref = mo.mfcc(s, mc.EDGE_RATE, overlap=overlap)
            assert np.isfinite(ref[:-1]).all() and np.isfinite(ref[-1]).all() != dead


def test_many_short_utterances_change_utterance_every_two_workgroups():
    sigs = mc.many_short_signals()
    assert len(sigs) == 300 and {len(s) for s in sigs} == {401, 402, 403, 404, 405}
    assert all(mc.kernel_frames(len(s), 400, 200) == 2 for s in sigs)


def test_structured_signals_are_what_they_claim():
    square, const, impulse, silence, tail, after = mc.structured_signals()
    assert all(s.dtype == np.int16 for s in (square, const, impulse, silence, tail, after))
    assert set(square.tolist()) == {-32768, 32767} and (square[1:] != square[:-1]).all()
    assert (const == const[0]).all() and const[0] != 0
    assert impulse[-1] == 32767 and mo.pre_emphasis(impulse)[-1] == 0 and mo.pre_emphasis(impulse)[-2] == 32767 - 0.98 * impulse[-2]
    assert not silence.any()
    fr = mc.scaled_frames(tail, mc.EDGE_RATE)
    assert len(fr) == 9 and not fr[8].any() and all(fr[f].any() for f in range(8))
    with np.errstate(all='ignore'):
        for s in (square, const, impulse, after):
            assert np.isfinite(mo.mfcc(s, mc.EDGE_RATE, d1=True, d2=True)).all()
        assert not np.isfinite(mo.mfcc(silence, mc.EDGE_RATE)).any()
        ref = mo.mfcc(tail, mc.EDGE_RATE, d1=True, d2=True)
    assert np.isfinite(ref[:4]).all() and np.isfinite(ref[:8, :13]).all() and not np.isfinite(ref[8, :13]).any()


def test_lds_rule_cases():
    """The refused size needs more than any part has for its work arrays alone; the large one lies between 64 KiB and 160 KiB."""
    assert 2 * mc.REFUSED_NFFT * 8 == 262144
    assert mc.kernel_geometry(16000, 0.025, 0.5, mc.REFUSED_NFFT, 26)['lds'] == 331160
    assert 64 * 1024 < mc.kernel_geometry(16000, 0.025, 0.5, mc.LARGE_NFFT, 26)['lds'] == 85400 < 160 * 1024
