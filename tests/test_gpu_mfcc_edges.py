"""csrc/mfcc.hip held to the float64 oracle stage by stage, at the edges of its geometry (tests/_mfcc_cases.py makes the inputs,
tests/test_mfcc_cases.py proves on the CPU that each reaches its edge).

A  the spectrum bin by bin: identity mel and DCT tables make the kernel's output ln |X[k]| for every bin, the Nyquist bin included, which
   the mel response weighs with 0 and the log and DCT would smear; held to np.fft.rfft by a rounding bound, on both transform paths, with
   frames shorter than, equal to and longer than the FFT, from nfft 16 to 2048;
B  mel, log, DCT and c0 with the real tables at the largest filter counts that leave no filter empty (the oracle is finite everywhere, so
   every entry is compared), and one case with empty filters and more than 256 of them;
C  every frame count from 1 to 6, step == size, step > size, step 2, 300 two-frame utterances, signals with structure; the delta kernel
   alone against mo.delta of the device's own statics;
D  the dynamic LDS a geometry needs is checked on the host before anything is allocated: refused, served above 64 KiB, context intact.
"""
import numpy as np
import pytest

import _mfcc_cases as mc
from oracle import mfcc_oracle as mo

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-8, 1e-8                                          # tests/test_gpu_mfcc.py against the oracle
ROUTES = (('pcl_mfcc', np.float64), ('pcl_mfcc_pcm16', np.int16))


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def last_error(eng):
    return eng._lib.pcl_last_error(eng._ctx).decode()


def both_routes(eng, sigs, rate, **kw):
    """mfcc_batch on the int16 and on the float64 route: equal bits, one result."""
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch
    got = mfcc_batch(sigs, rate, engine=eng, **kw)
    wide = mfcc_batch([s.astype(np.float64) for s in sigs], rate, engine=eng, **kw)
    assert all(g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, wide))
    return got


def hold_to_oracle(got, ref, what):
    """Same shape, same NaN, +inf and -inf entries, every finite entry within the tolerances."""
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), what
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=RTOL, atol=ATOL, err_msg=str(what))
    return fin


def oracle(sig, rate, **kw):
    with np.errstate(all='ignore'):
        return mo.mfcc(sig, rate, **kw)


# ------------------------------------------------------------------ A. the spectrum, bin by bin
@pytest.mark.parametrize('case', mc.SPECTRUM_CASES, ids=[mc.case_id(c) for c in mc.SPECTRUM_CASES])
def test_spectrum_bin_by_bin(eng, case):
    """|X[k]| of every frame and bin against np.fft.rfft of the oracle's frames, within
        8 * 2^-53 * log2(nfft) * sum |x_n| + 4 * 2^-52 * |X[k]|      (radix-2)
        2^-53 * len * sum |x_n| + 4 * 2^-52 * |X[k]|                 (direct summation)
    (derivation: _mfcc_cases.spectrum_bound).  The worst error / bound over the ten cases is recorded in profiles/r20_mfcc_edges.txt."""
    rate, st, nfft = case
    g = mc.kernel_geometry(rate, st, 0.5, nfft, nfft // 2 + 1)
    sigs = mc.spectrum_signals(*case)
    tables = mc.identity_tables(nfft)
    outs = []
    for name, dtype in ROUTES:
        rc, out = mc.call(eng, name, sigs, dtype, rate, st, 0.5, nfft, tables, 0)
        assert rc == 0, last_error(eng)
        outs.append(out)
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    mag = np.exp(outs[0])
    assert mag.shape == (16, g['nbin'])
    row, worst = 0, (0.0, None)
    for u, s in enumerate(sigs):
        ref, A = mc.spectrum_reference(s, rate, st, nfft)
        ratio = np.abs(mag[row:row + len(ref)] - ref) / mc.spectrum_bound(ref, A, g)
        f, k = np.unravel_index(np.argmax(ratio), ratio.shape)
        worst = max(worst, (float(ratio[f, k]), (u, int(f), int(k))))
        print('mfcc spectrum %-16s utt %d (%d frames): worst error / bound %.3e at frame %d bin %d;  DC %.3e  Nyquist %.3e'
              % (mc.case_id(case), u, len(ref), ratio[f, k], f, k, ratio[:, 0].max(), ratio[:, -1].max()))
        row += len(ref)
    print('mfcc spectrum %-16s %s nbin %d: worst error / bound %.3e at (utt, frame, bin) %s'
          % (mc.case_id(case), 'radix-2 logn %d' % g['logn'] if g['use_fft'] else 'direct len %d' % g['len'], g['nbin'], worst[0], worst[1]))
    assert worst[0] <= 1.0


# ------------------------------------------------------------------ B. mel, log, DCT, c0 with the real tables
@pytest.mark.parametrize('case', mc.TABLE_CASES, ids=[mc.case_id(c) for c in mc.TABLE_CASES])
def test_real_tables_where_the_oracle_is_finite(eng, case):
    rate, st, nfft, fb = case
    sigs = mc.table_signals(rate, st, nfft)
    for v, e, d1, d2 in mc.table_runs(fb):
        kw = dict(vec_num=v, sampletime=st, nfft=nfft, filterbanks=fb, cal_energy=e, d1=d1, d2=d2)
        for u, (s, got) in enumerate(zip(sigs, both_routes(eng, sigs, rate, **kw))):
            ref = oracle(s, rate, **kw)
            assert np.isfinite(ref).all()
            assert hold_to_oracle(got, ref, (case, v, e, u)).all()


def test_empty_filters_and_more_than_256_of_them(eng):
    c = mc.EMPTY_FILTER_CASE
    sigs = mc.table_signals(c['rate'], 0.025, c['nfft'])
    for e in (True, False):
        kw = dict(vec_num=c['vec_num'], nfft=c['nfft'], filterbanks=c['filterbanks'], cal_energy=e)
        for u, (s, got) in enumerate(zip(sigs, both_routes(eng, sigs, c['rate'], **kw))):
            fin = hold_to_oracle(got, oracle(s, c['rate'], **kw), ('empty filters', e, u))
            assert fin[:, 0].all() == e and not fin[:, 1:].any()     # c0 = ln(energy) is finite, nothing else is


# ------------------------------------------------------------------ C. frame counts, steps, deltas
def test_every_frame_count_and_the_delta_kernel_alone(eng):
    """Statics of 1 .. 6 frames against the oracle; the deltas against mo.delta of the DEVICE's statics, the delta-deltas against mo.delta of
    the device's deltas, each entry within 6 * 2^-53 * sum_i |i x_i| / 10 (_mfcc_cases.delta_bound): the delta kernel is held alone."""
    sigs = mc.frame_count_signals()
    got = both_routes(eng, sigs, mc.EDGE_RATE, d1=True, d2=True)
    assert tuple(len(m) for m in got) == mc.FRAME_COUNTS
    assert np.isnan(got[0]).all() and np.isnan(oracle(sigs[0], mc.EDGE_RATE, d1=True, d2=True)).all()
    worst = 0.0
    for u, (s, m) in enumerate(zip(sigs, got)):
        if u:
            assert hold_to_oracle(m, oracle(s, mc.EDGE_RATE, d1=True, d2=True), ('frames', len(m))).all()
        for src, dst in ((0, 13), (13, 26)):
            with np.errstate(all='ignore'):
                want, bound = mo.delta(m[:, src:src + 13]), mc.delta_bound(m[:, src:src + 13])
            have = m[:, dst:dst + 13]
            assert np.array_equal(np.isnan(have), np.isnan(want))
            fin = np.isfinite(want)
            assert fin.all() == (u > 0)
            if fin.any():
                assert (bound[fin] > 0).all()
                ratio = float((np.abs(have - want)[fin] / bound[fin]).max())
                print('mfcc delta %d frames, columns %d -> %d: worst error / bound %.3e' % (len(m), src, dst, ratio))
                worst = max(worst, ratio)
    print('mfcc delta kernel alone: worst error / bound %.3e' % worst)
    assert worst <= 1.0


@pytest.mark.parametrize('overlap', [1.0, 1.5, 0.005])
def test_step_at_and_past_the_frame_size_and_step_two(eng, overlap):
    sigs = mc.step_signals(overlap)
    got = both_routes(eng, sigs, mc.EDGE_RATE, overlap=overlap, d1=True, d2=True)
    finite_rows = 0
    for s, m in zip(sigs, got):
        fin = hold_to_oracle(m, oracle(s, mc.EDGE_RATE, overlap=overlap, d1=True, d2=True), (overlap, len(s)))
        finite_rows += int(fin.all(axis=1).sum())
    print('mfcc step: overlap %g, %d rows, %d finite in every entry' % (overlap, sum(len(m) for m in got), finite_rows))
    assert finite_rows >= {1.0: 10, 1.5: 5, 0.005: 11}[overlap]


def test_three_hundred_two_frame_utterances_every_row(eng):
    sigs = mc.many_short_signals()
    got = both_routes(eng, sigs, mc.EDGE_RATE, d1=True, d2=True)
    assert len(got) == 300
    for u, (s, m) in enumerate(zip(sigs, got)):
        assert hold_to_oracle(m, oracle(s, mc.EDGE_RATE, d1=True, d2=True), u).all() and m.shape == (2, 39)


def test_signals_with_structure(eng):
    """Full-scale square wave, constant, an impulse in the last sample, digital silence, a silent last frame: against the oracle, entry by
    entry where it is finite and by kind (NaN, +inf, -inf) where it is not."""
    sigs = mc.structured_signals()
    got = both_routes(eng, sigs, mc.EDGE_RATE, d1=True, d2=True)
    fins = [hold_to_oracle(m, oracle(s, mc.EDGE_RATE, d1=True, d2=True), u) for u, (s, m) in enumerate(zip(sigs, got))]
    assert [bool(f.all()) for f in fins] == [True, True, True, False, False, True]
    assert not fins[3].any() and fins[4][:4].all() and fins[4][:8, :13].all() and not fins[4][8, :13].any()


# ------------------------------------------------------------------ D. the LDS rule
def default_call(eng, name, dtype):
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_tables
    rc, out = mc.call(eng, name, mc.frame_count_signals(), dtype, mc.EDGE_RATE, 0.025, 0.5, 512, mfcc_tables(mc.EDGE_RATE, 13, 512, 26), 7)
    assert rc == 0, last_error(eng)
    return out


@pytest.mark.parametrize('name,dtype', ROUTES)
def test_an_fft_that_cannot_fit_in_lds_is_refused_before_anything_is_allocated(eng, name, dtype):
    from poccala_amd import Engine
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_tables
    nfft = mc.REFUSED_NFFT
    before = default_call(eng, name, dtype)
    stats = Engine.pool_stats()
    rc, _ = mc.call(eng, name, mc.frame_count_signals(), dtype, mc.EDGE_RATE, 0.025, 0.5, nfft, mfcc_tables(mc.EDGE_RATE, 13, nfft, 26), 7)
    msg = last_error(eng)
    print(msg)
    need = mc.kernel_geometry(mc.EDGE_RATE, 0.025, 0.5, nfft, 26)['lds']
    assert rc == -1 and msg.startswith(name + ': ') and 'nfft %d' % nfft in msg and '%d bytes' % need in msg
    limit = int(msg.rsplit(' ', 1)[1])
    assert 64 * 1024 <= limit < need                              # the device's own figure, in the message
    assert Engine.pool_stats() == stats                           # nothing was asked of the pool, nothing given back
    assert np.array_equal(bits(default_call(eng, name, dtype)), bits(before))


def test_nfft_4096_is_served_above_64_kib(eng):
    """85400 bytes of dynamic LDS: above the 64 KiB a launch gets unasked, below the device's limit -- served, and right."""
    nfft = mc.LARGE_NFFT
    rng = np.random.default_rng(9400)
    sigs = [mc.noise(rng, n) for n in (600, 1001, 2400)]
    for kw in (dict(d1=True, d2=True), dict(cal_energy=False)):
        for u, (s, m) in enumerate(zip(sigs, both_routes(eng, sigs, mc.EDGE_RATE, nfft=nfft, **kw))):
            assert hold_to_oracle(m, oracle(s, mc.EDGE_RATE, nfft=nfft, **kw), (nfft, u)).all()
