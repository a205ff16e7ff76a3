"""int16 PCM on the wire (pcl_mfcc_pcm16 / pcl_frontend_pcm16): the same samples give the same BITS as the float64 entry points -- at
odd sample offsets, at the one-frame / padded-frame / exact-fit edges, at full scale, for every position of a staging chunk's boundary
-- and the transfer's state (staging buffers, cached tables) lives and dies with the context.  Bits are compared as integers: the
one-frame utterance's rows are NaN (its window factor is 0 / 0, as in the reference), which np.array_equal on floats would call unequal."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATE = 16000                                                    # frame 400, step 200
LENGTHS = (400, 401, 599, 600, 601, 1235, 7777)                 # one frame | a padded second frame x2 | exact fit | a padded third | ... : later signals start at odd offsets
TOTAL = sum(LENGTHS)                                            # 11613 samples
VAD = dict(simple_size=1, alpha=0.5, beta=0.3)                  # a detector these short utterances pass (V5: T >= s; h + 1 < 2 s)
KNOB = 'PCL_PCM_CHUNK'


def make_signals():
    rng = np.random.default_rng(2024)
    sigs = []
    for n in LENGTHS:
        env = np.linspace(0.05, 1.0, n)                           # quiet start, loud end: the detector keeps part of every utterance
        sigs.append(np.clip(np.round(3000 * env * rng.standard_normal(n)), -32768, 32767).astype(np.int16))
    sigs[5][617:619] = (-32768, 32767)                           # full scale, side by side (617: an odd offset inside an odd-offset signal)
    return sigs


SIGS16 = make_signals()
SIGS64 = [s.astype(np.float64) for s in SIGS16]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def all_same(xs, ys):
    return len(xs) == len(ys) and all(same_bits(x, y) for x, y in zip(xs, ys))


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def default_chunk(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


def small_model(D, seed=3):
    from poccala_amd import synth
    mean, var, w, _ = synth.make_model(2, 4, D, seed=seed)
    return mean * 4.0, var * 8.0 + 4.0, w


def score_resident(eng, lens, begin, precision):
    """ln b of every state on the RESIDENT frames (the float32 matrix later stages read, or its float64 copy in parity mode)."""
    keep = lens > 0
    b = eng.all_state_batch(lens[keep], begin[keep])
    b.score(precision)
    B = [m.copy() for m in b.get('B')]
    b.close()
    return B


def frontend_and_score(eng, sigs, precision, **kw):
    lens, begin, rows = eng.frontend(sigs, RATE, fetch=True, **kw)
    return lens, begin, rows, score_resident(eng, lens, begin, precision)


def raw(eng, name, sigs, dtype, vec_num=13, nfft=512, filterbanks=26, mflags=7, flags=0, tables=None, vad=VAD):
    """One call of a front-end entry point through the ctypes binding: (rc, lens, begin, rows) for pcl_frontend*, (rc, rows) for pcl_mfcc*."""
    from poccala_amd._lib import as_c, ptr
    from poccala_amd.StatisticalModel.AudioProcessing import frame_count, mfcc_tables
    flat = as_c(np.concatenate(sigs), dtype) if len(sigs) else np.zeros(1, dtype=dtype)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    rows = int(sum(max(frame_count(len(s), RATE), 0) for s in sigs))
    dim = vec_num * (3 if mflags & 4 else 2 if mflags & 2 else 1)
    twc, tws, resp, dct = tables or mfcc_tables(RATE, vec_num, nfft, filterbanks)
    out = np.zeros((max(rows, 1), dim))
    fn = getattr(eng._lib, name)
    head = (eng._ctx, len(sigs), ptr(flat), ptr(off), RATE, 0.025, 0.5, nfft, filterbanks, vec_num, mflags, ptr(twc), ptr(tws), ptr(resp), ptr(dct))
    if 'frontend' in name:
        lens, begin = np.full(len(sigs), -7, dtype=np.int32), np.full(len(sigs), -7, dtype=np.int64)
        rc = fn(*head, vad['simple_size'], vad['alpha'], vad['beta'], flags, ptr(lens), ptr(begin), ptr(out), C.c_int64(rows))
        return rc, lens, begin, out[:max(int(lens.sum()), 0)] if rc == 0 else out
    return fn(*head, ptr(out), C.c_int64(rows)), out[:rows]


def last_error(eng):
    return eng._lib.pcl_last_error(eng._ctx).decode()


# ------------------------------------------------------------------ 1. same bits, both entry points
@pytest.mark.parametrize('kw', [dict(d1=True, d2=True), dict(cal_energy=False), dict()], ids=['39', '13-no-energy', '13'])
def test_mfcc_batch_int16_gives_the_float64_bits(eng, kw):
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch
    got = mfcc_batch(SIGS16, RATE, engine=eng, **kw)
    want = mfcc_batch(SIGS64, RATE, engine=eng, **kw)
    assert [len(m) for m in got] == [1, 2, 2, 2, 3, 6, 38]
    assert all_same(got, want)
    assert all(np.isfinite(m).all() for m in got[1:])            # (the one-frame utterance is NaN in both, as in the reference)


@pytest.mark.parametrize('vad', [True, False], ids=['vad', 'novad'])
@pytest.mark.parametrize('keep_f64', [False, True], ids=['f32', 'keep_f64'])
def test_frontend_int16_gives_the_float64_bits_host_and_resident(eng, vad, keep_f64):
    from poccala_amd import PCL_F32, PCL_F64
    prec = PCL_F64 if keep_f64 else PCL_F32
    eng.load_model(*small_model(39))
    kw = dict(vad=vad, keep_f64=keep_f64, **VAD)
    l16, b16, r16, B16 = frontend_and_score(eng, SIGS16, prec, **kw)
    l64, b64, r64, B64 = frontend_and_score(eng, SIGS64, prec, **kw)
    print('kept per utterance', l16.tolist())
    assert same_bits(l16, l64) and same_bits(b16, b64) and same_bits(r16, r64)
    assert l16.sum() > 0 and (vad or l16.tolist() == [1, 2, 2, 2, 3, 6, 38])
    assert all_same(B16, B64) and len(B16) == int((l16 > 0).sum())


def test_raw_entry_points_give_the_float64_bits(eng):
    from poccala_amd import PCL_F32
    rc64, m64 = raw(eng, 'pcl_mfcc', SIGS64, np.float64)
    rc16, m16 = raw(eng, 'pcl_mfcc_pcm16', SIGS16, np.int16)
    assert (rc64, rc16) == (0, 0) and m16.shape == (54, 39) and same_bits(m16, m64)
    eng.load_model(*small_model(39))
    res = {}
    for name, sigs, dt in (('pcl_frontend', SIGS64, np.float64), ('pcl_frontend_pcm16', SIGS16, np.int16)):
        for flags in (0, 1, 2, 3):                               # PCL_FRONTEND_NO_VAD = 1, PCL_FRONTEND_KEEP_F64 = 2
            rc, lens, begin, rows = raw(eng, name, sigs, dt, flags=flags)
            assert rc == 0, last_error(eng)
            res[name, flags] = (lens, begin, rows) + tuple(score_resident(eng, lens, begin, PCL_F32))
    for flags in (0, 1, 2, 3):
        assert all_same(res['pcl_frontend_pcm16', flags], res['pcl_frontend', flags])


# ------------------------------------------------------------------ 2. chunk edges
# 400: a boundary between utterances 0 | 1 (and 3 | 4, at 2000), others inside utterances, a last chunk of 13 samples;  401, 7: boundaries
# at odd and even offsets inside utterances, last chunks of 385 and 0 (exact) ... 7 = 1659 chunks;  4000: the first chunk holds utterances
# 0-5 whole, the last has 3613 samples;  11613: the call fits exactly;  20000 and the default: one chunk, partly filled
@pytest.mark.parametrize('fetch_route', ['mfcc', 'frontend'])
def test_chunk_boundaries_do_not_move_a_bit(eng, monkeypatch, fetch_route):
    from poccala_amd import PCL_F32
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch
    eng.load_model(*small_model(39))

    def run():
        if fetch_route == 'mfcc':
            return mfcc_batch(SIGS16, RATE, d1=True, d2=True, engine=eng)
        lens, begin, rows, B = frontend_and_score(eng, SIGS16, PCL_F32, vad=False)
        return [lens, begin, rows] + B

    def copies():                                                # H2D copies of the last call: one timed pair of events per chunk
        return eng.kernel_time('pcm_h2d')[1]

    eng.enable_timing(True)
    try:
        one_chunk = run()                                        # the knob unset: 2 Mi samples per chunk
        assert copies() == 1
        for chunk in (400, 7, 401, 4000, TOTAL, 20000, 400):     # set between calls on ONE engine: read per call (and back to a small one)
            monkeypatch.setenv(KNOB, str(chunk))
            assert all_same(run(), one_chunk), chunk
            assert copies() == -(-TOTAL // chunk), chunk         # the knob was read: that many chunks travelled
        monkeypatch.setenv(KNOB, '0')                            # not a size: the default
        assert all_same(run(), one_chunk) and copies() == 1
    finally:
        eng.enable_timing(False)


# ------------------------------------------------------------------ 3. the direct-summation branch
def test_non_power_of_two_nfft_on_the_int16_route(eng, monkeypatch):
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch
    monkeypatch.setenv(KNOB, '1000')
    got = mfcc_batch(SIGS16, RATE, nfft=480, d1=True, d2=True, engine=eng)
    want = mfcc_batch(SIGS64, RATE, nfft=480, d1=True, d2=True, engine=eng)
    assert all_same(got, want) and np.isfinite(got[-1]).all()
    assert not same_bits(got[-1], mfcc_batch(SIGS16, RATE, d1=True, d2=True, engine=eng)[-1])


# ------------------------------------------------------------------ 4. the cached tables
def test_tables_are_uploaded_again_when_geometry_or_contents_change(eng):
    from poccala_amd import Engine
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch, mfcc_tables
    fresh = Engine(0)
    try:
        want26 = mfcc_batch(SIGS16, RATE, filterbanks=26, engine=fresh)
    finally:
        fresh.close()
    fresh = Engine(0)
    try:
        want20 = mfcc_batch(SIGS16, RATE, filterbanks=20, engine=fresh)
    finally:
        fresh.close()
    assert not same_bits(want26[-1], want20[-1])
    for fb, want in ((26, want26), (20, want20), (26, want26), (26, want26)):
        assert all_same(mfcc_batch(SIGS16, RATE, filterbanks=fb, engine=eng), want), fb
    # the caller builds the tables: the same geometry with other contents is another set of tables
    twc, tws, resp, dct = mfcc_tables(RATE, 13, 512, 26)
    other = (twc, tws, resp, np.ascontiguousarray(dct[::-1]))
    fresh = Engine(0)
    try:
        rc, want_other = raw(fresh, 'pcl_mfcc_pcm16', SIGS16, np.int16, mflags=1, tables=other)
        assert rc == 0
    finally:
        fresh.close()
    rc, got = raw(eng, 'pcl_mfcc_pcm16', SIGS16, np.int16, mflags=1, tables=other)
    assert rc == 0 and same_bits(got, want_other) and not same_bits(got, np.concatenate(want26))
    rc, got = raw(eng, 'pcl_mfcc_pcm16', SIGS16, np.int16, mflags=1)
    assert rc == 0 and same_bits(got, np.concatenate(want26))


# ------------------------------------------------------------------ 5. a failed call leaves the frames alone
def test_short_signal_fails_before_anything_moves(eng, monkeypatch):
    from poccala_amd import PCL_F32, PoccalaHipError
    monkeypatch.setenv(KNOB, '512')
    eng.load_model(*small_model(39))
    lens, begin = eng.frontend(SIGS16, RATE, vad=False)
    before = score_resident(eng, lens, begin, PCL_F32)
    F = eng.F
    short = SIGS16[6][:399]
    with pytest.raises(PoccalaHipError) as e:
        eng.frontend([SIGS16[1], SIGS16[5], short, SIGS16[2]], RATE, vad=False)
    print(e.value)
    assert e.value.code == -1 and 'pcl_frontend_pcm16: signal 2 has 399 samples' in str(e.value)
    assert eng.F == F
    assert all_same(score_resident(eng, lens, begin, PCL_F32), before)
    rc, _ = raw(eng, 'pcl_mfcc_pcm16', [SIGS16[1], short], np.int16)
    assert rc == -1 and 'pcl_mfcc_pcm16: signal 1 has 399 samples' in last_error(eng)
    # the detector's own check (V5) runs before the first copy too
    with pytest.raises(PoccalaHipError) as e:
        eng.frontend(SIGS16, RATE)                               # simple_size = 16: utterance 0 has one frame
    assert e.value.code == -1 and 'utterance 0' in str(e.value)
    assert all_same(score_resident(eng, lens, begin, PCL_F32), before)


# ------------------------------------------------------------------ 6. route selection
class Recording(object):
    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        if name.startswith(('pcl_frontend', 'pcl_mfcc')):
            self.names.append(name)
        return getattr(self._lib, name)


def test_only_int16_arrays_take_the_int16_route(eng):
    rc, lens, begin, rows = raw(eng, 'pcl_frontend', SIGS64, np.float64, flags=1)
    assert rc == 0
    lib = eng._lib
    eng._lib = rec = Recording(lib)
    try:
        mixed = [s16 if u % 2 else s64 for u, (s16, s64) in enumerate(zip(SIGS16, SIGS64))]
        for sigs, entry in ((SIGS64, 'pcl_frontend'), (mixed, 'pcl_frontend'), ([s.astype(np.float32) for s in SIGS16], 'pcl_frontend'),
                            (SIGS16, 'pcl_frontend_pcm16')):
            del rec.names[:]
            got = eng.frontend(sigs, RATE, vad=False, fetch=True)
            assert rec.names == [entry]
            assert all_same(got, (lens, begin, rows))
        # no signal at all: the float64 route's rejection, before any call into the library
        del rec.names[:]
        for empty in ([], ()):
            with pytest.raises(ValueError):
                eng.frontend(empty, RATE)
        assert rec.names == []
    finally:
        eng._lib = lib
    # ... and in the library the two entry points refuse U = 0 alike
    rc64 = raw(eng, 'pcl_frontend', [], np.float64)[0]
    e64 = last_error(eng)
    rc16 = raw(eng, 'pcl_frontend_pcm16', [], np.int16)[0]
    e16 = last_error(eng)
    assert rc64 == rc16 == -1 and e64 == 'pcl_frontend: NULL / empty argument' and e16 == 'pcl_frontend_pcm16: NULL / empty argument'


# ------------------------------------------------------------------ 7. lifecycle
def test_engines_with_and_without_staging_close_cleanly(monkeypatch):
    from poccala_amd import Engine
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch
    want = None
    for chunk in ('300', '5000', '64', None):
        if chunk is None:
            monkeypatch.delenv(KNOB)
        else:
            monkeypatch.setenv(KNOB, chunk)
        e = Engine(0)
        lens, begin, rows = e.frontend(SIGS16, RATE, fetch=True, **VAD)
        if chunk == '5000':
            mfcc_batch(SIGS16, RATE, engine=e)                   # a second call on the same staging buffers
        e.close()
        want = want or (lens, begin, rows)
        assert all_same((lens, begin, rows), want)
    Engine(0).close()                                            # a context that never staged anything
    e = Engine(0)
    e.frontend(SIGS64, RATE, **VAD)                              # ... and one that only took the float64 route
    e.close()


# ------------------------------------------------------------------ 8. PCM -> words without a host round trip
from test_gpu_decode import lex, model_for  # noqa: E402,F401  (the decode tests' lexicon fixture and model helper, as they are)


def test_decode_batch_from_resident_frames(eng, lex):  # noqa: F811
    from poccala_amd import Decoder, PCL_F32
    from test_gpu_vad import speech_signal
    lx, units, _ = lex
    mean, var, w, trans = model_for(units, 2, 13, 31)
    tree = Decoder.load_inventory(eng, units, mean * 4.0, var * 8.0 + 4.0, w, trans, lx)
    rng = np.random.default_rng(8)
    sigs = [speech_signal(rng, 9000), np.zeros(8000, dtype=np.int16), speech_signal(rng, 12345), speech_signal(rng, 7001)]
    lens, begin, rows = eng.frontend(sigs, RATE, d1=False, d2=False, fetch=True)
    print('kept', lens.tolist())
    assert lens[1] == 0 and (np.delete(lens, 1) > 0).all()       # digital silence keeps no frame
    calls = []
    upload = eng.load_frames
    eng.load_frames = lambda frames: (calls.append(len(frames)), upload(frames))[1]
    try:
        res = Decoder.decode_batch((lens, begin), tree, engine=eng, precision=PCL_F32)
        assert calls == []                                       # the resident form uploads no frame
        keep = [u for u in range(len(lens)) if lens[u] > 0]
        host = Decoder.decode_batch([np.float32(rows[begin[u]:begin[u] + lens[u]]) for u in keep], tree, engine=eng, precision=PCL_F32)
        assert calls == [int(lens.sum())]
    finally:
        del eng.load_frames
    assert len(res) == 4 and res[1][0] == [] and res[1][1] == -np.inf
    for u, (words, score, detail) in zip(keep, host):
        print(u, res[u][0], res[u][1])
        assert res[u][0] == words and same_bits(np.float64(res[u][1]), np.float64(score))
        assert res[u][2]['final'] == detail['final'] and res[u][2]['n_tokens'].tolist() == detail['n_tokens'].tolist()


# ------------------------------------------------------------------ 9. the three halves cut the same rows
def test_mfcc_frontend_and_pitch_rows_agree_at_the_frame_edges(eng):
    """8 kHz: frame 200, step 100.  int16 signals of exactly one frame, one sample more (a second frame that is all padding but one
    sample) and 501 samples (1 + ceil(301 / 100) = 5 frames, the last one padded): the MFCC alone, the front-end's MFCC columns without
    and with the pitch columns, and the pitch columns against the stand-alone pitch call, byte for byte."""
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch, pitch_batch
    rng = np.random.default_rng(77)
    sigs = [np.round(2500 * rng.standard_normal(n)).astype(np.int16) for n in (200, 201, 501)]
    mats = mfcc_batch(sigs, 8000, d1=True, d2=True, engine=eng)
    assert [m.shape for m in mats] == [(1, 39), (2, 39), (5, 39)]
    want = np.concatenate(mats)
    lens0, begin0, rows0 = eng.frontend(sigs, 8000, vad=False, fetch=True)
    lens, begin, rows = eng.frontend(sigs, 8000, vad=False, pitch=True, fetch=True)
    assert lens0.tolist() == lens.tolist() == [1, 2, 5] and begin0.tolist() == begin.tolist() == [0, 1, 3]
    assert rows.shape == (8, 42)
    assert same_bits(rows0, want)
    assert same_bits(rows[:, :39], want)
    assert same_bits(rows[:, 39:], np.concatenate(pitch_batch(sigs, 8000, engine=eng)))
    assert np.isfinite(want[1:]).all() and np.isfinite(rows[:, 39:]).all()      # (the one-frame utterance's MFCC row is NaN everywhere, as in the reference)
