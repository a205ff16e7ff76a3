"""Drop-in for the feature-extraction part of StatisticalModel/AudioProcessing.py: `AudioProcessing.MFCC`
(wav -> (T, 13/26/39) float64 MFCC matrix), computed on the GPU (csrc/mfcc.hip) through `pcl_mfcc`, and `AudioProcessing.VAD`
(MFCC matrix -> the rows its voice-activity detector keeps), computed on the GPU (csrc/vad.hip) through `pcl_vad`.

This is SURVEY.md section 8(f) rows 4 and 6, the steps BEFORE the hot path.  Mirrored: MFCC(vec_num), init_audio,
data, params, mfcc(sampletime, overlap, nfft, cal_energy, d1, d2) (AudioProcessing.py:100-448); VAD(simple_size), init_mfcc,
mel_distance, osf, detect, mfcc (:450-543; plotting is not supported).  Added: `mfcc_batch` / `vad_batch` for many utterances in one
launch; `Engine.frontend` runs both and leaves the survivors resident on the device.  Recording / playback (pyaudio) are out of scope.
`AudioProcessing.Pitch` / `pitch_batch` have no counterpart in the reference: voicing, ln f0 and its delta on the MFCC's frame grid
(csrc/pitch.hip through `pcl_pitch`), the columns a toned unit inventory needs beside the cepstra.
The reference's conventions are kept exactly (they are pinned by tests/golden/G10_mfcc.npz):
the "Hamming window" is one factor per frame, the spectrum is the rFFT magnitude, every mel filter is two
rising ramps, the DCT kernel is cos(pi (2k-1) j / 2N) * 2/sqrt(N), c0 is ln(sum of magnitudes).
"""
import ctypes as C
import math
import wave

import numpy as np

from .._lib import PCL_PITCH_NCCF_IN, PCL_VAD_DIST_IN, PCL_VAD_OSF_IN, as_c, pack_signals, ptr
from ..runtime import default_engine


def frame_count(n_samples, framerate, sampletime=0.025, overlap=0.5):
    size = int(framerate * sampletime)
    step = int(size * overlap)
    return 1 + math.ceil((n_samples - size) / step)                     # AudioProcessing.py:216-219


def mel_filter_matrix(samplerate, nfft=512, filterbanks=26, low_hz=0.0, high_hz=None):
    """(filterbanks, nfft/2+1) frequency responses as mel_filter_bank builds them (AudioProcessing.py:312-335):
    centres linear in mel = 2595 ln(1 + f/700), FFT bins floor((nfft+1) f / rate), and for filter i a ramp from 0
    on [bin_i, bin_i+1) followed by ANOTHER ramp from 0 on [bin_i+1, bin_i+2)."""
    high_hz = high_hz or samplerate / 2
    lo_mel, hi_mel = 2595 * math.log(1 + low_hz / 700), 2595 * math.log(1 + high_hz / 700)
    centres_hz = 700 * (np.exp(np.linspace(lo_mel, hi_mel, filterbanks + 2) / 2595) - 1)
    bins = np.floor((nfft + 1) / samplerate * centres_hz)
    resp = np.zeros((filterbanks, nfft // 2 + 1))
    for i in range(filterbanks):
        for a, b in ((i, i + 1), (i + 1, i + 2)):
            start, stop = int(bins[a]), int(bins[b])
            for j in range(start, stop):
                resp[i][j] = (j - start) / (bins[b] - bins[a])
    return resp


def dct_basis(filterbanks, rank):
    """(rank, filterbanks): 2/sqrt(N) cos(pi (2k-1) j / (2N)) (AudioProcessing.py:362-369)."""
    k = np.arange(filterbanks)[None, :]
    j = np.arange(rank)[:, None]
    return (2 / filterbanks ** 0.5) * np.cos(np.pi * (2 * k - 1) * j / (2 * filterbanks))


def mfcc_flags(cal_energy=True, d1=False, d2=False):
    """The flag word of pcl_mfcc / pcl_frontend: 1 = c0 <- ln(energy), 2 = deltas, 4 = their deltas as well (only with d1)."""
    return (1 if cal_energy else 0) | (2 if d1 else 0) | (4 if (d1 and d2) else 0)


def mfcc_dim(vec_num, flags):
    return vec_num * (3 if flags & 4 else 2 if flags & 2 else 1)


def mfcc_batch(signals, framerate, vec_num=13, sampletime=0.025, overlap=0.5, nfft=512, filterbanks=26, cal_energy=True,
               d1=False, d2=False, engine=None):
    """MFCC matrices of many signals in one launch: list of (T_u, vec_num * {1,2,3}) float64 arrays.  When every signal is an np.int16
    array the samples travel as int16 (pcl_mfcc_pcm16) and give the same bits; anything else is sent as float64 (Engine.frontend's rule)."""
    eng = engine or default_engine()
    sigs, flat, off, pcm16 = pack_signals(signals)
    frames = [frame_count(len(s), framerate, sampletime, overlap) for s in sigs]
    rows = int(sum(frames))
    flags = mfcc_flags(cal_energy, d1, d2)
    twc, tws, resp, dct = mfcc_tables(framerate, vec_num, nfft, filterbanks)
    out = np.empty((rows, mfcc_dim(vec_num, flags)))
    call = eng._lib.pcl_mfcc_pcm16 if pcm16 else eng._lib.pcl_mfcc
    eng._check(call(eng._ctx, len(sigs), ptr(flat), ptr(off), int(framerate), float(sampletime), float(overlap),
                    int(nfft), int(filterbanks), int(vec_num), flags, ptr(twc), ptr(tws), ptr(resp), ptr(dct),
                    ptr(out), C.c_int64(rows)))
    cuts = np.cumsum(frames)[:-1]
    return np.split(out, cuts)


def mfcc_tables(framerate, vec_num=13, nfft=512, filterbanks=26):
    """The float64 tables pcl_mfcc / pcl_frontend take: twiddle cos / sin (nfft,), mel response, DCT basis."""
    n = np.arange(nfft)
    return (as_c(np.cos(2 * np.pi * n / nfft), np.float64), as_c(-np.sin(2 * np.pi * n / nfft), np.float64),
            as_c(mel_filter_matrix(framerate, nfft, filterbanks), np.float64), as_c(dct_basis(filterbanks, vec_num), np.float64))


def frame_count_padded(n_samples, framerate, sampletime=0.025, overlap=0.5):
    """frame_count, at least 1: the pitch rows of a signal shorter than one frame are one zero-padded frame."""
    return max(1, frame_count(n_samples, framerate, sampletime, overlap))


def pitch_lags(framerate, f_min=50.0, f_max=400.0):
    """(Lmin, Lmax, g): the integer lag grid ceil(rate / f_max) .. floor(rate / f_min) of pcl_pitch and its float64 table g = ln(lag)."""
    lmin, lmax = int(math.ceil(framerate / f_max)), int(math.floor(framerate / f_min))
    return lmin, lmax, as_c(np.log(np.arange(lmin, max(lmax, lmin) + 1, dtype=np.float64)), np.float64)


def pitch_batch(signals, framerate, sampletime=0.025, overlap=0.5, f_min=50.0, f_max=400.0, ballast=7000.0, soft_min_f0=10.0, pf=0.1,
                details=False, nccf=None, engine=None):
    """Pitch features of many signals in one call: list of (T_u, 3) float64 arrays [voicing, ln f0, delta ln f0] whose rows are the
    MFCC's (mfcc_batch with the same sampletime / overlap).  When every signal is an np.int16 array the samples travel as int16
    (pcl_pitch_pcm16) and give the same bits.  details=True: (rows, info) with info = dict(lag=[(T_u,) int32 lags in samples],
    nccf_bal=[(T_u, L)], nccf_raw=[(T_u, L)], lag_min, lag_max).  nccf=(bal_list, raw_list): the correlations are the caller's
    (PCL_PITCH_NCCF_IN; `signals` then only gives the lengths)."""
    eng = engine or default_engine()
    sigs, flat, off, pcm16 = pack_signals(signals, none_ok=True)
    frames = [frame_count_padded(len(s), framerate, sampletime, overlap) for s in sigs]
    rows = int(sum(frames))
    lmin, lmax, g = pitch_lags(framerate, f_min, f_max)
    L = len(g)
    if flat.size == 0:
        flat = np.zeros(1, dtype=flat.dtype)            # (a pointer to hand over; sig_off says nothing of it is read)
    out = np.empty((rows, 3))
    lag = np.empty(rows, dtype=np.int32) if details else None
    flags = 0
    if nccf is not None:
        flags = PCL_PITCH_NCCF_IN
        bal = as_c(np.concatenate([np.asarray(b, dtype=np.float64) for b in nccf[0]]), np.float64)
        raw = as_c(np.concatenate([np.asarray(r, dtype=np.float64) for r in nccf[1]]), np.float64)
        if bal.shape != (rows, L) or raw.shape != (rows, L):
            raise ValueError('pitch_batch: nccf arrays of shape %s / %s, the geometry gives (%d, %d)' % (bal.shape, raw.shape, rows, L))
    else:
        bal = np.empty((rows, L)) if details else None
        raw = np.empty((rows, L)) if details else None
    call = eng._lib.pcl_pitch_pcm16 if pcm16 else eng._lib.pcl_pitch
    eng._check(call(eng._ctx, len(sigs), ptr(flat), ptr(off), int(framerate), float(sampletime), float(overlap), float(f_min), float(f_max),
                    float(ballast), float(soft_min_f0), float(pf), ptr(g), int(L), flags, ptr(out), ptr(lag), ptr(bal), ptr(raw),
                    C.c_int64(rows)))
    cuts = np.cumsum(frames)[:-1]
    res = np.split(out, cuts)
    if not details:
        return res
    return res, dict(lag=np.split(lag, cuts), nccf_bal=np.split(bal, cuts), nccf_raw=np.split(raw, cuts), lag_min=lmin, lag_max=lmax)


def _vad_call(eng, mats, simple_size, alpha, beta, flags, want, dist=None, osf=None):
    """One pcl_vad call over a ragged list.  mats: feature matrices (or None with PCL_VAD_DIST_IN / _OSF_IN, then `dist` / `osf` are
    lists of the caller's vectors); want: subset of {'dist', 'osf', 'kept'}.  Returns dict of flat arrays + row_off."""
    src = mats if mats is not None else (dist if flags & PCL_VAD_DIST_IN else osf)
    lens = [len(m) for m in src]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows, U = int(off[-1]), len(lens)
    x, D = None, 0
    if mats is not None:
        mats = [np.asarray(m, dtype=np.float64) for m in mats]
        D = mats[0].shape[1]
        if any(m.ndim != 2 or m.shape[1] != D for m in mats):
            raise ValueError('vad: every utterance must be a (T, %d) matrix' % D)
        x = as_c(np.concatenate(mats), np.float64)
    d = as_c(np.concatenate(dist), np.float64).copy() if flags & PCL_VAD_DIST_IN else (np.empty(rows) if 'dist' in want else None)
    o = as_c(np.concatenate(osf), np.float64).copy() if flags & PCL_VAD_OSF_IN else (np.empty(rows) if 'osf' in want else None)
    kl = ki = thr = None
    if 'kept' in want:
        kl, ki, thr = np.empty(U, dtype=np.int32), np.empty(rows, dtype=np.int32), np.empty(U)
    eng._check(eng._lib.pcl_vad(eng._ctx, U, ptr(x), ptr(off), int(D), int(simple_size), float(alpha), float(beta), int(flags),
                                ptr(kl), ptr(ki), ptr(d), ptr(o), ptr(thr)))
    return dict(row_off=off, dist=d, osf=o, kept_len=kl, kept_idx=ki, thr=thr)


def vad_batch(mfcc_list, simple_size=16, alpha=0.5, beta=0.93, details=False, engine=None):
    """VAD.mfcc() of many utterances in one call: list of the kept rows (T'_u, D) float64 -- an utterance that keeps no frame
    gives a (0, D) array.  details=True: (rows, info) with info = dict(kept=[indices], dist=[...], osf=[...], thr=(U,))."""
    eng = engine or default_engine()
    mats = [np.asarray(m, dtype=np.float64) for m in mfcc_list]
    r = _vad_call(eng, mats, simple_size, alpha, beta, 0, ('dist', 'osf', 'kept') if details else ('kept',))
    off = r['row_off']
    kept = [r['kept_idx'][off[u]:off[u] + r['kept_len'][u]].astype(np.int64) for u in range(len(mats))]
    rows = [m[k] for m, k in zip(mats, kept)]
    if not details:
        return rows
    cut = off[1:-1]
    return rows, dict(kept=kept, dist=np.split(r['dist'], cut), osf=np.split(r['osf'], cut), thr=r['thr'])


class AudioProcessing(object):
    class MFCC(object):
        def __init__(self, vec_num=13):
            self.__wav = None
            self.__wdata = None
            self.__params = None
            self.__vec_num = vec_num

        @property
        def data(self):
            return self.__wdata

        @property
        def wav(self):
            return self.__wav

        @property
        def params(self):
            """(nchannels, sampwidth, framerate, nframes, comptype, compname) (AudioProcessing.py:118-126)."""
            return self.__params if self.__params is not None else self.__wav.getparams()

        def init_audio(self, wav=None, path=None, show_pic=False):
            """Read 16-bit PCM; stereo keeps the larger of the two channel samples; zero samples are removed
            (AudioProcessing.py:128-176)."""
            self.__wav = wav if wav is not None else wave.open(path, 'rb')
            self.__params = None
            raw = self.__wav.readframes(self.__wav.getnframes())
            data = np.frombuffer(raw, dtype=np.short).copy()
            if self.__wav.getnchannels() == 2:
                data = data.reshape(-1, 2)
                data = np.maximum(data[:, 0], data[:, 1])
            self.__wdata = data[data != 0]

        def set_signal(self, samples, framerate):
            """Use an in-memory signal instead of a wav file."""
            self.__wdata = np.asarray(samples)
            self.__params = (1, 2, int(framerate), len(self.__wdata), 'NONE', 'not compressed')

        def mfcc(self, sampletime=0.025, overlap=0.5, nfft=512, cal_energy=True, d1=False, d2=False):
            return mfcc_batch([self.__wdata], self.params[2], self.__vec_num, sampletime, overlap, nfft, 26, cal_energy,
                              d1, d2)[0]

    class VAD(object):
        """AudioProcessing.VAD (AudioProcessing.py:450-543) on the device: noise estimate from the first `simple_size` frames, distance
        of every frame to it, order-statistics filter, threshold.  The reference's conventions are kept exactly (golden G19; they are
        listed as V1-V5 in include/poccala_hip.h)."""

        def __init__(self, simple_size=16):
            self.__mfcc = None
            self.__simple_size = simple_size

        def init_mfcc(self, mfcc):
            self.__mfcc = mfcc

        def __features(self):
            m = np.asarray(self.__mfcc, dtype=np.float64)
            if len(m) < self.__simple_size:                       # the reference's own failure (:472)
                raise IndexError('index %d is out of bounds for axis 0 with size %d' % (len(m), len(m)))
            return m

        def mel_distance(self, alpha=0.5):
            """Distance of every frame to the noise vector (:462-478)."""
            return _vad_call(default_engine(), [self.__features()], self.__simple_size, alpha, 0.93, 0, ('dist',))['dist']

        def osf(self, mel_distance, beta=0.93):
            """Order-statistics filter over the distances (:480-507)."""
            d = np.asarray(mel_distance, dtype=np.float64)
            if len(d) != len(self.__mfcc):
                raise ValueError('osf: %d distances for %d frames' % (len(d), len(self.__mfcc)))
            if len(d) <= 2 * self.__simple_size:                  # no frame has a full window: the reference's loop does not run
                return d.copy()
            return _vad_call(default_engine(), None, self.__simple_size, 0.5, beta, PCL_VAD_DIST_IN, ('osf',), dist=[d])['osf']

        def detect(self, mel_distance, show_pic=False):
            """Rows whose (smoothed) distance lies above the threshold (:509-536)."""
            if show_pic:
                raise NotImplementedError('VAD.detect(show_pic=True): plotting is not supported')
            d = np.asarray(mel_distance, dtype=np.float64)
            if len(d) != len(self.__mfcc):
                raise ValueError('detect: %d distances for %d frames' % (len(d), len(self.__mfcc)))
            r = _vad_call(default_engine(), None, self.__simple_size, 0.5, 0.93, PCL_VAD_OSF_IN, ('kept',), osf=[d])
            return np.asarray(self.__mfcc)[r['kept_idx'][:r['kept_len'][0]]]

        def mfcc(self, show_pic=False):
            """The frames that survive the detector (:538-543)."""
            if show_pic:
                raise NotImplementedError('VAD.mfcc(show_pic=True): plotting is not supported')
            return vad_batch([self.__features()], self.__simple_size)[0]

    class Pitch(object):
        """Voicing, ln f0 and delta ln f0 of a signal on the MFCC's frame grid (no counterpart in the reference; rule P1-P5 of
        include/poccala_hip.h at pcl_pitch): a normalised cross-correlation over the lags rate / f_max .. rate / f_min and a dynamic
        programme over them, on the device.  Used like MFCC: init_audio / set_signal, then pitch()."""

        def __init__(self, f_min=50.0, f_max=400.0):
            self.__reader = AudioProcessing.MFCC()
            self.__f_min, self.__f_max = f_min, f_max

        @property
        def data(self):
            return self.__reader.data

        @property
        def params(self):
            return self.__reader.params

        def init_audio(self, wav=None, path=None):
            self.__reader.init_audio(wav=wav, path=path)

        def set_signal(self, samples, framerate):
            self.__reader.set_signal(samples, framerate)

        def pitch(self, sampletime=0.025, overlap=0.5, ballast=7000.0, soft_min_f0=10.0, pf=0.1):
            """(T, 3) float64: [voicing in -1 .. 1, ln f0, delta ln f0], one row per MFCC row."""
            return pitch_batch([self.__reader.data], self.params[2], sampletime, overlap, self.__f_min, self.__f_max, ballast, soft_min_f0,
                               pf)[0]
