"""Inputs of the MFCC edge tests (tests/test_gpu_mfcc_edges.py on the device, tests/test_mfcc_cases.py on the CPU): the geometries, the
signals and a restatement of the index arithmetic of csrc/mfcc.hip that the CPU companion holds every case against.  Everything here is
NumPy and the float64 oracle; nothing needs a device until `call()` is given an engine."""
import ctypes as C
import math

import numpy as np

from oracle import mfcc_oracle as mo

U53 = 2.0 ** -53


# ------------------------------------------------------------------ the kernel's index arithmetic, restated
def kernel_geometry(rate, sampletime, overlap, nfft, nfilt):
    """What FrameSpec::frame (frontend_host.h), mfcc_launch and mfcc_frame_kernel derive from a call's arguments (`size`, `step`, `nbin`, `len`, `use_fft`,
    `logn`, and the launch's dynamic LDS in bytes)."""
    size = int(rate * sampletime)
    step = int(size * overlap)
    logn = 0
    while (1 << logn) < nfft:
        logn += 1
    use_fft = (1 << logn) == nfft
    nbin = nfft // 2 + 1
    return dict(size=size, step=step, nfft=nfft, nbin=nbin, len=min(size, nfft), use_fft=use_fft, logn=logn,
                lds=(size + nbin + nfilt + 8 + (2 * nfft if use_fft else 0)) * 8)


def kernel_frames(n, size, step):
    """Frames of an n-sample utterance in the launcher's integer arithmetic: 1 + ceil((n - size) / step)."""
    return 1 + (n - size + step - 1) // step


def strided_trips(count, block=256):
    """Trips of `for (i = threadIdx.x; i < count; i += blockDim.x)` that thread 0 takes."""
    return -(-count // block)


# ------------------------------------------------------------------ signals
def noise(rng, n, sd=3000.0):
    """Gaussian int16 noise: no bin of any frame is exactly 0."""
    return np.clip(np.round(sd * rng.standard_normal(n)), -32768, 32767).astype(np.int16)


def scaled_frames(sig, rate, sampletime=0.025, overlap=0.5):
    """The frames the transform sees: the oracle's pre-emphasis, blocking and per-frame window factor."""
    fr = mo.frame_blocking(mo.pre_emphasis(sig), rate, sampletime, overlap)
    with np.errstate(all='ignore'):
        return fr * mo.frame_scale(len(fr))[:, None]


# ------------------------------------------------------------------ A. the spectrum through identity tables
# (rate, sampletime, nfft): what each reaches is restated, and asserted, in tests/test_mfcc_cases.py
SPECTRUM_CASES = [
    (16000, 0.025, 512),        # the default, size < nfft
    (16000, 0.025, 256),        # truncation on the radix-2 path
    (16000, 0.025, 400),        # size == nfft, direct summation
    (16000, 0.025, 300),        # truncation on the direct path
    (16000, 0.032, 512),        # size == nfft, radix-2
    (8000, 0.008, 64),          # small FFT
    (8000, 0.004, 32),          # small FFT
    (8000, 0.004, 16),          # size 32 > nfft
    (16000, 0.025, 1024),       # nbin = 513: three trips of the strided loops
    (48000, 0.025, 2048),       # size 1200, nbin = 1025
]


def case_id(case):
    return '-'.join(str(v) for v in case)


def spectrum_signals(rate, sampletime, nfft):
    """Four utterances of 2, 3, 4 and 7 frames in one call: an exact fit, two ragged last frames (one sample and all but one sample of
    padding) and a longer one at an odd sample offset."""
    g = kernel_geometry(rate, sampletime, 0.5, nfft, 1)
    size, step = g['size'], g['step']
    rng = np.random.default_rng(7000 + nfft + size)
    return [noise(rng, n) for n in (size + step, size + step + 1, size + 3 * step - 1, size + 6 * step)]


def identity_tables(nfft):
    """nfilt = rank = nbin, mel response and DCT the identity: the kernel's output row is ln |X[k]| for every bin."""
    n = np.arange(nfft)
    nbin = nfft // 2 + 1
    eye = np.eye(nbin)
    return np.cos(2 * np.pi * n / nfft), -np.sin(2 * np.pi * n / nfft), eye, eye.copy()


def spectrum_reference(sig, rate, sampletime, nfft):
    """(|rfft| of the oracle's frames, A = sum |x_n| over the samples that enter the transform), per frame."""
    fr = scaled_frames(sig, rate, sampletime)
    return np.abs(np.fft.rfft(fr, nfft)), np.abs(fr[:, :min(fr.shape[1], nfft)]).sum(axis=1)


def spectrum_bound(mag_ref, A, g):
    """Rounding of the transform as the kernel orders it, per bin.  Radix-2: logn stages, each a complex multiply by a rounded twiddle
    and an add, at most 8 roundings of relative size 2^-53 against a partial sum that |x|_1 bounds.  Direct summation: `len` fused
    multiply-adds by rounded twiddles, 1 rounding each.  The second term is the output's trip through log and exp."""
    growth = 8 * g['logn'] if g['use_fft'] else g['len']
    return growth * U53 * A[:, None] + 4 * 2.0 ** -52 * mag_ref


# ------------------------------------------------------------------ B. real tables where the oracle is finite
# (rate, sampletime, nfft, the largest filter count with no empty filter)
TABLE_CASES = [
    (16000, 0.025, 512, 39),
    (16000, 0.025, 256, 20),
    (16000, 0.025, 300, 23),
    (16000, 0.008, 128, 10),
    (8000, 0.008, 64, 11),
    (8000, 0.004, 32, 6),
    (44100, 0.025, 2048, 77),
    (48000, 0.025, 2048, 73),
    (16000, 0.025, 1024, 76),
]
EMPTY_FILTER_CASE = dict(rate=16000, nfft=512, filterbanks=300, vec_num=40)


def table_signals(rate, sampletime, nfft):
    g = kernel_geometry(rate, sampletime, 0.5, nfft, 1)
    size, step = g['size'], g['step']
    rng = np.random.default_rng(8000 + nfft + rate)
    return [noise(rng, n) for n in (size + step, size + 2 * step + 3, size + 7 * step - 1)]


def table_runs(filterbanks):
    """(vec_num, cal_energy, d1, d2) of the calls of one table case: vec_num in {1, 13, filterbanks}, the energy both ways."""
    return [(v, e, v == 13, v == 13 and e) for v in (1, 13, filterbanks) for e in (True, False)]


# ------------------------------------------------------------------ C. frame counts, steps, deltas
EDGE_RATE = 16000                                               # frame 400, step 200
FRAME_COUNT_LENGTHS = (400, 401, 599, 600, 601, 800, 801, 1000, 1200, 1400)
FRAME_COUNTS = (1, 2, 2, 2, 3, 3, 4, 4, 5, 6)


def frame_count_signals():
    rng = np.random.default_rng(9001)
    return [noise(rng, n) for n in FRAME_COUNT_LENGTHS]


def step_signals(overlap):
    """overlap 1.0: step == size;  1.5: step 600 > size, samples are skipped and 1100 and 1700 samples end in a frame of padding only;
    0.005: step 2, eleven frames that are almost the same."""
    rng = np.random.default_rng(9100 + int(1000 * overlap))
    lengths = {1.0: (800, 801, 1199, 2000), 1.5: (1000, 1100, 1600, 1700, 1001), 0.005: (420,)}[overlap]
    return [noise(rng, n) for n in lengths]


def many_short_signals():
    rng = np.random.default_rng(9200)
    return [noise(rng, 401 + u % 5) for u in range(300)]


def structured_signals():
    """Signals with structure, one call: a full-scale square wave, a constant, noise with a full-scale impulse in its last sample, digital
    silence, noise whose last frame is silence, and plain noise after them (its rows follow the -inf / NaN rows)."""
    rng = np.random.default_rng(9300)
    square = np.where(np.arange(1000) % 2 == 0, -32768, 32767).astype(np.int16)
    const = np.full(1001, 12345, dtype=np.int16)
    impulse = noise(rng, 999)
    impulse[-1] = 32767
    silence = np.zeros(1400, dtype=np.int16)
    tail = noise(rng, 2000)
    tail[1600:] = 0                                              # frame 8 = samples 1600 .. 1999
    return [square, const, impulse, silence, tail, noise(rng, 777)]


def delta_bound(src):
    """mo.delta's sum of five products and a division, one rounding each and one more where the device contracts: 6 * 2^-53 * sum |i x_i|
    / 10 per entry."""
    pad = np.pad(np.abs(src), ((2, 2), (0, 0)), mode='edge')
    t = len(src)
    return 6 * U53 * sum(abs(i) * pad[2 + i:2 + i + t] for i in range(-2, 3)) / 10


# ------------------------------------------------------------------ D. the LDS rule
REFUSED_NFFT = 16384                                            # 2 * 16384 doubles of work arrays alone: 262144 bytes
LARGE_NFFT = 4096


# ------------------------------------------------------------------ one call through the C binding
def call(eng, name, sigs, dtype, rate, sampletime, overlap, nfft, tables, mflags):
    """pcl_mfcc / pcl_mfcc_pcm16 with the caller's tables: (rc, rows)."""
    from poccala_amd._lib import as_c, ptr
    twc, tws, resp, dct = [as_c(t, np.float64) for t in tables]
    nfilt, rank = resp.shape[0], dct.shape[0]
    size = int(rate * sampletime)
    step = int(size * overlap)
    rows = int(sum(1 + math.ceil((len(s) - size) / step) for s in sigs))
    dim = rank * (3 if mflags & 4 else 2 if mflags & 2 else 1)
    flat = as_c(np.concatenate(sigs), dtype)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    out = np.zeros((rows, dim))
    rc = getattr(eng._lib, name)(eng._ctx, len(sigs), ptr(flat), ptr(off), int(rate), float(sampletime), float(overlap), int(nfft), nfilt, rank,
                                 mflags, ptr(twc), ptr(tws), ptr(resp), ptr(dct), ptr(out), C.c_int64(rows))
    return rc, out
