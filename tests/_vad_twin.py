"""NumPy float64 restatement of the reference's AudioProcessing.VAD (StatisticalModel/AudioProcessing.py:450-543): the host twin the
device kernels (csrc/vad.hip) are held against, the way tests/_segment_twin.py serves the segmental training.

Conventions (V1-V5 of include/poccala_hip.h, pcl_vad):
  V1  noise = (1/s) * (sum of the first s rows), then s times  noise = a*noise + (1-a)*x_i  (:467-472)
  V2  distance_t = sqrt(sum_d (noise_d - x_td)^2), summed over d in ascending order        (:475-477)
  V3  for s <= i < T - s: window d[i-s : i+s] (2s values), sorted ascending, h = int(beta*(2s+1)),
      out_i = (1-beta)*w[h] + beta*w[h+1]; every other frame keeps its distance            (:500-507)
  V4  thr = out[int(s/2)] * (max - min) / max; a frame is kept iff out_t - thr > 0         (:516-536)
  V5  T < s raises IndexError (:472); s <= T < 2s leaves the filter with nothing to do
Every step is one correctly rounded float64 operation at a time, in the order written, so a device kernel can match it bit for bit.
"""
import numpy as np


def noise_vector(x, s=16, alpha=0.5):
    x = np.asarray(x, dtype=np.float64)
    if len(x) < s:
        raise IndexError('VAD: %d frames, fewer than simple_size = %d' % (len(x), s))
    acc = x[0].copy()
    for i in range(1, s):
        acc = acc + x[i]
    noise = (1.0 / s) * acc
    for i in range(s):
        noise = alpha * noise + (1 - alpha) * x[i]
    return noise


def mel_distance(x, s=16, alpha=0.5):
    x = np.asarray(x, dtype=np.float64)
    noise = noise_vector(x, s, alpha)
    with np.errstate(all='ignore'):
        diff = noise[None, :] - x
        sq = diff * diff
        acc = np.zeros(len(x))
        for d in range(x.shape[1]):                 # ascending d, one add at a time
            acc = acc + sq[:, d]
        return np.sqrt(acc)


def osf_h(s, beta):
    return int(beta * (2 * s + 1))


def osf(dist, s=16, beta=0.93):
    dist = np.asarray(dist, dtype=np.float64)
    out = dist.copy()
    h = osf_h(s, beta)
    T = len(dist)
    if T - s > s and not (0 <= h and h + 1 < 2 * s):
        raise IndexError('VAD: order statistic %d of a window of %d' % (h + 1, 2 * s))
    with np.errstate(all='ignore'):
        for i in range(s, T - s):
            w = np.sort(dist[i - s:i + s])          # NaN sorts last
            out[i] = (1 - beta) * w[h] + beta * w[h + 1]
    return out


def threshold(sm, s=16):
    sm = np.asarray(sm, dtype=np.float64)
    with np.errstate(all='ignore'):
        mx, mn = sm.max(), sm.min()                 # NaN propagates
        return sm[int(s / 2)] * (mx - mn) / mx


def keep_mask(sm, s=16):
    with np.errstate(all='ignore'):
        return (np.asarray(sm, dtype=np.float64) - threshold(sm, s)) > 0.


def vad(x, s=16, alpha=0.5, beta=0.93):
    """dict(dist, osf, thr, kept): kept = ascending row indices that survive."""
    d = mel_distance(x, s, alpha)
    sm = osf(d, s, beta)
    return dict(dist=d, osf=sm, thr=threshold(sm, s), kept=np.nonzero(keep_mask(sm, s))[0])


def from_distances(d, s=16, beta=0.93):
    """V3 + V4 on given distances (the device's own, in the bit-equality tests)."""
    sm = osf(d, s, beta)
    return dict(osf=sm, thr=threshold(sm, s), kept=np.nonzero(keep_mask(sm, s))[0])


def vad_batch(mats, s=16, alpha=0.5, beta=0.93):
    """Ragged batch: (lens, begin, rows) as Engine.frontend reports them; an utterance that keeps nothing has length 0."""
    res = [vad(m, s, alpha, beta) for m in mats]
    lens = np.array([len(r['kept']) for r in res], dtype=np.int32)
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows = np.concatenate([np.asarray(m, dtype=np.float64)[r['kept']] for m, r in zip(mats, res)])
    return lens, begin, rows
