#!/usr/bin/env python3
"""One hash per entry point of the frame-level transforms (fMLLR, MLLT, LDA, CMVN) and of MLLR, of everything the call returns or leaves
resident, on small ragged inputs that cross every tile and chunk edge: for A/B runs of two builds of the library (same bits or not).
One process per library (POCCALA_HIP_LIB picks it) and per GEMM form (PCL_MLLR_VALU, PCL_LDA_VALU); compare the printed lines.
The chunk lengths are set here (PCL_MLLR_CHUNK = PCL_MLLT_CHUNK = 50, PCL_LDA_CHUNK = 64): every group has several chunks and a
chunk boundary falls inside an utterance."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.environ.update(PCL_MLLR_CHUNK='50', PCL_MLLT_CHUNK='50', PCL_LDA_CHUNK='64')
import numpy as np

import _adapt_twin as at
from poccala_amd import PCL_F64, Engine, synth

T_UTT = np.array([130, 64, 65, 40, 97, 50], dtype=np.int32)          # across the 64-frame tile of the reduction and the 32-frame tile of the apply
SPEAKER = np.array([0, 1, 1, 2, -1, 0], dtype=np.int32)              # speaker 1: every frame the same; speaker 2: 40 frames, below MIN_OCC
GAPS = np.array([3, 0, 2, 5, 0, 1], dtype=np.int64)
S_SPK, MIN_OCC, N_ITER = 3, 50.0, 20


def show(name, *arrays):
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(('%s%s' % (a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    print('%-44s %s' % (name, h.hexdigest()), flush=True)


def held(eng):
    return eng.frames_download(np.float64), eng.frames_download(np.float32)


def layout(T, gaps):
    begin = (np.cumsum(gaps) + np.concatenate([[0], np.cumsum(T[:-1].astype(np.int64))])).astype(np.int64)
    return begin, int(begin[-1] + T[-1] + 4)


def frame_rules(D):
    """fMLLR, both MLLT forms and the frame transform on one aligned batch"""
    tag = 'D=%d ' % D
    model = at.make_case(D)[0]
    rng = np.random.default_rng(31 * D)
    begin, F = layout(T_UTT, GAPS)
    frames = rng.standard_normal((F, D))
    for u in np.flatnonzero(SPEAKER == 1):
        frames[begin[u]:begin[u] + T_UTT[u]] = frames[begin[u]]      # duplicated frames: G of speaker 1 has rank 1
    labels = [rng.integers(0, at.J, size=max(1, min(4, int(T) // 8))).astype(np.int32) for T in T_UTT]
    trans = np.stack([synth.random_left_right_transmat(np.random.default_rng(4), 3) for _ in range(at.J)])
    eng = Engine(0)
    eng.load_model(*model)
    eng.load_units(trans)
    eng.load_frames(frames)
    b = eng.label_batch(labels, T_UTT, begin)
    b.score(PCL_F64)
    b.forward_backward()
    eng.fmllr_zero(S_SPK)
    b.accumulate_fmllr(SPEAKER)
    show(tag + 'accumulate_fmllr: G k beta', *eng.fmllr_stats())
    W, logdet, q, status = eng.fmllr_estimate(N_ITER, MIN_OCC)
    print(tag + 'fmllr statuses', status.tolist())
    show(tag + 'fmllr_estimate: W logdet q status', W, logdet, q, status)
    eng.stats_zero()
    b.accumulate(PCL_F64)
    keep = np.ones(at.J, dtype=np.int32)
    keep[2] = 0
    for name, sk, uk in (('every state', None, None), ('state_keep', keep, (SPEAKER >= 0).astype(np.int32))):
        eng.mllt_zero(sk)
        b.accumulate_mllt(uk)
        Fs, beta = eng.mllt_stats()
        show(tag + 'accumulate_mllt (%s): F beta' % name, Fs, np.array([beta]))
        est = eng.mllt_estimate(N_ITER, MIN_OCC)
        print(tag + 'mllt status (%s)' % name, est['status'])
        show(tag + 'mllt_estimate (%s): A logdet q G occ status' % name, est['A'], np.array([est['logdet']]), est['q_trace'], est['G'], est['occ'],
             np.array([est['status']]))
    b.close()
    eng.transform_frames(T_UTT, begin, SPEAKER)
    show(tag + 'transform_frames: f64 f32', *held(eng))
    eng.close()


def lda():
    D, R = 13, 4
    rng = np.random.default_rng(5)
    begin, F = layout(T_UTT, GAPS)
    frames = rng.standard_normal((F, D))
    cls = rng.integers(-1, R - 1, size=F).astype(np.int32)           # class 3 is empty
    eng = Engine(0)
    eng.load_frames(frames)
    eng.lda_zero(R, 1, 1)                                            # order 40: three tile rows
    eng.lda_accumulate(T_UTT, begin, cls)
    show('lda_accumulate: n s S', *eng.lda_stats())
    eng.splice_project(T_UTT, begin, 1, 1, rng.standard_normal((10, 3 * D)), rng.standard_normal(10))
    show('splice_project: f64 f32', *held(eng))
    eng.close()


def cmvn():
    D = 13
    T = np.array([1100, 63, 40], dtype=np.int32)                    # across the 1024-row chunk of the statistics
    spk = np.array([0, 1, -1], dtype=np.int32)
    begin, F = layout(T, np.array([2, 0, 3], dtype=np.int64))
    frames = np.random.default_rng(6).standard_normal((F, D)) * 3.0 + 1.0
    eng = Engine(0)
    eng.load_frames(frames)
    eng.cmvn_zero(2)
    eng.cmvn_accumulate(T, begin, spk)
    show('cmvn_accumulate: n s q', *eng.cmvn_stats())
    for norm_vars in (True, False):
        eng.load_frames(frames)
        status = eng.cmvn_apply(T, begin, spk, norm_vars, 1e-20, 1)
        show('cmvn_apply norm_vars=%d: status f64 f32' % norm_vars, status, *held(eng))
    for center in (True, False):
        eng.load_frames(frames)
        eng.cmvn_sliding(T, begin, 8, 1, center, True)
        show('cmvn_sliding center=%d: f64 f32' % center, *held(eng))
    eng.close()


def mllr():
    D = 1                                                            # the twin's smallest case
    model, frames, gamma = at.make_case(D)
    eng = Engine(0)
    eng.load_model(*model)
    eng.load_frames(np.asarray(frames, dtype=np.float64))
    F = len(frames)
    b = eng.all_state_batch(np.array([F], dtype=np.int32), np.array([0], dtype=np.int64))
    b.score(PCL_F64)
    with np.errstate(divide='ignore'):
        b.set_posteriors([np.concatenate([np.full((1, F), -np.inf), np.log(gamma.T), np.full((1, F), -np.inf)])])
    eng.stats_zero()
    b.accumulate(PCL_F64)
    b.close()
    show('mllr_estimate one class: W occ status', *eng.mllr_estimate(None, 1, 1.0))
    show('mllr_estimate three classes: W occ status', *eng.mllr_estimate(at.CLASSES3, 3, at.MIN_OCC3))
    eng.close()


if __name__ == '__main__':
    print('PCL_MLLR_VALU', os.environ.get('PCL_MLLR_VALU', '0'), 'PCL_LDA_VALU', os.environ.get('PCL_LDA_VALU', '0'))
    for D in (13, 39):
        frame_rules(D)
    lda()
    cmvn()
    mllr()
