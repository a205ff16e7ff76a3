"""Inputs and float64 references of the log-determinant tests (tests/test_gpu_logdet.py on the device, tests/test_logdet_cases.py on the
CPU).  Engine.load_model(..., logdet=True) (PCL_MODEL_LOGDET) swaps quirk Q1's constant -D/2 ln 2pi - 1/2 sum(var) for the textbook
-D/2 ln 2pi - 1/2 sum(ln var); the library computes that constant in seven places, and the cases here are the smallest
ones in which each of them decides a compared number.  Everything is NumPy and the oracle.

The reference, written out:  ln b(x) = lse_m [ ln w_m - D/2 ln 2pi - 1/2 sum_d ln var_md - 1/2 sum_d (x_d - mu_md)^2 / var_md ]  (`point`).
For the E-step and the M-step the oracle serves unchanged through an identity: a log-determinant model (mu, var, w) IS the Q1 model
(mu, var, w') with w'_m = w_m exp(1/2 (sum_d var_md - sum_d ln var_md)) (`q1_weights`); oracle/poccala_oracle.py reads weights only through
np.log(w), so w' need not sum to one.  Its largest exponent here is ~ 280 (variance 5e-7, D = 39), far below 709.

A MUTANT reference gives the mixtures of `q1_mask` the Q1 constant and the others the log-determinant one: what a site that ignored the flag
would compute when it handles exactly those mixtures (`point(..., q1_mask=...)`; all True is the Q1 reference itself).

Cases are dicts: name, mean / var / w (J, M, D) / (J, M) float64, frames (F, D) float32, and the batch layout of the case."""
import functools

import numpy as np

from oracle import poccala_oracle as po

LN2PI = float(np.log(2.0 * np.pi))
LOG2E = 1.4426950408889634
COND_MAX = 96.0                    # pcl_internal.h pcl_split_threshold: ctx->cond_max (default 96) whenever states may be split
F32_LOGLIK_ATOL = 5e-5             # tests/test_gpu_parity.py
S, E = 5, 3
KEYS = ('acc', 'alpha_acc', 'mean_acc', 'cov_acc')


# ------------------------------------------------------------------ references
def components(x, mean, var, w, q1_mask=None):
    """(T, M): ln w_m + the log-density of mixture m under the log-determinant constant (Q1's where q1_mask[m])."""
    x = np.asarray(x, dtype=np.float64)
    D = mean.shape[1]
    tail = np.log(var).sum(axis=1)
    if q1_mask is not None:
        tail = np.where(q1_mask, var.sum(axis=1), tail)
    with np.errstate(divide='ignore'):
        const = np.log(w) - 0.5 * D * LN2PI - 0.5 * tail
    diff = x[:, None, :] - mean[None]
    return const[None] - 0.5 * (diff * diff / var[None]).sum(axis=2)


def point(x, mean, var, w, q1_mask=None):
    """ln b(x_t) (T,) of one state, max-shifted log-sum-exp in float64."""
    comp = components(x, mean, var, w, q1_mask)
    top = comp.max(axis=1, keepdims=True)
    return (top + np.log(np.exp(comp - top).sum(axis=1, keepdims=True)))[:, 0]


def point_states(x, mean, var, w, q1_mask=None):
    """(J, T): every state on every frame; q1_mask None, True (the Q1 reference) or (J, M) bool."""
    J, M = w.shape
    if q1_mask is True:
        q1_mask = np.ones((J, M), dtype=bool)
    return np.stack([point(x, mean[j], var[j], w[j], None if q1_mask is None else q1_mask[j]) for j in range(J)])


def q1_weights(var, w, q1_mask=None):
    """w' with which the Q1 oracle computes the log-determinant model (mixtures of q1_mask keep w: the mutants)."""
    wp = w * np.exp(0.5 * (var.sum(axis=-1) - np.log(var).sum(axis=-1)))
    return wp if q1_mask is None else np.where(q1_mask, w, wp)


def off_pipe(mean, var, threshold=COND_MAX):
    """model_derive.hip state_prepass_kernel's rule, (J, M) bool: (float)(log2e sum_d (mu - (float) mean_m mu)^2 / (2 var)) > threshold."""
    c = mean.mean(axis=1, keepdims=True).astype(np.float32).astype(np.float64)
    return (LOG2E * ((mean - c) ** 2 * (0.5 / var)).sum(axis=2)).astype(np.float32) > np.float32(threshold)


def f32_parameter_loss(x, mean, var, w):
    """(J, T): what the float64 reference itself moves by when it is given the f32 roundings of mean and var (the frames are f32 already):
    the part of an f32 kernel's error that no arithmetic can avoid.  Where this nears a case's allowance the case has left the regime the
    bound was measured in."""
    r = lambda a: a.astype(np.float32).astype(np.float64)
    return np.abs(point_states(x, r(mean), r(var), w) - point_states(x, mean, var, w))


def oracle_model(mean, var, w, trans, q1_mask=None):
    wp = q1_weights(var, w, q1_mask)
    return {u: dict(trans=trans[u], gmms=[(mean[u * E + k], var[u * E + k], wp[u * E + k]) for k in range(E)]) for u in range(len(trans))}


def estep(c, mean=None, var=None, w=None, acc_q1_mask=None):
    """The oracle's E-step of a label case under the log-determinant model: dict(logp (U,), B [per utterance (N, T)], stats: linear-domain
    acc (J, M), alpha_acc (J,), mean_acc, cov_acc (J, M, D), log: the same merged in the log domain, per state, for gmm_update_param).
    acc_q1_mask (J, M): the ACCUMULATE pass alone takes the Q1 constant for those mixtures (alpha, beta and ln b stay the true ones)."""
    mean, var, w = (c['mean'] if mean is None else mean), (c['var'] if var is None else var), (c['w'] if w is None else w)
    J, M, D = mean.shape
    model = oracle_model(mean, var, w, c['trans'])
    mut = None if acc_q1_mask is None else oracle_model(mean, var, w, c['trans'], acc_q1_mask)
    lin = dict(acc=np.zeros((J, M)), alpha_acc=np.zeros(J), mean_acc=np.zeros((J, M, D)), cov_acc=np.zeros((J, M, D)))
    log = [dict(acc=np.full(M, -np.inf), alpha_acc=-np.inf, mean_acc=np.full((M, D), -np.inf), cov_acc=np.full((M, D), -np.inf)) for _ in range(J)]
    logp, Bs = [], []
    for u, lab in enumerate(c['labels']):
        x = c['frames'][c['begin'][u]:c['begin'][u] + c['lens'][u]].astype(np.float64)
        bw, accs, (_, _, b, _) = po.estep_utterance(x, list(lab), model)
        if mut is not None:
            accs = [po.UnitAcc(S, mut[unit]['gmms']) for unit in lab]
            po.update_acc(bw, [b], [x], accs, [mut[unit]['gmms'] for unit in lab])
        logp.append(float(bw['logp'][0]))
        Bs.append(b)
        for pos, unit in enumerate(lab):
            for k in range(E):
                j, a = unit * E + k, accs[pos].gmm[k]
                for key in KEYS:
                    with np.errstate(all='ignore'):
                        lin[key][j] += np.exp(a[key])
                    log[j][key] = np.logaddexp(log[j][key], a[key])
    return dict(logp=np.array(logp), B=Bs, stats=lin, log=log)


# ------------------------------------------------------------------ ladder, outlier
LADDER_J, LADDER_M, LADDER_T = 4, 70, 130
LADDER_DIMS = (13, 20, 39)
LADDER_SCALES = (0.25, 1.0, 4.0)
ZERO_WEIGHT = (1, 3)


@functools.lru_cache(maxsize=None)
def ladder(D):
    """J = 4, M = 70 (three m-tiles, the last of six mixtures), T = 130, one all-state utterance.  Variances U(0.5, 2) s_m with s_m cycling
    through 0.25, 1, 4: sum ln var differs by up to ~ 1.39 D nats between mixtures of one state while sum var moves the other way.  The
    means stay close enough to the state's centre for every mixture to be on the matrix pipe (asserted by the CPU companion).  One weight is
    exactly 0.  Frames come from the states' own mixtures, state t % J."""
    rng = np.random.default_rng(4100 + D)
    J, M, T = LADDER_J, LADDER_M, LADDER_T
    s = np.resize(LADDER_SCALES, M)
    var = rng.uniform(0.5, 2.0, (J, M, D)) * s[None, :, None]
    mean = rng.standard_normal((J, M, D)) * 0.35 * np.sqrt(s)[None, :, None]
    w = rng.dirichlet(np.ones(M), J)
    w[ZERO_WEIGHT] = 0.0
    w[ZERO_WEIGHT[0]] /= w[ZERO_WEIGHT[0]].sum()
    st, comp = np.arange(T) % J, rng.integers(0, M, T)
    x = (mean[st, comp] + np.sqrt(var[st, comp]) * rng.standard_normal((T, D))).astype(np.float32)
    return dict(name='ladder D=%d' % D, mean=mean, var=var, w=w, frames=x, state=st)


BROAD_SCALE, F16_MAX = 1024.0, 65504.0


@functools.lru_cache(maxsize=None)
def broad():
    """ladder's shape at D = 39 with every variance U(0.5, 2) * 1024 and the means 1.2 * 32 N(0, 1): an ordinary problem scaled by exact
    powers of two (the kernels' arithmetic is that of the unscaled problem, ln b lower by D/2 ln 1024), every mixture on the pipe, the
    mixtures of a state well apart (a frame's ln b rests on one or two of them).  Here sum var exceeds sum ln var by ~ 5e4, so K0 of
    state_prepass_kernel (max_m k'_m, which the folded-constant layout keeps k'_m relative to in two f16 pieces, summed with the
    quadratic terms in f32) taken with Q1's constant lies ~ 3.5e4 log2 units below every k'_m of the log-determinant: still inside f16,
    where nothing flags the tile, but at a magnitude whose f32 spacing is 2^-9 log2 units or more (`k_prime`, and the CPU companion)."""
    rng = np.random.default_rng(4150)
    J, M, T, D = LADDER_J, LADDER_M, LADDER_T, 39
    var = rng.uniform(0.5, 2.0, (J, M, D)) * BROAD_SCALE
    mean = rng.standard_normal((J, M, D)) * 1.2 * np.sqrt(BROAD_SCALE)
    w = rng.dirichlet(np.ones(M), J)
    st, comp = np.arange(T) % J, rng.integers(0, M, T)
    x = (mean[st, comp] + np.sqrt(var[st, comp]) * rng.standard_normal((T, D))).astype(np.float32)
    return dict(name='broad', mean=mean, var=var, w=w, frames=x, state=st)


def k_prime(mean, var, w, q1=False):
    """(J, M) float64: k'_m of the centred expansion in log2 units, as state_prepass_kernel and derive_kernel form it:
    log2e (ln w - D/2 ln 2pi - 1/2 tail - sum_d (mu - c)^2 / (2 var)), c = (float) mean_m mu, tail = sum ln var (sum var with q1)."""
    D = mean.shape[2]
    c = mean.mean(axis=1, keepdims=True).astype(np.float32).astype(np.float64)
    tail = var.sum(axis=2) if q1 else np.log(var).sum(axis=2)
    with np.errstate(divide='ignore'):
        return LOG2E * (np.log(w) - 0.5 * D * LN2PI - 0.5 * tail - ((mean - c) ** 2 * (0.5 / var)).sum(axis=2))


OUTLIER_T, OUTLIER_FRAMES, OUTLIER_FEATURE, OUTLIER_SIGMA = 260, (17, 256), 3, 400.0


@functools.lru_cache(maxsize=None)
def outlier():
    """ladder at D = 39 on 260 frames (a second 256-frame workgroup of four frames per state); frames 17 (first workgroup) and 256 (second)
    lie 400 sigma (of the widest variance) beyond every mean along feature 3 and are 0 elsewhere: the f16 kernel clamps them and flags the
    tile, the direct-form fix-up rescores it from the master rows."""
    c = ladder(39)
    rng = np.random.default_rng(4200)
    mean, var = c['mean'], c['var']
    J, M, D = mean.shape
    st, comp = np.arange(OUTLIER_T) % J, rng.integers(0, M, OUTLIER_T)
    x = (mean[st, comp] + np.sqrt(var[st, comp]) * rng.standard_normal((OUTLIER_T, D))).astype(np.float32)
    for t in OUTLIER_FRAMES:
        x[t] = 0.0
        x[t, OUTLIER_FEATURE] = OUTLIER_SIGMA * np.sqrt(var.max()) + np.abs(mean[:, :, OUTLIER_FEATURE]).max()
    return dict(name='outlier', mean=mean, var=var, w=c['w'], frames=x, state=st)


# ------------------------------------------------------------------ split
SPLIT_UNITS, SPLIT_M, SPLIT_D = 2, 48, 39
SPLIT_U, SPLIT_L, SPLIT_PER = 5, 3, 5


@functools.lru_cache(maxsize=None)
def split():
    """tests/test_gpu_parity.py split_model's construction (the synthetic model, mean ~ N(0, 1), var ~ U(0.5, 2), weights Dirichlet(1)) at
    2 units (J = 6), M = 48, D = 39: state j holds (j % 4) * 3 mixtures of variance 1e-3 .. 1e-2 -- 0, 3, 6, 9, 0 -- and the last state
    holds only such mixtures (it leaves the pipe whole).  Five utterances of three units, five frames per state; the frames of a state
    alternate between its tight and its broad mixtures, so both sides of every split carry compared numbers."""
    from poccala_amd import synth
    rng = np.random.default_rng(4300)
    mean, var, w, trans = synth.make_model(SPLIT_UNITS, SPLIT_M, SPLIT_D, seed=4301)
    J, M, D = mean.shape
    tight = []
    for j in range(J):
        n = (j % 4) * 3 if j < J - 1 else M
        idx = np.sort(rng.choice(M, n, replace=False))
        var[j, idx] = rng.uniform(1e-3, 1e-2, (n, D))
        tight.append(idx)
    labels = [list(rng.integers(0, SPLIT_UNITS, SPLIT_L)) for _ in range(SPLIT_U)]
    labels[0][0], labels[1][0] = 0, 1                                  # both units occur
    TU = SPLIT_L * E * SPLIT_PER
    lens, begin = np.full(SPLIT_U, TU, dtype=np.int64), np.arange(SPLIT_U, dtype=np.int64) * TU
    st = np.concatenate([np.repeat([unit * E + k for unit in lab for k in range(E)], SPLIT_PER) for lab in labels])
    comp = np.empty(len(st), dtype=np.int64)
    for i, j in enumerate(st):
        broad = np.setdiff1d(np.arange(M), tight[j])
        pool = tight[j] if (i % 2 == 0 and len(tight[j])) or not len(broad) else broad
        comp[i] = rng.choice(pool)
    x = (mean[st, comp] + np.sqrt(var[st, comp]) * rng.standard_normal((len(st), D))).astype(np.float32)
    rows = [np.concatenate([[-1], [unit * E + k for unit in lab for k in range(E)], [-2]]).astype(np.int32) for lab in labels]
    return dict(name='split', mean=mean, var=var, w=w, trans=trans, frames=x, state=st, comp=comp, tight=tight, labels=labels, lens=lens, begin=begin,
                rows=rows)


def compared_pairs(c):
    """(J, F) bool: the (state, frame) pairs the sentence batch of a label case scores (every row of an utterance on every frame of it)."""
    J = c['mean'].shape[0]
    out = np.zeros((J, c['frames'].shape[0]), dtype=bool)
    for u, rows in enumerate(c['rows']):
        out[rows[rows >= 0], c['begin'][u]:c['begin'][u] + c['lens'][u]] = True
    return out


# ------------------------------------------------------------------ collapsed
COLLAPSED_M, COLLAPSED_D, COLLAPSED_LENS, COLLAPSED_BROAD = 160, 39, (65, 257, 64), 20


@functools.lru_cache(maxsize=None)
def collapsed():
    """Three states of M = 160 (R MTS + 1 = 5 m-tiles at the shipped ring), D = 39, scored on 65, 257 and 64 frames of their own: state 0 has
    every mixture at a variance of 10^U(-6, -3) (times U(0.5, 2) per feature) -- no tile on the pipe --, state 1 all but 20, state 2 none.
    Under the log-determinant a collapsed mixture's constant is up to ~ 280 nats ABOVE a broad neighbour's.  Frames come from the state's
    own mixtures, alternating between tight and broad ones where both exist."""
    rng = np.random.default_rng(4400)
    M, D, lens = COLLAPSED_M, COLLAPSED_D, COLLAPSED_LENS
    mean = rng.standard_normal((3, M, D)) * 0.5
    var = rng.uniform(0.5, 2.0, (3, M, D))
    w = rng.uniform(0.5, 1.5, (3, M))
    w /= w.sum(axis=1, keepdims=True)
    tight = []
    for j, n in enumerate((M, M - COLLAPSED_BROAD, 0)):
        idx = np.sort(rng.choice(M, n, replace=False))
        var[j, idx] = (10.0 ** rng.uniform(-6, -3, n))[:, None] * rng.uniform(0.5, 2.0, (n, D))
        tight.append(idx)
    xs, comps = [], []
    for j, T in enumerate(lens):
        broad = np.setdiff1d(np.arange(M), tight[j])
        comp = np.array([rng.choice(tight[j] if (t % 2 == 0 and len(tight[j])) or not len(broad) else broad) for t in range(T)])
        xs.append(mean[j, comp] + np.sqrt(var[j, comp]) * rng.standard_normal((T, D)))
        comps.append(comp)
    begin = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return dict(name='collapsed', mean=mean, var=var, w=w, frames=np.concatenate(xs).astype(np.float32), state=np.repeat(np.arange(3), lens),
                comp=np.concatenate(comps), tight=tight, lens=list(lens), begin=begin)


# ------------------------------------------------------------------ survives
SURV_UNITS, SURV_M, SURV_D, SURV_U, SURV_T, SURV_L = 2, 8, 13, 7, 50, 3
SURV_SEG_FRAMES, SURV_K, SURV_MIXUP = 40, 4, 16


@functools.lru_cache(maxsize=None)
def survives():
    """tests/test_gpu_units.py problem(...)'s recipe at 2 units (J = 6), M = 8, D = 13: the synthetic model, seven ragged utterances of N(0, 1)
    frames, labels of three units; W is the mean transform of step 6 ([b | A], A = I + 0.1 N(0, 1): well conditioned), frame_state the owner
    map of the k-means step (40 frames per state from row 0)."""
    from poccala_amd import synth
    seed = 4500
    mean, var, w, trans = synth.make_model(SURV_UNITS, SURV_M, SURV_D, seed=seed)
    frames, lens, begin = synth.make_frames(SURV_U, SURV_T, SURV_D, seed=seed + 1, ragged=True)
    labels = [list(l) for l in synth.make_labels(SURV_U, SURV_L, SURV_UNITS, seed=seed + 2)]
    rng = np.random.default_rng(seed + 3)
    W = np.concatenate([0.2 * rng.standard_normal((SURV_D, 1)), np.eye(SURV_D) + 0.1 * rng.standard_normal((SURV_D, SURV_D))], axis=1)[None]
    J = mean.shape[0]
    frame_state = np.full(frames.shape[0], -1, dtype=np.int32)
    frame_state[:J * SURV_SEG_FRAMES] = np.repeat(np.arange(J), SURV_SEG_FRAMES)
    rows = [np.concatenate([[-1], [unit * E + k for unit in lab for k in range(E)], [-2]]).astype(np.int32) for lab in labels]
    return dict(name='survives', mean=mean, var=var, w=w, trans=trans, frames=frames, lens=lens, begin=begin, labels=labels, rows=rows, W=W,
                frame_state=frame_state)


# ------------------------------------------------------------------ what is compared, and the allowance of every compared ln b
def compared(c):
    """(J, F) bool: the (state, frame) pairs the device test of the case compares."""
    J, F = c['mean'].shape[0], c['frames'].shape[0]
    if 'rows' in c:
        return compared_pairs(c)
    out = np.zeros((J, F), dtype=bool)
    if 'lens' in c:                                                     # collapsed: every state on its own frames
        for j, (b, T) in enumerate(zip(c['begin'], c['lens'])):
            out[j, b:b + T] = True
        return out
    return ~out


def score_bounds(c, ref, f32_class):
    """(rtol (J,), atol (J, F)) of PCL_F32 ln b: 5e-5 absolute on ordinary states (tests/test_gpu_parity.py F32_LOGLIK_ATOL); for the states
    of f32_class (J,) bool -- off-pipe mixtures, a whole direct-form state, outlier frames -- 5e-6 relative + 5e-5 + the f32 evaluation bound
    (tests/test_gpu_score_ring.py, tests/test_gpu_parity.py assert_f32_class).  The evaluation bound weighs the mixtures with their
    posteriors: under the log-determinant those are the posteriors of the Q1 model with w'."""
    from _oracle_pool import f32_evaluation_bound_rows
    J, F = ref.shape
    rtol, atol = np.zeros(J), np.full((J, F), F32_LOGLIK_ATOL)
    for j in np.flatnonzero(f32_class):
        wp = q1_weights(c['var'], c['w'])
        rtol[j] = 5e-6
        atol[j] += f32_evaluation_bound_rows([(c['mean'][j], c['var'][j], wp[j])], c['frames'])[0]
    return rtol, atol


def allowance(c, ref, f32_class):
    rtol, atol = score_bounds(c, ref, f32_class)
    return atol + rtol[:, None] * np.abs(ref)
