"""Inputs of the segmental-training edge tests (tests/test_gpu_segment_edges.py on the device, tests/test_seg_cases.py on the CPU): owner
arrays, frames, given centres and starting models that put the ten kernels of csrc/gmm_segment.hip at their edges, a restatement of the
launcher's integer rules that the CPU companion holds every case against, and what the float64 twin (tests/_segment_twin.py) yields for
each case.  Everything here is NumPy and the twin; nothing needs a device.

Continuous data is drawn from a fixed first seed and re-drawn (seed + 1, ...) until the case's condition holds; the seed that held is
kept in the case ('seed').  Every builder is cached: a reference is computed once and shared by the tests that read it (read only).

sort case   dict(name, state (F,) int32 with -1 rows, J, F)
lloyd case  dict(name, n, K, D, prec, frames (F, D) float64 or float32, state, J = 2 (state 1: fewer than K frames), c0 (J, K, D), x (the
            trained state's frames as float64, in frame order), assign / sweeps / centres / margin (the twin's), roles)
seed case   dict(name, D, prec, K, seed, frames, state, J, xs (per-state float64 frames), want (positions), margin)
em case     dict(name, M, D, c_cov, logdet, max_iters, frames (float64), state, J, xs, mean0 / var0 / w0 (J, M, D), steps (per trained state:
            the twin's loop bodies), threshold (per precision: the q_threshold of the run), short (rows of the skipped last state or None))
"""
import functools

import numpy as np

import _segment_twin as tw

SEG_T = 256                      # gmm_segment.hip: threads per workgroup, rows per round, frames per Lloyd tile
KC = 32                          # seg_assign_kernel: centres staged per chunk
VAR_FLOOR = 1e-4                 # seg_centre_kernel: floor of the cluster variance
FAR = 1e3                        # where a centre (or a mean) nobody reaches sits


# ------------------------------------------------------------------ the launcher's integer rules, restated
def device_dim(d):
    """pcl_device_dim: the padded feature dimension the kernels have an instance for."""
    for o in (13, 26, 39, 47, 48, 64):
        if d <= o:
            return o
    return -1


def ceil_div(a, b):
    return -(-a // b)


def sort_tile(F, J):
    """pcl_seg_create: rows per tile of the counting sort."""
    per = max(2048, ceil_div(F, 4096), ceil_div(F * J, 1 << 26))
    return ceil_div(per, SEG_T) * SEG_T


def sort_tiles(F, J):
    return ceil_div(F, sort_tile(F, J))


def centre_chunks(K):
    """seg_assign_kernel: (first centre, centres in the chunk)"""
    return [(k0, min(KC, K - k0)) for k0 in range(0, K, KC)]


def seed_chunk(n):
    """seg_seed_kernel: rows per thread, threads that own a row"""
    chunk = ceil_div(n, SEG_T)
    return chunk, ceil_div(n, chunk)


def quarters(cnt):
    """seg_cluster_sum: rows of the four waves"""
    q = ceil_div(cnt, 4)
    lo = [min(cnt, w * q) for w in range(4)]
    return [min(cnt, l + q) - l for l in lo]


def mixture_rounds(M):
    """seg_mstep_q_kernel: mixtures strided over 256 threads"""
    return ceil_div(M, SEG_T)


def mpad(M):
    return ceil_div(M, 4) * 4


def scatter(parts, n_free, rng, free_scale=50.0):
    """per-state frame blocks -> (frames, state) with the rows shuffled (order inside a state kept) and n_free rows nobody owns"""
    d = parts[0].shape[1]
    owner = np.concatenate([np.full(len(p), j, dtype=np.int32) for j, p in enumerate(parts)] + [np.full(n_free, -1, dtype=np.int32)])
    state = owner[rng.permutation(len(owner))]
    frames = np.empty((len(owner), d))
    for j, p in enumerate(parts):
        frames[state == j] = p
    frames[state < 0] = rng.standard_normal((n_free, d)) * free_scale
    return frames, state


# ------------------------------------------------------------------ sort
SORT_F = (2047, 2048, 2049, 4097, 3 * 2048 + 5)
SORT_J = (1, 3, 300)


@functools.lru_cache(maxsize=None)
def sort_cases():
    out = []
    rng = np.random.default_rng(41)
    for F in SORT_F:
        for J in SORT_J:
            state = rng.integers(0, J, F).astype(np.int32)
            state[rng.random(F) < 0.07] = -1
            out.append(dict(name='F%d_J%d' % (F, J), state=state, J=J, F=F))
    F = 3 * 2048 + 5
    state = rng.integers(0, 3, F).astype(np.int32)
    state[rng.random(F) < 0.07] = -1
    mid = slice(2048, 4096)
    state[mid] = np.where(state[mid] == 1, 2, state[mid])
    out.append(dict(name='empty_middle_tile', state=state, J=3, F=F, absent=(1, 1)))
    F = 4097
    state = rng.integers(0, 3, F).astype(np.int32)
    state[rng.random(F) < 0.07] = -1
    state[2048 + 256:2048 + 512] = 2
    out.append(dict(name='one_state_round', state=state, J=3, F=F, full_round=(2048 + 256, 2)))
    return out


# ------------------------------------------------------------------ Lloyd from given centres
LLOYD_SHAPES = ((257, 33, 39), (300, 40, 40), (513, 64, 13), (256, 32, 64), (600, 65, 26), (255, 1, 48), (700, 300, 2))
IDENT_ROWS = 6
MARGIN = {'f64': 1e-9, 'f32': 1e-4}


def lloyd_roles(K):
    """which centre plays which part: dup {centre: its exact copy at a lower index}, far (never reached), ident (identical rows), regular"""
    dup = {32: 31, 33: 0} if K == 40 else {}
    n_far = max(1, K // 16) if K >= 8 else 0
    far = list(range(K - n_far, K))
    ident = K - n_far - 1 if K >= 8 else None
    regular = [k for k in range(K) if k not in dup and k not in far and k != ident]
    return dict(dup=dup, far=far, ident=ident, regular=regular)


def lloyd_with_margin(x, c0, dtype):
    """tw.lloyd, with the margin taken over the DISTINCT centres of each sweep (an exact copy of a centre ties by construction: the
    lower index wins) -> (assign, sweeps, centres, margin, first assignment)"""
    assign, sweeps, centres, _ = tw.lloyd(x, c0, 100, dtype)
    c = np.array(c0, dtype=np.float64)
    xs = x.astype(dtype)
    cur = np.full(len(x), -1, dtype=np.int32)
    margin, first = np.inf, None
    for _ in range(sweeps):
        new = ((xs[:, None, :] - c.astype(dtype)[None]) ** 2).sum(2).astype(np.float64).argmin(1).astype(np.int32)
        cu = np.unique(c.astype(dtype), axis=0)
        if len(cu) > 1:
            srt = np.sort(((xs[:, None, :] - cu[None]) ** 2).sum(2).astype(np.float64), axis=1)
            margin = min(margin, float(((srt[:, 1] - srt[:, 0]) / np.maximum(srt[:, 1], 1e-300)).min()))
        if first is None:
            first = new
        if np.array_equal(new, cur):
            break
        cur = new
        for kk in range(len(c)):
            if (cur == kk).any():
                c[kk] = x[cur == kk].mean(0)
    assert np.array_equal(cur, assign) and np.array_equal(c, centres)
    return assign, sweeps, centres, margin, first


def _lloyd_draw(n, K, D, seed):
    rng = np.random.default_rng(seed)
    roles = lloyd_roles(K)
    reg = roles['regular']
    n_reg = n - (IDENT_ROWS if roles['ident'] is not None else 0)
    tc = rng.standard_normal((len(reg), D))
    x = tc[rng.integers(0, len(reg), n_reg)] * 3 + 0.7 * rng.standard_normal((n_reg, D))
    c0 = np.zeros((K, D))
    c0[reg] = x[rng.choice(n_reg, len(reg), replace=False)]
    ident_rows = np.zeros(0, dtype=np.int64)
    if roles['ident'] is not None:
        p = 20.0 + (np.arange(D) % 3)                              # exact in float32; its multiples up to 6 too
        x = np.concatenate([x, np.tile(p, (IDENT_ROWS, 1))])
        perm = rng.permutation(n)
        x = x[perm]
        ident_rows = np.sort(np.argsort(perm)[n_reg:])
        c0[roles['ident']] = p + 0.25
    for i, k in enumerate(roles['far']):
        c0[k] = FAR + i
    for k, src in roles['dup'].items():
        c0[k] = c0[src]
    return x, c0, roles, ident_rows


def _lloyd_holds(x, c0, roles, ident_rows, prec):
    dtype = np.float64 if prec == 'f64' else np.float32
    xx = x if prec == 'f64' else x.astype(np.float32).astype(np.float64)
    assign, sweeps, centres, margin, first = lloyd_with_margin(xx, c0, dtype)
    ok = sweeps < 100 and (len(c0) == 1 or margin > MARGIN[prec])
    ok = ok and not np.isin(assign, roles['far']).any()
    if roles['ident'] is not None:
        ok = ok and np.array_equal(np.nonzero(assign == roles['ident'])[0], ident_rows)
    for k, src in roles['dup'].items():
        ok = ok and (first == src).any() and not (first == k).any()
    return ok, dict(x=xx, assign=assign, sweeps=sweeps, centres=centres, margin=margin, first=first)


@functools.lru_cache(maxsize=None)
def lloyd_draw(n, K, D, first_seed=100):
    """the first draw that holds the case's condition in BOTH precisions"""
    for seed in range(first_seed, first_seed + 400):
        x, c0, roles, ident_rows = _lloyd_draw(n, K, D, seed)
        res = {}
        for prec in ('f64', 'f32'):
            ok, res[prec] = _lloyd_holds(x, c0, roles, ident_rows, prec)
            if not ok:
                break
        else:
            return seed, x, c0, roles, ident_rows, res
    raise AssertionError('no draw holds the margin condition for %s' % ((n, K, D),))


@functools.lru_cache(maxsize=None)
def lloyd_case(n, K, D, prec):
    seed, x, c0, roles, ident_rows, res = lloyd_draw(n, K, D)
    rng = np.random.default_rng(seed + 7)
    n_nb = min(K - 1, 3)                                           # the neighbour state: fewer frames than clusters, never trained
    frames, state = scatter([x, rng.standard_normal((n_nb, D))], 9, rng)
    if prec == 'f32':
        frames = frames.astype(np.float32)
    c_all = np.stack([c0, rng.standard_normal((K, D))])
    return dict(name='n%d_K%d_D%d_%s' % (n, K, D, prec), n=n, K=K, D=D, prec=prec, seed=seed, frames=frames, state=state, J=2, c0=c_all,
                roles=roles, ident_rows=ident_rows, **res[prec])


# ------------------------------------------------------------------ cluster sizes
CLUSTER_SIZES = (0, 1, 2, 3, 4, 5, 9, 257)


@functools.lru_cache(maxsize=None)
def cluster_size_case(prec):
    """One state, given centres 50 apart and data 0.5 around them: after ONE sweep the model is cluster_model of a known assignment."""
    rng = np.random.default_rng(77)
    K, D = len(CLUSTER_SIZES), 13
    c0 = rng.standard_normal((K, D)) * 10
    label = rng.permutation(np.repeat(np.arange(K), CLUSTER_SIZES)).astype(np.int32)
    x = c0[label] + 0.5 * rng.standard_normal((len(label), D))
    frames = x.astype(np.float32) if prec == 'f32' else x
    xx = frames.astype(np.float64)
    assign, sweeps, centres, margin = tw.lloyd(xx, c0, 1, np.float64 if prec == 'f64' else np.float32)
    return dict(name='sizes_%s' % prec, n=len(label), K=K, D=D, prec=prec, frames=frames, state=np.zeros(len(label), dtype=np.int32), J=1,
                c0=c0[None], label=label, x=xx, assign=assign, sweeps=sweeps, centres=centres, margin=margin)


# ------------------------------------------------------------------ seeding
SEED_K = 6
SEED_N = (255, 256, 257, 511, 513, SEED_K)
SEED_DIMS = (13, 39, 40)
SEED_SEED = 12345


@functools.lru_cache(maxsize=None)
def seed_case(D, prec):
    """States 0-5: n = 255, 256, 257, 511, 513, K rows; 6: all rows equal; 7: three distinct rows; 8: fewer rows than K (skipped).  The
    draws depend on the state index, so a state's data is re-drawn on its own until the twin's margin is above 1e-9."""
    xs, margins, wants, seeds_used = [], [], [], []
    wide = (lambda a: a.astype(np.float32).astype(np.float64)) if prec == 'f32' else (lambda a: a)
    for j, n in enumerate(SEED_N):
        for s in range(300 + 10 * j, 300 + 10 * j + 10):
            x = wide(np.random.default_rng(1000 * D + s).standard_normal((n, D)) * 3)
            want, margin = tw.seeds(x, SEED_K, SEED_SEED, j)
            if margin > 1e-9:
                break
        else:
            raise AssertionError('no draw holds the seeding margin')
        xs.append(x), margins.append(margin), wants.append(want), seeds_used.append(s)
    rng = np.random.default_rng(D)
    xs.append(np.full((9, D), 2.5))                                           # total D^2 = 0
    xs.append(wide(np.repeat(rng.standard_normal((3, D)), 5, axis=0)))        # 3 distinct rows only
    xs.append(wide(rng.standard_normal((4, D))))                              # fewer frames than clusters: skipped
    for j in (6, 7):
        want, margin = tw.seeds(xs[j], SEED_K, SEED_SEED, j)
        margins.append(margin), wants.append(want)
    frames, state = scatter(xs, 11, rng)
    if prec == 'f32':
        frames = frames.astype(np.float32)
    return dict(name='seed_D%d_%s' % (D, prec), D=D, prec=prec, K=SEED_K, seed=SEED_SEED, frames=frames, state=state, J=len(xs), xs=xs,
                want=wants, margin=margins, seeds_used=seeds_used)


# ------------------------------------------------------------------ EM
EM_SHAPES = ((257, 13), (300, 39), (33, 40), (4, 64), (5, 2))
EM_ITERS = (1, 8)
Q_THRESHOLD = 1.28
Q_REL = {'f64': 1e-9, 'f32': 1e-4}              # what the device holds a Q to (bound_of, per M-step under f64)
Q_LADDER = (1.28, 4.0, 16.0, 64.0, 256.0)
# Conditioning of the shape cases under PCL_F32.  A state has one to three frames per mixture, so a variance is the spread of one to three
# numbers: anything from 0 upwards.  The f32 E-step's statistics carry an ABSOLUTE error of about 1e-6 of the state's largest entry (the atol
# tests/test_gpu_acc16_edges.py holds them to; unit-variance data 3 apart: entries of a few units, measured 1e-6 .. 4e-6 on the variance), so
# a variance v comes back within about 4e-6 / v: the 1e-4 contract can be asked only where the floor is 0.04 or more.  With c_covariance
# = 1e-3 the variances just above the floor came back 1.2e-3 .. 3.5e-3 off while PCL_F64 held 5e-12 on the same case: the case, not the
# kernel.  Likewise the frames sit around M separated centres (one start mean in each): on one overlapping cloud eight loop bodies of EM
# magnified a deviation 70-fold under PCL_F64 (2e-13 -> 1.4e-11), which under PCL_F32 (3e-5 per step) leaves the flat 1e-4 bound.
EM_SHAPE_FLOOR = 0.1


def em_start(x, M, rng):
    """means = data rows + noise, variances in [0.5, 2], uniform weights"""
    D = x.shape[1]
    mean0 = x[rng.choice(len(x), M, replace=False)] + 0.1 * rng.standard_normal((M, D))
    return mean0, rng.uniform(0.5, 2.0, (M, D)), np.full(M, 1.0 / M)


def em_steps(x, mean0, var0, w0, c_cov, n_bodies, logdet=False):
    """n_bodies loop bodies of the twin's EM, none refused: list of dict(mean, var, w, s2, big, q).  A run with a threshold is a prefix of
    it (a loop body does not depend on the threshold, only whether there is a next one does): `stop_rule` says which."""
    mean, var, w = (np.array(a, dtype=np.float64) for a in (mean0, var0, w0))
    out = []
    for _ in range(n_bodies):
        gamma = tw.expectation(x, mean, var, w, logdet)
        mean, var, w, s2, big = tw.maximization(x, gamma, c_cov, prev=(mean, var))
        out.append(dict(mean=mean, var=var, w=w, s2=s2, big=big, q=tw.q_closed(big, w, var, s2, logdet)))
    return out


def run_length(steps, threshold, max_iters):
    """loop bodies Clustering.GMM.em runs: up to and with the first whose Q does not grow by more than the threshold"""
    q_old = -np.inf
    for i, st in enumerate(steps[:max_iters]):
        if not st['q'] - q_old > threshold:
            return i + 1
        q_old = st['q']
    return min(max_iters, len(steps))


def clear_thresholds(steps, prec, max_iters, ladder=Q_LADDER):
    """The thresholds of the ladder at which every accept / stop decision of the run stays what it is when each Q moves by twice the bound
    the device is held to (1e-4 |Q| under f32, 1e-9 |Q| per M-step under f64; two Q's in a difference, and a factor two).  The reference's
    1.28 comes first; a large |Q| under f32 needs a larger one."""
    rel = 4 * (Q_REL[prec] * (max_iters if prec == 'f64' else 1))
    out = []
    for thr in ladder:
        n = run_length(steps, thr, max_iters)
        q = np.array([s['q'] for s in steps[:n]])
        if (np.abs(np.diff(q) - thr) > rel * np.abs(q[1:])).all():
            out.append(thr)
    return out


def _em_state(n, M, D, seed, c_cov, n_bodies, spread=1.0, logdet=False, min_share=1e-3, pattern=None, ladder=Q_LADDER, all_floored=False,
              clustered=False):
    """re-drawn until no Gamma is below min_share n / M in any loop body, a threshold of the ladder makes every decision clear and (all_floored)
    every un-floored variance of every loop body is below 0.9 c_cov"""
    for s in range(seed, seed + 200):
        rng = np.random.default_rng(s)
        x = rng.standard_normal((n, D)) * spread
        if clustered:                                             # M centres 3 apart per dimension, every one with a row: rows 0 .. M-1
            x += (rng.standard_normal((M, D)) * 3)[np.concatenate([np.arange(M), rng.integers(0, M, n - M)])]
        x = x.astype(np.float32).astype(np.float64)               # the same values under both precisions
        mean0, var0, w0 = em_start(x[:M] if clustered else x, M, rng)
        if pattern is not None:
            mean0 = pattern(mean0)
        steps = em_steps(x, mean0, var0, w0, c_cov, n_bodies, logdet)
        if pattern is None and min(st['big'].min() for st in steps) < min_share * n / M:
            continue
        if all_floored and max(st['s2'].max() for st in steps) > 0.9 * c_cov:
            continue
        clear = {p: clear_thresholds(steps, p, n_bodies, ladder) for p in ('f64', 'f32')}
        if not all(clear.values()):
            continue
        return dict(x=x, mean0=mean0, var0=var0, w0=w0, steps=steps, seed=s, clear=clear)
    raise AssertionError('no draw holds the EM condition')


def _em_pack(name, states, M, D, c_cov, logdet, max_iters, seed, short=None):
    rng = np.random.default_rng(seed)
    xs = [s['x'] for s in states]
    mean0, var0, w0 = [s['mean0'] for s in states], [s['var0'] for s in states], [s['w0'] for s in states]
    if short is not None:                                          # a state with fewer than M frames: skipped, its model kept
        xs.append(rng.standard_normal((short, D)))
        m, v, w = em_start(rng.standard_normal((M, D)), M, rng)
        mean0.append(m), var0.append(v), w0.append(w)
    frames, state = scatter(xs, 7, rng)
    return dict(name=name, M=M, D=D, c_cov=c_cov, logdet=logdet, max_iters=max_iters, frames=frames, state=state, J=len(xs), xs=xs,
                mean0=np.stack(mean0), var0=np.stack(var0), w0=np.stack(w0), steps=[s['steps'] for s in states], short=short,
                threshold={p: min(t for t in Q_LADDER if all(t in s['clear'][p] for s in states)) for p in ('f64', 'f32')})


@functools.lru_cache(maxsize=None)
def em_shape_case(M, D):
    """two states of M and 2 M + 1 .. 3 M frames; the 8-iteration run (its first loop body is the 1-iteration run)"""
    ns = (M, 3 * M) if M <= 64 else (M, 2 * M + 1)
    states = [_em_state(n, M, D, 500 + 10 * i + M, EM_SHAPE_FLOOR, max(EM_ITERS), clustered=True) for i, n in enumerate(ns)]
    return _em_pack('M%d_D%d' % (M, D), states, M, D, EM_SHAPE_FLOOR, False, max(EM_ITERS), M + D)


def _dead_mixture(mean0):
    mean0 = mean0.copy()
    mean0[2] += FAR
    return mean0


@functools.lru_cache(maxsize=None)
def em_special_case(kind):
    M, D = 4, 13
    if kind == 'gamma0':                    # mixture 2 a thousand away: exp underflows, its responsibilities are exactly 0
        st = [_em_state(11, M, D, 700, 1e-3, 8, pattern=_dead_mixture)]
        return _em_pack('gamma0', st, M, D, 1e-3, False, 8, 1)
    if kind == 'floor':                     # c_covariance = 0.6 above every s2: every variance is the floor
        st = [_em_state(12, M, D, 710, 0.6, 8, spread=0.5, all_floored=True)]
        return _em_pack('floor', st, M, D, 0.6, False, 8, 2)
    if kind == 'logdet':
        st = [_em_state(12, M, D, 720, 1e-3, 8, logdet=True)]
        return _em_pack('logdet', st, M, D, 1e-3, True, 8, 3)
    if kind == 'ragged':                    # two states that stop at different iterations beside one with fewer than M frames
        for s in range(730, 930):
            a = _em_state(40, M, D, s, 1e-3, 16, ladder=(Q_THRESHOLD,))
            b = _em_state(9, M, D, s + 1000, 1e-3, 16, ladder=(Q_THRESHOLD,))
            na, nb = (run_length(st['steps'], Q_THRESHOLD, 16) for st in (a, b))
            if na != nb and min(na, nb) > 1 and max(na, nb) < 16:
                return _em_pack('ragged', [a, b], M, D, 1e-3, False, 16, 4, short=M - 1)
        raise AssertionError('no draw stops at different iterations')
    raise KeyError(kind)


EM_SPECIAL = ('gamma0', 'floor', 'logdet', 'ragged')
