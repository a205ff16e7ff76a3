"""Inputs of the f16 accumulate edge tests (tests/test_gpu_acc16_edges.py on the device, tests/test_acc16_cases.py on the CPU): models,
frames and per-state ln gamma matrices that put csrc/gmm_accumulate_f16.hip at the edges of its tile pipeline, a restatement of the
launcher's and the producer's integer arithmetic that the CPU companion holds every case against, and the float64 reference
(oracle.poccala_oracle.gmm_update_acc).  Everything here is NumPy and the oracle; nothing needs a device.

A case is a dict: name, mean / var / w (J,M,D), frames (F,D) float64, lgamma (J+2,F) with the virtual rows (and every pair that is not a
survivor) at -inf, counts (J,) the surviving frames per state, prune (None or the log2 threshold of Engine.accumulate_prune), masked
(frames leave the f16 range), split (state -> off-pipe mixtures), outliers (state -> survivor positions the producer must take out)."""
import functools
import math

import numpy as np

from oracle import poccala_oracle as po

LOG2E = 1.4426950408889634074
LN2 = 0.693147180559945309417232121458
NSLOT, AHEAD, AW = 6, 5, 4                   # gmm_accumulate_f16.hip: ring slots, tiles in flight, waves per consumer workgroup
FMAXH = 6.0e4                                # what an f16 piece may hold
COND_MAX = 96.0                              # pcl_internal.h: a mixture whose centred expansion is beyond it leaves the matrix pipe
LG_LO = math.log(1e-3)
LADDER = [0, 1, 31, 32, 33, 64, 65, 96, 127, 128, 160, 161, 192, 193, 224, 0, 257, 416, 0]
LADDER_SPLIT_STATE, LADDER_SPLIT_MIX = 9, (2, 17, 32)


# ------------------------------------------------------------------ the launcher's and the producer's arithmetic, restated
def padded_dim(d):
    """The matrix-pipe dimension a host dimension is padded to (pcl_internal.h: PCL_MFMA_DIMS)."""
    return min(x for x in (13, 26, 39, 47) if x >= d)


def image_geometry(dpad):
    """Img<D>: k-steps, 1-KiB blocks per tile image, blocks the first NB % AW waves issue beyond the others, and the row / column tile of
    S^T that holds S0."""
    ks = (dpad + 7) // 8
    nb = 2 * ks + 1
    return dict(KS=ks, NB=nb, extra=nb % AW, s0_row=((ks - 1) & 1) * 16 + (dpad & 7), s0_tile=(ks - 1) >> 1)


def tiles_of(counts):
    return [(int(n) + 31) // 32 for n in counts]


def state_groups(counts, dpad, image_mb=2048, first_div=12):
    """size_groups of csrc/gmm_accumulate.hip on a scratch that has not grown yet: [(first state, states, tiles)].  The first group is
    small (the largest state, or a twelfth of the tiles); the tile numbering starts again at 0 in every group."""
    t = tiles_of(counts)
    worst, biggest = sum(t), max(t)
    by_budget = max((image_mb << 20) // (image_geometry(dpad)['NB'] * 1024), 1)
    cap = max(biggest, min(worst, by_budget))
    cap = max(cap, min(cap + cap // 4, max(by_budget, biggest)))
    out, first = [], 0
    while first < len(t):
        cap_g = max(biggest, min(cap, worst // first_div)) if first == 0 and first_div > 1 else cap
        last, s = first, 0
        while last < len(t) and s + t[last] <= cap_g:
            s += t[last]
            last += 1
        out.append((first, last - first, s))
        first = last
    return out


def tile_offsets(counts, dpad, image_mb=2048):
    """tile_off of every state inside its group (acc16_tiles_kernel): the ring slot of a state's first tile is tile_off % NSLOT."""
    t = tiles_of(counts)
    off = np.zeros(len(t), dtype=np.int64)
    for first, n, _ in state_groups(counts, dpad, image_mb):
        off[first:first + n] = np.concatenate([[0], np.cumsum(t[first:first + n])[:-1]])
    return off


def derive_replica(mean, var):
    """state_prepass_kernel of csrc/model_derive.hip for ONE state in float64: the expansion centre, which mixtures leave the pipe, and the
    power-of-two feature scales fscale[h][d] (h = 0: x'^2, h = 1: x').  Used to SELECT inputs; it judges nothing."""
    c = mean.mean(axis=0).astype(np.float32).astype(np.float64)
    dm, hr = mean - c, 0.5 / var
    off = (LOG2E * (dm * dm * hr).sum(axis=1)).astype(np.float32) > COND_MAX
    t0, t1 = (LOG2E * hr)[~off], np.abs(2.0 * LOG2E * dm * hr)[~off]
    fs = np.ones((2, mean.shape[1]))
    for d in range(mean.shape[1]):
        ea, eb = math.frexp(t0[:, d].max())[1], math.frexp(t0[:, d].min())[1]
        shift = min(max((ea - eb) // 2 - 1, 0), 7) if eb <= ea else 0
        for h, mx in ((0, t0[:, d].max()), (1, t1[:, d].max())):
            ex = math.frexp(mx)[1] if mx > 0.0 else 1
            fs[h, d] = math.ldexp(1.0, min(max(ex - shift - 1, -60), 60))
    return c, off, fs


def scaled_operands(x, c, fs):
    """|x'^2 fscale| and |x' fscale| of frames x (n,D), x' the centred frame in f32 as the producer forms it."""
    xc = (x.astype(np.float32) - c.astype(np.float32)).astype(np.float64)
    return np.abs(xc * xc * fs[0]), np.abs(xc * fs[1])


def leaves_f16(x, c, fs):
    """The producer's predicate per frame: a scaled operand beyond FMAXH."""
    a, b = scaled_operands(x, c, fs)
    return (a > FMAXH).any(axis=1) | (b > FMAXH).any(axis=1)


# ------------------------------------------------------------------ building blocks
def model(J, M, D, seed):
    from poccala_amd import synth
    mean, var, w, _ = synth.make_model((J + 2) // 3, M, D, seed=seed)
    return mean[:J].copy(), var[:J].copy(), w[:J].copy()


def draw_frames(rng, mean, var, F, states=None):
    """F frames, each from one mixture of one state of the model."""
    J, M, D = mean.shape
    st = rng.integers(0, J, F) if states is None else np.asarray(states)
    mix = rng.integers(0, M, F)
    return mean[st, mix] + np.sqrt(var[st, mix]) * rng.standard_normal((F, D))


def scatter(rng, F, counts):
    """lgamma (J+2,F): per state a scattered subset of the frames (every frame when the count is F), ln gamma uniform in [ln 1e-3, 0]."""
    lg = np.full((len(counts) + 2, F), -np.inf)
    for j, n in enumerate(counts):
        idx = np.sort(rng.choice(F, size=int(n), replace=False))
        lg[1 + j, idx] = rng.uniform(LG_LO, 0.0, size=int(n))
    return lg


def case(name, mean, var, w, frames, lgamma, counts, **kw):
    c = dict(name=name, mean=mean, var=var, w=w, frames=np.ascontiguousarray(frames, dtype=np.float64), lgamma=lgamma,
             counts=np.asarray(counts, dtype=np.int64), prune=None, masked=False, split={}, outliers={})
    c.update(kw)
    return c


def survivors(c, j):
    """Frame indices of state j that the active-frame list keeps, in list order."""
    thr = max(-150.0, c['prune'] if c['prune'] is not None else -1e300) * LN2
    return np.flatnonzero(c['lgamma'][1 + j] >= thr)


# ------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def ladder():
    """D = 39, M = 33 (two live waves, two idle), F = 416: tile counts 1..7, 9 and 13, empty states in front, in the middle and at the end,
    and one split state (three mixtures beyond the conditioning limit, at rows that shift every on-pipe mixture behind them)."""
    rng = np.random.default_rng(1601)
    mean, var, w = model(len(LADDER), 33, 39, 1601)
    frames = draw_frames(rng, mean, var, 416)
    j = LADDER_SPLIT_STATE
    for m in LADDER_SPLIT_MIX:                                   # tight and off centre: LOG2E kq = LOG2E 39 (1.5)^2 / (2 0.25) ~ 250 > 96
        mean[j, m] = mean[j].mean(axis=0) + 1.5 * rng.choice([-1.0, 1.0], size=39)
        var[j, m] = 0.25
    return case('ladder', mean, var, w, frames, scatter(rng, 416, LADDER), LADDER, split={j: LADDER_SPLIT_MIX})


DIMS_COUNTS = [0, 1, 31, 32, 33, 64, 160, 161, 192, 193, 224, 0]
DIMS = [13, 26, 47, 12, 40]


@functools.lru_cache(maxsize=None)
def dims(D):
    """The ladder cut to 1, 2, 5, 6 and 7 tiles at the other kernel instances (KS = 2, 4, 6; S0 on rows 21, 18, 23) and at host dimensions
    the library pads (12 -> 13, 40 -> 47)."""
    rng = np.random.default_rng(1700 + D)
    mean, var, w = model(len(DIMS_COUNTS), 33, D, 1700 + D)
    return case('dims D=%d' % D, mean, var, w, draw_frames(rng, mean, var, 256), scatter(rng, 256, DIMS_COUNTS), DIMS_COUNTS)


MIX_COUNTS = [33, 1, 224, 64, 0, 31, 193, 32, 40]
MIXTURES = [(1, 3), (31, 3), (32, 3), (33, 3), (128, 3), (129, 3), (160, 3), (129, 1), (129, 7), (129, 8), (129, 9)]


@functools.lru_cache(maxsize=None)
def mixtures(M, J):
    """D = 13, states of 1, 2 and 7 tiles: m-tiles that end mid-tile, one and two slices (129: the second slice has one live wave), and at
    M = 129 the state counts around 8 for the block -> (state, slice) map."""
    rng = np.random.default_rng(1800 + 16 * M + J)
    mean, var, w = model(J, M, 13, 1800 + M)
    counts = [33, 224, 31] if J == 3 else MIX_COUNTS[:J]
    return case('mixtures M=%d J=%d' % (M, J), mean, var, w, draw_frames(rng, mean, var, 256), scatter(rng, 256, counts), counts)


@functools.lru_cache(maxsize=None)
def scale():
    """D = 13, M = 33, three states of 8 tiles with their survivors in frame order:
    (a) the frames of tile t sit at mixture t's mean (sd 0.05): every mixture's scale first rises in another tile;
    (b) ln gamma = -100 for three tiles, then 0: every scale rises by 144 octaves at the fourth tile;
    (c) ln gamma = 0 for one tile, then -25: nothing rises after the first tile, the later posteriors sit 36 octaves down."""
    rng = np.random.default_rng(1900)
    mean, var, w = model(3, 33, 13, 1900)
    frames = draw_frames(rng, mean, var, 768, states=np.repeat([0, 1, 2], 256))
    for t in range(8):
        frames[32 * t:32 * t + 32] = mean[0, t] + 0.05 * rng.standard_normal((32, 13))
    lg = np.full((5, 768), -np.inf)
    lg[1, :256] = rng.uniform(LG_LO, 0.0, size=256)
    lg[2, 256:352], lg[2, 352:512] = -100.0, 0.0
    lg[3, 512:544], lg[3, 544:768] = 0.0, -25.0
    return case('scale', mean, var, w, frames, lg, [256, 256, 256])


@functools.lru_cache(maxsize=None)
def scale_prune():
    """(d) Engine.accumulate_prune(-20): frames at thr (1 -+ 1e-12), thr = -20 ln 2, kept and dropped in turn; 33 are kept, the last one
    alone in tile 2.  A second state keeps a plain scattered subset above the threshold."""
    rng = np.random.default_rng(1950)
    mean, var, w = model(3, 33, 13, 1950)
    frames = draw_frames(rng, mean, var, 160)
    thr = -20.0 * LN2
    lg = np.full((5, 160), -np.inf)
    lg[1, 0:66:2], lg[1, 1:66:2] = thr * (1.0 - 1e-12), thr * (1.0 + 1e-12)
    idx = np.sort(rng.choice(160, size=65, replace=False))
    lg[2, idx] = rng.uniform(LG_LO, 0.0, size=65)
    return case('scale prune', mean, var, w, frames, lg, [33, 65, 0], prune=-20.0)


@functools.lru_cache(maxsize=None)
def groups():
    """D = 47, M = 33, 20 states of 10 tiles (every state keeps all 320 frames): under a 1 MB image budget the states fall into four groups
    that alternate between the two image buffers."""
    rng = np.random.default_rng(2000)
    mean, var, w = model(20, 33, 47, 2000)
    return case('groups', mean, var, w, draw_frames(rng, mean, var, 320), scatter(rng, 320, [320] * 20), [320] * 20)


# masked: (survivors, survivor positions that are outliers)
MASKED_LAYOUT = [
    (128, (32, 35, 36, 63, 64 + 4, 96 + 31)),     # tile positions 0, 3, 4, 31 (tile 1), 4 (tile 2), 31 (the last frame of the state)
    (33, (32,)),                                  # the only frame of the last tile
    (96, tuple(range(32, 64))),                   # a whole middle tile
    (96, tuple(range(0, 32))),                    # the whole first tile
    (64, tuple(range(0, 64))),                    # every tile of the state
    (33, ()),                                     # nothing masked beside them
]
MASKED_TIGHT, MASKED_M, MASKED_ODIMS = 2, 6, 4


def _masked(seed):
    rng = np.random.default_rng(seed)
    J, M, D = len(MASKED_LAYOUT), MASKED_M, 13
    mean, var, w = model(J, M, D, seed)
    var[:, MASKED_TIGHT:] = rng.uniform(0.8, 1.3, size=(J, M - MASKED_TIGHT, D))
    mean[:, MASKED_TIGHT:] = mean[:, MASKED_TIGHT:].mean(axis=1, keepdims=True) + 0.3 * rng.standard_normal((J, M - MASKED_TIGHT, D))
    mean[:, MASKED_TIGHT:, :MASKED_ODIMS] = mean[:, MASKED_TIGHT:MASKED_TIGHT + 1, :MASKED_ODIMS]     # the wide mixtures agree in the outlier
    var[:, MASKED_TIGHT:, :MASKED_ODIMS] = var[:, MASKED_TIGHT:MASKED_TIGHT + 1, :MASKED_ODIMS]       # dimensions: posteriors stay spread
    var[:, :MASKED_TIGHT] = rng.uniform(4e-4, 6.5e-4, size=(J, MASKED_TIGHT, D))
    mean[:, :MASKED_TIGHT] = mean[:, MASKED_TIGHT:].mean(axis=1, keepdims=True) + 0.03 * rng.standard_normal((J, MASKED_TIGHT, D))
    counts = [n for n, _ in MASKED_LAYOUT]
    F = sum(counts)
    perm = rng.permutation(F)
    frames, lg, outl, at = np.zeros((F, D)), np.full((J + 2, F), -np.inf), {}, 0
    for j, (n, out) in enumerate(MASKED_LAYOUT):
        idx = np.sort(perm[at:at + n])
        at += n
        c, off, fs = derive_replica(mean[j], var[j])
        assert not off.any()
        mix = rng.integers(0, M, n)
        x = mean[j, mix] + np.sqrt(var[j, mix]) * rng.standard_normal((n, D))
        lgj = rng.uniform(LG_LO, math.log(0.02), size=n)
        wide_c = mean[j, MASKED_TIGHT:].mean(axis=0)
        for p in out:                                            # an outlier: the wide mixtures' centre, one dimension 2.1 .. 2.6 x beyond the f16 limit
            d = int(rng.integers(0, MASKED_ODIMS))
            x[p] = wide_c + 0.3 * rng.standard_normal(D)
            x[p, d] = c[d] + rng.choice([-1.0, 1.0]) * math.sqrt(rng.uniform(2.1, 2.6) * FMAXH / fs[0, d])
            lgj[p] = rng.uniform(math.log(0.5), 0.0)
        frames[idx], lg[1 + j, idx], outl[j] = x, lgj, tuple(out)
    return case('masked', mean, var, w, frames, lg, counts, masked=True, outliers=outl)


@functools.lru_cache(maxsize=None)
def masked():
    """D = 13, per state two tight mixtures (variance ~ 5e-4) at the centre of four wide ones (variance ~ 1): the tight ones set the state's
    feature scale, so a frame some 40 sigma of the WIDE mixtures out in one dimension leaves the f16 range (scaled x'^2 > 6e4) while the
    wide mixtures' posteriors stay f32-evaluable.  The producer must take exactly these frames out of the image, and the direct-form
    kernel must add them once.  The first seed whose draw meets every claim of tests/test_acc16_cases.py is the case."""
    for seed in range(2100, 2140):
        c = _masked(seed)
        if masked_claims(c) is None:
            return c
    raise AssertionError('no seed gives the masked case')


def masked_claims(c):
    """None when the masked case is what it says, else the first claim that fails."""
    from _oracle_pool import f32_evaluation_bound_rows
    for j, (n, out) in enumerate(MASKED_LAYOUT):
        idx = survivors(c, j)
        cen, _, fs = derive_replica(c['mean'][j], c['var'][j])
        a, b = scaled_operands(c['frames'][idx], cen, fs)
        big = np.maximum(a.max(axis=1), b.max(axis=1))
        is_out = np.zeros(n, dtype=bool)
        is_out[list(out)] = True
        if not (big[is_out] >= 2.0 * FMAXH).all() or not (big[~is_out] < 0.5 * FMAXH).all():
            return 'state %d: the outliers are not 2x beyond the limit and everything else under half of it' % j
        if not np.array_equal(leaves_f16(c['frames'][idx], cen, fs), is_out):
            return 'state %d: predicate' % j
        if out:
            ref = reference(c)
            x, lgj = c['frames'][idx], c['lgamma'][1 + j, idx]
            part = np.exp(po.gmm_component_loglik(x[is_out], c['mean'][j], c['var'][j], c['w'][j]) + (lgj[is_out] - po.gmm_point(x[is_out], c['mean'][j], c['var'][j], c['w'][j]))[:, None]).sum(axis=0)
            if not (part[MASKED_TIGHT:] >= 0.1 * ref['acc'][j][MASKED_TIGHT:]).all():
                return 'state %d: the outliers carry less than a tenth of a wide mixture' % j
        if f32_evaluation_bound_rows([(c['mean'][j], c['var'][j], c['w'][j])], c['frames'][idx]).max() > 5e-4:
            return 'state %d: f32 bound' % j
    return None


def plain_cases():
    """(id, builder) of every case without masked frames."""
    out = [('ladder', ladder)]
    out += [('dims-%d' % d, functools.partial(dims, d)) for d in DIMS]
    out += [('mixtures-M%d-J%d' % mj, functools.partial(mixtures, *mj)) for mj in MIXTURES]
    out += [('scale', scale), ('scale-prune', scale_prune), ('groups', groups)]
    return out


def all_cases():
    return plain_cases() + [('masked', masked)]


# ------------------------------------------------------------------ the reference
_REF = {}


def emissions(c):
    """ln b_j(o_t) of every state and frame in float64 with the virtual rows of an all-state batch: (J+2,F)."""
    J, F = c['mean'].shape[0], c['frames'].shape[0]
    B = np.full((J + 2, F), -np.inf)
    B[0] = 0.0
    for j in range(J):
        B[1 + j] = po.gmm_point(c['frames'], c['mean'][j], c['var'][j], c['w'][j])
    return B


def reference(c):
    """Clustering.GMM.update_acc of every state over its survivors through the oracle, linear domain; computed once per case."""
    if c['name'] in _REF:
        return _REF[c['name']]
    J, M, D = c['mean'].shape
    out = dict(acc=np.zeros((J, M)), alpha_acc=np.zeros(J), mean_acc=np.zeros((J, M, D)), cov_acc=np.zeros((J, M, D)))
    for j in range(J):
        idx = survivors(c, j)
        if not len(idx):
            continue
        x, lgj = c['frames'][idx], c['lgamma'][1 + j, idx]
        a = dict(acc=np.full(M, -np.inf), alpha_acc=-np.inf, mean_acc=np.full((M, D), -np.inf), cov_acc=np.full((M, D), -np.inf))
        po.gmm_update_acc(a, lgj, po.gmm_point(x, c['mean'][j], c['var'][j], c['w'][j]), x, c['mean'][j], c['var'][j], c['w'][j])
        with np.errstate(all='ignore'):
            for k in out:
                out[k][j] = np.exp(a[k])
    for v in out.values():
        v.setflags(write=False)
    _REF[c['name']] = out
    return out
