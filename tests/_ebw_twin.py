"""NumPy statement of the extended Baum-Welch update of include/poccala_hip.h (pcl_mstep_ebw, csrc/model_ebw.hip).  It IS the definition:
one rounded operation at a time in the order written here, which is the order the kernels run them (they are built without contraction).
The same code runs in np.longdouble as the rounding reference: allowance() is 4x the distance between the two plus 8 ulp of the value.
tests/test_ebw_twin.py holds the rule's own invariants; tests/test_gpu_ebw.py compares the device with it.

The discriminant of the quadratic for Dmin is (c + g v)^2 - 4 v (c g - x^2) = (c - g v)^2 + 4 v x^2 >= 0: in exact arithmetic the roots are
always real.  The "complex roots -> 0" branch can be reached through rounding only (and by a NaN); update() counts how often it was."""
import numpy as np

BIAS = 100.0                                   # mean_acc = sum gamma (o + BIAS): the accumulate pass's constant
DROPS = (None, 'ismooth', 'factor2', 'delta2', 'weights')


def ordered_sum(t):
    """sum over the mixtures of a state, (J, M) -> (J,), in the order pcl_mstep_ebw states: mixture m sits in thread m % 256; a thread adds its
    mixtures in ascending order, starting from 0; the 64 lanes of a wave are summed by a butterfly (partner lane ^ 32, 16, 8, 4, 2, 1); the
    four waves' sums are added in ascending order"""
    J, M = t.shape
    n = -(-M // 256)
    pad = np.zeros((J, n * 256), dtype=t.dtype)
    pad[:, :M] = t
    pad = pad.reshape(J, n, 256)
    a = np.zeros((J, 256), dtype=t.dtype)
    for i in range(n):
        a = a + pad[:, i]
    a = a.reshape(J, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, lane ^ o]
    s = a[:, 0, 0]
    for k in range(1, 4):
        s = s + a[:, k, 0]
    return s


def update(mean, var, w, num, den, E=2.0, tau=100.0, c_covariance=1e-3, weight_iters=100, dtype=np.float64, drop=None):
    """model (J,M,D), (J,M,D), (J,M); num / den: dicts acc (J,M), mean_acc, cov_acc (J,M,D) -> dict(mean, var, w, D (J,M), counts (4,),
    and diagnostics: prevar (the variance before the floor, nan for kept mixtures), keep (J,M), g (J,M), Dmin (J,M), negdisc (elements with
    a negative discriminant), keep_w (J,)).  drop: leave one term of the rule out (tests/test_ebw_twin.py)."""
    assert drop in DROPS
    if not (np.isfinite(E) and E > 0 and np.isfinite(tau) and tau >= 0 and np.isfinite(c_covariance) and c_covariance >= 0 and weight_iters >= 0):
        raise ValueError('ebw update: E = %r, tau = %r, c_covariance = %r, weight_iters = %r' % (E, tau, c_covariance, weight_iters))
    f = lambda a: np.asarray(a, dtype=dtype)
    mu, v, w0 = f(mean), f(var), f(w)
    gn0, gd = f(num['acc']), f(den['acc'])
    E_, tau_, floor_, bias = dtype(E), dtype(tau if drop != 'ismooth' else 0.0), dtype(c_covariance), dtype(BIAS)
    with np.errstate(all='ignore'):
        sh = bias + mu
        xn = f(num['mean_acc']) - sh * gn0[:, :, None]
        xd = f(den['mean_acc']) - sh * gd[:, :, None]
        cn, cd = f(num['cov_acc']), f(den['cov_acc'])
        sm = np.isfinite(gn0) & (gn0 > 0)
        xn = np.where(sm[:, :, None], xn + tau_ * xn / gn0[:, :, None], xn)
        cn = np.where(sm[:, :, None], cn + tau_ * cn / gn0[:, :, None], cn)
        gs = np.where(sm, gn0 + tau_, gn0)
        g, x, c = gs - gd, xn - xd, cn - cd
        gb = g[:, :, None]
        qb, qc = c + gb * v, c * gb - x * x
        disc = qb * qb - dtype(4.0) * v * qc
        r = (np.sqrt(np.where(disc >= 0, disc, 0)) - qb) / (dtype(2.0) * v)
        root = np.where((disc >= 0) & (r > 0), r, dtype(0.0))
        Dmin = root.max(axis=2)
        Dc = np.fmax(E_ * gd, (dtype(2.0) if drop != 'factor2' else dtype(1.0)) * Dmin)
        dn = g + Dc
        keep = ~np.isfinite(gn0) | ~np.isfinite(gd) | ~np.isfinite(x).all(axis=2) | ~np.isfinite(c).all(axis=2) | ((gn0 == 0) & (gd == 0)) \
            | ~(np.isfinite(dn) & (dn > 0))
        delta = x / dn[:, :, None]
        pre = (c + Dc[:, :, None] * v) / dn[:, :, None] - (delta * delta if drop != 'delta2' else dtype(0.0))
        low = ~(pre >= floor_)
        upd = ~keep[:, :, None]
        mean_o = np.where(upd, mu + delta, mu)
        var_o = np.where(upd, np.where(low, floor_, pre), v)
        # weights: Povey's iteration on the unsmoothed numerator
        live = w0 > 0
        k = np.where(live, gd / np.where(live, w0, 1), -np.inf)
        kmax = np.fmax.reduce(k, axis=1)
        kk = np.where(live, kmax[:, None] - k, dtype(0.0))
        keep_w = ((gn0 == 0) & (gd == 0)).all(axis=1)
        cw = w0.copy()
        for _ in range(0 if drop == 'weights' else weight_iters):
            t = np.where(live, gn0 + kk * cw, dtype(0.0))
            s = ordered_sum(t)
            keep_w = keep_w | ~(np.isfinite(s) & (s > 0))
            cw = np.where(keep_w[:, None], cw, t / np.where(keep_w, 1, s)[:, None])
        w_o = np.where(keep_w[:, None] | ~live, w0, cw)
    counts = np.array([(~keep).sum(), keep.sum(), (low & upd).sum(), keep_w.sum()], dtype=np.int64)
    return dict(mean=mean_o, var=var_o, w=w_o, D=np.where(keep, dtype(0.0), Dc), counts=counts, prevar=np.where(upd, pre, np.nan), keep=keep, g=g,
                Dmin=Dmin, negdisc=int((disc < 0).sum()), keep_w=keep_w)


def allowance(t64, tld, key):
    """what the device may differ from the float64 twin by: 4x the twin's own distance to the long-double run plus 8 ulp of the value"""
    a = np.asarray(t64[key], dtype=np.float64)
    return 4.0 * np.abs(a - np.asarray(tld[key])).astype(np.float64) + 8.0 * np.spacing(np.abs(a))


# ------------------------------------------------------------------ the inputs the tests run on
# Every mixture (flattened index k = j M + m) gets a role k % 8 and four numerator and four denominator frames of its own, with posterior
# weights that need not be below 1.  Within a state the means are 12 sigma apart along dimension 0, so a frame's mass goes to the mixture
# it was made for (the others get exp(-72) of it, and the far mixtures exactly 0).
ROLES = ('plain', 'g<0', 'Dmin>0', 'floored', 'empty', 'zero-weight', 'den-heavy', 'plain')
FAR = 1.0e6                                    # an 'empty' mixture's mean along dimension 0, beyond every other mean (12 sqrt(2) x 1100): exp(-(1e6)^2 / 4) is exactly 0
PER = 4                                        # frames per mixture and set


def roles(J, M):
    r = np.arange(J * M).reshape(J, M) % 8
    if M == 1:
        r[r == 5] = 0                          # a state of one mixture cannot have weight 0
    return r


def make_case(J, M, D, seed=0):
    """-> (mean, var, w), frames (F, D), gamma_num (F, J), gamma_den (F, J): state posteriors (not normalised) for two accumulate passes"""
    rng = np.random.default_rng(100003 * J + 1009 * M + D + seed)
    role = roles(J, M)
    mean = rng.standard_normal((J, M, D))
    var = rng.uniform(0.5, 2.0, (J, M, D))
    mean[:, :, 0] += 12.0 * np.sqrt(2.0) * np.arange(M)[None, :]
    w = rng.uniform(0.2, 1.0, (J, M))
    w[role == 5] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    frames, gnum, gden = [], [], []

    def add(j, pts, wn, wd):
        for p, a, b in zip(pts, wn, wd):
            frames.append(p)
            rn, rd = np.zeros(J), np.zeros(J)
            rn[j], rd[j] = a, b
            gnum.append(rn)
            gden.append(rd)

    z, one = np.zeros(PER), np.ones(PER)
    for j in range(J):
        for m in range(M):
            r, mu, sd = role[j, m], mean[j, m], np.sqrt(var[j, m])
            if r in (4, 5):
                continue
            noise = rng.standard_normal((2 * PER, D))
            if r == 0 or r == 7:               # numerator a little to one side and tighter, denominator to the other side and wider
                add(j, mu + 0.3 * sd + 0.9 * sd * noise[:PER], rng.uniform(20, 40, PER), z)
                add(j, mu - 0.2 * sd + 1.1 * sd * noise[PER:], z, rng.uniform(5, 15, PER))
            elif r == 1:                       # the denominator outweighs numerator + tau
                add(j, mu + 0.2 * sd + sd * noise[:PER], rng.uniform(5, 10, PER), z)
                add(j, mu - 0.1 * sd + sd * noise[PER:], z, rng.uniform(60, 80, PER))
            elif r == 2:                       # denominator mass 4 sigma off the mean and tight: x^2 > c g, a positive root
                add(j, mu + 0.3 * sd + 0.9 * sd * noise[:PER], rng.uniform(20, 40, PER), z)
                add(j, mu + 4.0 * sd + 0.1 * sd * noise[PER:], z, rng.uniform(10, 20, PER))
            elif r == 3:                       # the numerator at one point, almost no denominator: the new variance falls under the floor
                add(j, np.tile(mu + 0.1 * sd, (PER, 1)), 50.0 * one, z)
                add(j, mu + sd * noise[PER:], z, 0.002 * one)
            elif r == 6:                       # g < 0 without smoothing, g > 0 with tau = 100
                add(j, mu + 0.3 * sd + 0.9 * sd * noise[:PER], rng.uniform(10, 15, PER), z)
                add(j, mu - 0.2 * sd + 1.1 * sd * noise[PER:], z, rng.uniform(20, 25, PER))
    mean[:, :, 0] = np.where(role == 4, FAR + mean[:, :, 0], mean[:, :, 0])
    return (mean, var, w), np.array(frames), np.array(gnum), np.array(gden)


def numpy_stats(model, frames, gamma):
    """the accumulate pass in NumPy: gamma_t(j, m) = gamma_t(j) x the mixture's share of b_j(o_t) (the reference's density: -1/2 sum(var) in
    the constant) -> dict(acc, alpha_acc, mean_acc, cov_acc), linear sums, cov_acc about the model's means"""
    mean, var, w = model
    J, M, D = mean.shape
    acc, macc, cacc = np.zeros((J, M)), np.zeros((J, M, D)), np.zeros((J, M, D))
    for j in range(J):
        use = np.flatnonzero(gamma[:, j] > 0)
        if not len(use):
            continue
        x = frames[use]
        with np.errstate(divide='ignore'):
            lw = np.log(w[j])
        diff = x[:, None, :] - mean[j][None]
        lp = lw[None] - 0.5 * var[j].sum(axis=1)[None] - (diff ** 2 / (2 * var[j][None])).sum(axis=2)
        lp -= lp.max(axis=1, keepdims=True)
        p = np.exp(lp)
        g = gamma[use, j:j + 1] * p / p.sum(axis=1, keepdims=True)
        acc[j] = g.sum(axis=0)
        macc[j] = g.T @ (x + BIAS)
        cacc[j] = np.einsum('tm,tmd->md', g, diff ** 2)
    return dict(acc=acc, alpha_acc=gamma.sum(axis=0), mean_acc=macc, cov_acc=cacc)


# the shapes of tests/test_gpu_ebw.py: D in {1, 13, 39, 40, 48, 64} (40 and 48 sit below / at a device stride), M in {1, 3, 32, 33, 100}
# (one, below and across the 4-padding, a 64-mixture chunk's edge, two chunks), J in {1, 5, 70}; M = 300 and 1100 are the weight kernel's
# 4- and 16-slot instances (M > 256, M > 1024)
SHAPES = [(5, 3, 13), (1, 32, 39), (5, 33, 40), (70, 1, 1), (1, 100, 48), (5, 3, 64), (1, 300, 13), (1, 1100, 1)]
GRID = [(tau, E, it) for tau in (0.0, 100.0) for E in (1.0, 2.0) for it in (0, 1, 100)]


# ------------------------------------------------------------------ end to end: MMI iterations through the oracle and the twin
E2E = dict(units=6, M=2, D=4, U=8, T=40, L=3, seed=11, E=2.0, tau=100.0, iters=3)


def e2e_setup():
    """-> starting model (mean, var, w), unit transitions, frames (U T, D) float64, labels, T (U,), frame_begin (U,): frames drawn along the
    labels from a model, training started from a blurred copy of it"""
    from poccala_amd import synth
    c = E2E
    mean, var, w, trans = synth.make_model(c['units'], c['M'], c['D'], seed=c['seed'])
    labels = synth.make_labels(c['U'], c['L'], c['units'], seed=c['seed'] + 1)
    frames = synth.make_peaked_frames(labels, c['T'], mean, var, seed=c['seed'] + 2).astype(np.float64)
    rng = np.random.default_rng(c['seed'] + 3)
    start = (mean + 0.4 * rng.standard_normal(mean.shape), var * rng.uniform(1.0, 1.6, var.shape), w.copy())
    lens = np.full(c['U'], c['T'], dtype=np.int32)
    return start, trans, frames, labels, lens, (np.arange(c['U']) * c['T']).astype(np.int64)


def _estep(po, model, x, a, pi, rows, out):
    """one utterance over the graph (a, pi) whose emitting rows 1 .. N-2 are the states `rows`: ln P(O), statistics added to `out`"""
    mean, var, w = model
    b = np.vstack([np.zeros(len(x))] + [po.gmm_point(x, mean[j], var[j], w[j]) for j in rows] + [np.full(len(x), -np.inf)])
    alpha, beta = po.forward(a, pi, b), po.backward(a, b)
    with np.errstate(all='ignore'):
        lg = alpha + beta
        lg = lg - po.lse(lg, axis=0)[None, :]
    for r, j in enumerate(rows):
        g = np.exp(lg[1 + r])
        comp = po.gmm_component_loglik(x, mean[j], var[j], w[j])
        gm = g[:, None] * np.exp(comp - po.lse(comp, axis=1)[:, None])
        out['acc'][j] += gm.sum(axis=0)
        out['alpha_acc'][j] += g.sum()
        out['mean_acc'][j] += gm.T @ (x + BIAS)
        out['cov_acc'][j] += np.einsum('tm,tmd->md', gm, (x[:, None, :] - mean[j][None]) ** 2)
    return po.lse(alpha[:, -1])


def e2e_reference(E=None, iters=None):
    """the MMI loop on the CPU -> (objective per iteration, one more after the last update; final model)"""
    from oracle import poccala_oracle as po
    from poccala_amd.engine import embedded_structure, loop_structure
    model, trans, frames, labels, lens, begin = e2e_setup()
    c = E2E
    J, e = model[0].shape[0], 3
    a_den, pi_den = loop_structure(trans)
    trace = []
    for it in range((c['iters'] if iters is None else iters) + 1):
        zero = lambda: dict(acc=np.zeros((J, c['M'])), alpha_acc=np.zeros(J), mean_acc=np.zeros((J, c['M'], c['D'])), cov_acc=np.zeros((J, c['M'], c['D'])))
        num, den, obj = zero(), zero(), 0.0
        for u, lab in enumerate(labels):
            x = frames[begin[u]:begin[u] + lens[u]]
            a, pi = embedded_structure(len(lab), [trans[i] for i in lab])
            rows = (np.asarray(lab)[:, None] * e + np.arange(e)[None, :]).reshape(-1)
            obj += _estep(po, model, x, a, pi, rows, num) - _estep(po, model, x, a_den, pi_den, np.arange(J), den)
        trace.append(obj)
        if it < (c['iters'] if iters is None else iters):
            t = update(*model, num, den, E=c['E'] if E is None else E, tau=c['tau'])
            model = (t['mean'], t['var'], t['w'])
    return np.array(trace), model
