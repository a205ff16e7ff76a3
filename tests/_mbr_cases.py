"""Inputs and shared helpers of the minimum-Bayes-risk tests (tests/test_gpu_mbr.py and tests/test_gpu_mbr_edges.py on the device,
tests/test_mbr_cases.py on the CPU).  The case builders are NumPy and tests/_mbr_twin.py only; the helpers that touch a batch (make_batch,
against_twin, refused) import the package when they are called, so the CPU test can read the cases without a device.

An utterance is the tuple (la, lpi, rows, B): ln a (N, N), ln pi (N,), the row -> state map (N,) int32 with -1 for the entry and -2 for
the exit row, the emissions (N, T).  A case of CASES is a dict: name, kind ('chain' / 'dense' / 'mixed'), register (the batch is meant
for the register lists of hmm_mbr_kernel<2>: no row of any utterance has more than two predecessors or successors), utts, combos (the
(kappa, group, refkind) it runs under), holes (the indices of the utterances drawn with holes > 0).  Everything is seeded by the case's
name, so a case is the same arrays in every process.

What each case is for (csrc/hmm_mbr.hip):
  chain_waves / dense_waves   N in {127, 128, 129, 256, 257}: two waves with a row short, full, three waves with one row, four, five with
                              one row; T in {1, 2, 3, 5}, a T = 1 beside a T = 5
  chain_big / dense_big       N in {1023, 1024} beside N = 3: sixteen waves, the last a row short or full, and a workgroup of sixteen
                              waves of which fifteen hold no row; block_max / block_sum walk 16 partials
  mixed                       the utterances of chain_waves and one dense N = 65: the selection is made per batch, so the same chains
                              run through the general lists
  chain_holes / dense_holes   -inf emissions on emitting rows: alpha = -inf and beta = -inf beside finite neighbours, mbr_step with
                              m = -inf on ordinary rows, P(O) > 0 by a path kept finite
  imp_*                       four possible utterances; the tests make the one in position 1 impossible (a frame nobody emits): the
                              normaliser is -inf at every frame and block_lse returns early in all its waves
  stride                      more than 2048 x 256 elements: mbr_post_kernel's grid-stride loop takes a second trip
  id_chain8 / id_dense9       small shapes for the identities that do not go through the twin
  brute_holes                 N = 4, T = 5 with holes: small enough for every path one by one (CPU only)"""
import functools
import os
import re

import numpy as np

import _mbr_twin as tw

J = 66                       # states of the model the batches are made beside (synth.make_model(22, 2, 4, seed=5): 22 units of 3)
INVALID, STATE = -1, -3
WORST = {}
EDGE_COMBOS = ((0.1, 1, 'partly'), (1.0, 3, 'random'))
SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'poccala_amd', 'csrc', 'hmm_mbr.hip')


# ------------------------------------------------------------------ comparisons
def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def logs(a, pi):
    with np.errstate(divide='ignore'):
        return np.log(a), np.log(pi)


def share(tag, key, got, want, allow, worst=None):
    """The share of its allowance that `got` uses against `want`, asserted <= 1 and kept in `worst` (WORST unless given).

    Where `want` is not finite the two must agree in kind and place: the NaN masks are equal, and the infinities are equal in place and
    sign.  A NaN is not compared by its bytes: -inf - (-inf) need not carry the sign or payload on the device that it carries in NumPy
    (x86 sets the sign bit of the default NaN, the GPU does not).  This is stricter than a comparison of the non-finite entries' bytes
    about where the NaNs sit -- a NaN in place of an infinity fails whatever its bits -- and no longer depends on their bit pattern."""
    worst = WORST if worst is None else worst
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin, inf = np.isfinite(want), np.isinf(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, key, 'NaNs differ')
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), (tag, key, 'infinities differ')
    with np.errstate(invalid='ignore'):
        used = float((np.abs(got - want)[fin] / np.broadcast_to(allow, want.shape)[fin]).max()) if fin.any() else 0.0
    worst[key] = max(worst.get(key, 0.0), used)
    assert used <= 1.0, '%s: %s uses %.3f of its allowance' % (tag, key, used)
    return used


def against_twin(tag, b, per_utt, Bs, refs, kappa, group, twins=None, worst=None, only=None):
    """mbr_get of the batch against the twin, utterance by utterance -> (device results, twins, allowances).  twins: per utterance
    (float64 twin, long-double twin) made earlier, else they are made here; only: the utterances to hold (all unless given)."""
    got = b.mbr_get()
    out_t, out_a = [], []
    for u, (la, lpi, rows) in enumerate(per_utt):
        if only is not None and u not in only:
            out_t.append(None), out_a.append(None)
            continue
        if twins is not None:
            t64, tld = twins[u]
        else:
            t64 = tw.mbr(la, lpi, Bs[u], rows, refs[u], kappa=kappa, group=group)
            tld = tw.mbr(la, lpi, Bs[u], rows, refs[u], kappa=kappa, group=group, dtype=np.longdouble)
        al = tw.allowances(t64, tld, kappa)
        used = [share('%s utt %d' % (tag, u), key, got[key][u], t64[key], al[key], worst) for key in ('logp', 'c_avg', 'lgamma', 'g')]
        N = len(rows)
        assert np.abs(got['g'][u].sum(axis=0)).max() <= N * al['g'].max()          # the gradient of an expectation of a constant total mass
        out_t.append(t64), out_a.append(al)
        print('%s utt %d (N=%d T=%d): c_avg %.6g; shares logp %.3f c_avg %.3f lgamma %.3f g %.3f' % ((tag, u, N, Bs[u].shape[1], got['c_avg'][u]) + tuple(used)))
    return got, out_t, out_a


def refused(code, call):
    """call() raises PoccalaHipError with this code -> the exception"""
    import pytest
    from poccala_amd import PoccalaHipError
    with pytest.raises(PoccalaHipError) as e:
        call()
    assert e.value.code == code, e.value
    return e.value


def make_batch(eng, s):
    """the batch of explicit utterances with its emissions in place -> (batch, per utterance (la, lpi, row_state)).  s: model, frames,
    N, T, begin, utts [(la, lpi, rows, B)]."""
    from poccala_amd.engine import Batch
    eng.load_model(*s['model'])
    eng.load_frames(s['frames'])
    b = Batch(eng, s['N'], s['T'], s['begin'])
    b.set_transitions([u[0] for u in s['utts']], [u[1] for u in s['utts']])
    b.set_states([u[2] for u in s['utts']])
    b.set_emissions([u[3] for u in s['utts']])
    return b, [u[:3] for u in s['utts']]


# ------------------------------------------------------------------ builders
def seed_of(*name):
    return list(('/'.join(str(x) for x in name)).encode())


def emitting_path(a, pi, t, rng):
    """rows of a path of t frames along non-zero transitions that never enters the exit row (the last, which emits nothing): a walk from
    a row pi allows, every step drawn among the successors from which the walk can still go on."""
    n = len(pi)
    ok = np.ones(n, dtype=bool)
    ok[n - 1] = False
    while True:                                                      # rows from which a path of any length stays off the exit row
        nxt = ok & ((a[:, ok] > 0).any(axis=1))
        if np.array_equal(nxt, ok):
            break
        ok = nxt
    start = np.flatnonzero(ok & (pi > 0))
    assert start.size, 'no row to start a path in'
    path = [int(rng.choice(start))]
    for _ in range(t - 1):
        path.append(int(rng.choice(np.flatnonzero(ok & (a[path[-1]] > 0)))))
    return np.array(path)


def silenceable(a):
    """the emitting rows of a dense matrix that have successors, none of them the entry row (whose emission is always ln 1)"""
    return [r for r in range(1, len(a) - 1) if a[r].any() and a[r, 0] == 0]


def emissions(n, t, rng, holes=0.0, a=None, pi=None):
    """B (n, t): uniform(-40, 0), the entry row's ln 1 and the exit row's ln 0 as scoring writes them; with holes > 0 that share of the
    emitting rows' entries is -inf, but for one path kept finite so that P(O) > 0 by construction: for a chain (a is None) the staircase
    through the emitting rows 1, 2, ... (the last emitting row held once reached), for a dense matrix a path walked along its non-zero
    transitions (emitting_path), and one emitting row loses all its successors at one frame (beta = -inf there, which random holes
    give a chain but never a dense row).  holes = 0 draws nothing beyond the uniform matrix."""
    B = rng.uniform(-40.0, 0.0, (n, t))
    if holes > 0.0:
        # a dense row keeps a finite beta as long as one of its many successors emits (the entry row always does), so one emitting row
        # that enters neither the entry row nor the kept path's row of a frame has all its successors silenced at that frame
        silent = lambda keep: [(r, f) for f in range(1, t) for r in silenceable(a) if a[r, keep[f]] == 0]
        if a is None:
            keep = np.minimum(1 + np.arange(t), n - 2)
        else:
            keep = emitting_path(a, pi, t, rng)
            for _ in range(64):                                      # (another walk until such a row and frame exist)
                if silent(keep):
                    break
                keep = emitting_path(a, pi, t, rng)
            assert silent(keep), 'no row whose successors can all be silenced'
        gone = rng.random((n, t)) < holes
        gone[keep, np.arange(t)] = False
        if a is not None:
            at = silent(keep)
            r, f = at[int(rng.integers(len(at)))]
            gone[a[r] > 0, f] = True
        B[gone] = -np.inf
    B[0], B[n - 1] = 0.0, -np.inf
    return B


def utterance(kind, n, t, rng, holes=0.0):
    """(la, lpi, rows, B) of a left-to-right chain (tw.chain_structure) or a dense matrix with holes (tw.dense_structure)"""
    a, pi = tw.chain_structure(n, rng) if kind == 'chain' else tw.dense_structure(n, rng)
    while kind == 'dense' and holes > 0.0 and not silenceable(a):    # (a small matrix may have no such row: another draw)
        a, pi = tw.dense_structure(n, rng)
    rows = np.concatenate([[-1], rng.integers(0, J, n - 2), [-2]]).astype(np.int32)
    B = emissions(n, t, rng, holes) if kind == 'chain' else emissions(n, t, rng, holes, a, pi)
    return logs(a, pi) + (rows, B)


def impossible(utt, t):
    """a copy of the utterance with a frame nobody can emit: P(O) = 0"""
    la, lpi, rows, B = utt
    B = B.copy()
    B[:, t] = -np.inf
    return la, lpi, rows, B


def degrees(utts):
    """(max in-degree, max out-degree) over the utterances, counted as batch_plan.h counts them: entries with a finite ln a"""
    return (max(int(np.isfinite(u[0]).sum(axis=0).max()) for u in utts), max(int(np.isfinite(u[0]).sum(axis=1).max()) for u in utts))


def stride_limit():
    """(blocks, threads) of mbr_post_kernel's launch, read from pcl_launch_mbr_posteriors"""
    src = open(SOURCE).read()
    body = src[src.index('int pcl_launch_mbr_posteriors('):]
    m = re.search(r'std::min<long long>\(\(n \+ (\d+)\) / (\d+), (\d+)\)', body)
    threads = int(re.search(r'mbr_post_kernel, dim3\(blocks\), dim3\((\d+)\)', body).group(1))
    assert int(m.group(1)) + 1 == int(m.group(2)) == threads
    return int(m.group(3)), threads


STRIDE_N, STRIDE_T = 130, 5                                          # three waves with two rows in the last; 650 elements per utterance


def _build(name, kind, shapes, holes=0.0, combos=EDGE_COMBOS, register=None):
    rng = np.random.default_rng(seed_of(name))
    utts = [utterance(kind, n, t, rng, holes) for n, t in shapes]
    return dict(name=name, kind=kind, register=(kind == 'chain') if register is None else register, utts=utts, combos=tuple(combos),
                holes=tuple(range(len(utts))) if holes > 0.0 else ())


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    waves = [(127, 1), (128, 2), (129, 3), (256, 5), (257, 1), (257, 5)]
    c['chain_waves'] = _build('chain_waves', 'chain', waves)
    c['dense_waves'] = _build('dense_waves', 'dense', [(127, 1), (128, 2), (129, 3), (256, 5), (257, 2)])
    c['chain_big'] = _build('chain_big', 'chain', [(1023, 2), (1024, 5), (3, 5)])
    c['dense_big'] = _build('dense_big', 'dense', [(1023, 2), (1024, 3), (3, 5)])
    extra = _build('mixed', 'dense', [(65, 3)])
    c['mixed'] = dict(name='mixed', kind='mixed', register=False, utts=c['chain_waves']['utts'] + extra['utts'], combos=EDGE_COMBOS, holes=())
    c['chain_holes'] = _build('chain_holes', 'chain', [(5, 9), (66, 9), (130, 9)], holes=0.2)
    c['dense_holes'] = _build('dense_holes', 'dense', [(5, 9), (66, 9), (130, 9)], holes=0.2)
    c['imp_chain64'] = _build('imp_chain64', 'chain', [(64, 5), (64, 6), (64, 1), (64, 6)], combos=EDGE_COMBOS[:1])
    c['imp_chain130'] = _build('imp_chain130', 'chain', [(130, 5), (130, 6), (130, 1), (130, 6)], combos=EDGE_COMBOS[1:])
    c['imp_dense130'] = _build('imp_dense130', 'dense', [(130, 5), (130, 6), (130, 1), (130, 6)], combos=EDGE_COMBOS[:1])
    blocks, threads = 2048, 256                                      # (tests/test_mbr_cases.py holds these to the source)
    pair = _build('stride', 'chain', [(STRIDE_N, STRIDE_T), (STRIDE_N, STRIDE_T)])['utts']
    U = blocks * threads // (STRIDE_N * STRIDE_T) + 1                # the smallest batch past the grid: 807 utterances, 524 550 elements
    c['stride'] = dict(name='stride', kind='chain', register=True, utts=[pair[u % 2] for u in range(U)], combos=EDGE_COMBOS[:1], holes=())
    c['id_chain8'] = _build('id_chain8', 'chain', [(8, 6)])
    c['id_dense9'] = _build('id_dense9', 'dense', [(9, 6)])
    c['brute_holes'] = _build('brute_holes', 'dense', [(4, 5)], holes=0.2, combos=EDGE_COMBOS + ((0.3, CD_GROUP, 'random'),))
    return c


class _Cases(dict):
    """CASES['name'], made on first use (the large matrices are not built by an import)"""
    def __missing__(self, key):
        self.update(cases())
        return dict.__getitem__(self, key)


NAMES = ('chain_waves', 'dense_waves', 'chain_big', 'dense_big', 'mixed', 'chain_holes', 'dense_holes', 'imp_chain64', 'imp_chain130',
         'imp_dense130', 'stride', 'id_chain8', 'id_dense9', 'brute_holes')
IMPOSSIBLE = ('imp_chain64', 'imp_chain130', 'imp_dense130')
IMP_AT = 1                                                           # the position of the utterance the tests make impossible
CASES = _Cases()


def imp_frames(case):
    """the offending frames: the first, a middle one, the last"""
    T = case['utts'][IMP_AT][3].shape[1]
    return (0, T // 2, T - 1)


def refs_of(case, refkind, utts=None):
    """per utterance the (T,) int32 reference states: 'random' in [0, J), 'partly' with every other frame -1, 'all' = 'random' (every
    frame carries a reference), 'none' all -1.  Seeded by the case and the kind."""
    rng = np.random.default_rng(seed_of(case['name'], 'ref', 'random' if refkind == 'all' else refkind))
    out = []
    for u in (case['utts'] if utts is None else utts):
        r = rng.integers(0, J, u[3].shape[1]).astype(np.int32)
        if refkind == 'none':
            r[:] = -1
        if refkind == 'partly':
            r[::2] = -1
        out.append(r)
    if case['name'] == 'stride':                                     # copies of a kind share their reference too
        out = [out[u % 2] for u in range(len(out))]
    return out


# ------------------------------------------------------------------ the identities that do not go through the twin
CD_H, CD_KAPPA = 1e-4, 0.3                                           # tests/test_mbr_twin.py test_g_is_the_gradient_of_c_avg: its step, one of its scales
CD_GROUP = 22                                                        # three groups of states: rows and references agree often enough for g to be large


def one_group_margin(al, shape):
    """c_avg against sum_t sum_{emitting j} exp(ln gamma_t(j)): c_avg's allowance plus N T times ln gamma's (gamma <= 1, so an absolute
    error in ln gamma is at most that much in gamma)"""
    return float(al['c_avg'] + shape[0] * shape[1] * np.max(al['lgamma']))


def hold_kappa_moved(s, u, k):
    """s = mbr(kappa = k) on B, u = mbr(kappa = 1) on the float64 product k B.  kappa b is one rounded product either way and 1.0 x is x:
    ln P, c_avg and ln gamma have the same bits; g = (k gamma) x against k (gamma x): within 2 ulp."""
    assert same_bits(s['logp'], u['logp']) and same_bits(s['c_avg'], u['c_avg'])
    assert np.array_equal(np.isnan(s['lgamma']), np.isnan(u['lgamma']))
    keep = ~np.isnan(s['lgamma'])
    assert same_bits(s['lgamma'][keep], u['lgamma'][keep])
    assert (np.abs(s['g'] - k * u['g']) <= 2 * np.spacing(np.abs(s['g']))).all()


def central_tolerance(T, kappa):
    """tests/test_mbr_twin.py test_g_is_the_gradient_of_c_avg: truncation h^2 |c'''| / 6 with |c'''| <= 16 T kappa^3, rounding 8 eps T / h"""
    return CD_H * CD_H * 16.0 * T * kappa ** 3 / 6.0 + 8.0 * np.finfo(np.float64).eps * T / CD_H


def central_entry(t64, B):
    """the emitting (row, frame) with a finite emission where the twin's |g| is largest"""
    g = np.where(np.isfinite(B), np.abs(t64['g']), -1.0)
    g[0], g[-1] = -1.0, -1.0
    return tuple(int(x) for x in np.unravel_index(np.argmax(g), g.shape))


_TWINS = {}


def twin_of(key, utt, ref, kappa, group, ld=True):
    """(float64 twin, long-double twin or None) of one utterance, made once per key and left unchanged"""
    have = _TWINS.get(key)
    if have is None or (ld and have[1] is None):
        la, lpi, rows, B = utt
        t64 = have[0] if have else tw.mbr(la, lpi, B, rows, ref, kappa=kappa, group=group)
        tld = tw.mbr(la, lpi, B, rows, ref, kappa=kappa, group=group, dtype=np.longdouble) if ld else None
        have = _TWINS[key] = (t64, tld)
    return have


def batch_setup(case, utts=None):
    """what make_batch wants for a case (the model and some frames behind the batch; the emissions are set)"""
    from poccala_amd import synth
    utts = case['utts'] if utts is None else utts
    mean, var, w, _ = synth.make_model(J // 3, 2, 4, seed=5)
    N, T = [u[3].shape[0] for u in utts], [u[3].shape[1] for u in utts]
    frames = np.random.default_rng(seed_of(case['name'], 'frames')).standard_normal((sum(T), 4))
    return dict(model=(mean, var, w), frames=frames, N=np.array(N, dtype=np.int32), T=np.array(T, dtype=np.int32),
                begin=np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64), utts=utts)
