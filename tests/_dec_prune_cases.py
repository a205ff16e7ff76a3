"""Inputs of the decoder pruning / transfer harness tests (tests/test_gpu_dec_prune.py on the device, tests/test_dec_prune_cases.py on
the CPU): the named cases, a NumPy restatement of the radix select's rounds (the PATH twin: which rounds, which bin counts, which
return) and the reference every case is held to -- the project's own oracle (oracle.decoder_oracle.prune) plus a sort.  Everything
here is NumPy; nothing needs a device.

What the inputs never hold: NaN, +inf, and both zeros in one case.  The kernels cannot produce them (a score is lpi + 0.0 and sums of
finite or -inf terms), and the select orders bit patterns, not values: NaN has no place in the order, +inf would be the one key above
every score, and +0.0 / -0.0 are two keys but one score to `set()` in the oracle.  tests/test_dec_prune_cases.py asserts this of
every case.

A case: dict(name, family, n, score[n] float64, part[n] int32 (0 = the token finished this frame: its key is NOKEY), beam,
min_distinct, want = what the family promises, asserted from the twin alone by the CPU test)."""
import os
import re
import zlib

import numpy as np

from oracle import decoder_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'poccala_amd', 'csrc')
U64 = np.uint64
NOKEY = U64(0xFFFFFFFFFFFFFFFF)
SIGN = U64(1 << 63)
GOLDEN = U64(0x9E3779B97F4A7C15)
HEAD = ('n_old', 'kmin', 'kmax', 'bins', 'm', 'ran_distinct', 'prune', 'sel', 'rank', 'occ_left', 'hist_left', 's_int2')


# ------------------------------------------------------------------ the shipping instantiations, read from the kernels' own constants
def _int(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def geometry():
    g = open(os.path.join(CSRC, 'hmm_decode_dims.inc')).read()
    l = open(os.path.join(CSRC, 'hmm_decode_lr_dims.inc')).read()
    return {'general': dict(kind=0, NT=_int(g, r'#define PCL_DEC_DW (\d+)'), HB=_int(g, r'\bHB = (\d+)'), CAND=0),
            'lr': dict(kind=1, NT=_int(l, r'#define PCL_DECLR_DW (\d+)'), HB=_int(l, r'\bHB = (\d+)'), CAND=_int(l, r'\bCAND = (\d+)'))}


GEOMETRY = geometry()
# the KMAX each kernel is compiled for (hmm_decode.hip: the launcher's switch; hmm_decode_lr.hip: PCL_DECLR_LAUNCH)
INSTANTIATIONS = [('general', k) for k in (1, 2, 4, 8, 16)] + [('lr', k) for k in (8, 16)]


def inst_id(inst):
    return '%s-k%d' % inst


def sizes(NT, KMAX):
    return sorted({n for n in (1, 63, 64, 65, NT - 1, NT, NT + 1, (KMAX - 1) * NT + 1, KMAX * NT - 1, KMAX * NT) if 1 <= n <= KMAX * NT})


# ------------------------------------------------------------------ keys
def okey(score):
    """pcl_okey: the order-preserving bits of a float64."""
    b = np.ascontiguousarray(score, dtype=np.float64).view(U64)
    return np.where((b >> U64(63)) != 0, ~b, b | SIGN)


def from_keys(keys):
    """The scores whose pcl_okey is `keys`."""
    k = np.ascontiguousarray(keys, dtype=U64)
    return np.where((k >> U64(63)) != 0, k & ~SIGN, ~k).astype(U64).view(np.float64)


def hash_bins(keys):
    """pcl_prune_stats: how many of the 256 occupancy bins the keys touch."""
    keys = np.ascontiguousarray(keys, dtype=U64)
    return len(np.unique((keys * GOLDEN) >> U64(56))) if len(keys) else 0


def select_path(keys, m, HB, CAND):
    """pcl_select_kth restated round by round over the participating keys (m >= 1).  Returns dict(hb, shifts, counts: the chosen bin's
    count per round, cand_round: the 1-based round whose bin was ranked directly or None, ret: 'equal' | 'shift0' | 'cand', sel, rank,
    eq: the keys equal to sel)."""
    keys = np.ascontiguousarray(keys, dtype=U64)
    hbins = 1 << HB
    kmin, kmax = int(keys.min()), int(keys.max())
    out = dict(hb=None, shifts=[], counts=[], cand_round=None)
    rank = m - 1
    diff = kmin ^ kmax
    if diff == 0:
        sel, ret = kmin, 'equal'
    else:
        hb = diff.bit_length() - 1
        out['hb'] = hb
        lowmask = ((2 << hb) - 1) & 0xFFFFFFFFFFFFFFFF
        shift = max(hb - (HB - 1), 0)
        pmask = pval = 0
        while True:
            play = keys[(keys & U64(pmask)) == U64(pval)]
            h = np.bincount(((play >> U64(shift)) & U64(hbins - 1)).astype(np.int64), minlength=hbins)
            cum = np.cumsum(h)
            b = int(np.searchsorted(cum, rank, side='right'))              # the first bin whose running count exceeds rank
            rank -= int(cum[b] - h[b])
            out['shifts'].append(shift)
            out['counts'].append(int(h[b]))
            digits = (hbins - 1) << shift
            pmask |= digits
            pval = (pval & ~digits) | (b << shift)
            if shift == 0:
                sel, ret = (kmin & ~lowmask) | (pval & lowmask), 'shift0'
                break
            if CAND > 0 and h[b] <= CAND:
                c = np.sort(keys[(keys & U64(pmask)) == U64(pval)])
                sel = int(c[rank])
                rank -= int((c < U64(sel)).sum())
                ret = 'cand'
                out['cand_round'] = len(out['shifts'])
                break
            shift = max(shift - HB, 0)
    out.update(ret=ret, sel=sel, rank=rank, eq=int((keys == U64(sel)).sum()))
    return out


def reference(case, HB, CAND):
    """What the harness must report for a case: the gone set from oracle.decoder_oracle.prune over the participating tokens' scores, mapped
    back to token positions; n_old, kmin, kmax exactly; bins from the hash; and, where the oracle prunes, sel = the m-th smallest of
    the sorted keys and rank = m - 1 - count(keys < sel).  `path` is the twin's account of the select (for the path counts only)."""
    idx = np.flatnonzero(case['part'])
    sc = case['score'][idx]
    keys = okey(sc)
    n_old = len(idx)
    m = int(n_old * (1 - case['beam']))
    drop = do.prune([float(x) for x in sc], case['beam'], case['min_distinct'])
    gone = np.zeros(case['n'], np.uint8)
    gone[idx[sorted(drop)]] = 1
    bins = hash_bins(keys)
    ref = dict(n_old=n_old, m=m, gone=gone, prune=bool(drop), bins=bins,
               kmin=int(keys.min()) if n_old else int(NOKEY), kmax=int(keys.max()) if n_old else 0,
               ran_distinct=m > 0 and n_old >= case['min_distinct'] and bins < case['min_distinct'], sel=None, rank=None, path=None)
    if drop:
        srt = np.sort(keys)
        ref['sel'] = int(srt[m - 1])
        ref['rank'] = m - 1 - int((keys < srt[m - 1]).sum())
        ref['path'] = select_path(keys, m, HB, CAND)
    return ref


# ------------------------------------------------------------------ building blocks
def rng_of(*name):
    return np.random.default_rng(zlib.crc32('/'.join(str(x) for x in name).encode()))


def loglik(rng, n):
    """n different log-likelihood-like negatives (one exponent or two: what every decode-level test feeds the select)."""
    while True:
        s = -rng.uniform(1e3, 1e5, n)
        if len(np.unique(s)) == n:
            return s


def beam_for(n_old, m):
    """A beam with int(n_old (1 - beam)) == m, in the kernels' own arithmetic."""
    for beam in ((0.0,) if m == n_old else ()) + (1.0 - (m + 0.5) / n_old, 1.0 - (m + 0.25) / n_old, 1.0 - (m + 0.75) / n_old):
        if 0.0 <= beam <= 1.0 and int(n_old * (1.0 - beam)) == m:
            return beam
    raise AssertionError((n_old, m))


# bit-structured keys: a prefix that is a finite negative score's (its low 40 bits cleared), fields below.  key + 1 is the next float64
# toward +inf of the same score (np.nextafter), so a field of f bits is a chain of 2^f nextafter steps.
PREFIX = int(okey(np.array([-15000.0]))[0]) & ~((1 << 40) - 1)


def case(family, name, score, part=None, beam=0.5, md=1, **want):
    score = np.ascontiguousarray(score, dtype=np.float64)
    part = np.ones(len(score), np.int32) if part is None else np.ascontiguousarray(part, dtype=np.int32)
    return dict(family=family, name=name, n=len(score), score=score, part=part, beam=float(beam), min_distinct=int(md), want=want)


# ------------------------------------------------------------------ the families, one (family, name) per case and size
def participation(n, NT, rng):
    s = loglik(rng, n)
    C = -(-n // NT) * 64
    yield case('participation', 'all', s, md=8)
    yield case('participation', 'half', s, rng.integers(0, 2, n), md=8)
    one = np.zeros(n, np.int32)
    one[rng.integers(n)] = 1
    yield case('participation', 'one', s, one, md=8, n_old=1)
    yield case('participation', 'none', s, np.zeros(n, np.int32), md=8, n_old=0)
    w = (n - 1) // C                                                # the last wave that owns tokens: all of its tokens finished
    part = np.ones(n, np.int32)
    part[w * C:(w + 1) * C] = 0
    yield case('participation', 'wave', s, part, md=8, wave=w, C=C)


def key_range(n, HB, CAND, rng):
    yield case('key_range', 'loglik', loglik(rng, n))
    s = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-300, 300, n)
    if n >= 2:
        s[:2] = abs(s[0]), -abs(s[1])
    yield case('key_range', 'signs600', rng.permutation(s), hb=63 if n >= 2 else None)
    s = loglik(rng, n)
    if n >= 2:
        s[rng.random(n) < 0.25] = -np.inf
        s[0], s[1] = -np.inf, -1234.5
    yield case('key_range', 'some_ninf', rng.permutation(s))
    yield case('key_range', 'all_ninf', np.full(n, -np.inf), ret='equal')
    yield case('key_range', 'equal', np.full(n, -4321.125), ret='equal')
    for tag, hb in (('hb0', 0), ('hbHB-2', HB - 2), ('hbHB-1', HB - 1), ('hbHB', HB), ('hbHB+1', HB + 1)):
        r = rng.integers(0, 2 << hb, n).astype(np.int64)
        if n >= 2:
            r[0] |= 1 << hb
            r[1] &= ~(1 << hb)
        keys = (r | PREFIX).astype(U64)
        yield case('key_range', tag, from_keys(rng.permutation(keys)), hb=hb if n >= 2 else None)
    # the last round's shift clamped to 0 after a shift that is no multiple of HB: hb = HB + 3 -> shifts 4, 0.  One key carries the top
    # bit, the others share the top digit, so the first round's bin holds n - 1 keys: above CAND whenever n - 1 > CAND
    hb = HB + 3
    r = rng.integers(0, 1 << 4, n).astype(np.int64)
    r[0] |= 1 << hb
    yield case('key_range', 'clamp', from_keys(rng.permutation((r | PREFIX).astype(U64))),
               shifts=[4, 0] if n >= 3 and (CAND == 0 or n - 1 > CAND) else None)


def candidate_path(n, HB, CAND, rng):
    """Left-to-right instantiations (CAND > 0).  Keys = PREFIX | digit << 20 | low: the first round's digit is bits 20..31 (hb = 31).
    Group A shares digit 5 and holds the cut; group B has the digit's top bit set, every key a bin of its own or nearly."""
    def keys_of(lows_a, n_b):
        a = (np.asarray(lows_a, np.int64) | (5 << 20) | PREFIX)
        b = (rng.integers(0, 1 << 20, n_b).astype(np.int64) | (rng.integers(2048, 4096, n_b).astype(np.int64) << 20) | PREFIX)
        return from_keys(rng.permutation(np.concatenate([a, b]).astype(U64)))
    distinct = lambda k: rng.choice(1 << 20, k, replace=False)
    if n >= CAND + 1:
        yield case('candidate', 'bin_CAND', keys_of(distinct(CAND), n - CAND), beam=beam_for(n, CAND // 2), counts0=CAND, cand_round=1)
    if n >= CAND + 2:
        yield case('candidate', 'bin_CAND+1', keys_of(distinct(CAND + 1), n - CAND - 1), beam=beam_for(n, CAND // 2), counts0=CAND + 1,
                   cand_round=2)
        # round one's bin holds n - 1 keys; round two's digit (bits 8..19) takes few values, dealt round-robin, so its bins hold many
        # keys but at most CAND; the low 8 bits repeat, so equal keys abound
        nb = 2 * -(-(n - 1) // CAND)
        lows = ((np.arange(n - 1) % nb) * 37 + 11 << 8) | rng.integers(0, 256, n - 1)
        yield case('candidate', 'round2', keys_of(lows, 1), beam=0.5, counts0=n - 1, cand_round=2, counts1_min=CAND // 4)
    if n >= 2:
        a = min(CAND, n - 1)
        yield case('candidate', 'all_equal', keys_of(np.full(a, 777), n - a), beam=beam_for(n, max(1, a // 2)), cand_round=1, eq=a)
    if n >= 8:
        a = min(CAND, n - 1)
        m, R = a // 2, min(5, a // 2)
        for tag, L in (('run_first', m - 1), ('run_last', m - R)):
            v = np.sort(distinct(a - R + 1))
            lows = np.concatenate([v[:L], np.full(R, v[L]), v[L + 1:]])
            assert len(lows) == a
            yield case('candidate', tag, keys_of(lows, n - a), beam=beam_for(n, m), cand_round=1, eq=R, rank=0 if tag == 'run_first' else R - 1)


def cut_position(n, NT, rng):
    s = loglik(rng, n)
    yield case('cut', 'm1', s, beam=beam_for(n, 1) if n >= 2 else 0.0, m=1)
    if n >= 2:
        yield case('cut', 'm_n-1', s, beam=beam_for(n, n - 1), m=n - 1)
    yield case('cut', 'm_n', s, beam=0.0, m=n)
    yield case('cut', 'beam1', s, beam=1.0, m=0)
    if n >= 6:
        # a run of equal scores over a third of the tokens, with members forced into the first, a middle and the last wave that owns
        # tokens, in key slot 0 and (where a wave owns more than 64 tokens) slot 1
        C = -(-n // NT) * 64
        waves = -(-n // C)
        pos = set(rng.choice(n, max(3, n // 3), replace=False).tolist())
        for w in {0, waves // 2, waves - 1}:
            pos |= {p for p in (w * C, w * C + 64) if p < min(n, (w + 1) * C)}
        pos = np.array(sorted(pos))
        eq = len(pos)
        for tag, r in (('tie_first', 0), ('tie_mid', eq // 2), ('tie_last', eq - 1)):
            s = loglik(rng, n)
            v = np.sort(np.delete(s, pos))
            L = len(v) // 2
            s[pos] = (v[L - 1] + v[L]) / 2 if 0 < L < len(v) else -5e5 - r        # between its neighbours: L scores lie below the run
            L = int((np.delete(s, pos) < s[pos[0]]).sum())
            yield case('cut', tag, s, beam=beam_for(n, L + 1 + r), m=L + 1 + r, eq=eq, rank=r,
                       waves=len({int(p) // C for p in pos}), slots=len({(int(p) % C) // 64 for p in pos}), C=C)


def distinct_scores(n, rng):
    for md in (1, 3, 8, 300):
        for nd in (md - 1, md, md + 1):
            if 1 <= nd <= n:
                v = loglik(rng, nd)
                s = np.concatenate([v, rng.choice(v, n - nd)])
                yield case('distinct', 'md%d_nd%d' % (md, nd), rng.permutation(s), md=md, distinct=nd)
    for md in (3, 8):
        if n >= md:
            # two different scores in one occupancy bin: bins < min_distinct <= distinct, so the exact count overturns the map
            pool = loglik(rng, 2000)
            b = ((okey(pool) * GOLDEN) >> U64(56)).astype(np.int64)
            order = np.argsort(b, kind='stable')
            same = np.flatnonzero(b[order][1:] == b[order][:-1])[0]
            pair = order[[same, same + 1]]
            rest = [i for i in range(2000) if b[i] not in set(b[pair])]
            first = {}
            for i in rest:
                first.setdefault(b[i], i)
            v = pool[np.concatenate([pair, np.array(list(first.values())[:md - 2], dtype=np.int64)])]
            s = np.concatenate([v, rng.choice(v, n - md)])
            yield case('distinct', 'collide_md%d' % md, rng.permutation(s), md=md, distinct=md, bins=md - 1)


_CASES, _REFS = {}, {}


def cases_at(which, n):
    """Every family at one size.  A size's cases do not depend on KMAX, so the instantiations of a kernel share them (and their references:
    computed once, never changed)."""
    if (which, n) not in _CASES:
        g = GEOMETRY[which]
        NT, HB, CAND = g['NT'], g['HB'], g['CAND']
        fams = [participation(n, NT, rng_of('part', n)), key_range(n, HB, CAND, rng_of('range', n)), cut_position(n, NT, rng_of('cut', n)),
                distinct_scores(n, rng_of('distinct', n))]
        if CAND > 0:
            fams.append(candidate_path(n, HB, CAND, rng_of('cand', n)))
        _CASES[which, n] = [c for fam in fams for c in fam]
    return _CASES[which, n]


def prune_cases(inst):
    """Every case of one instantiation ('general' | 'lr', KMAX), every family at every size."""
    which, KMAX = inst
    return [c for n in sizes(GEOMETRY[which]['NT'], KMAX) for c in cases_at(which, n)]


def case_id(c):
    return '%s-%s-n%d' % (c['family'], c['name'], c['n'])


def reference_of(which, c):
    key = (which, case_id(c))
    if key not in _REFS:
        _REFS[key] = reference(c, GEOMETRY[which]['HB'], GEOMETRY[which]['CAND'])
    return _REFS[key]


def pack_prune(cases):
    """The harness's arrays: case c owns tokens off[c] .. off[c] + n[c]."""
    n = np.array([c['n'] for c in cases], np.int32)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    return dict(n=n, off=off, beam=np.array([c['beam'] for c in cases], np.float64),
                min_distinct=np.array([c['min_distinct'] for c in cases], np.int32),
                score=np.concatenate([c['score'] for c in cases]), part=np.concatenate([c['part'] for c in cases]))


# ------------------------------------------------------------------ transfer
TRANSFER_FAMILIES = ('random', 'equal', 'tied_best', 'all_ninf', 'descending', 'ascending')


def transfer_sizes(NT):
    return [0, 1, 63, 65, NT + 1, 16 * NT]


def tied_positions(n, NT):
    """Where the best score sits in the tied_best family: two lanes of wave 0, a lane of wave 1, and later strides of those lanes."""
    return [p for p in (0, 40, 74, NT, 74 + 2 * NT) if p < n]


def transfer_cases(NT):
    """dict(name, n, candidate, sc, nd, hs, map): token i's state is (sc[i], nd[i], hs[i]); `map` is a permutation of 0 .. n-1 with bit
    31 set on about half its entries, for the run that reads the state through map[i] & 0x7fffffff."""
    out = []
    for n in transfer_sizes(NT):
        for fam in TRANSFER_FAMILIES:
            rng = rng_of('transfer', fam, n)
            if fam == 'random':
                sc = -rng.uniform(1e3, 1e5, n)
            elif fam == 'equal':
                sc = np.full(n, -2222.5)
            elif fam == 'tied_best':
                sc = -rng.uniform(1e3, 1e5, n)
                sc[tied_positions(n, NT)] = -999.0
            elif fam == 'all_ninf':
                sc = np.full(n, -np.inf)
            elif fam == 'descending':
                sc = -1000.0 - np.arange(n, dtype=np.float64)
            else:
                sc = -1000.0 - np.arange(n, dtype=np.float64)[::-1]
            nd = rng.integers(0, 1 << 20, n).astype(np.int32)
            hs = rng.integers(-1, 1 << 20, n).astype(np.int32)
            perm = rng.permutation(n).astype(np.int64)
            fresh = rng.integers(0, 2, n).astype(np.int64) << 31
            for cand in sorted({1, 6, n, n + 3}):
                out.append(dict(name='%s-n%d-c%d' % (fam, n, cand), family=fam, n=n, candidate=cand, sc=np.ascontiguousarray(sc, dtype=np.float64),
                                nd=nd, hs=hs, map=(perm | fresh).astype(np.uint32).view(np.int32)))
    return out


def transfer_reference(c):
    """The stable descending sort's first min(candidate, n) entries: (n_out, node, score, hist)."""
    order = np.argsort(-c['sc'], kind='stable')[:min(c['candidate'], c['n'])]
    return len(order), c['nd'][order], c['sc'][order], c['hs'][order]


def pack_transfer(cases, use_map):
    """The harness's arrays.  use_map: the state of token i is stored at map[i] & 0x7fffffff."""
    n = np.array([c['n'] for c in cases], np.int32)
    cand = np.array([c['candidate'] for c in cases], np.int32)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(cand)[:-1]]).astype(np.int64)

    def stored(c, key):
        if not use_map:
            return c[key]
        a = np.empty_like(c[key])
        a[c['map'].view(np.uint32) & np.uint32(0x7fffffff)] = c[key]
        return a
    return dict(n=n, candidate=cand, off=off, out_off=out_off, sc=np.concatenate([stored(c, 'sc') for c in cases]),
                nd=np.concatenate([stored(c, 'nd') for c in cases]), hs=np.concatenate([stored(c, 'hs') for c in cases]),
                map=np.concatenate([c['map'] for c in cases]))
