"""CPU twin of the word lattice (pcl_batch_decode_lattice / pcl_batch_lattice_posteriors; csrc/lattice.hip).  TEST INFRASTRUCTURE.

Three parts:
  record_decode   the decoder's frame loop (oracle/decoder_oracle.decode; with a language model tests/_decoder_lm_twin.decode), RECORDING every
                  word-end donor in token order and (frame, seed) per history entry.  The existing twins cannot be edited and have no hook, so
                  the loop is restated here once, on their pieces (Token, prune, hand_over, emission_column, word_offer: imported, not copied);
                  tests/test_lattice_twin.py holds its (final, history) to theirs.
  build / posteriors   the lattice rule of include/poccala_hip.h in NumPy, sum for sum in the kernel's order (thread i of 256 takes list
                  positions i, i + 256, ...; a butterfly lane ^ 32 .. 1 over each wave; the four waves ascending), in float64 or long double.
  enumerate_paths a brute-force statement of Z, the arc posteriors and the best path for tiny lattices.
"""
import numpy as np

import _decoder_lm_twin as lt
from oracle import decoder_oracle as do

LT, LANES = 256, 64
NEG = -np.inf


def record_decode(tree, unit_trans, b_all, lm=None, beam=0.85, candidate=5, min_distinct=8, s=5, max_tokens=None, trace=None, info=None):
    """Returns (final, history, records, entries): final / history as the twin it restates; records = [(frame, tok, node, hist, score, term,
    word)] of every word-end donor, frames ascending and token order inside a frame; entries = [(frame, seed)] per history entry."""
    T = b_all.shape[1]
    units_of = [[int(u) for u in row[:n]] for row, n in zip(tree['node_units'], tree['node_nunits'])]
    roots = [int(r) for r in tree['roots']]
    kids = lambda n: [int(c) for c in tree['child_idx'][tree['child_ptr'][n]:tree['child_ptr'][n + 1]]]
    tokens, history, records, entries = [], [], [], []
    for r in roots:
        if max_tokens is not None and len(tokens) >= max_tokens:
            if info is not None:
                info['overflow'] = True
            break
        tok = do.Token(0.0, r, units_of[r], unit_trans, s)
        tok.hist = -1
        tok.viterbi(do.emission_column(tok.units, b_all, 0, s))
        tokens.append(tok)
    if trace is not None:
        trace.append(len(tokens))
    for t in range(1, T):
        n_start = len(tokens)
        done = [tok.viterbi(do.emission_column(tok.units, b_all, t, s)) for tok in tokens]
        live = {tok.node: tok for tok, d in zip(tokens, done) if not d}
        offers, order = {}, []
        for i, (tok, d) in enumerate(zip(tokens, done)):
            if not d:
                continue
            targets = [(c, tok.score, tok.hist) for c in kids(tok.node)]
            if tree['node_word'][tok.node]:
                term, word, offer = 0.0, 0, tok.score
                if lm is not None:
                    v = 0 if tok.hist < 0 else history[tok.hist][2]
                    term, word = lt.word_offer(lm, v, tok.node)
                    offer = tok.score + term
                records.append((t, i, tok.node, tok.hist, float(tok.score), float(term), int(word)))
                targets += [(r, offer, ('word', tok, word)) for r in roots]
            for node, score, hist in targets:
                if node not in offers:
                    offers[node] = (score, hist)
                    order.append(node)
                elif score > offers[node][0]:
                    offers[node] = (score, hist)
        winner = None
        for node in order:
            h = offers[node][1]
            if isinstance(h, tuple):
                if winner is None:
                    history.append((h[1].hist, h[1].node, h[2]) if lm is not None else (h[1].hist, h[1].node))
                    entries.append((t, float(offers[node][0])))
                    winner = len(history) - 1
                offers[node] = (offers[node][0], winner)
        created = []
        for node in order:
            score, hist = offers[node]
            rule = do.hand_over(score, live[node].score if node in live else None)
            if rule == 'take':
                live[node].score = score
                live[node].hist = hist
            elif rule == 'keep':
                pass
            elif max_tokens is not None and n_start + len(created) >= max_tokens:
                if info is not None:
                    info['overflow'] = True
            else:
                new = do.Token(score, node, units_of[node], unit_trans, s)
                new.hist = hist
                new.viterbi(do.emission_column(new.units, b_all, t, s))
                created.append(new)
        old = [tok for tok, d in zip(tokens, done) if not d]
        drop = do.prune([tok.score for tok in old], beam, min_distinct)
        old = [tok for i, tok in enumerate(old) if i not in drop]
        tokens = old + created
        if trace is not None:
            trace.append(len(tokens))
    best = sorted(range(len(tokens)), key=lambda i: -tokens[i].score)[:candidate]
    return [(tokens[i].node, tokens[i].score, tokens[i].hist) for i in best], history, records, entries


def build(records, entries, final, T, closing=True, subtract_seed=True, child_score=False):
    """The lattice in canonical order as a dict of arrays: frame, tok, node, hist, score, term, word, start, end (nodes: 0 = START, entry k =
    k + 1, END = H + 1), seed (H + 1,) per node but END, node_frame (H + 1,), H.  The three switches state the omissions the tests show to
    matter: closing=False ignores the closing arcs' scores (they close with ac 0), subtract_seed=False keeps ac = score, child_score=True
    takes s + term for the children (score + term in place of score)."""
    rec = sorted(records, key=lambda r: (r[0], r[1]))
    H = len(entries)
    of_frame = {f: k for k, (f, _) in enumerate(entries)}
    cols = [list(c) for c in zip(*rec)] if rec else [[] for _ in range(7)]
    frame, tok, node, hist, score, term, word = cols
    start = [h + 1 for h in hist]
    end = [of_frame[f] + 1 for f in frame]
    for c, (n, sc, h) in enumerate(final):
        frame.append(T - 1)
        tok.append(c)
        node.append(n)
        hist.append(h)
        score.append(float(sc))
        term.append(0.0)
        word.append(-1)
        start.append(h + 1)
        end.append(H + 1)
    lat = dict(frame=np.array(frame, np.int32), tok=np.array(tok, np.int32), node=np.array(node, np.int32), hist=np.array(hist, np.int32),
               score=np.array(score, np.float64), term=np.array(term, np.float64), word=np.array(word, np.int32), start=np.array(start, np.int32),
               end=np.array(end, np.int32), H=H, seed=np.array([0.0] + [sd for _, sd in entries]), node_frame=np.array([-1] + [f for f, _ in entries], np.int64),
               n_final=len(final))
    lat['switches'] = dict(closing=closing, subtract_seed=subtract_seed, child_score=child_score)
    return lat


def weights(lat, kappa, dtype=np.float64):
    sw = lat.get('switches', dict(closing=True, subtract_seed=True, child_score=False))
    s = lat['score'].astype(dtype)
    if sw['child_score']:
        s = s + lat['term'].astype(dtype)
    seed = lat['seed'].astype(dtype)[lat['start']] if sw['subtract_seed'] else np.zeros(len(s), dtype)
    with np.errstate(invalid='ignore'):
        ac = np.where(np.isneginf(s), dtype(NEG), s - seed)
    if not sw['closing']:
        ac = np.where(lat['word'] < 0, dtype(0.0), ac)
    return dtype(kappa) * ac + lat['term'].astype(dtype)


def _butterfly(v, op):
    v = v.copy()
    lanes = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, lanes ^ o])
    return v[:, 0]


def lse_list(v, dtype=np.float64):
    """The kernel's log-sum-exp of one node's list, in its order."""
    if len(v) == 0:
        return dtype(NEG)
    m = v.max()
    if np.isinf(m):
        return dtype(m)
    with np.errstate(under='ignore'):
        e = np.exp(v - m)
    rows = -(-len(e) // LT)
    pad = np.zeros(rows * LT, dtype)
    pad[:len(e)] = e
    pad = pad.reshape(rows, LT)
    acc = np.zeros(LT, dtype)
    used = np.zeros(LT, bool)
    for r in range(rows):                                                       # thread i: positions i, i + 256, ... in that order
        live = np.arange(LT) + r * LT < len(e)
        acc = np.where(live, acc + pad[r], acc)
        used |= live
    waves = _butterfly(acc.reshape(LT // LANES, LANES), lambda a, b: a + b)
    s = waves[0]
    for w in waves[1:]:
        s = s + w
    return m + np.log(s)


def posteriors(lat, kappa=1.0, use_word=False, dtype=np.float64):
    """alpha, beta, vit (H + 2,), lnZ, lnp per arc, best (arc indices), best_score, conf per word of the best path; status as the device's."""
    H, n = lat['H'], len(lat['frame'])
    start, end = lat['start'], lat['end']
    if lat['n_final'] == 0:
        return dict(status=2, lnZ=np.nan, lnp=np.full(n, np.nan), best=[], best_score=np.nan, conf=[])
    w = weights(lat, kappa, dtype)
    END = H + 1
    alpha, beta, vit = np.full(H + 2, NEG, dtype), np.full(H + 2, NEG, dtype), np.full(H + 2, NEG, dtype)
    bp = np.full(H + 2, -1)
    alpha[0] = vit[0] = 0.0
    beta[END] = 0.0
    into = [np.flatnonzero(end == k) for k in range(H + 2)]                     # (ascending arc index: the CSR by end node)
    out_of = [np.flatnonzero(start == k) for k in range(H + 2)]                 # (the stable counting sort)
    for k in range(1, H + 2):
        a = into[k]
        alpha[k] = lse_list(alpha[start[a]] + w[a], dtype)
        if len(a):
            y = vit[start[a]] + w[a]
            j = int(np.argmax(y))                                               # the earliest arc on ties
            vit[k], bp[k] = y[j], a[j]
    for k in range(H, -1, -1):
        a = out_of[k]
        beta[k] = lse_list(w[a] + beta[end[a]], dtype)
    lnZ = alpha[END]
    if not lnZ > NEG:
        return dict(status=8, lnZ=np.nan, lnp=np.full(n, np.nan), best=[], best_score=np.nan, conf=[], alpha=alpha, beta=beta)
    with np.errstate(invalid='ignore'):
        lnp = ((alpha[start] + w) + beta[end]) - lnZ
    best, k = [], END
    while k != 0 and bp[k] >= 0:
        best.append(int(bp[k]))
        k = int(start[bp[k]])
    best.reverse()
    nf = lat['node_frame']
    conf = []
    for a in best:
        fs, fe = int(nf[start[a]]), int(lat['frame'][a])
        by_word = use_word and lat['word'][a] >= 0
        ids = lat['word'] if by_word else lat['node']
        same = np.flatnonzero(ids == ids[a])
        pm = np.exp(lnp[a]) if fe <= fs else dtype(NEG)
        for tau in range(fs + 1, fe + 1):
            P = dtype(0.0)
            for j in same:                                                      # ascending arc order
                if nf[start[j]] < tau <= lat['frame'][j]:
                    P = P + np.exp(lnp[j])
            pm = max(pm, P)
        conf.append(pm)
    return dict(status=0, alpha=alpha, beta=beta, vit=vit, lnZ=lnZ, lnp=lnp, best=best, best_score=vit[END], conf=np.array(conf, dtype), w=w)


def allowances(t64, tld, lat):
    """What the device may differ from the float64 twin by: 4 x |float64 twin - long-double twin| plus an absolute term, derived as
    tests/_mbr_twin.allowances derives its own.

    The kernel runs the twin's operations in the twin's order; the weights (one product, one difference, one sum, no contraction) and the
    Viterbi sums are exact repeats.  What differs is the library's exp and log, each within 1 ulp of its result: one log-sum-exp moves its
    node's value by at most 2 ulp(amax), amax the largest finite |alpha|, |beta|.  alpha(n) chains at most n of them, beta(n) at most END - n:
        ln Z                         END steps:              2 END ulp(amax)
        ln p = alpha(s) + w + beta(e) - ln Z, s < e:  at most END - 1 steps in alpha(s) and beta(e) together, END in ln Z, and three
                                     roundings at amax:      (4 END + 2) ulp(amax) = d
        a confidence = sum over k <= n_arcs terms exp(ln p): each term off by d + 2^-52 relatively, the sum (at most `conf`, which the
                                     test bounds by 1 + allowance) by its roundings:  (d + (n_arcs + 1) 2^-52) max(conf, 1)."""
    END = lat['H'] + 1
    both = np.concatenate([t64['alpha'], t64['beta']])
    fin = np.abs(both[np.isfinite(both)])
    ulp = np.spacing(max(fin.max() if fin.size else 1.0, 1.0))
    d = (4.0 * END + 2.0) * ulp
    n = len(lat['frame'])
    conf64 = np.asarray(t64['conf'], np.float64)
    term = dict(lnZ=2.0 * END * ulp, lnp=d, best_score=0.0, conf=(d + (n + 1) * 2.0 ** -52) * np.maximum(conf64, 1.0))
    out = {}
    for key, add in term.items():
        a = np.asarray(t64[key], np.float64)
        with np.errstate(invalid='ignore'):
            dist = np.abs(a - np.asarray(tld[key])).astype(np.float64)
        out[key] = 4.0 * np.where(np.isfinite(dist), dist, 0.0) + add
    return out


def enumerate_paths(lat, kappa=1.0):
    """Every START -> END path by depth-first search: (Z, arc posteriors, best path, best score, node posteriors), in plain float64 sums."""
    w = weights(lat, kappa)
    H, n = lat['H'], len(w)
    out_of = [np.flatnonzero(lat['start'] == k) for k in range(H + 2)]
    paths = []

    def walk(node, arcs, total):
        if node == H + 1:
            paths.append((list(arcs), total))
            return
        for a in out_of[node]:
            walk(int(lat['end'][a]), arcs + [int(a)], total + w[a])
    walk(0, [], 0.0)
    with np.errstate(under='ignore'):
        p = np.array([np.exp(t) for _, t in paths])
    Z = p.sum()
    arc_post, node_post = np.zeros(n), np.zeros(H + 2)
    for (arcs, _), x in zip(paths, p):
        arc_post[arcs] += x / Z if Z > 0 else 0.0
        for k in {0} | {int(lat['end'][a]) for a in arcs}:
            node_post[k] += x / Z if Z > 0 else 0.0
    best = max(range(len(paths)), key=lambda i: (paths[i][1], [-a for a in paths[i][0]])) if paths else None
    return Z, arc_post, (paths[best][0] if best is not None else []), (paths[best][1] if best is not None else NEG), node_post


def random_lattice(rng, H, arcs_per_node, n_final=2, dead=0, neg_inf=0, T=None, n_ids=4):
    """A synthetic record set: H entries at frames 2, 4, ...; every entry receives arcs_per_node(k) arcs from random earlier nodes; n_final
    closing arcs.  dead: that many extra entries nothing leaves (no arc out, no closing arc from them); neg_inf: that many recorded arcs
    with a score of -inf.  Returns (records, entries, final, T)."""
    frames = [2 * (k + 1) for k in range(H)]
    T = frames[-1] + 3 if (T is None and H) else (T or 3)
    seeds = np.concatenate([[0.0], np.cumsum(rng.uniform(-30.0, -10.0, size=H))])
    dead_set = set(rng.choice(np.arange(1, H), size=min(dead, max(H - 1, 0)), replace=False).tolist()) if dead and H > 1 else set()
    records, entries = [], []
    for k in range(H):
        cnt = max(1, int(arcs_per_node(k)))
        ok = [h for h in range(-1, k) if (h + 1) not in dead_set]
        for i in range(cnt):
            h = int(rng.choice(ok))
            sc = seeds[h + 1] + (frames[k] - (frames[h] if h >= 0 else -1)) * rng.uniform(-6.0, -4.0)
            records.append((frames[k], i, int(rng.integers(n_ids)), h, float(sc), float(rng.uniform(-3.0, 0.0)), int(1 + rng.integers(n_ids))))
        entries.append((frames[k], float(seeds[k + 1])))
    spare = [i for i, r in enumerate(records) if r[1] >= 1]                     # (every entry keeps a finite arc: its first)
    for i in rng.choice(spare, size=min(neg_inf, len(spare)), replace=False).tolist() if neg_inf and spare else []:
        r = records[i]
        records[i] = r[:4] + (NEG,) + r[5:]
    ok = [h for h in range(-1, H) if (h + 1) not in dead_set]
    final = []
    for c in range(n_final):
        h = int(ok[-1]) if c == 0 else int(rng.choice(ok))
        final.append((int(rng.integers(n_ids)), float(seeds[h + 1] + (T - 1 - (frames[h] if h >= 0 else -1)) * rng.uniform(-6.0, -4.0)), h))
    final.sort(key=lambda f: -f[1])
    return records, entries, final, T
