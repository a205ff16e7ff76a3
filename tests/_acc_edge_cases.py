"""Inputs of the accumulate edge tests beyond the f16 pipeline (tests/test_gpu_acc_edges.py on the device, tests/test_acc_edge_cases.py on
the CPU): the active-frame list builder of csrc/gmm_accumulate.hip (acc_count* -> acc_scan_kernel -> acc_fill*, by segments and by rows) on
ragged batches, and the strict-f32 matrix-pipe kernel and the direct-form kernel at the edges of their own tilings.  tests/_acc16_cases.py
supplies model, draw_frames, case, emissions and reference; everything here is NumPy and the oracle.

A case is a dict of _acc16_cases.case plus: kind ('list' or 'shape'), T (U,), begin (U,), rows (per utterance the row -> state map, -1 the
entry row, -2 the exit row, which may also stand INSIDE a map), labels (None, or the unit ids a label batch is built from: rows is then what
the library derives), lgamma (per utterance (N_u, T_u), non-survivors at -inf; a shape case keeps the single (J+2, F) matrix of its one
all-state utterance), counts (J,) survivors per state over all its segments, claims (the edge it sits on, re-derived by the CPU companion),
defects (list cases: the list-builder defects it must show, see twin_lists).

Segment order (pcl_batch_set_states): state by state; inside a state first the FIRST row of the state in every utterance (utterance
order), then the further rows of utterances that name it more than once (utterance, row order).  A state's list is the concatenation of
its segments' survivors, frames ascending inside a segment."""
import functools

import numpy as np

import _acc16_cases as ac
from oracle import poccala_oracle as po

ENTRY, EXIT = -1, -2
LN2 = ac.LN2
SCAN_THREADS = 1024                           # acc_scan_kernel: one workgroup
STEP = dict(segs=64, rows=8)                  # frames a wave takes per trip: acc_fill_kernel, acc_fill_rows_kernel
ROW_GROUP, ROW_BLOCK = 8, 32                  # rows per wave, rows per block (ROWS_WPB = 4) of the row form
AW32, WG, FC = 8, 256, 32                     # gmm_accumulate.hip: m-tiles per MFMA32 workgroup, mixtures per direct-form slice, frames per LDS chunk
KEYS = ('acc', 'alpha_acc', 'mean_acc', 'cov_acc')
DEFECTS = ('drop', 'early', 'prev', 'gt', 'per')


# ------------------------------------------------------------------ the launcher's arithmetic, restated
def device_dim(d):
    """pcl_api.hip device_dim: the padded dimension the kernels have an instance for."""
    return min(x for x in (13, 26, 39, 47, 48, 64) if x >= d)


def route(variant, prec, d):
    """pcl_route: 1 the direct form, 3 the f32-input MFMA kernel, 7 the split-f16 producer / consumer."""
    if prec != 'f32' or variant < 3 or device_dim(d) not in (13, 26, 39, 47):
        return 1
    return variant


def tilings(M):
    """Mpad (direct form, multiples of 4), its slices and the live lanes of the last one; m-tiles of the matrix pipe, nslice of the MFMA32
    kernel and the live waves of its last slice."""
    mpad, nmt = (M + 3) // 4 * 4, (M + 31) // 32
    nslice_d, nslice = (mpad + WG - 1) // WG, (nmt + AW32 - 1) // AW32
    return dict(Mpad=mpad, direct_slices=nslice_d, direct_last_live=mpad - (nslice_d - 1) * WG, n_mtiles=nmt, nslice=nslice,
                mfma_last_live=nmt - (nslice - 1) * AW32)


def mfma32_blocks(M, ns):
    """run_mfma32's grid, and per block the (state, slice) the kernel maps it to (None: w >= n_states, the block returns)."""
    t = tilings(M)
    nslice = t['nslice']
    nb = (ns + 7) // 8 * 64 if nslice == 8 else ns * nslice
    out = []
    for b in range(nb):
        w, s = ((b & 7) + 8 * (b >> 6), (b >> 3) & 7) if nslice == 8 else divmod(b, nslice)
        out.append((w, s) if w < ns else None)
    return out


def scan_per(n_segs):
    return (n_segs + SCAN_THREADS - 1) // SCAN_THREADS


def threshold(c, prec='f32'):
    """build_active_lists: ln gamma at or above it survives."""
    return max(-1076.0 if prec == 'f64' else -150.0, c['prune'] if c['prune'] is not None else -1e300) * LN2


def off_pipe(mean, var):
    """state_prepass_kernel's conditioning test for ONE state in float64: which mixtures' centred expansion is beyond COND_MAX (the first
    lines of _acc16_cases.derive_replica, which cannot take a state whose mixtures ALL leave)."""
    c = mean.mean(axis=0).astype(np.float32).astype(np.float64)
    return (ac.LOG2E * ((mean - c) ** 2 * (0.5 / var)).sum(axis=1)).astype(np.float32) > ac.COND_MAX


def uses_valu(c, j):
    """pcl_state_acc_uses_valu at the default limits: more than half of the state's mixtures beyond the conditioning limit."""
    return int(off_pipe(c['mean'][j], c['var'][j]).sum()) > int(np.float32(0.5) * np.float32(c['mean'].shape[1]))


def accumulate_order(c):
    """order_states on a matrix-pipe route: the states with work, the well-conditioned ones first."""
    work = sorted({int(s) for r in c['rows'] for s in r if s >= 0})
    return [j for j in work if not uses_valu(c, j)] + [j for j in work if uses_valu(c, j)]


# ------------------------------------------------------------------ batches
def lgammas(c):
    return c['lgamma'] if isinstance(c['lgamma'], list) else [c['lgamma']]


def segments(c):
    """[(state, utterance, row)] in the library's segment order."""
    J = c['mean'].shape[0]
    per = [([], []) for _ in range(J)]
    for u, rows in enumerate(c['rows']):
        seen = set()
        for n, st in enumerate(rows):
            if st >= 0:
                per[st][st in seen].append((u, n))
                seen.add(int(st))
    return [(j, u, n) for j in range(J) for u, n in per[j][0] + per[j][1]]


def emissions(c):
    """Per utterance the float64 ln b of every row from the oracle (entry rows 0, exit rows -inf), (N_u, T_u)."""
    if c['name'] in _EMIT:
        return _EMIT[c['name']]
    if c['kind'] == 'shape':
        out = [ac.emissions(c)]
    else:
        J = c['mean'].shape[0]
        used = sorted({int(s) for r in c['rows'] for s in r if s >= 0})
        full = {j: po.gmm_point(c['frames'], c['mean'][j], c['var'][j], c['w'][j]) for j in used}
        out = []
        for u, rows in enumerate(c['rows']):
            lo, T = int(c['begin'][u]), int(c['T'][u])
            B = np.full((len(rows), T), -np.inf)
            for n, st in enumerate(rows):
                B[n] = 0.0 if st == ENTRY else (-np.inf if st == EXIT else full[int(st)][lo:lo + T])
            out.append(B)
        assert J >= len(used)
    _EMIT[c['name']] = out
    return out


_EMIT, _REF = {}, {}


def stats_of_lists(c, lists):
    """Clustering.GMM.update_acc through the oracle, one call per state over its list [(frame, ln gamma - ln b, gamma)], linear domain."""
    J, M, D = c['mean'].shape
    out = dict(acc=np.zeros((J, M)), alpha_acc=np.zeros(J), mean_acc=np.zeros((J, M, D)), cov_acc=np.zeros((J, M, D)))
    for j, ent in lists.items():
        if not ent:
            continue
        fr = np.array([e[0] for e in ent])
        with np.errstate(divide='ignore'):
            l = np.log(np.array([e[2] for e in ent]))
        a = dict(acc=np.full(M, -np.inf), alpha_acc=-np.inf, mean_acc=np.full((M, D), -np.inf), cov_acc=np.full((M, D), -np.inf))
        po.gmm_update_acc(a, l, l - np.array([e[1] for e in ent]), c['frames'][fr], c['mean'][j], c['var'][j], c['w'][j])
        with np.errstate(all='ignore'):
            for k in out:
                out[k][j] = np.exp(a[k])
    return out


def as_batch(c):
    """A case of _acc16_cases with the batch fields of this file (one all-state utterance); a case of this file as it is."""
    if 'kind' in c:
        return c
    J, F = c['mean'].shape[0], c['frames'].shape[0]
    return dict(c, kind='shape', T=np.array([F], dtype=np.int32), begin=np.zeros(1, dtype=np.int64), labels=None,
                rows=[np.concatenate([[ENTRY], np.arange(J), [EXIT]]).astype(np.int32)])


def reference(c):
    """The oracle's statistics, computed once per case and read-only.  A list case: update_acc per OCCURRENCE of a state (one segment: the
    utterance's frames, the row's ln gamma over its survivors and the row's ln b), linear domain, summed over the occurrences."""
    if c['kind'] == 'shape':
        return ac.reference(c)
    if c['name'] in _REF:
        return _REF[c['name']]
    J, M, D = c['mean'].shape
    out = dict(acc=np.zeros((J, M)), alpha_acc=np.zeros(J), mean_acc=np.zeros((J, M, D)), cov_acc=np.zeros((J, M, D)))
    B, thr = emissions(c), threshold(c)
    for j, u, n in segments(c):
        lg = c['lgamma'][u][n]
        keep = np.flatnonzero(lg >= thr)
        if not len(keep):
            continue
        x = c['frames'][int(c['begin'][u]):int(c['begin'][u]) + int(c['T'][u])][keep]
        a = dict(acc=np.full(M, -np.inf), alpha_acc=-np.inf, mean_acc=np.full((M, D), -np.inf), cov_acc=np.full((M, D), -np.inf))
        po.gmm_update_acc(a, lg[keep], B[u][n][keep], x, c['mean'][j], c['var'][j], c['w'][j])
        with np.errstate(all='ignore'):
            for k in out:
                out[k][j] += np.exp(a[k])
    for v in out.values():
        v.setflags(write=False)
    _REF[c['name']] = out
    return out


def bounds(c, j, key, prec):
    """(rtol, atol) the device test holds statistic `key` of state j to: the values of tests/test_gpu_accumulate.py."""
    ref = reference(c)
    rt, at = (1e-4, 1e-6) if prec == 'f32' else (1e-9, 1e-13)
    floor = at * float(np.abs(ref[key][j]).max())
    if key == 'cov_acc' and prec == 'f32':
        from _parity import cov_acc_atol
        floor = cov_acc_atol(ref['acc'][j], c['mean'][j], c['var'][j], floor)
    return rt, floor


# ------------------------------------------------------------------ the NumPy twin of the list builder
def twin_lists(c, form='rows', defect=None, prec='f32'):
    """count -> scan -> fill as the kernels do them, on arrays: cnt per segment, off = exclusive scan in SCAN_THREADS chunks of `per`
    segments, the entries (frame, lg - lb, exp(lg)) of segment k at off[k] + rank, a state's list = slots [off[lo], off[hi]).  Both forms
    build the same lists; `form` only says where a defect's step boundary lies (a kept frame t > 0 with t % STEP[form] == 0).
    defect: None, or
      'drop'  the entry at the step boundary is not written (its slot stays empty);
      'early' it is written one slot early (over its predecessor; its own slot stays empty);
      'prev'  it is counted and filed with the previous segment;
      'gt'    keep when lg > thr in place of lg >= thr;
      'per'   the scan's chunk length rounds down in place of up (segments beyond SCAN_THREADS * per are never scanned)."""
    assert defect is None or defect in DEFECTS
    segs, B, thr, step = segments(c), emissions(c), threshold(c, prec), STEP[form]
    lg_all = lgammas(c)
    ent = []
    for j, u, n in segs:
        lg, lb = lg_all[u][n], B[u][n]
        keep = np.flatnonzero(lg > thr if defect == 'gt' else lg >= thr)
        ent.append([(int(c['begin'][u]) + int(t), float(lg[t] - lb[t]), float(np.exp(lg[t])), int(t) > 0 and int(t) % step == 0) for t in keep])
    if defect == 'prev':
        for k in range(len(ent) - 1, 0, -1):
            mv = [e for e in ent[k] if e[3]]
            ent[k] = [e for e in ent[k] if not e[3]]
            ent[k - 1] = ent[k - 1] + [e[:3] + (False,) for e in mv]
    n = len(segs)
    cnt = np.array([len(e) for e in ent], dtype=np.int64)
    per = n // SCAN_THREADS if defect == 'per' else scan_per(n)
    off = np.zeros(n + 1, dtype=np.int64)
    lo = np.minimum(np.arange(SCAN_THREADS) * per, n)
    hi = np.minimum(lo + per, n)
    part = np.array([cnt[a:b].sum() for a, b in zip(lo, hi)])
    run = np.concatenate([[0], np.cumsum(part)])
    off[n] = run[-1]
    for t in range(SCAN_THREADS):
        r = run[t]
        for i in range(lo[t], hi[t]):
            off[i] = r
            r += cnt[i]
    flat, late = [None] * (int(cnt.sum()) + 1), []
    for k in range(n):
        for i, e in enumerate(ent[k]):
            slot = int(off[k]) + i
            if e[3] and defect == 'drop':
                continue
            if e[3] and defect == 'early':
                late.append((max(slot - 1, 0), e))
                continue
            flat[slot] = e
    for slot, e in late:
        flat[slot] = e
    lists, k = {}, 0
    for j in sorted({s[0] for s in segs}):
        k0 = k
        while k < n and segs[k][0] == j:
            k += 1
        lists[j] = [e[:3] for e in flat[int(off[k0]):int(off[k])] if e is not None]
    return lists


def boundary_owners(c, form):
    """States that own a kept frame on the step boundary of `form`."""
    thr, out = threshold(c), set()
    for j, u, n in segments(c):
        t = np.flatnonzero(lgammas(c)[u][n] >= thr)
        if ((t > 0) & (t % STEP[form] == 0)).any():
            out.add(j)
    return out


# ------------------------------------------------------------------ ragged batches for the list builder
PATTERNS = ('every', 'none', 'first', 'last', 'eighth', 'mid')          # 'none' between two patterns that keep frames
RAGGED_T = [129, 1, 7, 8, 9, 63, 64, 65]                                # (the longest first: every state's FIRST segment has survivors on the 64-frame step)
RAGGED_N = [34, 3, 8, 9, 32, 33, 34, 8]
LIST_J, LIST_M, LIST_D = 12, 4, 13
EMPTY_STATE = 11                                                         # named by rows, never kept: beg == end in both accumulate kernels


def pattern_frames(p, T):
    if p == 'mid' and T < 66:
        p = 'every'
    return dict(every=np.arange(T), none=np.arange(0), first=np.arange(1), last=np.arange(T - 1, T), eighth=np.arange(0, T, 8),
                mid=np.arange(63, 66))[p]


def unit_rows(units, n_emit):
    """Emitting rows of a label: three states per unit, cut to n_emit rows."""
    return np.concatenate([[3 * u, 3 * u + 1, 3 * u + 2] for u in units])[:n_emit]


def list_case(name, seed, T, rows, pattern_of, claims, defects, labels=None, prune=None, lg_of=None, empty=EMPTY_STATE):
    rng = np.random.default_rng(seed)
    mean, var, w = ac.model(LIST_J, LIST_M, LIST_D, seed)
    T = np.asarray(T, dtype=np.int32)
    begin = np.concatenate([[0], np.cumsum(T[:-1])]).astype(np.int64)
    frames = ac.draw_frames(rng, mean, var, int(T.sum()))
    rows = [np.asarray(r, dtype=np.int32) for r in rows]
    lg = [np.full((len(r), int(t)), -np.inf) for r, t in zip(rows, T)]
    counts, pats = np.zeros(LIST_J, dtype=np.int64), {}
    for u, r in enumerate(rows):
        for n, st in enumerate(r):
            if st < 0:
                continue
            p = 'none' if st == empty else pattern_of(u, n, int(st))
            idx = pattern_frames(p, int(T[u]))
            pats[(u, n)] = p
            lg[u][n, idx] = rng.uniform(ac.LG_LO, 0.0, size=len(idx)) if lg_of is None else lg_of(rng, u, n, idx)
            counts[st] += int((lg[u][n] >= max(-150.0, prune if prune is not None else -1e300) * LN2).sum())
    c = ac.case(name, mean, var, w, frames, lg, counts, prune=prune)
    c.update(kind='list', T=T, begin=begin, rows=rows, labels=labels, claims=claims, defects=defects, patterns=pats)
    return c


@functools.lru_cache(maxsize=None)
def ragged():
    """Eight utterances, T = 129, 1, 7, 8, 9, 63, 64, 65 and N = 34, 3, 8, 9, 32, 33, 34, 8 rows: one, two and five wave groups of the row
    form, a second 32-row block with one and two rows, rows beyond N in the last group, an exit and an entry row INSIDE the map of the
    N = 33 utterance.  Rows walk the units 0..3 (states 3u .. 3u + 2) again and again, so a state owns several segments inside an utterance
    and across them; the patterns cycle every / none / first / last / every eighth / frames 63-65 along the rows, shifted per utterance."""
    rows = []
    for u, n in enumerate(RAGGED_N):
        units = [(u + k) % 4 for k in range((n + 2) // 3)]
        r = np.concatenate([[ENTRY], unit_rows(units, n - 2), [EXIT]])
        if n == 33:
            r[13], r[14] = EXIT, ENTRY                                   # virtual rows in the middle of the second wave group
        rows.append(r)
    claims = dict(T=RAGGED_T, N=RAGGED_N, wave_groups=[5, 1, 1, 2, 4, 5, 5, 1], row_blocks=[2, 1, 1, 1, 1, 2, 2, 1], inner_virtual_rows=[(5, 13), (5, 14)],
                  patterns=set(PATTERNS), empty_state=EMPTY_STATE, multi_segment_states=True)
    return list_case('ragged', 2601, RAGGED_T, rows, lambda u, n, st: PATTERNS[(n + 2 * u) % 6], claims, ('drop', 'early', 'prev'))


LABELS = [[0], [1, 1], [0, 1, 2, 3, 0, 1, 2, 3, 1, 2], [3, 2, 1, 0, 3, 3, 2, 1, 0, 2, 1]]
LABELS_T = [9, 65, 64, 130]


@functools.lru_cache(maxsize=None)
def labels():
    """The same through Engine.label_batch (pcl_batch_create_labels derives the row maps): labels of 1, 2, 10 and 11 units, N = 5, 8, 32, 35,
    a unit twice in a row and three times in one label."""
    rows = [np.concatenate([[ENTRY], unit_rows(l, 3 * len(l)), [EXIT]]) for l in LABELS]
    claims = dict(T=LABELS_T, N=[5, 8, 32, 35], wave_groups=[1, 1, 4, 5], row_blocks=[1, 1, 1, 2], inner_virtual_rows=[], patterns=set(PATTERNS),
                  empty_state=EMPTY_STATE, multi_segment_states=True)
    return list_case('labels', 2602, LABELS_T, rows, lambda u, n, st: PATTERNS[(n + u) % 6], claims, ('drop', 'early', 'prev'), labels=LABELS)


SCAN_SEGS = [1023, 1025, 2049]


@functools.lru_cache(maxsize=None)
def scan(n_segs):
    """Utterances of T = 4 with three emitting rows each (one with one or two, to reach n_segs): acc_scan_kernel's chunk length per = 1, 2
    and 3.  Survivors in the first and the last segment, on both sides of every multiple of SCAN_THREADS, and in 40 drawn segments."""
    full, rest = divmod(n_segs, 3)
    rows = [np.concatenate([[ENTRY], unit_rows([(u + u // 4) % 4], 3), [EXIT]]) for u in range(full)]
    if rest:
        rows.append(np.concatenate([[ENTRY], unit_rows([1], rest), [EXIT]]))
    probe = dict(mean=np.zeros((LIST_J, 1, 1)), rows=rows)
    segs = segments(probe)
    assert len(segs) == n_segs
    rng = np.random.default_rng(2700 + n_segs)
    want = {0, n_segs - 1} | {k for e in range(SCAN_THREADS, n_segs, SCAN_THREADS) for k in (e - 1, e)} | {int(k) for k in rng.choice(n_segs, 40, replace=False)}
    hot = {(segs[k][1], segs[k][2]): ('every', 'first', 'last')[k % 3] for k in want}
    claims = dict(n_segs=n_segs, per=scan_per(n_segs), kept_segments=sorted(want), T=4)
    return list_case('scan %d' % n_segs, 2700 + n_segs, [4] * len(rows), rows, lambda u, n, st: hot.get((u, n), 'none'), claims, ('per',), empty=None)


PRUNE_T = [9, 65, 40]
PRUNE_LOG2 = -20.0


@functools.lru_cache(maxsize=None)
def prune():
    """Engine.accumulate_prune(-20) inside a ragged batch: state 0 (three segments) holds ONLY frames at thr (1 -+ 1e-12), thr = -20 ln 2,
    kept and dropped in turn, and one frame exactly AT thr (kept: >=); its statistics are 2^-20 of a frame each, nothing larger beside
    them.  The other states keep plain survivors far above the threshold."""
    thr = PRUNE_LOG2 * LN2
    rows = [np.concatenate([[ENTRY], unit_rows(l, 3 * len(l)), [EXIT]]) for l in ([0, 1], [2, 0, 3], [1, 0])]

    def lg_of(rng, u, n, idx):
        if rows[u][n] != 0:
            return rng.uniform(ac.LG_LO, 0.0, size=len(idx))
        v = np.where(idx % 2 == 0, thr * (1.0 - 1e-12), thr * (1.0 + 1e-12))
        v[idx == 8] = thr
        return v
    claims = dict(T=PRUNE_T, thr=thr, state=0, kept=5 + 33 + 20, at_thr=3)
    return list_case('prune', 2800, PRUNE_T, rows, lambda u, n, st: 'every' if st == 0 else PATTERNS[(n + u) % 6], claims, ('gt', 'drop'), prune=PRUNE_LOG2, lg_of=lg_of, empty=None)


def list_cases():
    out = [('ragged', ragged), ('labels', labels)]
    out += [('scan-%d' % n, functools.partial(scan, n)) for n in SCAN_SEGS]
    return out + [('prune', prune)]


# ------------------------------------------------------------------ model shapes for the two kernels: one all-state utterance
def shape_case(name, mean, var, w, frames, lg, counts, claims, **kw):
    J, F = mean.shape[0], frames.shape[0]
    c = ac.case(name, mean, var, w, frames, lg, counts, **kw)
    c.update(kind='shape', T=np.array([F], dtype=np.int32), begin=np.zeros(1, dtype=np.int64),
             rows=[np.concatenate([[ENTRY], np.arange(J), [EXIT]]).astype(np.int32)], labels=None, claims=claims, defects=())
    return c


SHAPE_M = [1, 33, 224, 255, 256, 257, 288]
SHAPE_COUNTS = [3, 33, 65]


@functools.lru_cache(maxsize=None)
def mixtures(M):
    """D = 13, states of 3, 33 and 65 survivors (a chunk of three frames; FC + 1; 2 FC + 1): 7, 8 and 9 m-tiles around AW = 8 (the second
    MFMA32 slice holds one live wave and seven dead ones), the direct form's second slice with 4 (M = 257: Mpad = 260) and 32 live lanes."""
    rng = np.random.default_rng(2900 + M)
    mean, var, w = ac.model(3, M, 13, 2900 + M)
    t = tilings(M)
    claims = dict(padded_D=13, route3=3, **t)
    return shape_case('shape mixtures M=%d' % M, mean, var, w, ac.draw_frames(rng, mean, var, 80), ac.scatter(rng, 80, SHAPE_COUNTS), SHAPE_COUNTS, claims)


WIDE = [(1793, 8), (1793, 9), (2048, 8), (2048, 9)]
WIDE_COUNTS = [3, 40, 0, 1, 33, 32, 31, 2, 5]


@functools.lru_cache(maxsize=None)
def wide(M, J):
    """D = 13, 40 frames, M = 1793 (57 m-tiles: the eighth slice has one live wave) and 2048 (64): nslice == 8, the block map
    w = (b & 7) + 8 (b >> 6) on a grid rounded up to eight states; at J = 9 the second block of eight has one live state."""
    rng = np.random.default_rng(3000 + M + J)
    mean, var, w = ac.model(J, M, 13, 3000 + M)
    t = tilings(M)
    claims = dict(padded_D=13, route3=3, grid=len(mfma32_blocks(M, J)), dead_blocks=sum(b is None for b in mfma32_blocks(M, J)), **t)
    return shape_case('shape wide M=%d J=%d' % (M, J), mean, var, w, ac.draw_frames(rng, mean, var, 40), ac.scatter(rng, 40, WIDE_COUNTS[:J]), WIDE_COUNTS[:J], claims)


SHAPE_D = [13, 14, 39, 40, 47, 48, 50, 64]
DIM_COUNTS = [3, 33, 0, 65]


@functools.lru_cache(maxsize=None)
def dims(D):
    """M = 33 (Mpad = 36: three padded lanes in the direct form, two m-tiles), host dimensions on and just beyond every instance:
    13 -> 13, 14 -> 26, 39 -> 39, 40 -> 47, 47 -> 47 (matrix pipe under variant 3), 48 -> 48, 50 -> 64, 64 -> 64 (direct form on every route)."""
    rng = np.random.default_rng(3100 + D)
    mean, var, w = ac.model(len(DIM_COUNTS), 33, D, 3100 + D)
    claims = dict(padded_D=device_dim(D), route3=route(3, 'f32', D), **tilings(33))
    return shape_case('shape dims D=%d' % D, mean, var, w, ac.draw_frames(rng, mean, var, 96), ac.scatter(rng, 96, DIM_COUNTS), DIM_COUNTS, claims)


SPLIT_STATE, SPLIT_MIX, SPLIT_M = 1, (2, 68), 70


@functools.lru_cache(maxsize=None)
def split():
    """D = 39, M = 70 (three m-tiles, the last of six mixtures): state 1 has one off-pipe mixture in its first and one in its last tile
    (tight and off centre: LOG2E 39 (1.5)^2 / (2 0.25) ~ 250 > 96); the subset launch adds them to what the matrix pipe left."""
    rng = np.random.default_rng(3200)
    mean, var, w = ac.model(3, SPLIT_M, 39, 3200)
    for m in SPLIT_MIX:
        mean[SPLIT_STATE, m] = mean[SPLIT_STATE].mean(axis=0) + 1.5 * rng.choice([-1.0, 1.0], size=39)
        var[SPLIT_STATE, m] = 0.25
    frames = ac.draw_frames(rng, mean, var, 80)
    lg = ac.scatter(rng, 80, [33, 65, 3])
    own = ac.survivors(dict(lgamma=lg, prune=None), SPLIT_STATE)[:16]  # some of the state's survivors sit on the off-pipe mixtures
    frames[own] = mean[SPLIT_STATE, np.resize(SPLIT_MIX, 16)] + 0.5 * rng.standard_normal((16, 39))
    claims = dict(padded_D=39, route3=3, split={SPLIT_STATE: SPLIT_MIX}, order=[0, 1, 2], **tilings(SPLIT_M))
    return shape_case('shape split', mean, var, w, frames, lg, [33, 65, 3], claims, split={SPLIT_STATE: SPLIT_MIX})


ILL_STATE, ILL_M = 1, 6


@functools.lru_cache(maxsize=None)
def ill():
    """D = 13, M = 6: every mixture of state 1 is tight (variance 0.25) and two units off the state's centre in every dimension, signs
    balanced per dimension (LOG2E 13 . 4 / 0.5 = 150 > 96): more than half of its mixtures are off the pipe, so the whole state goes to
    the direct form BEHIND states 0 and 2 -- the accumulate order is 0, 2, 1.  Its survivors are frames drawn from the state itself."""
    rng = np.random.default_rng(3300)
    mean, var, w = ac.model(3, ILL_M, 13, 3300)
    centre = mean[ILL_STATE].mean(axis=0)
    signs = np.stack([rng.permutation(np.repeat([-1.0, 1.0], ILL_M // 2)) for _ in range(13)], axis=1)
    mean[ILL_STATE], var[ILL_STATE] = centre + 2.0 * signs, 0.25
    st = rng.integers(0, 3, 80)
    st[:40] = ILL_STATE
    frames = ac.draw_frames(rng, mean, var, 80, states=st)
    lg = ac.scatter(rng, 80, [33, 0, 3])
    idx = np.sort(rng.choice(40, size=33, replace=False))
    lg[1 + ILL_STATE, idx] = rng.uniform(ac.LG_LO, 0.0, size=33)
    claims = dict(padded_D=13, route3=3, order=[0, 2, 1], valu_states=[ILL_STATE], **tilings(ILL_M))
    return shape_case('shape ill', mean, var, w, frames, lg, [33, 33, 3], claims)


def shape_cases():
    out = [('mixtures-M%d' % m, functools.partial(mixtures, m)) for m in SHAPE_M]
    out += [('wide-M%d-J%d' % mj, functools.partial(wide, *mj)) for mj in WIDE]
    out += [('dims-%d' % d, functools.partial(dims, d)) for d in SHAPE_D]
    return out + [('split', split), ('ill', ill)]


def all_cases():
    return list_cases() + shape_cases()


N_CASES = 6 + 7 + 4 + 8 + 2
