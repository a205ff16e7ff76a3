"""Phonetic decision tree on the device (row f16; csrc/tree_cluster.hip: pcl_tree_zero, pcl_tree_accumulate, pcl_batch_accumulate_tree,
pcl_tree_stats_download / _upload, pcl_tree_build; Engine.tree_*, Batch.accumulate_tree) against the NumPy twin of the rule
(tests/_tree_twin.py, whose own invariants and the cases' separation tests/test_tree_twin.py holds).

Bounds.  Statistics of frames on the grid k 2^-6, |x| < 8: every sum is exact in float64, so n, s, q are the twin's bit for bit in any
order.  Gaussian frames: n exact, |s - s_twin| <= (n - 1) 2^-53 sum |x| per entry and likewise q with sum x^2 -- the first-order bound
of ANY order of n - 1 rounded additions against the twin's sequential one -- and two runs the same bits.  Build: the tree arrays equal
the twin's (the cases are separated by 1e-9 B at every decision); every split gain within 64 * 2^-52 * B of the twin's, B = 0.5 sum over
(yes, no, leaf) of n (D (1 + ln 2 pi) + sum_d |ln v_d|): equal statistics give v bit for bit, only ln may differ by an ulp a term.
Install: bit for bit.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _tree_cases as tc
import _tree_twin as tw

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -3
CASES = tc.build_cases()
_BUILT = {}


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def built(name):
    if name not in _BUILT:
        c = CASES[name]
        _BUILT[name] = tw.build(c['n'], c['s'], c['q'], c['event_ctx'], c['P'], c['n_units'], c['q_member'], c['R0'], c['root_of'], c['min_count'],
                                c['min_gain'], c['max_leaves'], c['var_floor'])
    return _BUILT[name]


def exact(tag, got, t):
    n, s, q = got
    print('%s: n sum %d (twin %d), s and q differ from the twin in %d and %d entries' % (tag, n.sum(), t['n'].sum(), (s != t['s']).sum(), (q != t['q']).sum()))
    assert n.dtype == np.int64 and np.array_equal(n, t['n'])
    assert same_bits(s, t['s']) and same_bits(q, t['q'])


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize('kind', ['f32', 'f64'])
@pytest.mark.parametrize('D', [1, 13, 39, 40, 48])
def test_statistics_exact_on_the_grid(eng, monkeypatch, D, kind):
    monkeypatch.setenv('PCL_TREE_CHUNK', '4')
    frames, T, begin, frame_row, R = tc.frames_case(D)
    fr = np.asarray(frames, dtype=np.float32 if kind == 'f32' else np.float64)
    assert np.array_equal(fr.astype(np.float64), frames)         # the grid is exact in float32
    eng.load_frames(fr)
    eng.tree_zero(R)
    assert all(not x.any() for x in eng.tree_stats())
    eng.tree_accumulate(T, begin, frame_row)
    got = eng.tree_stats()
    t = tw.accumulate(tw.zero(R, D), frames, T, begin, frame_row)
    assert t['n'][:6].tolist() == [0, 1, 3, 4, 5, 9]
    exact('tree stats D=%d %s' % (D, kind), got, t)
    eng.tree_zero(R)
    eng.tree_accumulate(T, begin, frame_row)
    assert all(same_bits(x, y) for x, y in zip(got, eng.tree_stats()))          # two runs, the same bytes
    eng.tree_zero(R)                                                            # two calls add up
    eng.tree_accumulate(T[:2], begin[:2], frame_row)
    eng.tree_accumulate(T[2:], begin[2:], frame_row)
    exact('tree stats D=%d %s, two calls' % (D, kind), eng.tree_stats(), t)
    for R_small in (1, 2):
        rows = np.where(frame_row >= 0, frame_row % R_small, -1).astype(np.int32)
        eng.tree_zero(R_small)
        eng.tree_accumulate(T, begin, rows)
        exact('tree stats D=%d %s R=%d' % (D, kind, R_small), eng.tree_stats(), tw.accumulate(tw.zero(R_small, D), frames, T, begin, rows))


@pytest.mark.parametrize('chunk', [None, '7'])
def test_statistics_of_gaussian_frames_within_the_bound(eng, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv('PCL_TREE_CHUNK', chunk)
    D, R, F = 39, 7, 3000
    rng = np.random.default_rng(77)
    frames = rng.standard_normal((F, D)) * 3 + 1
    T, begin = np.array([1400, 1500], dtype=np.int32), np.array([1550, 20], dtype=np.int64)
    frame_row = rng.integers(-1, R, size=F).astype(np.int32)
    frame_row[rng.integers(0, F, size=F // 2)] = 0                # one row with more than half of the frames: several chunks by default too
    eng.load_frames(frames)
    eng.tree_zero(R)
    eng.tree_accumulate(T, begin, frame_row)
    n, s, q = eng.tree_stats()
    t = tw.accumulate(tw.zero(R, D), frames, T, begin, frame_row)
    assert np.array_equal(n, t['n']) and n.max() > 600
    for name, g in (('s', s), ('q', q)):
        bound = np.maximum(t['n'] - 1, 0)[:, None] * 2.0 ** -53 * t[name + 'abs']
        err = np.abs(g - t[name])
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))
        print('tree stats gaussian chunk=%s: %s worst error / bound = %.3e' % (chunk, name, worst))
        assert worst <= 1.0
    eng.tree_zero(R)
    eng.tree_accumulate(T, begin, frame_row)
    assert all(same_bits(x, y) for x, y in zip((n, s, q), eng.tree_stats()))


def test_statistics_from_a_label_batch(eng, monkeypatch):
    """Source (b): four short utterances, one dropped by the drop rule (two frames for four units), one label position skipped with -1.
    The expected map comes from align_segments' own owner map and the labels (every label names a unit once, so the owner unit IS the
    position); the frames are on the grid, so the sums are exact."""
    from poccala_amd import PCL_F64, synth
    from poccala_amd.AcousticModel.ContextTree import triphone_events
    monkeypatch.setenv('PCL_TREE_CHUNK', '4')
    S, n_units, D, M = 5, 5, 13, 2
    P = S - 2
    labels = [[0, 1, 2], [3, 1], [0, 1, 2, 3], [4, 0, 2]]
    T = np.array([40, 25, 2, 33], dtype=np.int32)
    begin = np.array([70, 5, 40, 120], dtype=np.int64)
    F = 160
    rng = np.random.default_rng(5)
    mean, var, w, _ = synth.make_model(n_units, M, D, seed=41, s=S)
    frames = rng.standard_normal((F, D))
    for lab, t, b in zip(labels, T, begin):
        st = (np.asarray(lab)[:, None] * P + np.arange(P)[None, :]).reshape(-1)
        st = st[np.arange(t) * len(st) // max(int(t), 1)]
        frames[b:b + t] = mean[st, 0] * 4 + np.sqrt(var[st, 0]) * rng.standard_normal((t, D))
    frames = np.clip(np.round(frames * 64) / 64, -7.984375, 7.984375)
    eng.load_model(mean * 4, var, w)
    eng.load_units(np.stack([synth.random_left_right_transmat(rng, S) for _ in range(n_units)]))
    eng.load_frames(frames)
    b = eng.label_batch([np.asarray(l, dtype=np.int32) for l in labels], T, begin)
    b.score(PCL_F64)
    b.viterbi()
    seg, dropped, state = b.align_segments(want_map=True)
    seg.close()
    print('tree stats from a batch: dropped %s' % (dropped,))
    assert dropped == [2]
    event_ctx, label_event = triphone_events(labels, n_units)
    label_event = label_event.copy()
    off = np.concatenate([[0], np.cumsum([len(l) for l in labels])])
    label_event[off[0] + 1] = -1                                   # utterance 0, position 1: its frames are skipped
    R = len(event_ctx) * P
    frame_row = np.full(F, -1, dtype=np.int32)
    for u, lab in enumerate(labels):
        for t in range(begin[u], begin[u] + T[u]):
            if state[t] >= 0:
                ev = label_event[off[u] + lab.index(state[t] // P)]
                if ev >= 0:
                    frame_row[t] = ev * P + state[t] % P
    assert (frame_row >= 0).sum() > 60 and (frame_row[begin[0]:begin[0] + T[0]] < 0).any() and (frame_row[begin[2]:begin[2] + 2] < 0).all()
    eng.tree_zero(R)
    b.accumulate_tree(label_event)
    t = tw.accumulate(tw.zero(R, D), frames, T, begin, frame_row)
    exact('tree stats from a batch', eng.tree_stats(), t)
    b.accumulate_tree(label_event)                                # additive
    exact('tree stats from a batch, twice', eng.tree_stats(), tw.accumulate(t, frames, T, begin, frame_row))
    before = eng.tree_stats()
    bad = label_event.copy()
    bad[3] = len(event_ctx)
    with pytest.raises(Exception) as ei:
        b.accumulate_tree(bad)
    assert ei.value.code == INVALID and 'label_event[3]' in str(ei.value)
    assert all(same_bits(x, y) for x, y in zip(before, eng.tree_stats()))
    b.close()


# ------------------------------------------------------------------ build
def drive(eng, c, **kw):
    eng.load_frames(np.zeros((4, c['D'])))
    eng.tree_zero(len(c['n']))
    eng.tree_stats_load(c['n'], c['s'], c['q'])
    p = dict(min_count=c['min_count'], min_gain=c['min_gain'], max_leaves=c['max_leaves'], var_floor=c['var_floor'])
    p.update(kw)
    return eng.tree_build(c['event_ctx'], c['P'], c['n_units'], c['q_member'], c['root_of'], n_roots=c['R0'], **p)


def hold_tree(tag, tree, t):
    print('%s: %d nodes, %d states (twin %d, %d)' % (tag, tree.n_nodes, tree.n_states, len(t['node_cand']), int((t['node_state'] >= 0).sum())))
    for f in ('node_cand', 'node_child', 'node_state', 'node_n', 'row_state', 'leaf_n'):
        assert same_bits(getattr(tree, f), t[f]), f
    assert same_bits(tree.leaf_s, t['leaf_s']) and same_bits(tree.leaf_q, t['leaf_q'])
    assert tree.split_gain.shape == t['split_gain'].shape
    if len(t['split_gain']):
        err, bound = np.abs(tree.split_gain - t['split_gain']), 64 * 2.0 ** -52 * t['gain_B']
        print('%s: split gains, worst error / bound = %.3e' % (tag, float(np.max(err / bound))))
        assert (err <= bound).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_build_is_the_twins(eng, name):
    c = CASES[name]
    tree = drive(eng, c)
    hold_tree('tree build %s' % name, tree, built(name))
    again = drive(eng, c)
    assert same_bits(tree.split_gain, again.split_gain) and same_bits(tree.node_cand, again.node_cand)


def test_build_end_to_end_from_frames(eng, monkeypatch):
    monkeypatch.setenv('PCL_TREE_CHUNK', '4')
    D, P, n_units = 13, 1, 4
    frames, T, begin, frame_row, R = tc.frames_case(D)
    event_ctx = tc.all_events(n_units)[:R]
    q_member = tc.member([{u} for u in range(n_units + 1)] + [{0, 1}], n_units)
    root_of = np.arange(n_units, dtype=np.int32)
    eng.load_frames(frames)
    eng.tree_zero(R)
    eng.tree_accumulate(T, begin, frame_row)
    tree = eng.tree_build(event_ctx, P, n_units, q_member, root_of, min_count=3, max_leaves=12, var_floor=1e-3)
    st = tw.accumulate(tw.zero(R, D), frames, T, begin, frame_row)
    t = tw.build(st['n'], st['s'], st['q'], event_ctx, P, n_units, q_member, n_units, root_of, 3, 0.0, 12, 1e-3)
    assert all(d['thr'] >= 1e-9 and d.get('sep', 1.0) >= 1e-9 for d in t['decisions'])
    hold_tree('tree build from frames', tree, t)


# ------------------------------------------------------------------ install
def test_install_is_the_twins_model_and_trains(eng):
    from poccala_amd import PCL_F64, synth
    from poccala_amd.engine import embedded_row_states, embedded_structure, make_sentence_batch
    c, t = CASES['shared_root'], built('shared_root')
    S = c['P'] + 2
    rng = np.random.default_rng(3)
    labels = [[0, 3, 1], [2, 2, 0, 1]]
    T, begin = np.array([30, 41], dtype=np.int32), np.array([0, 30], dtype=np.int64)
    frames = rng.standard_normal((71, c['D']))
    trans = np.stack([synth.random_left_right_transmat(rng, S) for _ in range(c['n_units'])])
    eng.load_frames(frames)
    eng.load_units(trans)
    eng.tree_zero(len(c['n']))
    eng.tree_stats_load(c['n'], c['s'], c['q'])
    stats = eng.tree_stats()
    tree = eng.tree_build(c['event_ctx'], c['P'], c['n_units'], c['q_member'], c['root_of'], n_roots=c['R0'], min_count=c['min_count'],
                          min_gain=c['min_gain'], max_leaves=c['max_leaves'], var_floor=c['var_floor'], install=True)
    hold_tree('tree install', tree, t)
    mean, var, w = tw.seed_model(t, c['var_floor'])
    got = eng.model_download()
    print('tree install: model (%d, %d, %d), differs from the twin in %d / %d / %d entries' % (eng.J, eng.M, eng.D, (got[0] != mean).sum(),
                                                                                           (got[1] != var).sum(), (got[2] != w).sum()))
    assert (eng.J, eng.M, eng.D) == (tree.n_states, 1, c['D'])
    assert same_bits(got[0], mean) and same_bits(got[1], var) and same_bits(got[2], w)
    assert all(same_bits(x, y) for x, y in zip(stats, eng.tree_stats()))        # the tree statistics are untouched
    assert same_bits(eng.frames_download(np.float64), frames)

    def lnb():
        b = eng.all_state_batch(np.array([71], dtype=np.int32), np.array([0], dtype=np.int64))
        b.score(PCL_F64)
        out = b.get('B')[0]
        b.close()
        return out
    b_installed = lnb()
    eng.load_model(mean, var, w)
    assert same_bits(b_installed, lnb())                          # as an upload of the same arrays
    # tied-state batches: make_sentence_batch(unit_state_ids=) against set_states by hand
    ids = [tree.unit_state_ids(l) for l in labels]
    assert all(i.max() < tree.n_states for i in ids)
    b1, n1 = make_sentence_batch(eng, labels, T, begin, trans, S, unit_state_ids=ids)
    b2 = eng.batch(n1, T, begin)
    with np.errstate(divide='ignore'):
        sa = [embedded_structure(len(l), [trans[i] for i in l], S) for l in labels]
        b2.set_transitions([np.log(a) for a, _ in sa], [np.log(pi) for _, pi in sa])
    b2.set_states([embedded_row_states(i, S) for i in ids])
    logp = []
    for b in (b1, b2):
        b.score(PCL_F64)
        b.forward_backward()
        logp.append(np.asarray(b.get('logp')))
    print('tree install: tied batches logp %s' % (logp[0].tolist(),))
    assert np.isfinite(logp[0]).all() and same_bits(logp[0], logp[1])
    b1.close()
    b2.close()
    eng.mixup(2)                                                  # the chain that grows the seed model goes on from here
    assert eng.M == 2 and eng.model_download()[0].shape == (tree.n_states, 2, c['D'])


def test_install_is_refused_for_an_empty_leaf(eng):
    c, t = CASES['zero_root'], built('zero_root')
    rng = np.random.default_rng(4)
    eng.load_model(rng.standard_normal((3, 2, c['D'])), np.ones((3, 2, c['D'])), np.full((3, 2), 0.5))
    before = eng.model_download()
    hold_tree('tree zero_root', drive(eng, c), t)
    empty = int(np.flatnonzero(t['node_n'][:c['R0']] == 0)[0])
    with pytest.raises(Exception) as ei:
        drive(eng, c, install=True)
    print('tree install refused: %s' % ei.value)
    assert ei.value.code == INVALID and 'node %d ' % empty in str(ei.value)
    assert (eng.J, eng.M) == (3, 2) and all(same_bits(x, y) for x, y in zip(before, eng.model_download()))


# ------------------------------------------------------------------ refusals
def refused(eng, code, text, call):
    """`call` returns `code` with `text` in pcl_last_error and leaves the resident statistics and the model as they were."""
    stats = eng.tree_stats() if eng._tree_shape()[0] else None
    model = eng.model_download() if eng.J else None
    with pytest.raises(Exception) as ei:
        call()
    print('refused (%d): %s' % (ei.value.code, ei.value))
    assert ei.value.code == code and text in str(ei.value)
    if stats is not None:
        assert all(same_bits(x, y) for x, y in zip(stats, eng.tree_stats()))
    if model is not None:
        assert all(same_bits(x, y) for x, y in zip(model, eng.model_download()))


def test_refusals(eng):
    c = CASES['q1']
    D, R = c['D'], len(c['n'])
    rng = np.random.default_rng(8)
    lib, ctx = eng._lib, eng._ctx
    T, begin = np.array([5, 5], dtype=np.int32), np.array([0, 6], dtype=np.int64)
    rows = np.zeros(12, dtype=np.int32)
    assert lib.pcl_tree_zero(ctx, 4) == STATE and b'no frames' in lib.pcl_last_error(ctx)
    eng.load_frames(rng.standard_normal((12, D)))
    for call in (lambda: eng.tree_accumulate(T, begin, rows), eng.tree_stats, lambda: drive_build(eng, c)):
        refused(eng, STATE, 'no statistics', call)
    refused(eng, INVALID, 'R = 0', lambda: eng.tree_zero(0))
    refused(eng, INVALID, 'rows', lambda: eng.tree_zero(2 ** 32 // (8 * (2 * D + 1)) + 1))
    eng.load_model(rng.standard_normal((2, 1, D)), np.ones((2, 1, D)), np.ones((2, 1)))
    eng.tree_zero(R)
    eng.tree_stats_load(c['n'], c['s'], c['q'])
    bad = rows.copy()
    bad[7] = R
    refused(eng, INVALID, 'frame_row[7]', lambda: eng.tree_accumulate(T, begin, bad))
    bad[7] = -2
    refused(eng, INVALID, 'frame_row[7]', lambda: eng.tree_accumulate(T, begin, bad))
    refused(eng, INVALID, 'overlap', lambda: eng.tree_accumulate(T, np.array([0, 4], dtype=np.int64), rows))
    n_bad, s_bad = c['n'].copy(), c['s'].copy()
    n_bad[1] = -1
    s_bad[2, 0] = np.inf
    refused(eng, INVALID, 'negative', lambda: eng.tree_stats_load(n_bad, c['s'], c['q']))
    refused(eng, INVALID, 'not finite', lambda: eng.tree_stats_load(c['n'], s_bad, c['q']))
    ev = c['event_ctx']

    def build(**kw):
        a = dict(event_ctx=ev, P=c['P'], n_units=c['n_units'], q_member=c['q_member'], root_of=c['root_of'], n_roots=c['R0'], install=True)
        a.update(kw)
        return lambda: eng.tree_build(**a)
    refused(eng, INVALID, 'events', build(event_ctx=ev[:-1]))                                    # E P != R
    e2 = ev.copy()
    e2[3, 0] = c['n_units'] + 1
    refused(eng, INVALID, 'event 3', build(event_ctx=e2))
    e2 = ev.copy()
    e2[3, 1] = c['n_units']
    refused(eng, INVALID, 'event 3', build(event_ctx=e2))
    r2 = c['root_of'].copy()
    r2[1] = c['R0']
    refused(eng, INVALID, 'root_of[1]', build(root_of=r2))
    refused(eng, INVALID, 'maps to root', build(n_roots=c['R0'] + 1))
    refused(eng, INVALID, 'Q = 0', build(q_member=np.zeros((0, c['n_units'] + 1), dtype=np.uint8)))
    refused(eng, INVALID, 'Q = 1366', build(q_member=np.zeros((1366, c['n_units'] + 1), dtype=np.uint8)))
    refused(eng, INVALID, 'max_leaves', build(max_leaves=c['R0'] - 1))
    for g in (-1.0, np.nan, np.inf):
        refused(eng, INVALID, 'min_gain', build(min_gain=g))
    for v in (0.0, -1.0, np.nan):
        refused(eng, INVALID, 'var_floor', build(var_floor=v))
    refused(eng, INVALID, 'min_count', build(min_count=0))
    eng.load_frames(rng.standard_normal((12, D + 1)))                                            # the width changed since tree_zero
    refused(eng, STATE, 'dimension', lambda: eng.tree_accumulate(T, begin, rows))
    refused(eng, STATE, 'dimension', build())


def test_refusals_of_the_batch_entry(eng):
    """pcl_batch_accumulate_tree refuses, in this order, what both accumulate entries refuse of the context (no statistics, the frame
    width changed), then what pcl_batch_align_segments refuses of the batch (not label-built, no Viterbi pass, an inventory that no
    longer fits), then its own argument (an event outside [-1, E)).  Every refusal leaves statistics and model as they were; a good call
    in between shows that it left the batch usable too.  "No frames" cannot be reached with a batch: statistics exist only after a
    pcl_tree_zero, which needs frames, and frames are replaced, never dropped -- the entry asks for statistics first."""
    from poccala_amd import PCL_F64, synth
    from poccala_amd.AcousticModel.ContextTree import triphone_events
    S, n_units, D = 5, 3, 13
    P = S - 2
    labels = [[0, 1], [2, 0, 1]]
    T, begin = np.array([20, 25], dtype=np.int32), np.array([0, 20], dtype=np.int64)
    rng = np.random.default_rng(9)
    mean, var, w, _ = synth.make_model(n_units, 1, D, seed=43, s=S)
    frames = rng.standard_normal((45, D))
    eng.load_model(mean, var, w)
    eng.load_units(np.stack([synth.random_left_right_transmat(rng, S) for _ in range(n_units)]))
    eng.load_frames(frames)
    event_ctx, label_event = triphone_events(labels, n_units)
    E, R = len(event_ctx), len(event_ctx) * P
    b = eng.label_batch([np.asarray(l, dtype=np.int32) for l in labels], T, begin)
    refused(eng, STATE, 'no statistics', lambda: b.accumulate_tree(label_event))
    eng.tree_zero(R)
    eng.tree_accumulate(T, begin, rng.integers(-1, R, size=45).astype(np.int32))               # something to leave unchanged
    assert eng.tree_stats()[0].sum() > 20
    refused(eng, STATE, 'pcl_batch_viterbi first', lambda: b.accumulate_tree(label_event))
    hb = eng.batch(np.array([P * len(l) + 2 for l in labels], dtype=np.int32), T, begin)
    refused(eng, STATE, 'not created from labels', lambda: hb.accumulate_tree(label_event))
    hb.close()
    b.score(PCL_F64)
    b.viterbi()
    for at, value in ((2, -2), (4, E), (0, -(2 ** 31))):
        bad = label_event.copy()
        bad[at] = value
        refused(eng, INVALID, 'label_event[%d] = %d' % (at, value), lambda: b.accumulate_tree(bad))
    with pytest.raises(ValueError):
        b.accumulate_tree(label_event[:-1])
    n0 = int(eng.tree_stats()[0].sum())
    b.accumulate_tree(label_event)
    print('batch entry after its refusals: %d frames added' % (int(eng.tree_stats()[0].sum()) - n0))
    assert n0 < int(eng.tree_stats()[0].sum()) <= n0 + 45
    eng.load_model(rng.standard_normal((n_units * P + 1, 1, D)), np.ones((n_units * P + 1, 1, D)), np.ones((n_units * P + 1, 1)))
    refused(eng, INVALID, 'GMM states', lambda: b.accumulate_tree(label_event))
    eng.load_model(mean, var, w)
    eng.tree_zero(R + 1)
    refused(eng, INVALID, 'no multiple', lambda: b.accumulate_tree(label_event))
    eng.load_frames(rng.standard_normal((45, D + 1)))                                            # the width changed since tree_zero
    refused(eng, STATE, 'dimension', lambda: b.accumulate_tree(label_event))
    b.close()


def test_a_refused_batch_entry_leaves_the_batch_to_the_other_owner_map_pass(eng):
    """pcl_batch_accumulate_tree and pcl_batch_align_segments make the same owner map of the batch's paths.  A call of the first that is
    refused for its own argument says so in these words, and the next call on the same batch -- the other pass -- makes the whole map;
    the tree pass then counts exactly the frames that map gives an owner."""
    from poccala_amd import PCL_F64, synth
    from poccala_amd.AcousticModel.ContextTree import triphone_events
    S, n_units, D = 5, 2, 13
    P = S - 2
    labels = [[0], [1, 0]]
    T, begin, F = np.array([8, 12], dtype=np.int32), np.array([0, 8], dtype=np.int64), 20
    rng = np.random.default_rng(10)
    mean, var, w, _ = synth.make_model(n_units, 2, D, seed=44, s=S)
    eng.load_model(mean, var, w)
    eng.load_units(np.stack([synth.random_left_right_transmat(rng, S) for _ in range(n_units)]))
    eng.load_frames(rng.standard_normal((F, D)))
    event_ctx, label_event = triphone_events(labels, n_units)
    E = len(event_ctx)
    assert (label_event >= 0).all()
    eng.tree_zero(E * P)
    b = eng.label_batch([np.asarray(l, dtype=np.int32) for l in labels], T, begin)
    b.score(PCL_F64)
    b.viterbi()
    bad = label_event.copy()
    bad[1] = E
    refused(eng, INVALID, 'pcl_batch_accumulate_tree: label_event[1] = %d is neither -1 nor an event in [0, %d)' % (E, E), lambda: b.accumulate_tree(bad))
    seg, dropped, state = b.align_segments(want_map=True)
    kept = int((state >= 0).sum())
    print('owner map after the refusal: %d of %d frames kept, dropped %s' % (kept, F, dropped))
    assert state.shape == (F,) and int(seg.counts.sum()) == kept and 0 < kept <= F and (state < n_units * P).all()
    seg.close()
    b.accumulate_tree(label_event)
    assert int(eng.tree_stats()[0].sum()) == kept
    b.close()


def drive_build(eng, c):
    return eng.tree_build(c['event_ctx'], c['P'], c['n_units'], c['q_member'], c['root_of'], n_roots=c['R0'])
