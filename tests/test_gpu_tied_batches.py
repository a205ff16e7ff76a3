"""Resident tying and label-built batches over tied states on the device (row f17; csrc/tying.hip: pcl_tying_upload / _drop / _lookup,
pcl_batch_create_labels_tied, pcl_batch_get_states, and the label-based entry points on a tied batch) against the NumPy twin
(tests/_tied_twin.py; tests/test_tied_twin.py proves on the CPU that its trees and corpora reach the edges they claim) and against the
host-built route (Tree.unit_state_ids + make_sentence_batch(unit_state_ids=)).

Every result is an integer or comes from the same kernels on the same inputs, so every comparison is for equality, bit for bit -- as
tests/test_gpu_units.py::test_label_batch_equals_host_built_batch holds the monophone label batch to its host-built twin."""
import copy

import numpy as np
import pytest

import _tied_twin as tt

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -3
D = 13
NU = tt.N_UNITS


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def unit_trans(S, seed=3):
    from poccala_amd import synth
    rng = np.random.default_rng(seed)
    return np.stack([synth.random_left_right_transmat(rng, S) for _ in range(NU)])


def device_built(eng, P):
    c = tt.build_case(P)
    eng.load_frames(np.zeros((4, c['D'])))
    eng.tree_zero(len(c['n']))
    eng.tree_stats_load(c['n'], c['s'], c['q'])
    return eng.tree_build(c['event_ctx'], P, NU, c['q_member'], c['root_of'], n_roots=c['R0'], min_count=c['min_count'], min_gain=c['min_gain'],
                          max_leaves=c['max_leaves'], var_floor=c['var_floor'])


def frames_along(rng, F, labels, T, begin, pos_states, mean, var):
    """Rows of an utterance walk through the tied states of its label, mixture 0 of each; rows nobody owns are noise"""
    fr = rng.standard_normal((F, D)) * 3
    for lab, t, b, ps in zip(labels, T, begin, pos_states):
        st = ps.reshape(-1)
        st = st[np.arange(t) * len(st) // max(int(t), 1)]
        fr[b:b + t] = mean[st, 0] + np.sqrt(var[st, 0]) * rng.standard_normal((int(t), D))
    return fr


def resident(eng, tree, S, M, labels, T, begin, F, seed):
    """Units, a (J_t, M, D) model, frames that follow the labels' tied states, and the tying: everything a tied batch needs"""
    trans = unit_trans(S)
    model = tt.model_for(tree.n_states, M, D, seed)
    rng = np.random.default_rng(seed + 1)
    eng.load_units(trans)
    eng.load_model(*model)
    eng.load_frames(frames_along(rng, F, labels, T, begin, tt.pos_states(tree, labels), model[0], model[1]))
    eng.load_tying(tree)
    return trans, model


# ------------------------------------------------------------------ 1. lookup
@pytest.mark.parametrize('kind', ['roots', 'chain', 'built'])
@pytest.mark.parametrize('P', [1, 3])
def test_lookup_is_tree_lookup(eng, P, kind):
    tree = tt.roots_only(P) if kind == 'roots' else tt.chain(P) if kind == 'chain' else device_built(eng, P)
    eng.load_units(unit_trans(P + 2))
    eng.load_tying(tree)
    ctx = tt.all_contexts()
    want = tt.lookup_all(tree, ctx)
    got = eng.tying_lookup(ctx)
    print('lookup %s P=%d: %d nodes, %d states, %d contexts, %d entries differ' % (kind, P, tree.n_nodes, tree.n_states, len(ctx), int((got != want).sum())))
    assert got.dtype == np.int32 and got.shape == (len(ctx), P) and np.array_equal(got, want)
    for n in (1, 64, 65, 4097):
        at = (np.arange(n) * 7 + 3) % len(ctx)
        assert np.array_equal(eng.tying_lookup(ctx[at]), want[at]), n
    assert same_bits(got, eng.tying_lookup(ctx))


# ------------------------------------------------------------------ 2. the batch
def run_estep(eng, b):
    from poccala_amd import PCL_F64
    b.score(PCL_F64)
    b.forward_backward()
    b.viterbi()
    out = {w: b.get(w) for w in ('B', 'lgamma', 'ksai', 'gamma', 'pi', 'path', 'logp', 'point')}
    eng.stats_zero()
    b.accumulate(PCL_F64)
    out['stats'] = eng.stats_download()
    return out


def hold_equal(tag, x, y):
    for w in ('B', 'lgamma', 'ksai', 'gamma', 'pi', 'path'):
        assert len(x[w]) == len(y[w]) and all(same_bits(p, q) for p, q in zip(x[w], y[w])), (tag, w)
    for w in ('logp', 'point'):
        assert same_bits(x[w], y[w]), (tag, w)
    assert sorted(x['stats']) == sorted(y['stats']) and all(same_bits(x['stats'][k], y['stats'][k]) for k in x['stats']), (tag, 'stats')


@pytest.mark.parametrize('kind', ['chain', 'built'])
@pytest.mark.parametrize('S', [3, 5])
def test_tied_batch_is_the_host_built_batch(eng, S, kind):
    from poccala_amd.engine import make_sentence_batch
    P = S - 2
    tree = tt.chain(P) if kind == 'chain' else tt.built_twin(P)
    labels, T, begin, F = tt.edge_corpus(seed=S)
    trans, _ = resident(eng, tree, S, 2, labels, T, begin, F, seed=10 + S)
    want_rows = tt.row_states(tree, labels)
    for tag, idx in (('U=70', list(range(len(labels)))), ('U=1', [4])):          # (utterance 4: L = 130)
        lab, t, bg = [labels[u] for u in idx], T[idx], begin[idx]
        ref, n = make_sentence_batch(eng, lab, t, bg, trans, S, unit_state_ids=[tree.unit_state_ids(l) for l in lab])
        b = eng.label_batch([np.asarray(l, dtype=np.int32) for l in lab], t, bg, tied=True)
        rows = b.row_states()
        ndiff = sum(int((r != w).sum()) for r, w in zip(rows, [want_rows[u] for u in idx]))
        print('tied batch S=%d %s %s: %d utterances, %d rows, %d differ from the twin' % (S, kind, tag, len(idx), int(b.N.sum()), ndiff))
        assert np.array_equal(b.N, n) and np.array_equal(b.N, P * np.array([len(l) for l in lab]) + 2)
        assert all(same_bits(r, want_rows[u]) for r, u in zip(rows, idx))
        assert all(same_bits(r, q) for r, q in zip(rows, ref.row_states()))
        assert all(same_bits(p, q) for p, q in zip(b.pos_states(), tt.pos_states(tree, lab)))
        x, y = run_estep(eng, b), run_estep(eng, ref)
        assert tag == 'U=1' or np.isfinite(x['logp']).sum() >= len(idx) // 2
        hold_equal(tag, x, y)
        if tag == 'U=70':
            # another tying becomes resident, then none: the batch keeps the states it was made with
            eng.load_tying(tt.roots_only(P))
            assert not np.array_equal(eng.tying_lookup(tt.all_contexts()), tt.lookup_all(tree, tt.all_contexts()))
            hold_equal('after another tying', run_estep(eng, b), x)
            eng.drop_tying()
            hold_equal('after the drop', run_estep(eng, b), x)
            assert all(same_bits(r, q) for r, q in zip(b.row_states(), rows)) and all(same_bits(p, q) for p, q in zip(b.pos_states(), tt.pos_states(tree, lab)))
            eng.load_tying(tree)
        b.close()
        ref.close()


# ------------------------------------------------------------------ 3. transitions
@pytest.mark.parametrize('S', [3, 5])
def test_transitions_on_a_tied_batch(eng, S):
    from poccala_amd import PCL_F64, synth
    P = S - 2
    tree = tt.built_twin(P)
    labels, T, begin, F = tt.align_corpus()
    T = np.maximum(T, 12)                                           # (every utterance has a path here; they may overlap: nothing below asks for owners)
    labs = [np.asarray(l, dtype=np.int32) for l in labels]
    trans, model = resident(eng, tree, S, 2, labels, T, begin, F + 40, seed=30 + S)

    def em_round(b, emissions=None):
        eng.hmm_acc_zero()
        if emissions is None:
            b.score(PCL_F64)
        else:
            b.set_emissions(emissions)
        b.forward_backward()
        lp0 = np.asarray(b.get('logp')).copy()
        b.accumulate_hmm()
        acc = eng.hmm_acc_download()
        eng.mstep_transitions()
        units = eng.units_download()
        b.refresh_transitions()
        if emissions is None:
            b.score(PCL_F64)
        else:
            b.set_emissions(emissions)
        b.forward_backward()
        return lp0, acc, units, np.asarray(b.get('logp')).copy()

    tied = eng.label_batch(labs, T, begin, tied=True)
    tied.score(PCL_F64)
    B = [x.copy() for x in tied.get('B')]
    t_lp0, t_acc, t_units, t_lp1 = em_round(tied)
    tied.close()
    # the monophone batch of the same labels: the same sentence HMMs, handed the tied batch's emissions
    eng.load_units(trans)
    eng.load_model(*synth.make_model(NU, 2, D, seed=5, s=S)[:3])
    mono = eng.label_batch(labs, T, begin)
    m_lp0, m_acc, m_units, m_lp1 = em_round(mono, B)
    mono.close()
    print('transitions S=%d: ln P(O) before %s\n after %s' % (S, t_lp0.tolist(), t_lp1.tolist()))
    assert np.isfinite(t_lp0).all() and np.isfinite(t_acc[1]).any()
    assert same_bits(t_acc[0], m_acc[0]) and same_bits(t_acc[1], m_acc[1]) and same_bits(t_units, m_units)
    assert same_bits(t_lp0, m_lp0) and same_bits(t_lp1, m_lp1) and (t_lp1 != t_lp0).all()
    assert not same_bits(t_units, trans)


# ------------------------------------------------------------------ 4. owner map, tree and LDA statistics
@pytest.mark.parametrize('S', [3, 5])
def test_owner_map_and_statistics_on_a_tied_batch(eng, S):
    from poccala_amd import PCL_F64
    from poccala_amd.AcousticModel.ContextTree import triphone_events
    P = S - 2
    tree = tt.built_twin(P)
    labels, T, begin, F = tt.align_corpus()
    resident(eng, tree, S, 1, labels, T, begin, F, seed=50 + S)
    b = eng.label_batch([np.asarray(l, dtype=np.int32) for l in labels], T, begin, tied=True)
    b.score(PCL_F64)
    b.viterbi()
    paths = b.get('path')
    want, want_dropped, pos, k = tt.owner_map(tree, paths, labels, S, T, begin, F)
    seg, dropped, state = b.align_segments(want_map=True)
    print('owner map S=%d: dropped %s, %d of %d rows owned, %d entries differ' % (S, dropped, int((want >= 0).sum()), F, int((state != want).sum())))
    assert dropped == want_dropped and 2 in dropped and len(dropped) < len(labels) and state.dtype == np.int32 and np.array_equal(state, want)
    assert (want[:int(begin.min())] == -1).all() and (want[int((begin + T).max()):] == -1).all() and (want[begin[2]:begin[2] + T[2]] == -1).all()
    counts, order = np.asarray(seg.counts), np.asarray(seg.order)
    assert len(counts) == tree.n_states == eng.J and np.array_equal(counts, np.bincount(want[want >= 0], minlength=tree.n_states))
    assert np.array_equal(order, np.concatenate([np.flatnonzero(want == j) for j in range(tree.n_states)]))
    seg2, dropped2, state2 = b.align_segments(want_map=True)                   # twice: the same bytes
    assert dropped2 == dropped and same_bits(state2, state) and same_bits(np.asarray(seg2.order), order)
    seg.close()
    seg2.close()
    # second-pass tree statistics from the context-dependent alignment
    ev, le = triphone_events(labels, NU)
    le = le.copy()
    le[1] = -1
    R = len(ev) * P
    rows = tt.tree_rows(le, labels, P, T, begin, F, pos, k)
    got = []
    for _ in range(2):
        eng.tree_zero(R)
        b.accumulate_tree(le)
        got.append(eng.tree_stats())
    eng.tree_zero(R)
    eng.tree_accumulate(T, begin, rows)
    ref = eng.tree_stats()
    print('tree statistics from the tied batch S=%d: %d frames in %d rows' % (S, int(ref[0].sum()), int((ref[0] > 0).sum())))
    assert ref[0].sum() == (rows >= 0).sum() > 50
    assert all(same_bits(x, y) for x, y in zip(got[0], ref)) and all(same_bits(x, y) for x, y in zip(got[0], got[1]))
    # LDA: the class is the tied state, or state_class[tied state]
    sc = (np.arange(tree.n_states) % 4 - 1).astype(np.int32)
    for state_class, n_classes, cls in ((None, tree.n_states, want), (sc, 3, np.where(want >= 0, sc[np.maximum(want, 0)], -1).astype(np.int32))):
        got = []
        for _ in range(2):
            eng.lda_zero(n_classes, 1, 1)
            b.accumulate_lda(state_class)
            got.append(eng.lda_stats())
        eng.lda_zero(n_classes, 1, 1)
        eng.lda_accumulate(T, begin, cls)
        ref = eng.lda_stats()
        print('LDA statistics from the tied batch S=%d, %d classes: %d rows' % (S, n_classes, int(ref[0].sum())))
        assert ref[0].sum() == (cls >= 0).sum() > 50
        assert all(same_bits(x, y) for x, y in zip(got[0], ref)) and all(same_bits(x, y) for x, y in zip(got[0], got[1]))
    b.close()


# ------------------------------------------------------------------ 5. the chain, end to end
def test_chain_from_monophones_to_trained_tied_states(eng):
    """monophone alignment -> accumulate_tree -> tree_build(install) -> load_tying -> tied label batch -> EM with transitions -> mixup ->
    EM -> align_segments -> k-means + EM on the tied states' segments; the pattern of test_install_is_the_twins_model_and_trains."""
    from poccala_amd import PCL_F64, synth
    from poccala_amd.AcousticModel.ContextTree import questions, triphone_events
    S, P = 5, 3
    rng = np.random.default_rng(8)
    U = 24
    labels = [[int(x) for x in rng.integers(0, NU, size=int(rng.integers(2, 5)))] for _ in range(U)]
    T = rng.integers(28, 41, size=U).astype(np.int32)
    begin = np.concatenate([[0], np.cumsum(T[:-1] + 2)]).astype(np.int64)
    F = int(begin[-1] + T[-1] + 3)
    labs = [np.asarray(l, dtype=np.int32) for l in labels]
    mean, var, w, _ = synth.make_model(NU, 1, D, seed=12, s=S)
    mono_ps = [np.asarray(l)[:, None] * P + np.arange(P)[None, :] for l in labels]
    eng.load_units(unit_trans(S))
    eng.load_model(mean * 4, var, w)
    eng.load_frames(frames_along(rng, F, labels, T, begin, mono_ps, mean * 4, var))
    b = eng.label_batch(labs, T, begin)
    b.score(PCL_F64)
    b.viterbi()
    ev, le = triphone_events(labels, NU)
    eng.tree_zero(len(ev) * P)
    b.accumulate_tree(le)
    b.close()
    n = eng.tree_stats()[0]
    qm = questions([{u} for u in range(NU + 1)] + [{0, 1}, {2, 3, NU}, {1, 4}], NU)
    tree = eng.tree_build(ev, P, NU, qm, np.tile(np.arange(P, dtype=np.int32), NU), min_count=12, max_leaves=P + 9, install=True)
    Jt = tree.n_states
    print('chain: %d frames counted, %d nodes, J_t = %d' % (int(n.sum()), tree.n_nodes, Jt))
    assert n.sum() > 300 and Jt > P and (eng.J, eng.M) == (Jt, 1)
    eng.load_tying(tree)
    tb = eng.label_batch(labs, T, begin, tied=True)
    assert all(same_bits(p, q) for p, q in zip(tb.pos_states(), tt.pos_states(tree, labels)))

    def em():
        eng.stats_zero()
        eng.hmm_acc_zero()
        tb.score(PCL_F64)
        tb.forward_backward()
        lp = np.asarray(tb.get('logp')).copy()
        tb.accumulate(PCL_F64)
        tb.accumulate_hmm()
        eng.mstep()
        eng.mstep_transitions()
        tb.refresh_transitions()
        m = eng.model_download()
        assert np.isfinite(lp).all() and all(np.isfinite(x).all() for x in m) and m[0].shape[0] == Jt == eng.J
        assert np.isfinite(eng.units_download()).all()
        return lp.sum()

    lps = [em(), em()]
    eng.mixup(2)
    assert eng.M == 2 and eng.model_download()[0].shape == (Jt, 2, D)
    lps.append(em())
    print('chain: sum ln P(O) per iteration %s' % (lps,))
    assert np.isfinite(lps).all()
    tb.score(PCL_F64)
    tb.viterbi()
    seg, dropped, state = tb.align_segments(want_map=True)
    want, want_dropped, _, _ = tt.owner_map(tree, tb.get('path'), labels, S, T, begin, F)
    assert dropped == want_dropped and np.array_equal(state, want) and len(dropped) < U and len(np.asarray(seg.counts)) == Jt
    sweeps = seg.kmeans(2, seed=11, precision=PCL_F64)
    iters, q = seg.em(precision=PCL_F64)
    m = eng.model_download()
    print('chain: segments of %d states trained, EM loop bodies %s' % (int((np.asarray(seg.counts) > 0).sum()), np.asarray(iters).tolist()))
    assert m[0].shape == (Jt, 2, D) and all(np.isfinite(x).all() for x in m) and eng.J == Jt
    seg.close()
    tb.close()


# ------------------------------------------------------------------ 6. refusals
def refused(eng, code, text, call, probe=None):
    """`call` returns `code` with `text` in the message and leaves the model and the resident tying (seen through `probe` lookups) as they were"""
    model = eng.model_download() if eng.J else None
    before = eng.tying_lookup(probe) if probe is not None else None
    with pytest.raises(Exception) as ei:
        call()
    print('refused (%d): %s' % (ei.value.code, ei.value))
    assert ei.value.code == code and text in str(ei.value)
    if model is not None:
        assert all(same_bits(x, y) for x, y in zip(model, eng.model_download()))
    if probe is not None:
        assert same_bits(before, eng.tying_lookup(probe))


def test_refusals(eng):
    from poccala_amd import PCL_F64, synth
    S, P = 5, 3
    tree, other = tt.built_twin(P), tt.chain(P)
    labels, T, begin, F = tt.align_corpus()
    labs = [np.asarray(l, dtype=np.int32) for l in labels]
    probe = tt.all_contexts()
    trans = unit_trans(S)
    model = tt.model_for(tree.n_states, 1, D, 70)
    eng.load_units(trans)
    eng.load_model(*model)
    eng.load_frames(np.random.default_rng(1).standard_normal((F, D)))
    refused(eng, STATE, 'no resident tying', lambda: eng.label_batch(labs, T, begin, tied=True))
    refused(eng, STATE, 'no resident tying', lambda: eng.tying_lookup(probe))
    eng.load_tying(tree)
    # a model of another J
    eng.load_model(*tt.model_for(tree.n_states + 1, 1, D, 71))
    refused(eng, STATE, 'tied states', lambda: eng.label_batch(labs, T, begin, tied=True), probe)
    eng.load_model(*model)
    # the monophone entry keeps its refusal on the tied model
    refused(eng, STATE, 'units x %d emitting states need %d' % (P, NU * P), lambda: eng.label_batch(labs, T, begin), probe)

    def broken(f):
        t = copy.deepcopy(other)
        for name in ('node_cand', 'node_child', 'node_state', 'root_of'):
            setattr(t, name, getattr(t, name).copy())
        f(t)
        return t
    inner = int(np.flatnonzero(other.node_cand >= 0)[5])
    leaves = np.flatnonzero(other.node_cand < 0)
    faults = [
        ('children', lambda t: t.node_child.__setitem__((inner, 0), inner)),                  # a child == its parent
        ('children', lambda t: t.node_child.__setitem__((inner, 1), inner - 1)),              # a child < its parent
        ('children', lambda t: t.node_child.__setitem__((inner, 1), t.n_nodes)),
        ('outside [0, %d)' % other.n_states, lambda t: t.node_state.__setitem__(leaves[3], other.n_states)),
        ('named by two leaves', lambda t: t.node_state.__setitem__(leaves[3], t.node_state[leaves[9]])),
        ('candidate', lambda t: t.node_cand.__setitem__(inner, 3 * other.Q)),
        ('root_of', lambda t: t.root_of.__setitem__(4, P)),
        ('root_of', lambda t: t.root_of.__setitem__(0, -1)),
    ]
    for text, f in faults:
        refused(eng, INVALID, text, lambda: eng.load_tying(broken(f), n_roots=other.n_roots), probe)
    refused(eng, INVALID, 'tied states for', lambda: eng.load_tying(other, n_states=other.n_nodes + 1), probe)
    refused(eng, INVALID, 'state positions', lambda: eng.load_tying(tt.chain(1)), probe)                      # P != S - 2
    refused(eng, INVALID, 'n_units', lambda: eng.load_tying(tt.roots_only(P, n_units=NU - 1)), probe)
    refused(eng, INVALID, 'centre %d' % NU, lambda: eng.tying_lookup(np.array([[0, 1, 2], [1, NU, 0]], dtype=np.int32)), probe)
    refused(eng, INVALID, 'neighbours', lambda: eng.tying_lookup(np.array([[0, 1, NU + 1]], dtype=np.int32)), probe)
    refused(eng, INVALID, 'neighbours', lambda: eng.tying_lookup(np.array([[-1, 1, 0]], dtype=np.int32)), probe)
    assert np.array_equal(eng.tying_lookup(probe), tt.lookup_all(tree, probe))                                # the first tying, through all of it
    # a tied batch after the model was replaced by one of another J
    b = eng.label_batch(labs, T, begin, tied=True)
    b.score(PCL_F64)
    b.viterbi()
    eng.load_model(*synth.make_model(NU, 1, D, seed=5, s=S)[:3])
    refused(eng, STATE, 'the model now has %d' % (NU * P), lambda: b.score(PCL_F64), probe)
    refused(eng, INVALID, 'tied states', lambda: b.align_segments(), probe)
    refused(eng, STATE, 'changed since the batch was created', lambda: b.refresh_transitions(), probe)
    eng.load_model(*model)
    seg, dropped = b.align_segments()                                                                         # ... and back: usable again
    seg.close()
    b.close()
    eng.drop_tying()
    eng.drop_tying()                                                                                          # (nothing to drop: no refusal)
    refused(eng, STATE, 'no resident tying', lambda: eng.tying_lookup(probe))


# ------------------------------------------------------------------ 7. C-ABI
def test_new_symbols_are_exported(eng):
    import os
    import re
    from poccala_amd import _lib as L
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'poccala_hip.h')).read()
    for name in ('pcl_tying_upload', 'pcl_tying_drop', 'pcl_tying_lookup', 'pcl_batch_create_labels_tied', 'pcl_batch_get_states'):
        assert re.search(r'\bint %s\(' % name, text), name
        assert hasattr(L.load(), name) and name in L.PROTOTYPES, name
