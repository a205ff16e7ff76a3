"""CPU checks of the decision-tree row (f16): the NumPy twin's own properties (tests/_tree_twin.py), the host helpers of
poccala_amd/AcousticModel/ContextTree.py, make_sentence_batch's unit_state_ids argument, the C-ABI names, and -- for every build case
tests/test_gpu_tree.py runs -- the separation condition: at every decision every candidate of a different partition lies at least
1e-9 B below the winner, and no count-valid candidate lies within 1e-9 B of min_gain.  A case that is not separated FAILS here: no
decision is left uncompared on the device."""
import os

import numpy as np
import pytest

import _tree_cases as tc
import _tree_twin as tw

SEP = 1e-9
CASES = tc.build_cases()
_BUILT = {}


def built(name):
    if name not in _BUILT:
        c = CASES[name]
        _BUILT[name] = tw.build(c['n'], c['s'], c['q'], c['event_ctx'], c['P'], c['n_units'], c['q_member'], c['R0'], c['root_of'], c['min_count'],
                                c['min_gain'], c['max_leaves'], c['var_floor'])
    return _BUILT[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_case_is_separated(name):
    t = built(name)
    for i, d in enumerate(t['decisions']):
        print('%s decision %d: %s' % (name, i, {k: v for k, v in d.items()}))
        if d['kind'] == 'split':
            assert d['sep'] >= SEP, (name, i, d)
        assert d['thr'] >= SEP, (name, i, d)


@pytest.mark.parametrize('name', sorted(CASES))
def test_twin_tree_properties(name):
    c, t = CASES[name], built(name)
    N, R0 = len(t['node_cand']), c['R0']
    leaves = t['node_cand'] < 0
    assert (N - R0) % 2 == 0 and len(t['split_gain']) == (N - R0) // 2
    assert leaves.sum() == R0 + (N - R0) // 2 <= (c['max_leaves'] or 10 ** 9)
    assert np.array_equal(np.sort(t['node_state'][leaves]), np.arange(leaves.sum())) and (np.diff(t['node_state'][leaves]) > 0).all()
    # the leaf counts partition the root counts, node by node
    for i in np.flatnonzero(~leaves):
        no, yes = t['node_child'][i]
        assert t['node_n'][i] == t['node_n'][no] + t['node_n'][yes]
        assert min(t['node_n'][no], t['node_n'][yes]) >= c['min_count']
    assert t['node_n'][:R0].sum() == c['n'].sum() == t['leaf_n'].sum()
    assert np.array_equal(t['leaf_n'], t['node_n'][leaves])
    # the global choice is greedy: the gains are non-increasing in split order only while the split's node was a leaf before the
    # one in front of it -- a child may gain more than its parent did
    node_of_split = np.flatnonzero(~leaves)[np.argsort([t['node_child'][i][0] for i in np.flatnonzero(~leaves)])]
    for k in range(1, len(node_of_split)):
        if node_of_split[k] < R0 + 2 * (k - 1):                   # existed when split k - 1 was chosen
            assert t['split_gain'][k] <= t['split_gain'][k - 1]
    assert (t['split_gain'] >= c['min_gain']).all()
    # every seen context's lookup is its row's state
    tree = tw.as_tree(t, c['P'], c['n_units'], c['event_ctx'], c['q_member'], c['root_of'])
    for e, (l, ce, r) in enumerate(c['event_ctx']):
        for k in range(c['P']):
            assert tree.lookup(l, ce, r, k) == t['row_state'][e * c['P'] + k]
    assert tree.n_states == leaves.sum()


def test_edge_cases_do_what_their_names_say():
    t = built('min_count')
    off = built('min_count_off')
    c = CASES['min_count']
    first = off['decisions'][0]
    no, yes = off['node_child'][first['node']]
    assert min(off['node_n'][no], off['node_n'][yes]) < c['min_count']                     # the best split is the forbidden one
    assert t['decisions'][0]['cand'] != first['cand'] and t['decisions'][0]['gain'] < first['gain']
    assert len(built('max_leaves_r0')['split_gain']) == 0 and len(built('max_leaves_mid')['split_gain']) == 3
    assert len(built('max_leaves_mid')['node_cand']) < len(built('one_row_root')['node_cand'])
    g = built('min_gain')
    assert g['decisions'][-1]['kind'] == 'stop' and len(g['split_gain']) >= 1
    z, cz = built('zero_root'), CASES['zero_root']
    empty = [i for i in range(cz['R0']) if z['node_n'][i] == 0]
    assert len(empty) == 1 and z['node_cand'][empty[0]] < 0
    o, co = built('one_row_root'), CASES['one_row_root']
    assert (o['node_cand'][6:8] < 0).all() and (o['node_n'][6:8] > 0).all()                # centre 3's roots: one row each
    s, cs = built('shared_root'), CASES['shared_root']
    Q = cs['q_member'].shape[0]
    assert cs['R0'] == cs['P']
    assert any(Q <= cnd < 2 * Q for cnd in s['node_cand'])                                   # a centre question wins somewhere
    u, cu = built('unseen_rows'), CASES['unseen_rows']
    assert (cu['n'] == 0).sum() == 5 and (u['row_state'] >= 0).all()
    v, cv = built('var_floor'), CASES['var_floor']
    nn = v['leaf_n'].astype(float)
    assert np.all(v['leaf_q'][:, 0] / nn - (v['leaf_s'][:, 0] / nn) ** 2 < cv['var_floor'])
    b, cb = built('big_leaf'), CASES['big_leaf']
    assert cb['R0'] == 1 and len(cb['n']) == 100 and 3 * cb['q_member'].shape[0] > 8
    d = built('dup_compl')                                        # of equal candidates the lowest wins: never the duplicate, never the complement behind it
    qd = CASES['dup_compl']['q_member'] != 0
    Qd = len(qd)
    behind = {j for j in range(Qd) for i in range(j) if (qd[i] == qd[j]).all() or (qd[i] != qd[j]).all()}
    assert behind == {1, 2, 4, 6}
    assert all(cnd % Qd not in behind for cnd in d['node_cand'] if cnd >= 0)
    assert CASES['q1']['q_member'].shape[0] == 1 and CASES['q65']['q_member'].shape[0] == 65 and CASES['one_unit']['n_units'] == 1


def test_twin_statistics_are_additive_and_sequential():
    frames, T, begin, frame_row, R = tc.frames_case(13)
    st = tw.accumulate(tw.zero(R, 13), frames, T, begin, frame_row)
    assert st['n'][:6].tolist() == [0, 1, 3, 4, 5, 9]
    two = tw.accumulate(tw.accumulate(tw.zero(R, 13), frames, T[:2], begin[:2], frame_row), frames, T[2:], begin[2:], frame_row)
    for k in ('n', 's', 'q'):
        assert np.array_equal(st[k], two[k])                      # the grid: every order agrees
    inside = np.zeros(len(frames), dtype=bool)
    for t, b in zip(T, begin):
        inside[b:b + t] = True
    assert st['n'].sum() == (inside & (frame_row >= 0)).sum() < inside.sum() < len(frames)


def test_helpers_and_tree_round_trip(tmp_path):
    from poccala_amd.AcousticModel.ContextTree import Tree, questions, triphone_events
    ev, le = triphone_events([[0, 1, 0], [1], [0, 1, 0, 1]], 2)
    assert ev.dtype == np.int32 and le.dtype == np.int32
    assert ev.tolist() == [[0, 1, 0], [0, 1, 2], [1, 0, 1], [1, 0, 2], [2, 0, 1], [2, 1, 2]]
    assert le.tolist() == [4, 0, 3, 5, 4, 0, 2, 1]
    with pytest.raises(ValueError):
        triphone_events([[2]], 2)
    q = questions([{0}, [1, 2], ()], 2)
    assert q.dtype == np.uint8 and q.tolist() == [[1, 0, 0], [0, 1, 1], [0, 0, 0]]
    with pytest.raises(ValueError):
        questions([{3}], 2)
    c, t = CASES['shared_root'], built('shared_root')
    tree = tw.as_tree(t, c['P'], c['n_units'], c['event_ctx'], c['q_member'], c['root_of'])
    path = os.path.join(str(tmp_path), 'tree.npz')
    tree.save(path)
    with np.load(path, allow_pickle=False) as z:                  # arrays only
        assert all(z[k].dtype != object for k in z.files)
    back = Tree.load(path)
    assert back.P == tree.P and back.n_units == tree.n_units
    for f in Tree.FIELDS:
        a, b = getattr(tree, f), getattr(back, f)
        assert a.dtype == b.dtype and np.array_equal(a, b), f
    ids = back.unit_state_ids([0, 3, 1])
    assert ids.shape == (3, c['P']) and ids.dtype == np.int32
    assert ids[1, 0] == back.lookup(0, 3, 1, 0) and ids[0, 1] == back.lookup(c['n_units'], 0, 3, 1) and ids[2, 0] == back.lookup(3, 1, c['n_units'], 0)


def test_unit_state_ids_default_reproduces_the_rows():
    """make_sentence_batch(unit_state_ids=the default ids) hands set_states the rows it always did: a pure-host check with a stub engine."""
    from poccala_amd import engine as E

    class StubBatch(object):
        def set_transitions(self, a, pi):
            self.a, self.pi = a, pi

        def set_states(self, rows):
            self.rows = rows

    class StubEngine(object):
        def batch(self, n, T, fb):
            self.b = StubBatch()
            return self.b

    S, e = 5, 3
    labels = [[0, 2, 1], [1], [2, 2, 0, 1]]
    trans = np.stack([np.triu(np.ones((S, S))) / np.arange(S, 0, -1)[:, None] for _ in range(3)])
    T, fb = np.array([9, 4, 12], dtype=np.int32), np.array([0, 9, 13], dtype=np.int64)
    b0, n0 = E.make_sentence_batch(StubEngine(), labels, T, fb, trans, S)
    ids = [np.asarray(l)[:, None] * e + np.arange(e)[None, :] for l in labels]
    b1, n1 = E.make_sentence_batch(StubEngine(), labels, T, fb, trans, S, unit_state_ids=ids)
    assert np.array_equal(n0, n1)
    for r0, r1, i in zip(b0.rows, b1.rows, ids):
        assert r0.dtype == r1.dtype == np.int32 and np.array_equal(r0, r1)
        assert np.array_equal(r1, E.embedded_row_states(i, S))
    tied = [np.zeros_like(i) + 7 for i in ids]
    b2, _ = E.make_sentence_batch(StubEngine(), labels, T, fb, trans, S, unit_state_ids=tied)
    assert all((r[1:-1] == 7).all() for r in b2.rows)
    with pytest.raises(ValueError):
        E.make_sentence_batch(StubEngine(), labels, T, fb, trans, S, unit_state_ids=ids[:2])
    with pytest.raises(ValueError):
        E.make_sentence_batch(StubEngine(), labels, T, fb, trans, S, unit_state_ids=[i[:, :2] for i in ids])


def test_cabi_names_are_bound():
    import poccala_amd._lib as L
    for name in ('pcl_tree_zero', 'pcl_tree_accumulate', 'pcl_batch_accumulate_tree', 'pcl_tree_stats_shape', 'pcl_tree_stats_download', 'pcl_tree_stats_upload',
                 'pcl_tree_build'):
        assert name in L.PROTOTYPES, name
    assert len(L.PROTOTYPES['pcl_tree_build'][1]) == 26
