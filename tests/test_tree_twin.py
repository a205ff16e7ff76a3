"""CPU checks of the decision-tree row (f16): the NumPy twin's own properties (tests/_tree_twin.py), the host helpers of
poccala_amd/AcousticModel/ContextTree.py, make_sentence_batch's unit_state_ids argument, the C-ABI names, and -- for every build case
tests/test_gpu_tree.py runs -- the separation condition: at every decision every candidate of a different partition lies at least
1e-9 B below the winner, and no count-valid candidate lies within 1e-9 B of min_gain.  A case that is not separated FAILS here: no
decision is left uncompared on the device.  The same for the cases of tests/test_gpu_tree_edges.py, and that each of them reaches the
edge it is named after: an equal candidate in a later group, leaves that tie exactly, counts beyond 2^32, the widths at which the
statistics kernel loads a frame's tail element by element, and an input whose sums tell the stated summation order from others."""
import os

import numpy as np
import pytest

import _tree_cases as tc
import _tree_twin as tw

SEP = 1e-9
EDGE = tc.edge_cases()                                            # tests/test_gpu_tree_edges.py runs these
CASES = dict(tc.build_cases(), **EDGE)
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


def test_edge_build_cases_reach_their_edges():
    for name, D in (('wide64', 64), ('d1', 1), ('d39', 39), ('d14', 14), ('d40', 40), ('d49', 49)):
        c = EDGE[name]
        assert c['D'] == D and c['n_units'] == 3 and c['P'] in (1, 2) and c['max_leaves'] <= c['R0'] + 4 and len(built(name)['split_gain']) >= 3
    assert 3 * EDGE['q8_full_groups']['q_member'].shape[0] == 3 * tw.GROUP                 # three full groups
    assert {cnd // tw.GROUP for cnd in built('q8_full_groups')['node_cand'] if cnd >= 0} >= {0, 1}
    # duplicate and complement one group apart: a winner with an equal in a LATER group, of either kind
    cd = EDGE['dup_across_groups']
    qd = cd['q_member'] != 0
    assert len(qd) == 9 and (qd[8] == qd[0]).all() and (qd[7] != qd[1]).all()
    later = [d for d in built('dup_across_groups')['decisions'] if d['kind'] == 'split' and d['later_group_ties'] > 0]
    print('dup_across_groups: winners with an equal in a later group: %s' % [d['cand'] for d in later])
    assert {d['cand'] % 9 for d in later} >= {0, 1}                                          # set 0's duplicate, set 1's complement
    assert all(d['cand'] % 9 not in (7, 8) for d in built('dup_across_groups')['decisions'] if d['kind'] == 'split')
    cq = EDGE['q1365']
    assert cq['q_member'].shape == (1365, 7) and 22 <= len(cq['event_ctx']) <= 26 and cq['max_leaves'] == cq['R0'] + 3
    assert len(built('q1365')['split_gain']) == 3 and any(d['later_group_ties'] > 0 for d in built('q1365')['decisions'])
    # mirrored centres: exact ties between leaves, at the roots and after the first split; one of the two builds stops inside a tie
    last = []
    for name in ('mirror_roots_even', 'mirror_roots_odd'):
        c, t = EDGE[name], built(name)
        ev, P = c['event_ctx'], c['P']
        r0, r1 = np.flatnonzero(ev[:, 1] == 0), np.flatnonzero(ev[:, 1] == 1)
        assert c['root_of'][0] != c['root_of'][P] and all(c[k][r0].tobytes() == c[k][r1].tobytes() for k in ('n', 's', 'q'))
        ties = [i for i, d in enumerate(t['decisions']) if d['kind'] == 'split' and d['xleaf_ties'] > 0]
        print('%s: decisions with an equal in another leaf: %s' % (name, ties))
        assert len(ties) >= 2 and max(ties) > 0                   # behind the first split the leaves are no longer listed in node order
        for i in ties:                                            # the lowest node id won
            d = t['decisions'][i]
            assert all(t['decisions'][k]['node'] > d['node'] for k in range(i + 1, len(t['decisions'])) if t['decisions'][k].get('gain') == d['gain'])
        last.append(t['decisions'][-1]['xleaf_ties'])
    assert EDGE['mirror_roots_even']['max_leaves'] % 2 == 0 and EDGE['mirror_roots_odd']['max_leaves'] % 2 == 1
    assert min(last) == 0 < max(last)                             # one stops between a leaf and its mirror image, the other behind both
    # big_counts IS min_count times 2^23: the same decisions, sep and thr to the bit, the gains scaled exactly, counts beyond 2^32
    b, m, cb = built('big_counts'), built('min_count'), EDGE['big_counts']
    assert b['node_n'].max() > 2 ** 32 and cb['min_count'] > 2 ** 31 and np.array_equal(b['node_n'], m['node_n'] * tc.BIG)
    assert np.array_equal(b['node_cand'], m['node_cand']) and np.array_equal(b['split_gain'], m['split_gain'] * tc.BIG)
    assert len(b['decisions']) == len(m['decisions'])
    for x, y in zip(b['decisions'], m['decisions']):
        assert x['thr'] == y['thr'] and x.get('sep') == y.get('sep') and x.get('cand') == y.get('cand')


def test_ordered_twin_is_the_sequential_one_where_orders_agree():
    """accumulate_ordered against accumulate: bit for bit on the grid (every order is exact there), within accumulate's first-order bound
    (n - 1) 2^-53 sum |x| on Gaussian frames, for several chunk lengths and over two calls."""
    frames, T, begin, frame_row, R = tc.frames_case(13)
    st = tw.accumulate(tw.zero(R, 13), frames, T, begin, frame_row)
    for chunk in (1, 4, 7, 256):
        o = tw.accumulate_ordered(tw.zero(R, 13), frames, T, begin, frame_row, chunk)
        two = tw.accumulate_ordered(tw.accumulate_ordered(tw.zero(R, 13), frames, T[:2], begin[:2], frame_row, chunk), frames, T[2:], begin[2:], frame_row, chunk)
        for k in ('n', 's', 'q'):
            assert o[k].dtype == st[k].dtype and o[k].tobytes() == st[k].tobytes() == two[k].tobytes(), (chunk, k)
    o32 = tw.accumulate_ordered(tw.zero(R, 13), frames.astype(np.float32), T, begin, frame_row, 4)      # widened first
    assert all(o32[k].tobytes() == st[k].tobytes() for k in ('n', 's', 'q'))
    frames, T, begin, frame_row, R = tc.order_case()
    D = frames.shape[1]
    st = tw.accumulate(tw.zero(R, D), frames, T, begin, frame_row)
    for chunk in (1, 7, 256):
        o = tw.accumulate_ordered(tw.zero(R, D), frames, T, begin, frame_row, chunk)
        assert np.array_equal(o['n'], st['n'])
        for k in ('s', 'q'):
            bound = np.maximum(st['n'] - 1, 0)[:, None] * 2.0 ** -53 * st[k + 'abs']
            worst = float(np.max(np.abs(o[k] - st[k]) / bound))
            print('ordered twin, chunk %d: %s worst difference / bound = %.3e, %d entries differ' % (chunk, k, worst, (o[k] != st[k]).sum()))
            assert worst <= 1.0


def test_order_case_tells_the_orders_apart():
    """The input of the GPU order test (tests/test_gpu_tree_edges.py) has what the issue asks of it, and its sums DO depend on the order:
    every wrong order differs from the stated one in at least one byte, in float64 and in float32, at every chunk length the GPU test
    runs.  Entries of q that differ out of 117, chunk 7, float64 / float32 input: runs added last first 77 / 83, a run summed in
    descending frame row 44 / 11, a row's frames swapped pair by pair (a scatter that is not stable) 83 / 68, q + x x rounded once (a
    contracted multiply-add) 19 / none: a float32 value's square is exact in float64, so only float64 frames can show a contraction,
    and float32 values' plain sums are exact in any order here, so for them only q tells the orders apart."""
    frames, T, begin, frame_row, R = tc.order_case()
    F, D = frames.shape
    assert F == 2 * 2048 + 37 and R == 9 and len(T) == 2
    assert begin[0] == 0 and begin[1] + T[1] == F and begin[0] + T[0] < begin[1]             # rows 0 and F - 1 are inside, a gap between
    assert frame_row[2047] == frame_row[2048] >= 0 and frame_row[4095] == frame_row[4096] >= 0
    assert frame_row[0] >= 0 and frame_row[F - 1] >= 0 and (frame_row[begin[0] + T[0]:begin[1]] >= 0).any() and (frame_row == -1).any()
    right = tw.accumulate_ordered(tw.zero(R, D), frames, T, begin, frame_row, 7)
    assert right['n'][0] > F // 2 and (right['n'] > 0).all()
    for fr, kind in ((frames, 'f64'), (frames.astype(np.float32), 'f32')):
        for chunk in (1, 7, 256):
            ok = tw.accumulate_ordered(tw.zero(R, D), fr, T, begin, frame_row, chunk)
            # (at chunk 1 a run holds one frame: nothing inside it to reverse)
            for wrong in ('runs_reversed', 'unstable', 'fused') + (('frames_reversed',) if chunk > 1 else ()):
                if wrong == 'fused' and (kind, chunk) != ('f64', 7):
                    continue                                      # (the exact multiply-add runs entry by entry in Python: once)
                bad = tw.accumulate_ordered(tw.zero(R, D), fr, T, begin, frame_row, chunk, wrong=wrong)
                ds, dq = int((bad['s'] != ok['s']).sum()), int((bad['q'] != ok['q']).sum())
                print('order case %s chunk %d, %s: s differs in %d, q in %d of %d entries' % (kind, chunk, wrong, ds, dq, ok['q'].size))
                # (float32 frames widened: 24-bit values, whose sums over a few thousand frames are exact in any order and whose squares
                # are exact products -- there only q tells the orders apart, and a contracted multiply-add shows in float64 frames alone)
                assert np.array_equal(bad['n'], ok['n']) and dq > 0 and (ds > 0 or wrong == 'fused' or kind == 'f32')
    # chunk lengths give different sums too: the knob is not a no-op on this input
    assert right['s'].tobytes() != tw.accumulate_ordered(tw.zero(R, D), frames, T, begin, frame_row, 256)['s'].tobytes()


def test_statistics_edge_cases_reach_their_edges():
    """The widths at which the statistics kernel's element-by-element load runs (csrc/tree_cluster.hip, tree_partial_kernel): lane g
    loads the G columns from d0 = G g (d0 < D) of frame row f in one piece iff f FD + d0 + G <= F FD; for the last row that is
    d0 + G <= FD, FD the device width.  float32 (G = 4): FD = 13 has d0 = 12 (D = 13), FD = 26 has d0 = 24 (D = 25, 26), FD = 39 has
    d0 = 36 (D = 37 .. 39), FD = 47 has d0 = 44 (D = 45 .. 47); 48 and 64 are multiples of 4.  float64 (G = 2): the odd widths, d0 = FD - 1:
    D = 13, 39, 47."""
    assert tc.tail_load_dims(4) == [13, 25, 26, 37, 38, 39, 45, 46, 47] and tc.tail_load_dims(2) == [13, 39, 47]
    assert [d for d in tc.WIDTH_DIMS if d in tc.tail_load_dims(4)] == [13, 26, 37, 39, 45, 47]
    assert [d for d in tc.WIDTH_DIMS if d in tc.tail_load_dims(2)] == [13, 39, 47]
    assert {min(x for x in tc.DEVICE_DIMS if x >= d) for d in tc.WIDTH_DIMS} == set(tc.DEVICE_DIMS)
    api = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'poccala_amd', 'csrc', 'pcl_api.hip')).read()
    assert 'const int pipe[] = {13, 26, 39, 47};' in api and 'const int opts[] = {48, 64};' in api
    for D in tc.WIDTH_DIMS:
        frames, T, begin, frame_row, R = tc.width_case(D)
        F = len(frames)
        assert F == 64 and T.tolist() == [F] and begin.tolist() == [0] and 0 <= frame_row[F - 1] != frame_row[F - 2] >= 0
        assert np.array_equal(frames.astype(np.float32).astype(np.float64), frames)
    for T in (16384, 16385, 40000):
        frames, Tu, begin, frame_row, R = tc.long_case(T)
        assert Tu.tolist() == [T] and frames.shape == (T + 5, 2) and R == 5
        around = frame_row[begin[0] + np.arange(16382, min(16387, T))]
        assert len(set(around.tolist())) == len(around) and (around >= 0).all()


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
