"""CPU proofs for tests/_seg_cases.py: every case of the segmental-training edge tests (tests/test_gpu_segment_edges.py) reaches the edge of
csrc/gmm_segment.hip it is named for.  The launcher's few integer rules are restated in _seg_cases and held here against the source text
where that is cheap; the cases are then held against the restated rules and against the twin."""
import os
import re

import numpy as np
import pytest

import _seg_cases as sc
import _segment_twin as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLOYD = [(n, k, d, p) for (n, k, d) in sc.LLOYD_SHAPES for p in ('f64', 'f32')]


def source():
    return open(os.path.join(ROOT, 'poccala_amd', 'csrc', 'gmm_segment.hip')).read()


def test_restated_rules_are_the_source_text():
    text = source()
    assert 'constexpr int SEG_T = 256;' in text and 'constexpr int KC = 32;' in text
    assert 'std::max<long long>(std::max<long long>(2048, (F + 4095) / 4096), (F * (long long)J + (1LL << 26) - 1) >> 26)' in text
    assert 'const int chunk = (n + SEG_T - 1) / SEG_T;' in text
    assert 'const int q = (cnt + 3) / 4, lo = min(cnt, w * q), hi = min(cnt, lo + q);' in text
    assert 'for (int m = threadIdx.x; m < M; m += SEG_T)' in text
    assert 'if (!(v >= 1e-4)) v = 1e-4;' in text
    assert sorted(int(d) for d in re.findall(r'SEG_ASSIGN\((\d+)\)', text)) == [13, 26, 39, 47, 48, 64]
    api = open(os.path.join(ROOT, 'poccala_amd', 'csrc', 'pcl_api.hip')).read()
    assert 'const int pipe[] = {13, 26, 39, 47};' in api and 'const int opts[] = {48, 64};' in api and 'const int Mpad = (M + 3) / 4 * 4;' in api
    assert [sc.device_dim(d) for d in (1, 2, 13, 14, 39, 40, 47, 48, 49, 64, 65)] == [13, 13, 13, 26, 39, 47, 47, 48, 64, 64, -1]
    assert sc.sort_tile(2047, 300) == 2048 and sc.sort_tile(9_000_000, 3) == 2304 and sc.sort_tile(1 << 24, 65535) == 16384
    assert sc.quarters(5) == [2, 2, 1, 0] and sc.quarters(1) == [1, 0, 0, 0] and sc.quarters(257) == [65, 65, 65, 62]
    assert sc.seed_chunk(255) == (1, 255) and sc.seed_chunk(256) == (1, 256) and sc.seed_chunk(257) == (2, 129) and sc.seed_chunk(513) == (3, 171)


# ---------------------------------------------------------------------- sort
def test_sort_cases_reach_every_tile_count_and_round_edge():
    cases = sc.sort_cases()
    assert {(c['F'], c['J']) for c in cases} >= {(F, J) for F in sc.SORT_F for J in sc.SORT_J}
    tiles = {c['name']: sc.sort_tiles(c['F'], c['J']) for c in cases}
    for c in cases:
        assert sc.sort_tile(c['F'], c['J']) == 2048
        assert c['state'].dtype == np.int32 and c['state'].min() == -1 and c['state'].max() == c['J'] - 1
        assert tiles[c['name']] == {2047: 1, 2048: 1, 2049: 2, 4097: 3, 6149: 4}[c['F']]
        # not sorted already, and some state has two rows in one 256-row round (the order inside a round is compared)
        owned = c['state'][c['state'] >= 0]
        assert c['J'] == 1 or (np.diff(owned) < 0).any()
        first = c['state'][:256]
        assert max(np.bincount(first[first >= 0])) >= 2
    assert (2047 % 256, 2049 % 2048, 4097 % 2048, 6149 % 2048) == (255, 1, 1, 5)           # a last round of 255, 1, 1 and 5 rows
    assert sc.ceil_div(300, 256) == 2                                                       # a second workgroup of the column scan
    big = [c for c in cases if c['J'] == 300 and c['F'] >= 4097]
    assert all((np.bincount(c['state'][c['state'] >= 0], minlength=300)[256:] > 0).all() for c in big)
    (c,) = [c for c in cases if c['name'] == 'empty_middle_tile']
    j, t = c['absent']
    per_tile = [(c['state'][i:i + 2048] == j).sum() for i in range(0, c['F'], 2048)]
    assert per_tile[t] == 0 and per_tile[t - 1] > 0 and per_tile[t + 1] > 0 and len(per_tile) == 4
    (c,) = [c for c in cases if c['name'] == 'one_state_round']
    r0, j = c['full_round']
    assert r0 % 256 == 0 and (c['state'][r0:r0 + 256] == j).all() and (c['state'][:r0] == j).any() and (c['state'][r0 + 256:] == j).any()


# ---------------------------------------------------------------------- Lloyd
def test_lloyd_shapes_cover_every_instance_and_chunk_edge():
    assert {sc.device_dim(d) for (_, _, d) in sc.LLOYD_SHAPES} == {13, 26, 39, 47, 48, 64}
    assert {d for (_, _, d) in sc.LLOYD_SHAPES if sc.device_dim(d) != d} == {40, 2}                # host dimensions that pad
    chunks = {k: sc.centre_chunks(k) for (_, k, _) in sc.LLOYD_SHAPES}
    assert chunks[33][-1] == (32, 1) and chunks[40][-1] == (32, 8) and chunks[65][-1] == (64, 1)    # a partial second / third chunk
    assert chunks[64] == [(0, 32), (32, 32)] and chunks[32] == [(0, 32)] and chunks[1] == [(0, 1)] and len(chunks[300]) == 10
    assert max(k for (_, k, _) in sc.LLOYD_SHAPES) > 256                                            # the strided clear of the K offsets
    last = {n: n % 256 for (n, _, _) in sc.LLOYD_SHAPES}                                            # rows in the last 256-frame tile
    assert last[257] == 1 and last[513] == 1 and last[256] == 0 and last[255] == 255 and last[300] == 44 and last[600] == 88


@pytest.mark.parametrize('n,K,D,prec', LLOYD)
def test_lloyd_case_holds_its_conditions(n, K, D, prec):
    c = sc.lloyd_case(n, K, D, prec)
    roles = c['roles']
    x, a = c['x'], c['assign']
    print('%s: seed %d, sweeps %d, margin %.2e, cluster sizes %s' % (c['name'], c['seed'], c['sweeps'], c['margin'], np.bincount(a, minlength=K).tolist()))
    assert np.array_equal(c['frames'][c['state'] == 0].astype(np.float64), x) and len(x) == n
    assert c['frames'].dtype == (np.float64 if prec == 'f64' else np.float32)
    assert (c['state'] == 1).sum() == min(K - 1, 3) < K and (c['state'] == -1).sum() == 9
    assert 2 <= c['sweeps'] < 100
    if K > 1:
        assert c['margin'] > sc.MARGIN[prec]
    counts = np.bincount(a, minlength=K)
    assert (counts[roles['far']] == 0).all()
    if K >= 8:
        assert len(roles['far']) >= 1 and counts[roles['ident']] == sc.IDENT_ROWS
        rows = x[a == roles['ident']]
        assert (rows == rows[0]).all()                                                      # identical rows: variance 0, floored
        assert (tw.cluster_model(x, a, c['centres'])[1][roles['ident']] == sc.VAR_FLOOR).all()
        assert np.array_equal(rows[0].astype(np.float32).astype(np.float64), rows[0])
    if K == 40:
        assert roles['dup'] == {32: 31, 33: 0}
        for k, src in roles['dup'].items():
            assert np.array_equal(c['c0'][0, k], c['c0'][0, src]) and k >= sc.KC > src      # the tie crosses the chunk boundary
            assert (c['first'] == src).sum() > 0 and (c['first'] == k).sum() == 0
    else:
        assert len(np.unique(c['c0'][0], axis=0)) == K                                      # no other ties
    # the twin on the case's own numbers, through its public routine
    mean, var, w, a2, sw2 = tw.kmeans(x, K, 0, init_centres=c['c0'][0]) if prec == 'f64' else (None,) * 5
    if prec == 'f64':
        assert np.array_equal(a2, a) and sw2 == c['sweeps']


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_cluster_size_case_has_the_sizes(prec):
    c = sc.cluster_size_case(prec)
    assert np.array_equal(c['assign'], c['label']) and c['sweeps'] == 1 and c['margin'] > 0.5
    assert np.bincount(c['assign'], minlength=c['K']).tolist() == list(sc.CLUSTER_SIZES) == [0, 1, 2, 3, 4, 5, 9, 257]
    idle = {n: sc.quarters(n).count(0) for n in sc.CLUSTER_SIZES}
    assert idle == {0: 4, 1: 3, 2: 2, 3: 1, 4: 0, 5: 1, 9: 1, 257: 0}                       # waves without a row
    assert sc.quarters(9) == [3, 3, 3, 0] and all(sum(sc.quarters(n)) == n for n in range(600))
    mean, var, w = tw.cluster_model(c['x'], c['assign'], c['centres'])
    assert (var[0] == sc.VAR_FLOOR).all() and w[0] == 0 and np.array_equal(mean[0], c['c0'][0, 0])     # the empty cluster
    assert (var[1] == sc.VAR_FLOOR).all() and (var[2:] > sc.VAR_FLOOR).all()                            # one row: floored


# ---------------------------------------------------------------------- seeding
@pytest.mark.parametrize('D', sc.SEED_DIMS)
@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_seed_case_holds_its_margin_and_chunks(D, prec):
    c = sc.seed_case(D, prec)
    ns = [len(x) for x in c['xs']]
    assert ns[:6] == [255, 256, 257, 511, 513, c['K']] and ns[6:] == [9, 15, 4] and ns[8] < c['K']
    assert [sc.seed_chunk(n) for n in ns[:6]] == [(1, 255), (1, 256), (2, 129), (2, 256), (3, 171), (1, 6)]   # chunk 1 -> 2 -> 3, idle threads
    print('%s: twin margins %s' % (c['name'], ['%.1e' % m for m in c['margin']]))
    for j in range(8):
        x = c['frames'][c['state'] == j].astype(np.float64)
        assert np.array_equal(x, c['xs'][j])
        want, margin = tw.seeds(x, c['K'], c['seed'], j)
        assert np.array_equal(want, c['want'][j]) and margin == c['margin'][j] and margin > 1e-9
        distinct = len(np.unique(x, axis=0))
        assert len(np.unique(x[want], axis=0)) == min(c['K'], distinct)
    assert len(np.unique(c['xs'][6], axis=0)) == 1 and len(np.unique(c['xs'][7], axis=0)) == 3
    assert c['frames'].dtype == (np.float64 if prec == 'f64' else np.float32)
    if prec == 'f32':
        assert all(np.array_equal(x.astype(np.float32).astype(np.float64), x) for x in c['xs'])


# ---------------------------------------------------------------------- EM
def test_em_shapes_cover_the_mixture_stride_and_padding():
    assert {m: sc.mixture_rounds(m) for (m, _) in sc.EM_SHAPES} == {257: 2, 300: 2, 33: 1, 4: 1, 5: 1}
    assert {m for (m, _) in sc.EM_SHAPES if sc.mpad(m) != m} == {257, 33, 5}
    assert {d: sc.device_dim(d) for (_, d) in sc.EM_SHAPES} == {13: 13, 39: 39, 40: 47, 64: 64, 2: 13}


def check_em_case(c, dead=None):
    M = c['M']
    trained = len(c['steps'])
    assert c['J'] == trained + (c['short'] is not None)
    if c['short'] is not None:
        assert (c['state'] == c['J'] - 1).sum() == c['short'] < M
    assert (c['var0'] >= 0.5).all() and (c['var0'] <= 2).all() and (c['w0'] == 1.0 / M).all()
    for j, steps in enumerate(c['steps']):
        x = c['xs'][j]
        n = len(x)
        assert M <= n <= 3 * M or c['name'] == 'ragged'
        assert np.array_equal(c['frames'][c['state'] == j], x) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
        for prec in ('f64', 'f32'):
            thr = c['threshold'][prec]
            assert thr in sc.clear_thresholds(steps, prec, c['max_iters'])
            run = sc.run_length(steps, thr, c['max_iters'])
            r = tw.em(x, c['mean0'][j], c['var0'][j], c['w0'][j], c_covariance=c['c_cov'], threshold=thr, max_iters=c['max_iters'], logdet=c['logdet'])
            assert r['iters'] == run and np.array_equal(r['q_seq'], [s['q'] for s in steps[:run]])
            assert np.array_equal(r['mean'], steps[run - 1]['mean']) and np.array_equal(r['var'], steps[run - 1]['var'])
        big = np.array([s['big'] for s in steps])
        print('%s state %d: n %d, smallest Gamma %.3g (n / M = %.3g), thresholds %s' % (c['name'], j, n, big.min(), n / M, c['threshold']))
        if dead is None:
            assert big.min() >= 1e-3 * n / M
        else:
            assert (big[:, dead] == 0).all() and np.delete(big, dead, axis=1).min() >= 1e-3 * n / M


@pytest.mark.parametrize('M,D', sc.EM_SHAPES)
def test_em_shape_case_holds_its_conditions(M, D):
    c = sc.em_shape_case(M, D)
    assert [len(x) for x in c['xs']] == ([M, 3 * M] if M <= 64 else [M, 2 * M + 1]) and c['max_iters'] == 8 and not c['logdet']
    check_em_case(c)


def test_em_special_cases_hold_their_conditions():
    c = sc.em_special_case('gamma0')
    check_em_case(c, dead=2)
    for s in c['steps'][0]:
        assert s['w'][2] == 0 and np.array_equal(s['mean'][2], c['mean0'][0, 2]) and np.array_equal(s['var'][2], c['var0'][0, 2])
        assert np.isfinite(s['q']) and abs(s['w'].sum() - 1) < 1e-12
    c = sc.em_special_case('floor')
    check_em_case(c)
    assert all(s['s2'].max() < c['c_cov'] == 0.6 and (s['var'] == 0.6).all() for s in c['steps'][0])
    c = sc.em_special_case('logdet')
    check_em_case(c)
    assert c['logdet']
    s = c['steps'][0][0]
    assert abs(tw.q_closed(s['big'], s['w'], s['var'], s['s2'], True) - tw.q_closed(s['big'], s['w'], s['var'], s['s2'], False)) > 1e-3 * abs(s['q'])
    c = sc.em_special_case('ragged')
    check_em_case(c)
    runs = [sc.run_length(st, 1.28, c['max_iters']) for st in c['steps']]
    assert c['threshold'] == {'f64': 1.28, 'f32': 1.28} and runs[0] != runs[1] and min(runs) > 1 and max(runs) < c['max_iters'] and c['short'] == 3


def test_twin_keeps_a_mixture_nobody_reaches():
    """E4 of the twin against the kernel's rule, on numbers small enough to read."""
    x = np.array([[0.0], [1.0], [2.0]])
    gamma = np.array([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]])
    prev = (np.array([[5.0], [7.0]]), np.array([[2.0], [3.0]]))
    mean, var, w, s2, big = tw.maximization(x, gamma, 1e-3, prev=prev)
    assert mean.tolist() == [[1.0], [7.0]] and var[1, 0] == 3.0 and w.tolist() == [1.0, 0.0] and s2[1, 0] == 0.0
    q = tw.q_closed(big, w, var, s2)
    assert q == 3 * (0.0 - 0.5 * (tw.LN2PI + var[0, 0] + 1.0))
    r = tw.em(x, prev[0] * 0 + [[1.0], [1e3]], prev[1], np.array([0.5, 0.5]), max_iters=3)
    assert r['w'][1] == 0 and r['mean'][1, 0] == 1e3 and r['var'][1, 0] == 3.0 and np.isfinite(r['q_seq']).all()
