"""The NumPy twin of the LDA rule (tests/_lda_twin.py; the rule: include/poccala_hip.h, row f12) held to its own invariants: the splice at
the edges of a 3-row utterance by hand, a whitened within-class covariance and a diagonal between-class covariance after the projection,
a planted discriminant subspace recovered, and tied states folded into classes.  The second half holds the inputs of
tests/test_gpu_lda_edges.py to the edges they are made for -- planted class counts, empty classes, labelled rows of no utterance, the
chunks and launch rounds the counts give -- so that no GPU test passes because its input missed the edge."""
import numpy as np

import _lda_twin as tw


def test_splice_edges_by_hand():
    # rows 0 and 4 belong to nobody; the utterance is rows 1 .. 3 = a, b, c
    fr = np.array([[90., 91.], [1., 2.], [3., 4.], [5., 6.], [92., 93.]])
    a, b, c = fr[1], fr[2], fr[3]
    xs, owned = tw.splice(fr, [3], [1], 2, 1)
    assert owned.tolist() == [False, True, True, True, False] and xs.shape == (5, 8)
    assert np.array_equal(xs[1], np.concatenate([a, a, a, b]))          # both left neighbours clamp to the first row
    assert np.array_equal(xs[2], np.concatenate([a, a, b, c]))
    assert np.array_equal(xs[3], np.concatenate([a, b, c, c]))          # the right neighbour clamps to the last row
    assert not xs[0].any() and not xs[4].any()
    one, _ = tw.splice(fr, [1], [2], 4, 4)                              # an utterance of one row: both clamps act on it
    assert np.array_equal(one[2], np.tile(b, 9))
    same, _ = tw.splice(fr, [3], [1], 0, 0)                             # no context: the rows themselves
    assert np.array_equal(same[1:4], fr[1:4])
    two, _ = tw.splice(fr, [2, 2], [0, 2], 1, 1)                        # neighbours in the matrix, never in the splice
    assert np.array_equal(two[1], np.concatenate([fr[0], fr[1], fr[1]])) and np.array_equal(two[2], np.concatenate([fr[2], fr[2], fr[3]]))


def test_statistics_are_the_plain_sums():
    fr, T, begin, cls = tw.make_case(5)
    st = tw.stats(fr, T, begin, cls, tw.R_CASE, 1, 2)
    xs, owned = tw.splice(fr, T, begin, 1, 2)
    assert st['n'][3] == 0 and st['n'].sum() == ((cls >= 0) & owned).sum() < (cls >= 0).sum()     # class 3 empty; labelled rows of no utterance left out
    r = 2
    rows = np.flatnonzero((cls == r) & owned)
    assert st['n'][r] == len(rows) > 32
    np.testing.assert_allclose(st['s'][r], sum(xs[g] for g in rows), rtol=1e-12)
    np.testing.assert_allclose(st['S'][r], sum(np.outer(xs[g], xs[g]) for g in rows), rtol=1e-12)
    assert (st['Sabs'] >= np.abs(st['S']) * (1 - 1e-12)).all()


def test_projected_data_is_whitened_within_and_diagonal_between():
    rng = np.random.default_rng(3)
    D, left, right, R = 4, 1, 1, 6
    T = np.array([30, 50, 1, 45, 60, 38], dtype=np.int32)
    begin = np.concatenate([[2], 2 + np.cumsum(T[:-1] + 3)]).astype(np.int64)
    F = int(begin[-1] + T[-1] + 2)
    cls = np.full(F, -1, dtype=np.int32)
    fr = rng.standard_normal((F, D))
    mix = rng.standard_normal((D, D))
    for t, b in zip(T, begin):
        c = rng.integers(0, R, size=t)
        cls[b:b + t] = c
        fr[b:b + t] = rng.standard_normal((t, D)) @ mix + 2.0 * rng.standard_normal((R, D))[c]
    st = tw.stats(fr, T, begin, cls, R, left, right)
    Ds = D * (left + right + 1)
    for D_out in (Ds, 5, 2):
        A, b, lam = tw.estimate(st['n'], st['s'], st['S'], D_out, eps=0.0)
        y, _, _ = tw.project(fr, T, begin, left, right, A, b)
        W, B, m = tw.class_covariances(y, cls, R)
        print('D_out %d: |W - I| %.2e, |B - diag(lambda)| %.2e, |mean| %.2e, lambda %s' % (D_out, np.abs(W - np.eye(D_out)).max(),
                                                                                       np.abs(B - np.diag(lam)).max(), np.abs(m).max(), lam))
        assert np.abs(W - np.eye(D_out)).max() <= 1e-9
        assert np.abs(B - np.diag(lam)).max() <= 1e-9
        assert np.abs(m).max() <= 1e-9
        assert (np.diff(lam) <= 0).all()
        assert (A[np.arange(D_out), np.abs(A).argmax(axis=1)] > 0).all()                          # the sign rule


# The planted case at its fixed seed: the largest principal angle between the two leading rows of A and the planted subspace, measured on
# the twin: 0.0819 rad (the data is a sample: 720 rows, noise variance 1, class means a few units apart; the replicated edge rows make the
# within-class covariance of the spliced vectors slightly anisotropic).  Bound = 10 x that.
PLANTED_ANGLE = 0.0819


def test_planted_subspace_is_recovered():
    fr, T, begin, cls, basis = tw.planted_case()
    st = tw.stats(fr, T, begin, cls, 4, 1, 1)
    A, b, lam = tw.estimate(st['n'], st['s'], st['S'], 3)
    angle = tw.principal_angle(A[:2], basis)
    print('planted: principal angle %.4f rad, eigenvalues %s' % (angle, lam))
    assert angle <= 10 * PLANTED_ANGLE
    assert lam[1] > 100 * max(lam[2], 1e-12)                               # two discriminant directions, then nothing
    y, _, _ = tw.project(fr, T, begin, 1, 1, A[:2], b[:2])
    assert tw.nearest_mean_error(y, np.where(cls >= 0, cls, -1), 4) <= 0.05


def test_state_class_folding_is_a_relabelled_map():
    fr, T, begin, cls = tw.make_case(3)
    state = np.where(cls >= 0, cls * 2 + (np.arange(len(cls)) % 2), -1).astype(np.int32)      # 10 states, two per class
    sc = np.repeat(np.arange(5, dtype=np.int32), 2)
    sc[9] = -1                                                                                # a state that belongs to no class
    folded = tw.fold(state, sc)
    assert np.array_equal(folded, np.where(state == 9, -1, cls))
    a = tw.stats(fr, T, begin, folded, 5, 1, 1)
    b = tw.stats(fr, T, begin, np.where(state == 9, -1, cls), 5, 1, 1)
    for k in ('n', 's', 'S'):
        assert np.array_equal(a[k], b[k])
    per_state = tw.stats(fr, T, begin, state, 10, 1, 1)                                       # identity: every state a class
    assert np.array_equal(tw.fold(state, None), state)
    np.testing.assert_allclose(per_state['S'][0] + per_state['S'][1], a['S'][0], rtol=1e-12)
    assert per_state['n'][0] + per_state['n'][1] == a['n'][0]


# ------------------------------------------------------------------ the inputs of tests/test_gpu_lda_edges.py reach the edges they are for
def planted(D, lengths, counts, left, right):
    fr, T, begin, cls = tw.plant_case(D, lengths, counts)
    return fr, T, begin, cls, tw.stats(fr, T, begin, cls, len(counts), left, right)


def test_edge_shapes_are_every_tile_count_and_order_edge():
    assert [s[4] for s in tw.EDGE_SHAPES] == [1, 1, 2, 3, 4, 5, 6, 7, 8] and tw.EDGE_SHAPES[0][3] == 2
    for D, left, right, n, NT in tw.EDGE_SHAPES:
        assert D * (left + right + 1) + 1 == n <= 128 and -(-n // tw.TILE) == NT
    orders = [s[3] for s in tw.EDGE_SHAPES]
    assert [n for n in orders if n % 16 == 0] == [16, 64, 112, 128]                                # no padding column, the ones column last
    assert [n for n in orders if n % 16 == 1] == [17, 65]                                          # the ones column alone in its tile
    assert [s[4] for s in tw.EDGE_SHAPES if (16 * s[4]) % 32 == 0] == [2, 4, 6, 8]                 # the padded row stride
    # the statistics case at these dimensions: class 3 empty, class 2 above two chunks of 16, rows -1, labelled rows of no utterance;
    # a context beyond every utterance at the cap
    assert max(tw.LENGTHS) < 63 + 63 + 1 and sorted(tw.LENGTHS)[3] < 9 + 8 + 1                      # ... and beyond four of the seven at (9, 8)
    for D in sorted({s[0] for s in tw.EDGE_SHAPES}):
        fr, T, begin, cls = tw.make_case(D)
        _, owned = tw.splice(fr, T, begin, 0, 0)
        n = np.bincount(cls[owned & (cls >= 0)], minlength=tw.R_CASE)
        assert T.tolist() == tw.LENGTHS and n[3] == 0 and n[2] > 32 and (n[[0, 1, 2, 4]] > 0).all()
        assert (cls[owned] == -1).any() and (cls[~owned] >= 0).any()


def test_planted_counts_are_exact():
    for D, lengths, counts in ((3, tw.KEDGE_LENGTHS, tw.KEDGE_COUNTS), (16, tw.KEDGE_LENGTHS, tw.KEDGE_COUNTS), (3, tw.ROUND_LENGTHS, tw.ROUND_COUNTS),
                               (13, tw.ROUND40_LENGTHS, tw.ROUND40_COUNTS)):
        fr, T, begin, cls, st = planted(D, lengths, counts, 1, 0)
        _, owned = tw.splice(fr, T, begin, 0, 0)
        assert T.tolist() == lengths and np.array_equal(st['n'], counts)                          # the planted counts, exactly
        assert np.array_equal(np.flatnonzero(st['n'] == 0), np.flatnonzero(np.asarray(counts) == 0))
        assert (cls[~owned] >= 0).all() and (~owned).sum() > len(lengths)                         # labelled rows of no utterance: not kept
        assert np.bincount(cls[cls >= 0], minlength=len(counts)).sum() > st['n'].sum()
        assert (cls[owned] == -1).sum() == sum(lengths) - sum(counts) > 0                         # rows of an utterance that are skipped
        utt = np.searchsorted(begin, np.arange(len(cls)), side='right') - 1
        for r in np.flatnonzero(np.asarray(counts) >= 3):                                         # a class is scattered over the utterances
            assert len(set(utt[owned & (cls == r)])) >= 2
        again = tw.plant_case(D, lengths, counts)
        assert all(np.array_equal(a, b) for a, b in zip((fr, T, begin, cls), again))
    with np.testing.assert_raises(ValueError):
        tw.plant_case(3, [4, 5], [6, 4])


def test_k_edge_counts_reach_every_k_step():
    counts = tw.KEDGE_COUNTS
    assert [c for c in counts if c] == [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97] and len(counts) == 16
    assert counts[7] == 0 and counts[-1] == 0 and sum(counts) <= sum(tw.KEDGE_LENGTHS) < 500
    one = tw.chunk_plan(counts)                                                                    # the default: every class one chunk
    assert one['rows'] == [c for c in counts if c] and one['rounds'] == 1
    steps = {c: tw.chunk_steps(c) for c in one['rows']}
    for c in (33, 63, 65, 97):
        assert steps[c]['steps'] >= 2 and steps[c]['second']                                      # a second k0 iteration, both k-steps of a wave
    assert steps[33]['early'] and steps[65]['early'] and steps[97]['early'] and not steps[63]['early']       # the break in a LATER step (one row left)
    assert steps[97]['steps'] == 4 and steps[64] == dict(steps=2, second=True, early=False) and steps[32] == dict(steps=1, second=True, early=False)
    assert steps[16] == dict(steps=1, second=False, early=True) and steps[17] == dict(steps=1, second=True, early=True) and steps[31] == dict(steps=1, second=True, early=False)
    assert [steps[c]['early'] for c in (1, 3, 4, 5, 15)] == [True] * 5                            # the break off a multiple of 4
    p33 = tw.chunk_plan(counts, 33)
    lo = p33['cls_chunk0']
    assert p33['rows'][lo[13]:lo[14]] == [33, 32] and p33['rows'][lo[14]:lo[15]] == [33, 33, 31] and lo[7] == lo[8] and lo[15] == lo[16]
    assert tw.chunk_plan(counts, 5)['rows'][:6] == [1, 3, 4, 5, 5, 5] and tw.chunk_plan(counts, 1)['chunks'] == sum(counts) == 446
    assert all(tw.chunk_plan(counts, c)['rounds'] == 1 for c in (1, 5, 33))


def test_round_counts_cross_the_round_edges():
    p = tw.chunk_plan(tw.ROUND_COUNTS, 1)
    assert p['chunks'] == 2554 and p['rounds'] == 3 and p['cls_chunk0'].tolist() == [0, 1024, 1024, 2524, 2524, 2554, 2554]
    assert p['cls_chunk0'][1] == tw.ROUND and p['split'] == [2]                                    # class 0 ends on the edge; class 2 in rounds 1 and 2
    assert (p['cls_chunk0'][2] // tw.ROUND, (p['cls_chunk0'][3] - 1) // tw.ROUND) == (1, 2)
    assert tw.chunk_plan(tw.ROUND_COUNTS)['rounds'] == 1 and tw.chunk_plan(tw.ROUND_COUNTS)['rows'] == [1024, 1024, 476, 30]
    q = tw.chunk_plan(tw.ROUND40_COUNTS, 1)
    assert q['chunks'] == 1100 and q['rounds'] == 2 and q['split'] == [2] and 1000 < sum(tw.ROUND40_COUNTS) <= sum(tw.ROUND40_LENGTHS)
    # the partials of a round: chunks x tiles x 2 KB, under 15 MB
    assert min(p['chunks'], tw.ROUND) * 1 * 2048 < 15e6 and min(q['chunks'], tw.ROUND) * 6 * 2048 < 15e6
    assert sum(tw.ROUND_COUNTS) <= sum(tw.ROUND_LENGTHS) < 20000


def test_long_case_lies_behind_one_pass_of_the_key_grid():
    fr, T, begin, cls = tw.long_case()
    st = tw.stats(fr, T, begin, cls, tw.LONG_R, 1, 1)
    assert T.tolist() == [5, 64 * 256 + 300, 3] and len(fr) < 20000 and np.gcd(tw.LONG_PERIOD, 256) == 1
    want = sum(np.bincount(np.arange(t) % tw.LONG_PERIOD, minlength=tw.LONG_PERIOD)[:tw.LONG_R] for t in T)
    assert np.array_equal(st['n'], want) and (st['n'] > 2 * tw.CHUNK_DEFAULT).all()               # every class: three chunks of the default length
    tail = cls[begin[1] + 64 * 256:begin[1] + T[1]]
    assert set(tail.tolist()) == set(range(-1, tw.LONG_R))                                         # every class has rows behind the mark
    _, owned = tw.splice(fr, T, begin, 0, 0)
    assert (cls[~owned] == 0).all() and (~owned).sum() > 5


def test_chained_projection_is_one_the_device_accepts():
    (D, l1, r1, o1), (D2, l2, r2, o2) = tw.CHAIN
    assert o1 <= D * (l1 + r1 + 1) <= 127 and D2 == o1 and o2 <= D2 * (l2 + r2 + 1) <= 127      # D_out <= Ds <= 127 at both stages
    assert next(w for w in tw.DEVICE_DIMS if o1 <= w) == 47 > o1 and o2 == 64                     # the first stage's rows are held padded
