"""The NumPy twin of the LDA rule (tests/_lda_twin.py; the rule: include/poccala_hip.h, row f12) held to its own invariants: the splice at
the edges of a 3-row utterance by hand, a whitened within-class covariance and a diagonal between-class covariance after the projection,
a planted discriminant subspace recovered, and tied states folded into classes."""
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
