"""The CMVN twin's own invariants (tests/_cmvn_twin.py restates include/poccala_hip.h row f14 in NumPy; tests/test_gpu_cmvn.py holds the
device to it).  No GPU.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import _cmvn_twin as tw

EPS = 2.0 ** -53


def stats_of(frames, T, begin, spk, S=tw.S_SPK):
    return tw.accumulate(tw.zero(S, frames.shape[1]), frames, T, begin, spk)


@pytest.mark.parametrize('D', [1, 13, 40])
def test_the_ordered_sums_agree_with_the_direct_long_double_sums(D):
    frames, T, begin, spk = tw.make_case(D)
    st = stats_of(frames, T, begin, spk)
    s_ld, q_ld = tw.accumulate_ld(tw.S_SPK, frames, T, begin, spk)
    assert st['n'].tolist() == [193, 129, 21, 0]
    for name, got, ref, ab in (('s', st['s'], s_ld, st['sabs']), ('q', st['q'], q_ld, st['qabs'])):
        err = np.abs(got.astype(tw.LD) - ref).astype(np.float64)
        bound = st['n'][:, None] * EPS * ab                          # a float64 sum of n terms, any order (q: + one rounding per square)
        bound = bound + (EPS * ab if name == 'q' else 0)
        print('D=%d %s: worst error / bound = %.3e' % (D, name, np.max(err[bound > 0] / bound[bound > 0])))
        assert (err <= bound).all()


@pytest.mark.parametrize('norm_vars', [True, False])
def test_normalised_speakers_have_zero_mean_and_unit_variance(norm_vars):
    D = 13
    frames, T, begin, spk = tw.make_case(D)
    st = stats_of(frames, T, begin, spk)
    y, status = tw.apply(frames, T, begin, spk, st['n'], st['s'], st['q'], norm_vars, 1e-20, tw.MIN_COUNT)
    assert status.tolist() == [tw.OK, tw.OK, tw.LOW_COUNT, tw.LOW_COUNT]
    for s in (0, 1):
        rows = np.concatenate([np.arange(begin[u], begin[u] + T[u]) for u in np.flatnonzero(spk == s)])
        x, ys = frames[rows].astype(tw.LD), y[rows].astype(tw.LD)
        n = len(rows)
        m, sd = x.mean(axis=0), np.sqrt(np.maximum((x * x).mean(axis=0) - x.mean(axis=0) ** 2, tw.LD(1e-20)))
        scale = sd if norm_vars else np.ones(D, dtype=tw.LD)
        # the mean of y inherits the error of m (n eps sum|x| / n) and one rounding per element, relative to the column's scale
        mean_bound = ((n + 3) * EPS * np.abs(x).mean(axis=0) / scale).astype(np.float64) + 4 * EPS * np.abs(ys).mean(axis=0).astype(np.float64)
        mean = np.abs(ys.mean(axis=0)).astype(np.float64)
        print('speaker %d norm_vars=%s: worst |mean| / bound = %.3e' % (s, norm_vars, np.max(mean / mean_bound)))
        assert (mean <= mean_bound).all()
        if norm_vars:
            live = np.arange(D) != 0 if s == 1 else np.ones(D, dtype=bool)        # speaker 1's column 0 is constant: floored, y = 0
            var = ((ys * ys).mean(axis=0) - ys.mean(axis=0) ** 2).astype(np.float64)
            # v carries the cancellation of q / n - m m: (n + 4) eps (q / n + m m) / v relative
            var_bound = ((n + 4) * EPS * ((x * x).mean(axis=0) + m * m) / (sd * sd)).astype(np.float64) + 8 * EPS
            print('speaker %d: worst |var - 1| / bound = %.3e' % (s, np.max(np.abs(var[live] - 1) / var_bound[live])))
            assert (np.abs(var[live] - 1) <= var_bound[live]).all()
            if s == 1:
                assert not y[rows, 0].any()


def test_mean_only_is_exactly_x_minus_m_and_the_rest_keeps_its_bits():
    D = 5
    frames, T, begin, spk = tw.make_case(D)
    st = stats_of(frames, T, begin, spk)
    y, status = tw.apply(frames, T, begin, spk, st['n'], st['s'], st['q'], False, 1e-20, tw.MIN_COUNT)
    on = tw.touched(len(frames), T, begin, [s >= 0 and status[s] == tw.OK for s in spk])
    assert on.sum() == 193 + 129
    assert y[~on].tobytes() == frames[~on].tobytes()
    for u in np.flatnonzero((spk == 0) | (spk == 1)):
        m = st['s'][spk[u]] / np.float64(st['n'][spk[u]])
        rows = slice(begin[u], begin[u] + T[u])
        assert y[rows].tobytes() == (frames[rows] - m).tobytes()
    r32 = tw.as_rows32(frames.astype(np.float32), y, on)
    assert r32[~on].tobytes() == frames.astype(np.float32)[~on].tobytes() and r32[on].tobytes() == y[on].astype(np.float32).tobytes()


def test_accumulation_over_two_calls_is_one_call_to_rounding_and_n_exactly():
    D = 13
    frames, T, begin, spk = tw.make_case(D)
    one = stats_of(frames, T, begin, spk)
    two = tw.zero(tw.S_SPK, D)
    tw.accumulate(two, frames, T[:3], begin[:3], spk[:3])
    tw.accumulate(two, frames, T[3:], begin[3:], spk[3:])
    assert np.array_equal(one['n'], two['n'])
    for k in ('s', 'q'):                                              # here even the bits: utterance sums are added in the same order
        assert one[k].tobytes() == two[k].tobytes()
    # ... and with the calls the other way round, to rounding
    rev = tw.zero(tw.S_SPK, D)
    tw.accumulate(rev, frames, T[3:], begin[3:], spk[3:])
    tw.accumulate(rev, frames, T[:3], begin[:3], spk[:3])
    for k in ('s', 'q'):
        err, bound = np.abs(one[k] - rev[k]), 4 * EPS * one[k + 'abs']
        print('%s: two calls reversed, worst error / bound %.3e' % (k, np.max(err[bound > 0] / bound[bound > 0])))
        assert (err <= bound).all()


def test_refusals():
    D = 3
    frames, T, begin, spk = tw.make_case(D)
    st = stats_of(frames, T, begin, spk)
    n, s, q = st['n'], st['s'], st['q']
    bad_q = q.copy()
    bad_q[0, 1] = np.inf
    y, status = tw.apply(frames, T, begin, spk, n, s, bad_q, True, 1e-20, tw.MIN_COUNT)
    assert status.tolist() == [tw.NOT_FINITE, tw.OK, tw.LOW_COUNT, tw.LOW_COUNT]
    for u in np.flatnonzero(spk != 1):
        assert y[begin[u]:begin[u] + T[u]].tobytes() == frames[begin[u]:begin[u] + T[u]].tobytes()
    assert tw.statuses(n, s, bad_q, 1000).tolist() == [tw.LOW_COUNT] * 4                      # the count is tested first
    inf_frames = frames.copy()
    inf_frames[begin[0] + 5, 2] = np.inf
    sti = stats_of(inf_frames, T, begin, spk)
    assert tw.statuses(sti['n'], sti['s'], sti['q'], tw.MIN_COUNT).tolist() == [tw.NOT_FINITE, tw.OK, tw.LOW_COUNT, tw.LOW_COUNT]
    for kw in (dict(T=np.array([10, 10]), begin=np.array([0, 5])), dict(T=np.array([10]), begin=np.array([len(frames) - 5])),
               dict(T=np.array([-1]), begin=np.array([0]))):
        with pytest.raises(ValueError):
            tw.check_args(len(frames), kw['T'], kw['begin'])
    for kw in (dict(spk=[4]), dict(spk=[-2]), dict(var_floor=0.0), dict(var_floor=np.nan), dict(var_floor=np.inf), dict(min_count=0)):
        a = dict(spk=[0], S=4, norm_vars=True, var_floor=1e-20, min_count=1)
        a.update(kw)
        with pytest.raises(ValueError):
            tw.check_args(len(frames), [10], [0], **a)
    tw.check_args(len(frames), [10], [0], [0], 4, False, 0.0, 1)                               # the floor is not read without norm_vars
    for w, mw in ((0, 1), (8, 0), (8, 9), ((1 << 20) + 1, 1)):
        with pytest.raises(ValueError):
            tw.sliding(frames, T, begin, w, mw, True)


@pytest.mark.parametrize('window', [7, 8])
@pytest.mark.parametrize('center', [True, False])
def test_window_bounds_against_brute_force(window, center):
    for min_window in (1, window):
        for T in (1, 2, window - 1, window, window + 1, 3 * window):
            lo_all, hi_all = tw.window_bounds_all(T, window, min_window, center)
            for t in range(T):
                lo, hi = tw.window_bounds(t, T, window, min_window, center)
                assert (lo, hi) == (lo_all[t], hi_all[t])
                assert 0 <= lo <= t < hi <= T
                if center:
                    # brute force: among all windows of min(window, T) rows inside [0, T), the one whose start is nearest t - window // 2
                    size = min(window, T)
                    want = min(range(T - size + 1), key=lambda a: abs(a - (t - window // 2)))
                    assert (lo, hi) == (want, want + size), (T, t)
                else:
                    # brute force: the last `window` rows up to t, grown forward to min_window rows where the utterance has them
                    rows = [r for r in range(T) if t - window < r <= t]
                    nxt = t + 1
                    while len(rows) < min_window and nxt < T:
                        rows.append(nxt)
                        nxt += 1
                    assert (lo, hi) == (rows[0], rows[-1] + 1), (T, t)


@pytest.mark.parametrize('center', [True, False])
def test_the_blocked_prefix_differenced_is_the_direct_window_sum(center):
    rng = np.random.default_rng(5)
    T, D, window = 64 * 5 + 17, 3, 100
    x = rng.standard_normal((T, D)) * 3 + 10
    P = tw.prefix(x)
    assert not P[0].any()
    lo, hi = tw.window_bounds_all(T, window, 1, center)
    xl = x.astype(tw.LD)
    worst = 0.0
    for t in range(T):
        got = P[hi[t]] - P[lo[t]]
        ref = xl[lo[t]:hi[t]].sum(axis=0)
        # each prefix is a float64 sum of up to hi terms: hi eps sum|terms up to hi| each, plus the difference's rounding
        bound = (hi[t] + lo[t] + 1) * EPS * np.abs(x[:hi[t]]).sum(axis=0)
        worst = max(worst, np.max(np.abs(got.astype(tw.LD) - ref).astype(np.float64) / bound))
    print('center=%s: worst |P[hi] - P[lo] - direct| / bound = %.3e' % (center, worst))
    assert worst <= 1.0
    y = tw.sliding(x, [T], [0], window, 1, center, True, 1e-20)
    yl = tw.sliding_ld(x, window, 1, center, True, 1e-20)
    err = np.max(np.abs(y.astype(tw.LD) - yl).astype(np.float64))
    print('sliding: max |y64 - y_longdouble| = %.3e' % err)
    # a prefix of up to T terms loses T eps of its sum; q / n - m m (mean 10, sd 3) amplifies that by (q / n + m m) / v ~ 23; y is O(4)
    assert err <= 4 * 23 * T * EPS


def test_sliding_leaves_other_rows_alone_and_reads_only_its_own_utterance():
    frames, T, begin, _ = tw.make_case(4)
    y = tw.sliding(frames, T, begin, 8, 1, False, True, 1e-20)
    on = tw.touched(len(frames), T, begin)
    assert y[~on].tobytes() == frames[~on].tobytes()
    for u in range(len(T)):                                             # one utterance alone gives the same rows
        if T[u]:
            alone = tw.sliding(frames, T[u:u + 1], begin[u:u + 1], 8, 1, False, True, 1e-20)
            assert alone[begin[u]:begin[u] + T[u]].tobytes() == y[begin[u]:begin[u] + T[u]].tobytes()
