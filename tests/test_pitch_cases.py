"""The claims of tests/_pitch_cases.py, held on the CPU (tests/test_gpu_pitch_edges.py runs the cases on the device).

  carries its edge   every case is on the line it is named for: the lag grid has exactly L lags, the LDS cases need exactly 65536 and
                     65544 bytes, the batch has an utterance on both sides of row 256 and of row 512, the twin itself takes the
                     den == 0 / den == inf / db == 0 branches of P2 and each of the six branches of P5 a counted number of times, and so on.
                     An edge that silently is not there is a test that checks nothing.
  can fail           for five defects a kernel could have, a local copy of the twin's function WITH the defect disagrees with the twin on
                     the named case, in the quantity the device test compares and by more than its allowance.
No GPU."""
import numpy as np
import pytest

import _pitch_cases as pc
import _pitch_twin as pt


def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


# ------------------------------------------------------------------ carries its edge
@pytest.mark.parametrize('L', sorted(pc.LAG_GRID))
def test_lag_grid_cases_have_exactly_their_lags(L):
    c = pc.lag_grid(L)
    size, step, lmin, lmax = pc.geometry(c)
    assert lmax - lmin + 1 == L == pc.lags(c)
    assert 2 <= L <= 1024 and (L + 63) // 64 == {2: 1, 63: 1, 1023: 16, 1024: 16}[L]      # waves of the workgroup
    assert pc.lds_bytes(c) <= pc.LDS_LIMIT // 4                                          # far below the LDS limit
    T = pc.frames(c)
    assert T[1] == 1 and 5 <= T[0] <= 10
    lag = pc.expect(c)[0]['lag']
    print(c['name'], 'T', T, 'lags taken', np.unique(lag))
    if L == 2:                                           # li > 0 && li < L - 1 is never true; both lags are taken all the same
        assert set(np.unique(lag)) == {lmin, lmax}


def test_lds_cases_are_the_last_accepted_window_and_the_first_refused():
    for extra, size in ((0, 7808), (1, 7809)):
        c = pc.lds(extra)
        got_size, step, lmin, lmax = pc.geometry(c)
        assert got_size == size == int(c['rate'] * c['kw']['sampletime']) and (lmin, lmax) == (40, 320)
        assert pc.lds_bytes(c) == (size + lmax + 64) * 8 == 65536 + 8 * extra
        assert pc.frames(c) == [3]
    assert pc.lds_bytes(pc.lds(0)) == pc.LDS_LIMIT and pc.lds_bytes(pc.lds(1)) == pc.LDS_LIMIT + 8


def test_frame_geometry_cases():
    c = pc.overlap_one()
    size, step, _, _ = pc.geometry(c)
    assert size == step == 200 and pc.frames(c) == [4, 1] and (len(c['sigs'][0]) - size) % step != 0
    c = pc.odd_size()
    size, step, _, _ = pc.geometry(c)
    assert (size, step) == (201, 100) and size % 2 == 1 and pc.frames(c) == [6, 2]
    assert (len(c['sigs'][0]) - size) % step == 33 and (len(c['sigs'][1]) - size) % step == 0
    for alone in (False, True):
        c = pc.ragged_tail(alone)
        size, step, lmin, lmax = pc.geometry(c)
        n, T = len(c['sigs'][0]), pc.frames(c)[0]
        assert T == 4 and (T - 1) * step + size == n                                      # the last frame's own samples are inside ...
        assert (T - 2) * step + size + lmax <= n                                          # ... as is all of the frame before it
        assert len(c['sigs']) == (1 if alone else 2)
    full = pc.ragged_tail()['sigs'][1]
    assert full.dtype == np.int16 and set(np.unique(full)) == {-32768, 32767}
    assert np.array_equal(pc.ragged_tail()['sigs'][0], pc.ragged_tail(True)['sigs'][0])


@pytest.mark.parametrize('given', [False, True])
def test_the_batch_straddles_rows_256_and_512(given):
    c = pc.straddle(given)
    T, off = pc.frames(c), pc.row_off(c)
    assert tuple(T) == pc.straddle_frames() and pc.lags(c) == 65
    assert 512 < off[-1] < 700 and len(T) == 46 and set(T) == set(range(1, 21)) | {pc.STRADDLE_T}
    hit = pc.straddling(c)
    print(c['name'], 'rows', off[-1], 'straddling (utterance, k):', hit, [(int(off[u]), int(off[u + 1])) for u, _ in hit])
    assert {k for _, k in hit} == {1, 2}
    for u, k in hit:
        assert off[u] < 256 * k < off[u] + T[u] and 256 * k - off[u] >= 2 and off[u + 1] - 256 * k >= 2
    assert [T[u] for u, _ in hit if T[u] == pc.STRADDLE_T] == [pc.STRADDLE_T] * 2
    if given:
        assert all(b.shape == (t, 65) for b, t in zip(c['nccf'][0], T))
    else:                                                # some step does not divide n - size
        size, step, _, _ = pc.geometry(c)
        assert sum((len(x) - size) % step != 0 for x in c['sigs'] if len(x) > size) > 20


def test_p2_cases_take_the_twins_degenerate_branches():
    n = {}
    for which in pc.P2_CASES:
        c = pc.p2(which)
        assert pc.lags(c) == 65 and pc.frames(c) == [6, 1]
        terms = [pc.p2_terms(c, u) for u in range(2)]
        for u, (p, den, db) in enumerate(terms):         # the copy of the sums is the twin's
            bal, raw = pc.nccf_of_windows(pt.windows(c['sigs'][u], *pc.geometry(c)[:2], pc.geometry(c)[3]), pc.geometry(c)[0],
                                          *pc.geometry(c)[2:], c['kw'].get('ballast', pt.BALLAST))
            assert np.array_equal(bal, pc.expect(c)[u]['bal']) and np.array_equal(raw, pc.expect(c)[u]['raw'])
        n[which] = dict(den0=sum(int(((den == 0.0) & (p != 0.0)).sum()) for p, den, db in terms),
                        inf=sum(int(np.isinf(den).sum()) for p, den, db in terms),
                        db0=sum(int((db == 0.0).sum()) for p, den, db in terms),
                        entries=sum(p.size for p, den, db in terms))
        for r in pc.expect(c):                           # finite inputs: no NaN in anything the device test compares
            assert np.isfinite(r['out']).all() and np.isfinite(r['bal']).all() and np.isfinite(r['raw']).all()
    print(n)
    assert n['underflow']['den0'] == n['underflow']['entries'] > 0                        # den == 0 with p != 0, everywhere
    u = pc.expect(pc.p2('underflow'))
    assert all(np.all(r['raw'] == 0.0) and np.any(r['bal'] != 0.0) for r in u)
    assert n['overflow']['inf'] > 0 and all(np.all(r['raw'] == 0.0) and np.all(r['bal'] == 0.0) for r in pc.expect(pc.p2('overflow')))
    assert n['ballast0-silence']['db0'] == n['ballast0-silence']['entries'] > 0
    for r in pc.expect(pc.p2('ballast0')):
        assert np.array_equal(r['bal'], r['raw']) and np.abs(r['raw']).max() > 0.3
    assert n['ballast0']['db0'] == 0
    x = pc.p2('int16-extremes')['sigs'][0]
    assert x.dtype == np.int16 and set(np.unique(x)) == {-32768, 32767}
    assert min(np.abs(s).min() for s in pc.p2('dc-offset')['sigs']) > 2.9e7 and pc.p2('dc-offset')['sigs'][0].dtype == np.float64


def test_p5_case_takes_every_branch():
    c = pc.p5()
    _, _, lmin, lmax = pc.geometry(c)
    total = None
    for r in pc.expect(c):
        n = pc.p5_branches(r['raw'], r['lag'] - lmin)
        total = n if total is None else {k: total[k] + n[k] for k in n}
    print(total)
    assert all(v > 0 for v in total.values()), total
    assert total['li == 0'] >= 4 and total['li == L - 1'] >= 4
    # the track did take the lag each frame was built for, the two next to the ends among them
    lag = np.concatenate([r['lag'] for r in pc.expect(c)]) - lmin
    assert np.array_equal(lag, np.concatenate([b.argmax(axis=1) for b in c['nccf'][0]]))
    assert 1 in lag and pc.lags(c) - 2 in lag
    shift = np.concatenate([pt.refine(r['raw'], r['lag'] - lmin, lmin) - r['lag'] for r in pc.expect(c)])
    assert (shift == 0.5).sum() > total['clamped +0.5'] and (shift == -0.5).sum() == total['clamped -0.5']   # 'exact+' sits ON 0.5


def test_track_cases():
    T = {w: pc.frames(pc.track(w)) for w in pc.TRACK_CASES}
    assert T['T600-L65'] == [600] and pc.lags(pc.track('T600-L65')) == 65
    assert T['T300-L281'] == [300] and pc.lags(pc.track('T300-L281')) == 281
    assert T['mixed'] == [1, 2, 3, 257, 1]
    assert pc.track('pf0')['kw']['pf'] == 0.0 and 1 in T['pf0']
    f = pc.fac(pc.track('negative-fac'))
    assert f.min() < 0.0 < f.max() and f[0] == 0.5 and np.isclose(f[-1], -1.1)
    for w in pc.TRACK_CASES:                             # the coarse grid: every frame of bal holds equal values
        for b in pc.track(w)['nccf'][0]:
            assert all(len(np.unique(row)) < len(row) for row in b)
    # pf = 0: every lane's argmin is the previous column's first minimum -- and that minimum is a tie in most columns
    c = pc.track('pf0')
    b = c['nccf'][0][0]
    assert np.mean([(row == row.max()).sum() > 1 for row in b]) > 0.9


# ------------------------------------------------------------------ can fail: planted defects
def test_delta_clamped_to_the_batch_is_caught_on_the_straddle_case():
    c = pc.straddle()
    ref = pc.expect(c)
    off = pc.row_off(c)
    col = np.concatenate([r['out'][:, 1] for r in ref])
    bad = pt.delta(col)                                  # t +- 1, t +- 2 clamped to the batch's rows
    good = np.concatenate([r['out'][:, 2] for r in ref])
    for u, k in pc.straddling(c):
        sl = slice(off[u], off[u + 1])
        scale = np.spacing(np.abs(col[sl]).max())
        d = np.abs(bad[sl] - good[sl]) / scale
        print('utterance', u, 'rows', off[u], off[u + 1], 'delta off by up to %.3g ulp of ln f0' % d.max())
        assert d.max() > 1e6 and d.max() > 4.0           # the device test allows 4
        assert np.array_equal(bad[off[u] + 2:off[u + 1] - 2], good[off[u] + 2:off[u + 1] - 2])   # (only the utterance's edges)
    assert sum(not np.array_equal(bad[off[u]:off[u + 1]], good[off[u]:off[u + 1]]) for u in range(len(ref))) >= len(ref) - 2


def windows_variant(flat, off, u, size, step, lmax, read_on=False, plain_mean=False):
    """pt.windows on utterance u of the concatenated samples, with the two defects to plant"""
    n = off[u + 1] - off[u]
    T = pt.frame_count(n, size, step)
    W = size + lmax
    end = len(flat) if read_on else off[u + 1]           # read_on: the tail runs into the next utterance's samples
    pad = np.zeros((T - 1) * step + W)
    seg = np.asarray(flat[off[u]:end], dtype=np.float64)[:len(pad)]
    pad[:len(seg)] = seg
    w = np.stack([pad[t * step:t * step + W] for t in range(T)])
    if plain_mean:                                       # one ascending sum
        tot = np.zeros(T)
        for i in range(size):
            tot = tot + w[:, i]
    else:
        part = np.zeros((T, 64))
        for i0 in range(0, size, 64):
            blk = w[:, i0:min(i0 + 64, size)]
            part[:, :blk.shape[1]] = part[:, :blk.shape[1]] + blk
        tot = np.zeros(T)
        for j in range(64):
            tot = tot + part[:, j]
    return w - (tot / float(size))[:, None]


def variant_nccf(c, u, **defect):
    size, step, lmin, lmax = pc.geometry(c)
    off = np.concatenate([[0], np.cumsum([len(x) for x in c['sigs']])])
    flat = np.concatenate([np.asarray(x, dtype=np.float64) for x in c['sigs']])
    return pc.nccf_of_windows(windows_variant(flat, off, u, size, step, lmax, **defect), size, lmin, lmax, c['kw'].get('ballast', pt.BALLAST))


def test_a_tail_that_reads_the_next_utterance_is_caught_on_the_ragged_tail_case():
    c = pc.ragged_tail()
    ref = pc.expect(c)[0]
    bal, raw = variant_nccf(c, 0)
    assert np.array_equal(bal, ref['bal']) and np.array_equal(raw, ref['raw'])           # the copy without the defect IS the twin
    bal, raw = variant_nccf(c, 0, read_on=True)
    rows = np.flatnonzero((raw != ref['raw']).any(axis=1))
    print('rows whose raw differs:', rows, 'by up to', np.abs(raw - ref['raw']).max())
    assert list(rows) == [3] and np.abs(raw - ref['raw']).max() > 0.1
    # and the twin's answer for it does not depend on what follows
    alone = pc.expect(pc.ragged_tail(True))[0]
    assert all(np.array_equal(alone[k], ref[k]) for k in ('out', 'lag', 'bal', 'raw'))


def test_a_plain_ascending_mean_is_caught_on_the_dc_offset_case():
    c = pc.p2('dc-offset')
    n = 0
    for u in range(2):
        ref = pc.expect(c)[u]
        bal, raw = variant_nccf(c, u)
        assert np.array_equal(bal, ref['bal']) and np.array_equal(raw, ref['raw'])
        bal, raw = variant_nccf(c, u, plain_mean=True)
        n += int((bal != ref['bal']).sum())
        print('utterance', u, 'bal entries with other bits:', int((bal != ref['bal']).sum()), 'of', bal.size)
    assert n > 0
    # without the offset the integer samples sum exactly in either order: the offset IS what makes the order show
    plain = pc.p2('int16-extremes')
    assert np.array_equal(variant_nccf(plain, 0, plain_mean=True)[0], pc.expect(plain)[0]['bal'])


def refine_wrapping(raw, idx, lmin):
    """pt.refine without the li > 0 test: lag index -1 is NumPy's (and a wrapped pointer's) L - 1"""
    T, L = raw.shape
    out = np.empty(T)
    for t in range(T):
        li = int(idx[t])
        shift = 0.0
        if li < L - 1:
            ym, y0, yp = raw[t, li - 1], raw[t, li], raw[t, li + 1]
            den = (ym - 2.0 * y0) + yp
            if den < 0.0:
                shift = min(0.5, max(-0.5, 0.5 * (ym - yp) / den))
        out[t] = float(lmin + li) + shift
    return out


def test_a_refinement_that_wraps_at_the_first_lag_is_caught_on_the_p5_case():
    c = pc.p5()
    _, _, lmin, _ = pc.geometry(c)
    worst = []
    for r in pc.expect(c):
        idx = r['lag'] - lmin
        assert np.array_equal(np.log(c['rate'] / pt.refine(r['raw'], idx, lmin)), r['out'][:, 1])
        bad = np.log(c['rate'] / refine_wrapping(r['raw'], idx, lmin))
        u = ulps(bad, r['out'][:, 1])
        assert np.all(u[idx != 0] == 0.0)
        if (idx == 0).any():
            worst.append(u[idx == 0].min())
    print('ln f0 of the rows at li = 0 off by at least', worst, 'ulp')
    assert len(worst) == 2 and min(worst) > 1e6 and min(worst) > 4.0


def track_ties_to_the_largest(bal, rate, lmin, g, soft_min_f0=pt.SOFT_MIN_F0, pf=pt.PF):
    """pt.track with `cand <= m` where the rule says `cand < m`"""
    T, L = bal.shape
    fac = 1.0 - soft_min_f0 * np.arange(lmin, lmin + L, dtype=np.float64) / float(rate)
    c = 1.0 - bal * fac[None, :]
    d = g[:, None] - g[None, :]
    trans = pf * (d * d)
    best = c[0].copy()
    bp = np.zeros((T, L), dtype=np.int64)
    for t in range(1, T):
        cand = best[None, :] + trans
        arg = L - 1 - np.argmin(cand[:, ::-1], axis=1)   # the last of equal minima
        best = c[t] + cand[np.arange(L), arg]
        bp[t] = arg
    idx = np.zeros(T, dtype=np.int64)
    idx[T - 1] = int(np.argmin(best))
    for t in range(T - 1, 0, -1):
        idx[t - 1] = bp[t, idx[t]]
    return idx


def test_ties_to_the_largest_lag_are_caught_on_the_pf0_case():
    c = pc.track('pf0')
    _, _, lmin, lmax = pc.geometry(c)
    g = pt.log_lags(lmin, lmax)
    differ = []
    for bal, r in zip(c['nccf'][0], pc.expect(c)):
        bad = track_ties_to_the_largest(bal, c['rate'], lmin, g, **pc.track_kw(c)) + lmin
        differ.append(int((bad != r['lag']).sum()))
    print('frames whose lag differs, per utterance:', differ, 'of', pc.frames(c))
    assert differ[0] > 10 and differ[1] == 0             # (T = 1 has no predecessor to tie over)
    # where no minimum is a tie the copy IS the twin: the defect is the only difference
    rng = np.random.default_rng(1)
    free = rng.uniform(-1, 1, (12, lmax - lmin + 1))
    assert np.array_equal(track_ties_to_the_largest(free, c['rate'], lmin, g), pt.track(free, c['rate'], lmin, g))
