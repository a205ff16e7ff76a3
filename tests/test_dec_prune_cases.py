"""CPU companion of tests/test_gpu_dec_prune.py: every case of tests/_dec_prune_cases.py reaches the edge it is there for.  The edges
are stated against `select_path`, a NumPy restatement of the rounds of pcl_select_kth (hmm_decode_common.h), and against the hash of
pcl_prune_stats; the conditions the device test rests on are asserted here, where no device is needed."""
import numpy as np
import pytest

import _dec_prune_cases as dc

U64 = np.uint64
ALL = sorted({(which, n) for which, k in dc.INSTANTIATIONS for n in dc.sizes(dc.GEOMETRY[which]['NT'], k)})


def everything(which):
    return [(c, dc.reference_of(which, c)) for w, n in ALL if w == which for c in dc.cases_at(which, n)]


def of(which, family, name=None):
    return [(c, r) for c, r in everything(which) if c['family'] == family and name in (None, c['name'])]


def keys_of(c):
    return dc.okey(c['score'][c['part'] != 0])


def hb_of(keys):
    d = int(keys.min()) ^ int(keys.max())
    return d.bit_length() - 1 if d else None


def test_geometry_is_the_kernels_own():
    g, l = dc.GEOMETRY['general'], dc.GEOMETRY['lr']
    assert (1 << g['HB']) == 256 and g['CAND'] == 0 and g['NT'] % 64 == 0 and g['NT'] >= 256
    assert l['CAND'] > 0 and l['NT'] % 64 == 0 and l['NT'] >= 256 and (1 << l['HB']) % l['NT'] == 0
    for which, k in dc.INSTANTIATIONS:
        NT = dc.GEOMETRY[which]['NT']
        want = {1, 63, 64, 65, NT - 1, NT, NT + 1, (k - 1) * NT + 1, k * NT - 1, k * NT}
        assert set(dc.sizes(NT, k)) == {n for n in want if n <= k * NT}


@pytest.mark.parametrize('which', ['general', 'lr'])
def test_inputs_stay_inside_the_kernels_contract(which):
    """No NaN, no +inf, not both zeros; and the packed arrays address every token exactly once."""
    for c, r in everything(which):
        s = c['score']
        assert not np.isnan(s).any() and not (s == np.inf).any(), dc.case_id(c)
        z = s[s == 0]
        assert len(set(np.signbit(z).tolist())) <= 1, dc.case_id(c)
        assert c['part'].dtype == np.int32 and len(c['part']) == c['n'] == len(s)
        assert 0.0 <= c['beam'] <= 1.0
    ids = [dc.case_id(c) for c, _ in everything(which)]
    assert len(ids) == len(set(ids))
    for inst in dc.INSTANTIATIONS:
        if inst[0] == which:
            cases = dc.prune_cases(inst)
            p = dc.pack_prune(cases)
            assert p['n'].max() <= inst[1] * dc.GEOMETRY[which]['NT'] and len(p['score']) == len(p['part']) == int(p['n'].sum())
            assert (p['off'][1:] == p['off'][:-1] + p['n'][:-1]).all() and p['off'][0] == 0


@pytest.mark.parametrize('which', ['general', 'lr'])
def test_the_twin_selects_what_the_sort_selects(which):
    """The path twin is only trusted for its account of the rounds because its result is the sort's, case by case."""
    seen = 0
    for c, r in everything(which):
        if r['prune']:
            assert (r['path']['sel'], r['path']['rank']) == (r['sel'], r['rank']), dc.case_id(c)
            assert 0 <= r['rank'] < r['path']['eq']
            assert int(r['gone'].sum()) == r['m']
            seen += 1
        else:
            assert not r['gone'].any()
    assert seen > 100


@pytest.mark.parametrize('which', ['general', 'lr'])
def test_participation_family(which):
    NT = dc.GEOMETRY[which]['NT']
    for c, r in of(which, 'participation'):
        n, part = c['n'], c['part']
        if c['name'] == 'all':
            assert r['n_old'] == n
        elif c['name'] == 'half':
            assert n < 63 or 0 < r['n_old'] < n
        elif c['name'] == 'one':
            assert r['n_old'] == 1 and not r['prune']
        elif c['name'] == 'none':
            assert r['n_old'] == 0 and not r['prune'] and r['kmin'] == 2 ** 64 - 1 and r['kmax'] == 0 and r['bins'] == 0
        else:
            C, w = -(-n // NT) * 64, c['want']['wave']
            assert C == c['want']['C'] and w == (n - 1) // C
            assert not part[w * C:(w + 1) * C].any() and part[:w * C].all() and part[(w + 1) * C:].all()
    assert {c['name'] for c, _ in of(which, 'participation')} == {'all', 'half', 'one', 'none', 'wave'}
    assert any(c['want']['wave'] >= 2 and r['prune'] for c, r in of(which, 'participation', 'wave'))


@pytest.mark.parametrize('which', ['general', 'lr'])
def test_key_range_family(which):
    HB, CAND = dc.GEOMETRY[which]['HB'], dc.GEOMETRY[which]['CAND']
    names = {'loglik', 'signs600', 'some_ninf', 'all_ninf', 'equal', 'hb0', 'hbHB-2', 'hbHB-1', 'hbHB', 'hbHB+1', 'clamp'}
    assert {c['name'] for c, _ in of(which, 'key_range')} == names
    first_round_at_0 = clamped = 0
    for c, r in of(which, 'key_range'):
        n, keys, want, p = c['n'], keys_of(c), c['want'], r['path']
        assert r['n_old'] == n and r['prune'] == (n >= 2) and (p is None or p['hb'] == hb_of(keys))
        if c['name'] == 'loglik':
            assert n < 64 or 40 <= hb_of(keys) <= 55                      # low exponent bits at most: all the decode-level tests reach
        elif c['name'] == 'signs600':
            assert hb_of(keys) == want['hb'] and (n < 2 or ((c['score'] > 0).any() and (c['score'] < 0).any()))
            a = np.abs(c['score'])
            assert n < 64 or np.log10(a.max()) - np.log10(a.min()) > 550
        elif c['name'] == 'some_ninf':
            assert n < 2 or (np.isinf(c['score']).any() and np.isfinite(c['score']).any())
        elif c['name'] in ('all_ninf', 'equal'):
            assert hb_of(keys) is None and (p is None or (p['ret'] == 'equal' and p['shifts'] == [] and p['eq'] == n))
        elif c['name'].startswith('hb'):
            hb = want['hb']
            assert hb_of(keys) == hb and (n < 2 or hb == {'hb0': 0, 'hbHB-2': HB - 2, 'hbHB-1': HB - 1, 'hbHB': HB, 'hbHB+1': HB + 1}[c['name']])
            # a chain of np.nextafter steps: the next key up is the next float64 up
            k = np.unique(keys)
            assert (dc.from_keys(k + U64(1)) == np.nextafter(dc.from_keys(k), np.inf)).all()
            if n >= 2 and hb < HB:
                assert p['shifts'] == [0] and p['ret'] == 'shift0'
                first_round_at_0 += 1
            if n >= 2 and hb >= HB:
                assert p['shifts'][0] == hb - (HB - 1) and p['shifts'][0] % HB != 0
                assert (p['shifts'] == [hb - (HB - 1), 0] and p['ret'] == 'shift0') or (p['ret'] == 'cand' and p['counts'][0] <= CAND)
        else:
            assert n < 2 or hb_of(keys) == HB + 3
            if want['shifts']:
                assert p['shifts'] == want['shifts'] == [4, 0] and p['ret'] == 'shift0' and p['counts'][0] == n - 1
                clamped += 1
            else:
                assert n < 3 or (CAND > 0 and n - 1 <= CAND and p['ret'] == 'cand')
    assert first_round_at_0 >= 20 and clamped >= 3


def test_candidate_path_family():
    HB, CAND, NT = (dc.GEOMETRY['lr'][k] for k in ('HB', 'CAND', 'NT'))
    assert not of('general', 'candidate')
    names = {'bin_CAND', 'bin_CAND+1', 'round2', 'all_equal', 'run_first', 'run_last'}
    for k in (8, 16):
        assert {c['name'] for c in dc.prune_cases(('lr', k)) if c['family'] == 'candidate'} == names
    for c, r in of('lr', 'candidate'):
        want, p = c['want'], r['path']
        assert r['prune'] and r['n_old'] == c['n'] and p['hb'] == 31 and p['shifts'][0] == 31 - (HB - 1) and p['ret'] == 'cand'
        assert p['cand_round'] == want['cand_round'] == len(p['counts']) and p['counts'][-1] <= CAND
        if 'counts0' in want:
            assert p['counts'][0] == want['counts0']
        if c['name'] == 'bin_CAND':
            assert p['counts'] == [CAND]
        elif c['name'] == 'bin_CAND+1':
            assert p['counts'][0] == CAND + 1 and p['counts'][1] <= CAND
        elif c['name'] == 'round2':
            assert p['counts'][0] > CAND >= p['counts'][1] >= want['counts1_min'] and p['eq'] > 1
        elif c['name'] == 'all_equal':
            assert p['counts'][0] == p['eq'] == want['eq'] <= CAND                   # the candidate list holds one value, eq times
        else:
            assert p['counts'][0] <= CAND and p['eq'] == want['eq'] >= 3 and p['rank'] == want['rank']
            assert p['rank'] == (0 if c['name'] == 'run_first' else p['eq'] - 1)
    # every size has the cases it can hold; the small ones (at most CAND keys in all) are ranked in round one
    assert {c['n'] for c, _ in of('lr', 'candidate', 'all_equal')} == {n for w, n in ALL if w == 'lr' and n >= 2}
    assert {c['n'] for c, _ in of('lr', 'candidate', 'bin_CAND')} == {n for w, n in ALL if w == 'lr' and n > CAND}


@pytest.mark.parametrize('which', ['general', 'lr'])
def test_cut_position_family(which):
    NT = dc.GEOMETRY[which]['NT']
    assert {c['name'] for c, _ in of(which, 'cut')} == {'m1', 'm_n-1', 'm_n', 'beam1', 'tie_first', 'tie_mid', 'tie_last'}
    wide = 0
    for c, r in of(which, 'cut'):
        n, want = c['n'], c['want']
        assert r['n_old'] == n
        if c['name'] == 'm1' and n == 1:
            assert r['m'] == 1 and c['beam'] == 0.0
        else:
            assert r['m'] == want['m']
        assert r['prune'] == (r['m'] > 0)
        if c['name'] == 'm_n':
            assert r['m'] == n and r['gone'].all()
        elif c['name'] == 'beam1':
            assert c['beam'] == 1.0 and not r['gone'].any()
        elif c['name'].startswith('tie'):
            C = -(-n // NT) * 64
            assert r['path']['eq'] == want['eq'] >= 3 and r['rank'] == want['rank'] == {'tie_first': 0, 'tie_mid': want['eq'] // 2,
                                                                                     'tie_last': want['eq'] - 1}[c['name']]
            pos = np.flatnonzero(dc.okey(c['score']) == U64(r['sel']))
            assert len({int(p) // C for p in pos}) == want['waves'] >= min(3, -(-n // C))
            assert len({(int(p) % C) // 64 for p in pos}) == want['slots'] >= (2 if C >= 128 else 1)
            wide += want['waves'] >= 3 and want['slots'] >= 2
    assert wide >= (3 if which == 'lr' else 3)
    for k in [k for w, k in dc.INSTANTIATIONS if w == which and k >= 2]:          # (one key slot per lane at KMAX 1: no second slot to span)
        assert any(c['want']['waves'] >= 3 and c['want']['slots'] >= 2 for c in dc.prune_cases((which, k)) if c['name'].startswith('tie'))


@pytest.mark.parametrize('which', ['general', 'lr'])
def test_distinct_scores_family(which):
    seen, overturned, held = set(), 0, 0
    for c, r in of(which, 'distinct'):
        md, want = c['min_distinct'], c['want']
        distinct = len(set(c['score'].tolist()))
        assert distinct == want['distinct'] and r['n_old'] == c['n'] and r['bins'] <= min(distinct, 256)
        assert r['prune'] == (r['m'] > 0 and distinct >= md)
        seen.add((md, distinct - md))
        if c['name'].startswith('collide'):
            assert r['bins'] == want['bins'] == md - 1 < md <= distinct
        if r['ran_distinct']:
            assert r['bins'] < md <= r['n_old'] and r['m'] > 0
            overturned += r['prune']                                   # bins < min_distinct <= distinct: the exact count overturns the map
            held += not r['prune']
    assert seen == {(md, d) for md in (1, 3, 8, 300) for d in (-1, 0, 1)} - {(1, -1)}
    assert any(c['name'] == 'collide_md3' and r['ran_distinct'] and r['prune'] for c, r in of(which, 'distinct'))
    assert any(c['name'] == 'collide_md8' and r['ran_distinct'] and r['prune'] for c, r in of(which, 'distinct'))
    assert any(c['min_distinct'] == 300 and r['ran_distinct'] and r['prune'] for c, r in of(which, 'distinct'))      # min_distinct > 256 bins
    assert overturned >= 10 and held >= 10


@pytest.mark.parametrize('inst', dc.INSTANTIATIONS, ids=dc.inst_id)
def test_every_instantiation_takes_every_path(inst):
    which = inst[0]
    rets = [dc.reference_of(which, c)['path']['ret'] for c in dc.prune_cases(inst) if dc.reference_of(which, c)['prune']]
    assert set(rets) == ({'equal', 'shift0', 'cand'} if which == 'lr' else {'equal', 'shift0'})
    assert any(dc.reference_of(which, c)['ran_distinct'] for c in dc.prune_cases(inst))
    assert any(dc.reference_of(which, c)['path']['hb'] == 63 for c in dc.prune_cases(inst) if dc.reference_of(which, c)['prune'])


@pytest.mark.parametrize('which', ['general', 'lr'])
def test_transfer_cases(which):
    NT = dc.GEOMETRY[which]['NT']
    cases = dc.transfer_cases(NT)
    assert {c['n'] for c in cases} == {0, 1, 63, 65, NT + 1, 16 * NT}
    assert {c['family'] for c in cases} == set(dc.TRANSFER_FAMILIES)
    for c in cases:
        n, sc = c['n'], c['sc']
        assert {x['candidate'] for x in cases if x['n'] == n and x['family'] == c['family']} == {1, 6, n, n + 3}
        assert not np.isnan(sc).any() and not (sc == np.inf).any() and not (sc == 0).any()
        idx = c['map'].view(np.uint32) & np.uint32(0x7fffffff)
        assert sorted(idx.tolist()) == list(range(n)) and (n < 63 or 0 < (c['map'] < 0).sum() < n)
        n_out, nd, s, hs = dc.transfer_reference(c)
        assert n_out == min(c['candidate'], n) and (s[1:] <= s[:-1]).all()
        if c['family'] == 'tied_best' and dc.tied_positions(n, NT):
            pos = dc.tied_positions(n, NT)
            assert (sc[pos] == sc.max()).all() and (sc == sc.max()).sum() == len(pos)
            if n > NT:
                assert len({(p % NT) // 64 for p in pos}) >= 2                       # different waves ...
                assert any(p % NT == q % NT and p != q for p in pos for q in pos)    # ... and different strides of one lane
                assert pos[2] < pos[3] and pos[2] % NT > pos[3] % NT                 # token order is not thread order
        elif c['family'] == 'all_ninf':
            assert n == 0 or (sc == -np.inf).all()
        elif c['family'] == 'equal':
            assert len(set(sc.tolist())) <= 1
        elif c['family'] == 'descending':
            assert (np.diff(sc) < 0).all()
        elif c['family'] == 'ascending':
            assert (np.diff(sc) > 0).all()
    p = dc.pack_transfer(cases, True)
    q = dc.pack_transfer(cases, False)
    c = cases[-1]
    assert (p['sc'][p['off'][-1]:][c['map'].view(np.uint32) & np.uint32(0x7fffffff)] == q['sc'][q['off'][-1]:]).all()
