"""The claims of tests/_acc16_cases.py, held on the CPU: every case reaches the edge of csrc/gmm_accumulate_f16.hip it is named for, and its
inputs are ones an f32-class evaluation can be held to the float64 oracle on (tests/test_gpu_acc16_edges.py does that on the device)."""
import math

import numpy as np
import pytest

import _acc16_cases as ac
from _oracle_pool import f32_evaluation_bound_rows

CASES = ac.all_cases()


def state_bound(c, j):
    idx = ac.survivors(c, j)
    return float(f32_evaluation_bound_rows([(c['mean'][j], c['var'][j], c['w'][j])], c['frames'][idx]).max()) if len(idx) else 0.0


@pytest.mark.parametrize('mk', [m for _, m in CASES], ids=[i for i, _ in CASES])
def test_case_is_well_formed(mk):
    """Virtual rows and non-survivors at -inf, survivor counts as stated, survivors scattered (not a prefix) unless the case orders them on
    purpose, ln gamma in [ln 1e-3, 0] (the scale cases set their own) and distinct per frame where it is drawn."""
    c = mk()
    J, M, D = c['mean'].shape
    lg = c['lgamma']
    assert lg.shape == (J + 2, c['frames'].shape[0]) and np.isneginf(lg[0]).all() and np.isneginf(lg[-1]).all()
    assert c['frames'].dtype == np.float64 and (c['frames'] + 100.0 > 0).all()          # (the reference takes ln(o + 100))
    for j in range(J):
        idx = ac.survivors(c, j)
        assert len(idx) == c['counts'][j]
        vals = lg[1 + j, idx]
        if c['name'].startswith('scale'):
            continue
        assert ((vals >= ac.LG_LO) & (vals <= 0.0)).all() and len(np.unique(vals)) == len(vals)
        if 0 < len(idx) < lg.shape[1]:
            assert idx[-1] >= len(idx), 'state %d keeps a prefix of the frames' % j
    assert ac.padded_dim(D) in (13, 26, 39, 47) and ac.padded_dim(D) % 8 != 0


@pytest.mark.parametrize('mk', [m for _, m in CASES], ids=[i for i, _ in CASES])
def test_f32_evaluation_bound(mk):
    """What any f32 evaluation of a survivor's exponent may lose: at most 2.5e-5 nats outside the masked case, 5e-4 inside (so the masked
    rtol 1e-4 + 4 x the bound stays under 2.1e-3)."""
    c = mk()
    worst = max(state_bound(c, j) for j in range(c['mean'].shape[0]))
    cap = 5e-4 if c['masked'] else 2.5e-5
    assert worst <= cap, worst
    assert 1e-4 + 4.0 * cap <= 2.1e-3


def test_every_tile_count_and_ring_phase():
    c = ac.ladder()
    t = ac.tiles_of(c['counts'])
    assert set(range(1, 8)) | {9, 13} <= set(t)
    assert {ac.AHEAD, ac.AHEAD + 1, ac.NSLOT + 1} <= set(t)
    assert t[0] == 0 and t[-1] == 0 and 0 in t[1:-1]
    off = ac.tile_offsets(c['counts'], 39)
    assert {int(o) % ac.NSLOT for o, n in zip(off, t) if n} == set(range(ac.NSLOT))
    assert len(ac.state_groups(c['counts'], 39)) == 2              # (the launcher's small first group: the numbering restarts once)
    last = {int(n) - 32 * ((int(n) - 1) // 32) for n in c['counts'] if n}
    assert {1, 31, 32} <= last
    # the groups case adds the phases of states that follow each other in steps of ten tiles, under either budget
    g = ac.groups()
    assert {int(o) % ac.NSLOT for o in ac.tile_offsets(g['counts'], 47, 1)} == {0, 2, 4}
    assert len(ac.state_groups(g['counts'], 47, 1)) >= 3 and ac.state_groups(g['counts'], 47, 1)[1][2] * ac.image_geometry(47)['NB'] * 1024 <= 1 << 20


def test_ladder_split_state():
    c = ac.ladder()
    for j in range(c['mean'].shape[0]):
        _, off, _ = ac.derive_replica(c['mean'][j], c['var'][j])
        assert tuple(np.flatnonzero(off)) == tuple(c['split'].get(j, ()))
    assert c['counts'][ac.LADDER_SPLIT_STATE] > 32 and ac.LADDER_SPLIT_MIX[0] < 31      # on-pipe mixtures shift rows, across an m-tile edge
    for _, mk in ac.all_cases()[1:]:
        k = mk()
        assert not any(ac.derive_replica(k['mean'][j], k['var'][j])[1].any() for j in range(k['mean'].shape[0])), k['name']


def test_dims_geometry():
    got = {d: ac.image_geometry(ac.padded_dim(d)) for d in ac.DIMS + [39]}
    assert [got[d]['KS'] for d in (13, 26, 47, 39)] == [2, 4, 6, 5]
    assert [got[d]['extra'] for d in (13, 26, 47, 39)] == [1, 1, 1, 3]
    assert [got[d]['s0_row'] for d in (13, 26, 47, 39)] == [21, 18, 23, 7]
    assert ac.padded_dim(12) == 13 and ac.padded_dim(40) == 47
    for d in ac.DIMS:
        assert set(ac.tiles_of(ac.dims(d)['counts'])) == {0, 1, 2, 5, 6, 7}


def test_mixture_slices():
    ms = sorted({m for m, _ in ac.MIXTURES})
    assert ms == [1, 31, 32, 33, 128, 129, 160]
    slices = {m: -(-(-(-m // 32)) // ac.AW) for m in ms}
    assert [slices[m] for m in ms] == [1, 1, 1, 1, 1, 2, 2]
    assert -(-129 // 32) - ac.AW == 1                              # one live wave in the second slice
    assert sorted(j for m, j in ac.MIXTURES if m == 129) == [1, 3, 7, 8, 9]
    for m, j in ac.MIXTURES:
        t = set(ac.tiles_of(ac.mixtures(m, j)['counts'])) - {0}
        assert t <= {1, 2, 7} and (j == 1 or t == {1, 2, 7})


def test_scale_cases():
    c = ac.scale()
    assert ac.tiles_of(c['counts']) == [8, 8, 8]
    a = ac.survivors(c, 0)
    assert np.array_equal(a, np.arange(256))
    for t in range(8):                                             # tile t: mixture t of state 0 is the one responsible
        x = c['frames'][32 * t:32 * t + 32]
        from oracle import poccala_oracle as po
        assert (po.gmm_component_loglik(x, c['mean'][0], c['var'][0], c['w'][0]).argmax(axis=1) == t).all()
    b, cc = c['lgamma'][2, ac.survivors(c, 1)], c['lgamma'][3, ac.survivors(c, 2)]
    assert (b[:96] == -100.0).all() and (b[96:] == 0.0).all() and (cc[:32] == 0.0).all() and (cc[32:] == -25.0).all()
    assert -100.0 > -150.0 * ac.LN2                                # above the f32 pass's own cut
    p = ac.scale_prune()
    thr = -20.0 * ac.LN2
    row = p['lgamma'][1, :66]
    assert (row[0::2] > thr).all() and (row[1::2] < thr).all() and (np.abs(row / thr - 1.0) < 2e-12).all()
    assert np.array_equal(ac.survivors(p, 0), np.arange(0, 66, 2)) and p['counts'][0] == 33
    assert (p['lgamma'][2][np.isfinite(p['lgamma'][2])] > thr).all()


def test_masked_claims():
    c = ac.masked()
    assert ac.masked_claims(c) is None
    pos = set()
    for j, (n, out) in enumerate(ac.MASKED_LAYOUT):
        assert c['outliers'][j] == tuple(out) and c['counts'][j] == n
        pos |= {p % 32 for p in out} if len(out) < 32 else set()
        v = c['var'][j]
        assert (v[:ac.MASKED_TIGHT] < 1e-3).all() and (v[ac.MASKED_TIGHT:] > 0.5).all()
    assert {0, 3, 4, 31} <= pos
    assert ac.MASKED_LAYOUT[1] == (33, (32,))                              # the only frame of a last tile
    assert ac.MASKED_LAYOUT[2][1] == tuple(range(32, 64)) and ac.MASKED_LAYOUT[3][1] == tuple(range(32))
    assert ac.MASKED_LAYOUT[4][1] == tuple(range(ac.MASKED_LAYOUT[4][0]))  # every tile
    # tens of sigma of the wide mixtures
    for j, (n, out) in enumerate(ac.MASKED_LAYOUT):
        if out:
            idx = ac.survivors(c, j)[list(out)]
            z = np.abs(c['frames'][idx][:, None, :] - c['mean'][j][None, ac.MASKED_TIGHT:]) / np.sqrt(c['var'][j][None, ac.MASKED_TIGHT:])
            assert 20.0 < z.max(axis=(1, 2)).min() and z.max() < 80.0


def test_reference_is_shared_and_read_only():
    c = ac.mixtures(33, 3)
    r = ac.reference(c)
    assert ac.reference(c) is r and not r['acc'].flags.writeable
    assert math.isclose(r['alpha_acc'][0], np.exp(c['lgamma'][1][np.isfinite(c['lgamma'][1])]).sum(), rel_tol=1e-12)
    np.testing.assert_allclose(r['acc'].sum(axis=1), r['alpha_acc'], rtol=1e-10)
