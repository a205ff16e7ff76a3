"""csrc/gmm_accumulate_f16.hip (the default f32 E-step statistics: tile producer, six-slot LDS-DMA ring consumer) held to the float64 oracle
at the edges of its pipeline.  tests/_acc16_cases.py makes the inputs and tests/test_acc16_cases.py proves on the CPU that each reaches its
edge: every tile count from 1 to 7 (AHEAD = 5, AHEAD + 1, NSLOT + 1 among them), 9 and 13; a first tile on each of the six ring slots; last
tiles of 1, 31 and 32 frames; empty states; idle waves; m-tiles that end mid-tile; one and two slices; state counts around the 8-block
map; every kernel instance (D = 13, 26, 39, 47) and padded host dimensions; per-mixture scales that rise in different tiles; a pruning
threshold between neighbouring frames; frames and whole tiles taken out of the image by the mask; a split state; several state groups.

Per case: load_model, load_frames, all_state_batch, score, then set_emissions with the ORACLE'S float64 ln b_j(o_t) and set_posteriors with
the case's ln gamma, stats_zero, accumulate, stats_download.  The reference (oracle.poccala_oracle.gmm_update_acc over each state's
survivors, every state) therefore depends on nothing the device computed.  acc, alpha_acc, mean_acc, cov_acc per state through
_parity.hold: rtol 1e-4, atol 1e-6 of the state's largest entry, + cov_acc_atol for cov_acc; the masked case at rtol 1e-4 + 4 x the
per-frame f32 evaluation bound of the state's survivors (computed from the reference's inputs alone, <= 2.1e-3); PCL_F64 at 1e-9 / 1e-13,
which separates a wrong case from a wrong f16 path.  Empty states come back exactly zero, cov_acc >= 0 everywhere.  One state's arithmetic
does not depend on its neighbours, so three checks are bitwise: a case run twice; a second pass without stats_zero (read-modify-write
flush) against twice the first (FRESH flush); the ladder's states accumulated alone (first tile on slot 0) against inside the ladder."""
import numpy as np
import pytest

import _acc16_cases as ac
from _oracle_pool import f32_evaluation_bound_rows
from _parity import cov_acc_atol, hold

pytestmark = pytest.mark.gpu
KEYS = ('acc', 'alpha_acc', 'mean_acc', 'cov_acc')
PLAIN, ALL = ac.plain_cases(), ac.all_cases()
_EMIT = {}


@pytest.fixture(scope='module')
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def ids(cases):
    return [i for i, _ in cases]


def emissions(c):
    if c['name'] not in _EMIT:
        _EMIT[c['name']] = ac.emissions(c)
    return _EMIT[c['name']]


class Opened:
    """A case resident on an engine: model, frames, an all-state batch scored and given the oracle's emissions."""

    def __init__(self, eng, c, prec='f32'):
        from poccala_amd import PCL_F32, PCL_F64
        self.eng, self.c, self.P = eng, c, PCL_F32 if prec == 'f32' else PCL_F64
        eng.load_model(c['mean'], c['var'], c['w'])
        eng.load_frames(c['frames'])
        self.b = eng.all_state_batch([c['frames'].shape[0]], [0])
        self.b.score(self.P)
        self.b.set_emissions([emissions(c)])

    def stats(self, lgamma=None, passes=1):
        """stats_zero, `passes` accumulate calls on the given ln gamma (default: the case's), the downloaded statistics."""
        self.b.set_posteriors([self.c['lgamma'] if lgamma is None else lgamma])
        if self.c['prune'] is not None:
            self.eng.accumulate_prune(self.c['prune'])
        try:
            self.eng.stats_zero()
            for _ in range(passes):
                self.b.accumulate(self.P)
            return self.eng.stats_download()
        finally:
            self.eng.accumulate_prune(-1e300)

    def close(self):
        self.b.close()


def same_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint64), np.ascontiguousarray(b[k]).view(np.uint64)) for k in KEYS)


def hold_case(c, st, prec):
    """Every state against the oracle; returns the largest share of a bound that was used."""
    ref = ac.reference(c)
    tag = 'acc16 edges %s %s' % (c['name'], prec)
    used = 0.0
    for j in range(c['mean'].shape[0]):
        if c['counts'][j] == 0:
            assert all(not np.any(st[k][j]) for k in KEYS), '%s: empty state %d is not zero' % (tag, j)
            continue
        rt, at = (1e-4, 1e-6) if prec == 'f32' else (1e-9, 1e-13)
        if c['masked'] and prec == 'f32':
            bound = float(f32_evaluation_bound_rows([(c['mean'][j], c['var'][j], c['w'][j])], c['frames'][ac.survivors(c, j)]).max())
            rt = 1e-4 + 4.0 * bound
            assert rt <= 2.1e-3
        for k in KEYS:
            want = np.asarray(ref[k][j])
            floor = at * float(np.abs(want).max())
            if k == 'cov_acc' and prec == 'f32':
                floor = cov_acc_atol(ref['acc'][j], c['mean'][j], c['var'][j], floor)
            m = hold(tag, k, np.asarray(st[k][j]), want, rt, floor)
            used = max(used, m['used'])
    assert (st['cov_acc'] >= 0.0).all(), tag
    print('%s: %.3g of the bound' % (tag, used))
    return used


@pytest.mark.parametrize('mk', [m for _, m in ALL], ids=ids(ALL))
def test_statistics_default_precision(eng, mk):
    c = mk()
    o = Opened(eng, c)
    try:
        st = o.stats()
        again = o.stats()
    finally:
        o.close()
    hold_case(c, st, 'f32')
    assert same_bytes(st, again), 'two runs of the same case differ'


@pytest.mark.parametrize('mk', [m for _, m in ALL], ids=ids(ALL))
def test_statistics_f64(eng, mk):
    c = mk()
    o = Opened(eng, c, 'f64')
    try:
        st = o.stats()
    finally:
        o.close()
    hold_case(c, st, 'f64')


TWICE = [(i, m) for i, m in PLAIN if i != 'ladder']                  # no masked frames, no split state: the f16 kernels are the whole pass


@pytest.mark.parametrize('mk', [m for _, m in TWICE], ids=ids(TWICE))
def test_second_pass_adds_the_same_bits(eng, mk):
    """The first pass after stats_zero stores (FRESH), a second one reads, adds and writes: exactly twice the first."""
    c = mk()
    o = Opened(eng, c)
    try:
        once = o.stats()
        twice = o.stats(passes=2)
    finally:
        o.close()
    assert same_bytes({k: 2.0 * once[k] for k in KEYS}, twice)


def test_ladder_states_alone_give_the_same_bits(eng):
    """Alone, a state's first tile is tile 0 of its group (ring slot 0) and no other workgroup runs beside it; inside the ladder its first tile
    sits on the slot the states before it leave."""
    c = ac.ladder()
    o = Opened(eng, c)
    try:
        full = o.stats()
        for j in np.flatnonzero(c['counts']):
            lg = np.full_like(c['lgamma'], -np.inf)
            lg[1 + j] = c['lgamma'][1 + j]
            alone = o.stats(lg)
            assert same_bytes({k: alone[k][j] for k in KEYS}, {k: full[k][j] for k in KEYS}), 'state %d' % j
            others = np.arange(len(c['counts'])) != j
            assert all(not np.any(alone[k][others]) for k in KEYS), 'state %d alone touched another state' % j
    finally:
        o.close()


def test_state_groups_alternate_between_the_image_buffers(monkeypatch):
    """PCL_ACC_IMAGE_MB = 1 (read per call) on an engine whose scratch has not grown: 78 tile images per buffer, four state groups.  Same bytes
    as under the default budget, and within bounds of the oracle."""
    from poccala_amd import Engine
    c = ac.groups()
    e = Engine(0)
    try:
        e.enable_timing(True)
        o = Opened(e, c)
        monkeypatch.setenv('PCL_ACC_IMAGE_MB', '1')
        e.kernel_time('acc_consume')
        small = o.stats()
        n_groups = e.kernel_time('acc_consume')[1]
        monkeypatch.delenv('PCL_ACC_IMAGE_MB')
        whole = o.stats()
        n_whole = e.kernel_time('acc_consume')[1]
        o.close()
    finally:
        e.close()
    print('state groups: %d at 1 MB, %d at the default budget' % (n_groups, n_whole))
    assert n_groups >= 3, n_groups
    assert n_groups > n_whole
    assert same_bytes(small, whole)
    hold_case(c, small, 'f32')
