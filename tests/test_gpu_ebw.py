"""MMI by extended Baum-Welch on the device (csrc/model_ebw.hip: pcl_ebw_hold / pcl_ebw_drop / pcl_ebw_stats_download / pcl_mstep_ebw;
Engine.ebw_hold / ebw_drop / ebw_stats / mstep_ebw / loop_batch) against the NumPy statement of the rule (tests/_ebw_twin.py, whose own
invariants tests/test_ebw_twin.py holds).

Both statistics sets come from real accumulate passes under PCL_F64 on a batch whose state posteriors are set with set_posteriors; the twin
is fed what ebw_stats(), stats_download() and model_download() return, so only the new kernels are under comparison.

Bound.  Nothing here is a float32 path.  Per case the float64 twin is measured against the same code in long double; the device may differ
from the float64 twin by 4x that distance plus 8 ulp of the value (it differs from the twin in the order of the weight iteration's sums
only: the kernels are built without contraction and run the twin's operations in the twin's order).  D_out and the four counts: the same
allowance, and exact.  Kept mixtures, and through the scoring check all padding: bit for bit.  Every figure is printed before it is asserted.

Complex roots: the discriminant is (c - g v)^2 + 4 v x^2, never negative in exact arithmetic; the twin counts the elements where rounding
made it so (none in these cases), and the branch is the one a NaN takes.

End to end (6 units, J = 18, M = 2, D = 4, 8 x 40 frames, label batches against the unit loop, three iterations): every ln P(O) under PCL_F64
is held to 1e-9 relative, so the objective of an iteration may differ from the oracle's by 1e-9 (sum |ln P_num| + sum
|ln P_den|); the statistics carry the same 1e-9, the update divides by g + D >= E gd with (gn + gd + tau) / (g + D) below 10 in this setup,
and three iterations compound it: 1e-7 relative plus 1e-7 absolute on the final model."""
import numpy as np
import pytest

import _ebw_twin as tw

pytestmark = pytest.mark.gpu
F64_RTOL = 1e-9              # PCL_F64
WORST = {}


@pytest.fixture()
def eng():
    from poccala_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


_CASES = {}


def case(shape):
    if shape not in _CASES:
        _CASES[shape] = tw.make_case(*shape)
    return _CASES[shape]


def two_sets(eng, model, frames, gnum, gden, hold=True):
    """model and frames up; the numerator pass, ebw_hold, the denominator pass -> (batch, numerator as downloaded before the hold, denominator)"""
    from poccala_amd import PCL_F64
    eng.load_model(*model)
    eng.load_frames(np.asarray(frames, dtype=np.float64))
    F = len(frames)
    b = eng.all_state_batch(np.array([F], dtype=np.int32), np.array([0], dtype=np.int64))
    b.score(PCL_F64)
    out = []
    for k, gamma in enumerate((gnum, gden)):
        with np.errstate(divide='ignore'):
            lg = np.concatenate([np.full((1, F), -np.inf), np.log(gamma.T), np.full((1, F), -np.inf)])
        b.set_posteriors([lg])
        eng.stats_zero()
        b.accumulate(PCL_F64)
        out.append(eng.stats_download())
        if k == 0 and hold:
            eng.ebw_hold()
    return b, out[0], out[1]


def check_against_twin(tag, got, model, num, den, **kw):
    t64 = tw.update(*model, num, den, **kw)
    tld = tw.update(*model, num, den, dtype=np.longdouble, **kw)
    mean, var, w, D, counts = got
    for key, val in (('mean', mean), ('var', var), ('w', w), ('D', D)):
        with np.errstate(invalid='ignore'):
            share = np.abs(val - t64[key]) / tw.allowance(t64, tld, key)
        WORST[key] = max(WORST.get(key, 0.0), float(share.max()))
        print('%s: %s uses %.3f of its allowance' % (tag, key, share.max()))
        assert share.max() <= 1.0, (tag, key)
    print('%s: counts %s (twin %s), elements with a negative discriminant %d' % (tag, counts, t64['counts'].tolist(), t64['negdisc']))
    assert [counts[k] for k in ('updated', 'kept', 'floored', 'weights_kept')] == t64['counts'].tolist()
    keep = t64['keep']
    assert same_bits(mean[keep], model[0][keep]) and same_bits(var[keep], model[1][keep]) and (D[keep] == 0).all()
    return t64


@pytest.mark.parametrize('shape', tw.SHAPES, ids=lambda s: 'J%d-M%d-D%d' % s)
def test_the_update_is_the_twins(eng, shape):
    from poccala_amd import PCL_F64
    J, M, Dm = shape
    model, frames, gnum, gden = case(shape)
    role = tw.roles(J, M)
    for tau, E, iters in tw.GRID:
        b, num, den = two_sets(eng, model, frames, gnum, gden)
        if (tau, E, iters) == tw.GRID[0]:
            held = eng.ebw_stats()
            assert all(same_bits(held[k], num[k]) for k in num)                      # the held set is what was live ...
            empty = (role == 4) | (role == 5)
            assert (num['acc'][empty] == 0).all() and (den['acc'][empty] == 0).all() and empty.any()
            if M > 1:
                assert (model[2] == 0).any()
        before = eng.model_download()
        assert all(same_bits(a, c) for a, c in zip(before, model))
        counts, D = eng.mstep_ebw(E=E, tau=tau, c_covariance=1e-3, weight_iters=iters, want_D=True)
        after = eng.model_download()
        tag = 'ebw J=%d M=%d D=%d tau=%g E=%g iters=%d' % (J, M, Dm, tau, E, iters)
        t = check_against_twin(tag, (*after, D, counts), model, num, den, E=E, tau=tau, c_covariance=1e-3, weight_iters=iters)
        upd = ~t['keep']
        assert (t['g'][upd] < 0).any() and (t['Dmin'][upd] > 0).any() and counts['floored'] > 0 and counts['kept'] > 0   # the case carries them
        if (tau, E, iters) in (tw.GRID[0], tw.GRID[-1]):
            # every scoring path sees the model an upload of the downloaded arrays would give (padding included: a padded mean, variance
            # or weight that the update touched breaks this), and a second run from the same inputs gives the same bits
            b.score(PCL_F64)
            B1 = b.get('B')[0]
            b.close()
            b2, _, _ = two_sets(eng, model, frames, gnum, gden)
            counts2, D2 = eng.mstep_ebw(E=E, tau=tau, c_covariance=1e-3, weight_iters=iters, want_D=True)
            assert counts2 == counts and same_bits(D2, D) and all(same_bits(a, c) for a, c in zip(eng.model_download(), after))
            b2.close()
            eng.load_model(*after)
            b3 = eng.all_state_batch(np.array([len(frames)], dtype=np.int32), np.array([0], dtype=np.int64))
            b3.score(PCL_F64)
            assert same_bits(b3.get('B')[0], B1)
            b3.close()
        else:
            b.close()
    print('worst share of the allowance per quantity so far: %s' % WORST)


def test_hold_leaves_the_live_block_alone(eng):
    model, frames, gnum, gden = case(tw.SHAPES[0])
    b, num, den = two_sets(eng, model, frames, gnum, gden, hold=False)
    live = eng.stats_download()
    eng.ebw_hold()
    assert all(same_bits(eng.stats_download()[k], live[k]) for k in live)
    assert all(same_bits(eng.ebw_stats()[k], live[k]) for k in live)
    eng.stats_zero()
    assert all(same_bits(eng.ebw_stats()[k], live[k]) for k in live)                # ... and the held set does not follow the live block
    eng.ebw_drop()
    eng.ebw_drop()                                                                   # (nothing held: nothing happens)
    b.close()


def refused(eng, code, call):
    from poccala_amd import PoccalaHipError
    before = eng.model_download()
    with pytest.raises(PoccalaHipError) as e:
        call()
    assert e.value.code == code, e.value
    assert all(same_bits(a, c) for a, c in zip(eng.model_download(), before))


def test_refusals(eng):
    from poccala_amd import PoccalaHipError
    INVALID, STATE = -1, -3
    with pytest.raises(PoccalaHipError):
        eng.ebw_hold()                                                               # no model
    model, frames, gnum, gden = case(tw.SHAPES[0])
    b, num, den = two_sets(eng, model, frames, gnum, gden, hold=False)
    refused(eng, STATE, eng.mstep_ebw)                                               # nothing held
    refused(eng, STATE, eng.ebw_stats)
    for drop in (lambda: eng.mixup(4), lambda: eng.load_model(*model), lambda: eng.mstep(), lambda: eng.mstep_map(10.0), eng.ebw_drop):
        eng.ebw_hold()
        drop()
        refused(eng, STATE, eng.mstep_ebw)
    eng.load_model(*model)
    eng.ebw_hold()
    for kw in (dict(E=0.0), dict(E=-1.0), dict(E=float('nan')), dict(E=float('inf')), dict(tau=-1.0), dict(tau=float('nan')), dict(c_covariance=-1e-3),
               dict(c_covariance=float('inf')), dict(weight_iters=-1)):
        refused(eng, INVALID, lambda: eng.mstep_ebw(**kw))
    eng.mstep_ebw()                                                                  # still held after the refusals; the update itself drops it
    refused(eng, STATE, eng.mstep_ebw)
    b.close()


def test_mmi_iterations_follow_the_oracle(eng):
    from poccala_amd import PCL_F64
    c = tw.E2E
    ref_trace, ref_model = tw.e2e_reference()
    print('oracle + twin objective: %s, steps %s' % (ref_trace, np.diff(ref_trace)))
    assert (np.diff(ref_trace) > 1.0).all()                                          # the setup raises the objective at every iteration, clearly
    model, trans, frames, labels, lens, begin = tw.e2e_setup()
    eng.load_model(*model)
    eng.load_units(trans)
    eng.load_frames(frames)
    num_b = eng.label_batch(labels, lens, begin)
    den_b = eng.loop_batch(lens, begin, trans)
    trace, scale = [], []
    for it in range(c['iters'] + 1):
        lp = []
        for k, b in enumerate((num_b, den_b)):
            b.score(PCL_F64)
            b.forward_backward(fix_pi=True)
            lp.append(b.get('logp'))
            if it < c['iters']:
                eng.stats_zero()
                b.accumulate(PCL_F64)
                if k == 0:
                    eng.ebw_hold()
        trace.append(lp[0].sum() - lp[1].sum())
        scale.append(np.abs(lp[0]).sum() + np.abs(lp[1]).sum())
        if it < c['iters']:
            eng.mstep_ebw(E=c['E'], tau=c['tau'])
    trace, scale = np.array(trace), np.array(scale)
    print('device objective: %s; off the oracle by %s of the bound' % (trace, np.abs(trace - ref_trace) / (F64_RTOL * scale)))
    assert (np.abs(trace - ref_trace) <= F64_RTOL * scale).all()
    for name, got, want in zip(('mean', 'var', 'w'), eng.model_download(), ref_model):
        share = np.abs(got - want) / (1e-7 + 1e-7 * np.abs(want))
        print('final %s: %.3g of the bound' % (name, share.max()))
        assert share.max() <= 1.0
    num_b.close()
    den_b.close()
