"""CPU-side checks of the int16 PCM route of the front-end: the two entry points are bound with the float64 ones' arity, and
Engine.frontend / mfcc_batch choose the route by the samples' dtype alone -- int16 arrays and nothing else travel as int16."""
import ctypes as C

import numpy as np
import pytest

import poccala_amd._lib as L


def test_the_pcm16_entry_points_are_bound_like_their_float64_twins():
    for name, twin, arity in (('pcl_mfcc_pcm16', 'pcl_mfcc', 17), ('pcl_frontend_pcm16', 'pcl_frontend', 23)):
        assert name in L.PROTOTYPES, name
        res, args = L.PROTOTYPES[name]
        assert res is C.c_int and len(args) == arity
        assert (res, args) == L.PROTOTYPES[twin]              # same arguments: the sample pointer is a void pointer in both


i16 = lambda *v: np.array(v, dtype=np.int16)                    # noqa: E731


@pytest.mark.parametrize('signals,want', [
    ([i16(1, 2), i16(3)], True),
    ((i16(1, 2),), True),
    ([np.array([1.0, 2.0])], False),                          # float samples that hold integers: not rounded, not narrowed
    ([np.array([1.0, 2.0], dtype=np.float32)], False),
    ([i16(1, 2), np.array([3.0])], False),                    # mixed
    ([i16(1, 2), np.array([3], dtype=np.int32)], False),      # another integer width
    ([np.array([3], dtype=np.uint16)], False),
    ([[1, 2, 3]], False),                                     # a Python list
    ([], False),                                              # nothing: the float64 route rejects it, as it always did
])
def test_route_predicate(signals, want):
    assert L.all_int16(signals) is want


class StubLib(object):
    """Stands in for the loaded library: records which front-end entry point was called, with how many signals and samples."""

    def __init__(self):
        self.calls = []

    def _entry(self, name):
        def fn(*args):
            width = int(np.diff(np.ctypeslib.as_array(C.cast(args[3], C.POINTER(C.c_int64)), (args[1] + 1,))).sum())
            self.calls.append((name, args[1], width))
            return 0
        return fn

    def __getattr__(self, name):
        if name in ('pcl_frontend', 'pcl_frontend_pcm16', 'pcl_mfcc', 'pcl_mfcc_pcm16'):
            return self._entry(name)
        raise AttributeError(name)


@pytest.fixture()
def stub_engine():
    from poccala_amd import Engine
    eng = Engine.__new__(Engine)                                # no context: nothing here reaches a device
    eng._lib, eng._ctx = StubLib(), None
    return eng


SIG = np.arange(1, 801)


@pytest.mark.parametrize('signals,entry', [
    ([SIG.astype(np.int16), SIG[:500].astype(np.int16)], 'pcl_frontend_pcm16'),
    ([SIG.astype(np.float64), SIG[:500].astype(np.float64)], 'pcl_frontend'),
    ([SIG.astype(np.int16), SIG[:500].astype(np.float64)], 'pcl_frontend'),
    ([SIG.astype(np.int32), SIG[:500].astype(np.int16)], 'pcl_frontend'),
    ([SIG.tolist(), SIG[:500].astype(np.int16)], 'pcl_frontend'),
])
def test_engine_frontend_takes_the_int16_route_for_int16_only(stub_engine, signals, entry):
    stub_engine.frontend(signals, 16000)
    assert stub_engine._lib.calls == [(entry, 2, 1300)]


@pytest.mark.parametrize('dtype,entry', [(np.int16, 'pcl_mfcc_pcm16'), (np.float64, 'pcl_mfcc'), (np.int64, 'pcl_mfcc')])
def test_mfcc_batch_follows_the_same_rule(stub_engine, dtype, entry):
    from poccala_amd.StatisticalModel.AudioProcessing import mfcc_batch
    mats = mfcc_batch([SIG.astype(dtype)], 16000, engine=stub_engine)
    assert stub_engine._lib.calls == [(entry, 1, 800)] and mats[0].shape == (3, 13)
