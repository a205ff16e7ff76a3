"""Child process of tests/test_gpu_lifecycle.py::test_a_context_with_every_lazy_member_gives_everything_back: twice, a context whose lazily
made members all exist at teardown (timer event pairs read and unread, the int16 front-end's staging stream / buffers / events, a used
descriptor stager, a communicator), then a context destroyed at once, where none of them exists.  Every C call's status is checked here;
the pool's books after each context go out as one JSON line.  Run with PCL_DESTROY_SYNC=1 so that block reuse does not depend on timing."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from poccala_amd import Engine, PCL_F32, synth                                # noqa: E402

UNITS, M, D = 3, 4, 13


def destroy(eng, batches=()):
    """Batch and context destruction by hand: Engine.close() and Batch.close() do not look at the status."""
    for b in batches:
        h, b._b = b._b, None
        assert eng._lib.pcl_batch_destroy(h) == 0
    assert not eng._pinned                                                    # (nothing here asked for page-locked result buffers)
    ctx, eng._ctx = eng._ctx, None
    assert eng._lib.pcl_destroy(ctx) == 0


def full_context():
    mean, var, w, trans = synth.make_model(UNITS, M, D, seed=3)
    rng = np.random.default_rng(5)
    pcm = (3000.0 * np.sin(np.arange(16000) * 0.05) + 200.0 * rng.standard_normal(16000)).astype(np.int16)    # one second at 16 kHz
    eng = Engine(0)                                                           # (every Engine method below raises on a status other than PCL_OK)
    eng.enable_timing(True)
    eng.load_model(mean, var, w)
    eng.load_units(np.stack(trans))
    lens, begin = eng.frontend([pcm], 16000, d1=False, d2=False, vad=False)   # int16: the staging stream, its buffers and events; "mfcc" and "pcm_h2d" timers
    assert lens[0] > 0
    b = eng.label_batch([[0, 1]], lens, begin)                                # descriptor uploads: the stager
    b.score(PCL_F32)                                                          # (more timer groups, never read)
    eng.comm_init_host(0, 1, lambda mine: [mine])
    ms, launches = eng.kernel_time('mfcc')                                    # one group read (its pairs go), "pcm_h2d" and the scoring groups stay
    assert launches >= 1, (ms, launches)
    destroy(eng, [b])


def main():
    out = dict(before=Engine.pool_stats(), after=[])
    for _ in range(2):
        full_context()
        out['after'].append(Engine.pool_stats())
    destroy(Engine(0))
    out['after'].append(Engine.pool_stats())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
