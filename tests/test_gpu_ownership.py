"""Every owner of device memory in the host runtime gives back what it took: tools/ownership_walk.py, a fresh process (the pool is
process-wide and other tests hold engines), walks model, units, frames, label batch, both scoring precisions, forward-backward,
Viterbi, asynchronous fetch, accumulate, M-step, regroup, realignment + k-means + EM on a segment set, lexicon + decode, the int16
front-end, flat start, a second model and the streaming slots -- twice -- and three calls the host-side validation refuses."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_owner_returns_its_blocks_and_a_second_walk_allocates_nothing():
    env = dict(os.environ, PCL_DESTROY_SYNC='1')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'ownership_walk.py')], cwd=ROOT, capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(r))
    assert len(r['refused']) == 6                                             # three per walk
    for c in r['refused']:
        assert c['raised'] and c['code'] < 0, c
        assert c['blocks_after'] == c['blocks_before'], c
    first, second = r['walks']
    for w in (first, second):                                                 # every handle is destroyed: a condition, not a measurement
        assert w['handed_out_blocks'] == 0 and w['handed_out_bytes'] == 0, w
    assert first['device_allocs'] > first['device_allocs_before']
    assert second['device_allocs'] == second['device_allocs_before'], 'the second walk went to hipMalloc: %r' % (second,)
