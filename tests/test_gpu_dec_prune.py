"""The decoders' pruning select and transfer (hmm_decode_common.h: pcl_prune_stats, pcl_prune_distinct, pcl_select_kth, pcl_prune_mark,
pcl_transfer) run alone in tests/dec_prune_harness.hip, in every shipping instantiation, against the project's own oracle plus a sort:
integer and bit-pattern equality throughout, no tolerance anywhere.  The cases and what each reaches: tests/_dec_prune_cases.py; that
they reach it: tests/test_dec_prune_cases.py, on the CPU.  One child process per instantiation (tests/_dec_prune_run.py)."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import _dec_prune_cases as dc
import _dec_prune_run as runner

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 120


def run_child(tmp_path, args, arrays):
    lib = os.environ.get('DECTEST_LIB') or runner.DEFAULT_LIB
    assert os.path.exists(lib), '%s is missing: run make -C poccala_amd/csrc' % lib
    src, dst = str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz')
    np.savez(src, **arrays)
    p = subprocess.run([sys.executable, os.path.join(HERE, '_dec_prune_run.py')] + args + [src, dst], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0 and 'DECTEST OK' in p.stdout, 'the harness child ended with %d:\n%s\n%s' % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return np.load(dst)


@pytest.mark.parametrize('inst', dc.INSTANTIATIONS, ids=dc.inst_id)
def test_prune_steps_equal_the_oracle_and_a_sort(tmp_path, inst):
    which, kmax = inst
    g = dc.GEOMETRY[which]
    cases = dc.prune_cases(inst)
    packed = dc.pack_prune(cases)
    out = run_child(tmp_path, ['prune', which, str(kmax)], packed)
    assert out['geometry'].tolist() == [g['NT'], g['HB'], g['CAND']]           # the harness was built with the constants the cases assume
    head, gone = out['head'], out['gone']
    refs = [dc.reference_of(which, c) for c in cases]
    paths = collections.Counter(r['path']['ret'] for r in refs if r['prune'])
    print('%s: %d cases, %d tokens; select returns: diff == 0 %d, shift 0 %d, candidates %d; distinct run %d; pruned %d' % (
        dc.inst_id(inst), len(cases), int(packed['n'].sum()), paths['equal'], paths['shift0'], paths['cand'], sum(r['ran_distinct'] for r in refs),
        sum(r['prune'] for r in refs)))
    bad = []
    for c, r, off, h in zip(cases, refs, packed['off'], head):
        for p in range(2):
            got = dict(zip(dc.HEAD, (int(x) for x in h[p])))
            want = dict(n_old=r['n_old'], kmin=r['kmin'], kmax=r['kmax'], bins=r['bins'], m=r['m'], ran_distinct=int(r['ran_distinct']),
                        prune=int(r['prune']), occ_left=0, hist_left=0, s_int2=0)
            if r['prune']:
                want.update(sel=r['sel'], rank=r['rank'])
            diff = {k: (got[k], v) for k, v in want.items() if got[k] != v}
            if not np.array_equal(gone[p, off:off + c['n']], r['gone']):
                diff['gone'] = (np.flatnonzero(gone[p, off:off + c['n']] != r['gone'])[:8].tolist(), int(r['gone'].sum()))
            if diff:
                bad.append((dc.case_id(c), 'pass %d' % p, diff))
        if not np.array_equal(h[0], h[1]) or not np.array_equal(gone[0, off:off + c['n']], gone[1, off:off + c['n']]):
            bad.append((dc.case_id(c), 'the second pass differs from the first', h.tolist()))
    assert not bad, '%d of %d cases, by family %s; the first: %s' % (len({b[0] for b in bad}), len(cases),
                                                                    dict(collections.Counter(b[0].split('-')[0] for b in bad)), bad[:4])


@pytest.mark.parametrize('which,mode', [('general', 'identity'), ('lr', 'map')])
def test_transfer_equals_the_stable_descending_sort(tmp_path, which, mode):
    """The general kernel reads token i's state at i; the left-to-right kernel through its index list, whose entries carry bit 31."""
    NT = dc.GEOMETRY[which]['NT']
    cases = dc.transfer_cases(NT)
    packed = dc.pack_transfer(cases, mode == 'map')
    out = run_child(tmp_path, ['transfer', which, mode], packed)
    print('%s / %s: %d cases, %d tokens' % (which, mode, len(cases), int(packed['n'].sum())))
    bad = []
    for c, o, n_out in zip(cases, packed['out_off'], out['out_n']):
        want_n, nd, sc, hs = dc.transfer_reference(c)
        rows = [out[k][o:o + c['candidate']] for k in ('out_node', 'out_score', 'out_hist')]
        ok = (n_out == want_n and np.array_equal(rows[0][:want_n], nd) and np.array_equal(rows[1][:want_n].view(np.uint64), sc.view(np.uint64))
              and np.array_equal(rows[2][:want_n], hs))
        ok = ok and (rows[0][want_n:] == -7).all() and (rows[1][want_n:] == 7.0).all() and (rows[2][want_n:] == -7).all()     # nothing written beyond n_out
        if not ok:
            bad.append((c['name'], int(n_out), want_n, rows[0][:6].tolist(), nd[:6].tolist()))
    assert not bad, '%d of %d cases; the first: %s' % (len(bad), len(cases), bad[:4])
