"""Helper of tests/test_gpu_dec_prune.py, run as a child process: loads the pruning / transfer harness (tests/dec_prune_harness.hip, built
into poccala_amd/libpoccala_dectest.so; DECTEST_LIB names another build, e.g. one of tools/dec_prune_mutants.sh) with ctypes, hands it
the packed cases of an .npz file and writes what came back to another.  The harness does its own hipMalloc / hipMemcpy: nothing of the
package is imported, so a fault in a helper under test ends this process and nothing else.

    python tests/_dec_prune_run.py prune general|lr KMAX in.npz out.npz
    python tests/_dec_prune_run.py transfer general|lr identity|map in.npz out.npz

Exit status 0 and a line `DECTEST OK`, or non-zero with the reason on stderr."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, 'poccala_amd', 'libpoccala_dectest.so')
HEAD = 12
KIND = {'general': 0, 'lr': 1}


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def arr(z, key, dtype):
    return np.ascontiguousarray(z[key], dtype=dtype)


def main(argv):
    path = os.environ.get('DECTEST_LIB') or DEFAULT_LIB
    if not os.path.exists(path):
        sys.stderr.write('%s is missing: run make -C poccala_amd/csrc\n' % path)
        return 3
    lib = C.CDLL(path)
    what, which, arg, src, dst = argv
    z = np.load(src)
    n, off = arr(z, 'n', np.int32), arr(z, 'off', np.int64)
    if what == 'prune':
        beam, md = arr(z, 'beam', np.float64), arr(z, 'min_distinct', np.int32)
        score, part = arr(z, 'score', np.float64), arr(z, 'part', np.int32)
        total = len(score)
        head = np.zeros((len(n), 2, HEAD), np.uint64)
        gone = np.zeros((2, total), np.uint8)
        geo = np.zeros(3, np.int32)
        rc = lib.dectest_prune_run(C.c_int(KIND[which]), C.c_int(int(arg)), C.c_int(len(n)), ptr(n, C.c_int), ptr(off, C.c_longlong),
                                   ptr(beam, C.c_double), ptr(md, C.c_int), C.c_longlong(total), ptr(score, C.c_double), ptr(part, C.c_int),
                                   ptr(head, C.c_ulonglong), ptr(gone, C.c_ubyte), ptr(geo, C.c_int))
        if rc == 0:
            np.savez(dst, head=head, gone=gone, geometry=geo)
    elif what == 'transfer':
        cand, out_off = arr(z, 'candidate', np.int32), arr(z, 'out_off', np.int64)
        sc, nd, hs, mp = arr(z, 'sc', np.float64), arr(z, 'nd', np.int32), arr(z, 'hs', np.int32), arr(z, 'map', np.int32)
        total, out_total = len(sc), int(cand.sum())
        out_n = np.zeros(len(n), np.int32)
        out_node = np.full(max(out_total, 1), -7, np.int32)          # (what a case does not write keeps this fill)
        out_hist = np.full(max(out_total, 1), -7, np.int32)
        out_score = np.full(max(out_total, 1), 7.0, np.float64)
        rc = lib.dectest_transfer_run(C.c_int(KIND[which]), C.c_int(1 if arg == 'map' else 0), C.c_int(len(n)), ptr(n, C.c_int), ptr(cand, C.c_int),
                                      ptr(off, C.c_longlong), ptr(out_off, C.c_longlong), C.c_longlong(total), C.c_longlong(out_total),
                                      ptr(sc, C.c_double), ptr(nd, C.c_int), ptr(hs, C.c_int), ptr(mp, C.c_int), ptr(out_n, C.c_int),
                                      ptr(out_node, C.c_int), ptr(out_score, C.c_double), ptr(out_hist, C.c_int))
        if rc == 0:
            np.savez(dst, out_n=out_n, out_node=out_node, out_score=out_score, out_hist=out_hist)
    else:
        sys.stderr.write('unknown job %r\n' % what)
        return 2
    if rc != 0:
        sys.stderr.write('the harness returned %d\n' % rc)
        return 1
    print('DECTEST OK')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
