"""The twin of the resident tying and the tied label batch (tests/_tied_twin.py) on the CPU: every tree and corpus that
tests/test_gpu_tied_batches.py runs on the device reaches the edge it claims, the twin's owner map is the monophone twin's where the tying
is the monophone model, and the validator of pcl_tying_upload (poccala_amd/csrc/tying_check.h) holds under the host's sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _realign_twin as rt
import _tied_twin as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def test_validator_pack_and_walk_under_the_host_sanitizers(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which('hipcc'):
        pytest.fail('hipcc is needed to build the check (it is what builds the library)')
    exe = str(tmp_path / 'tying_host_check')
    cmd = [HIPCC if os.path.exists(HIPCC) else 'hipcc', '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-fno-omit-frame-pointer',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           os.path.join(ROOT, 'tests', 'tying_host_check.cpp'), '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'tying_host_check: OK' in run.stdout and 'ACCEPTED' not in run.stdout
    assert 'ERROR: AddressSanitizer' not in run.stderr and 'runtime error' not in run.stderr, run.stderr


@pytest.mark.parametrize('P', [1, 3])
def test_the_chain_is_walked_to_its_last_level(P):
    tree = tt.chain(P)
    Q = tree.Q
    assert Q == 24 and tree.n_states == 73 * P and tree.n_nodes == P + 2 * 72 * P
    inner = tree.node_cand[tree.node_cand >= 0]
    assert sorted(inner.tolist()) == sorted(list(range(3 * Q)) * P)          # every (position, question) pair, once per chain
    edge = tree.q_member[:, tree.n_units]
    assert 0 < edge.sum() < Q                                                # the edge symbol: a member of some questions, not of others
    ctx = tt.all_contexts()
    depth = np.array([[tt.walk_depth(tree, l, c, r, k) for k in range(P)] for l, c, r in ctx.tolist()])
    print('chain P=%d: depths %d .. %d, %d walks longer than 64' % (P, depth.min(), depth.max(), int((depth > 64).sum())))
    assert depth.max() == 72 and depth.min() == 1 and len(set(depth.reshape(-1).tolist())) >= 6
    for k in range(P):
        l, c, r = tt.chain_follower(k)
        assert tt.walk_depth(tree, l, c, r, k) == 72
    assert tt.chain_follower(0)[0] == tree.n_units == tt.chain_follower(0)[2]   # ... one of them between two utterance edges
    states = tt.lookup_all(tree, ctx)
    assert states.min() >= 0 and states.max() < tree.n_states and len(np.unique(states)) >= 6
    # children behind their parent, as pcl_tying_upload demands
    at = np.flatnonzero(tree.node_cand >= 0)
    assert (tree.node_child[at] > at[:, None]).all()


@pytest.mark.parametrize('P', [1, 3])
def test_the_other_trees(P):
    ctx = tt.all_contexts()
    assert ctx.shape == ((tt.N_UNITS + 1) ** 2 * tt.N_UNITS, 3)
    ro = tt.roots_only(P)
    got = tt.lookup_all(ro, ctx)
    mono = ctx[:, 1:2] * P + np.arange(P)[None, :]
    assert ro.n_states == ro.n_nodes == tt.N_UNITS * P and (got != mono).any() and np.array_equal(got, tt.N_UNITS * P - 1 - mono)
    assert np.array_equal(tt.lookup_all(tt.roots_only(P, reverse=False), ctx), mono)
    bt = tt.built_twin(P)
    depth = np.array([[tt.walk_depth(bt, l, c, r, k) for k in range(P)] for l, c, r in ctx.tolist()])
    print('built P=%d: %d nodes, %d states, depths %d .. %d' % (P, bt.n_nodes, bt.n_states, depth.min(), depth.max()))
    assert bt.n_states == P + 11 != tt.N_UNITS * P and depth.max() >= 3 and depth.min() >= 1
    pos = bt.node_cand[bt.node_cand >= 0] // bt.Q
    assert {0, 1} <= set(pos.tolist())                                       # questions about a neighbour and about the centre (the chain asks about all three)
    assert bt.n_roots == P
    qm, cand, child, state, root_of = bt.tying_arrays()
    assert all(a.flags['C_CONTIGUOUS'] for a in (qm, cand, child, state, root_of)) and child.shape == (bt.n_nodes, 2) and qm.dtype == np.uint8


def test_the_corpora_hold_their_edges():
    labels, T, begin, F = tt.edge_corpus()
    lens = [len(l) for l in labels]
    assert len(labels) == 70 and lens[0] == 1 and lens[1] == 2 and max(lens) == 130 and lens.count(130) == 1
    assert labels[2][0] == labels[2][1] and len(set(labels[3])) == 1 and len(set(lens)) > 5
    assert T.min() >= 5 and T.max() <= 40
    order = np.argsort(begin)
    assert (begin[order][1:] >= (begin + T)[order][:-1]).all() and begin.min() > 0 and (begin + T).max() < F
    assert ((begin[order][1:] - (begin + T)[order][:-1]) > 0).any()
    assert tt.contexts_of([2]) == [(5, 2, 5)] and tt.contexts_of([0, 4]) == [(5, 0, 4), (0, 4, 5)]
    labels, T, begin, F = tt.align_corpus()
    assert T[2] < len(set(labels[2])) and labels[1][0] == labels[1][1] and begin.min() > 0 and (begin + T).max() < F
    # the contexts are triphone_events'
    from poccala_amd.AcousticModel.ContextTree import triphone_events
    ev, le = triphone_events(labels, tt.N_UNITS)
    flat = [c for lab in labels for c in tt.contexts_of(lab)]
    assert np.array_equal(ev[le], np.array(flat))


def staircase_paths(labels, T, P, rng):
    """A monotone path through rows 1 .. P L per utterance (the rows a left-to-right alignment visits), some rows skipped"""
    paths = []
    for lab, t in zip(labels, T):
        n = P * len(lab)
        rows = np.sort(rng.integers(1, n + 1, size=int(t)))
        paths.append(rows.astype(np.int32))
    return paths


@pytest.mark.parametrize('S', [3, 5])
def test_owner_map_twin(S):
    P = S - 2
    labels, T, begin, F = tt.align_corpus()
    rng = np.random.default_rng(S)
    paths = staircase_paths(labels, T, P, rng)
    mono, mono_dropped = rt.realign(paths, labels, S, T, begin, F)
    # the monophone model as a tying: the tied owner map IS the monophone one
    state, dropped, pos, k = tt.owner_map(tt.roots_only(P, reverse=False), paths, labels, S, T, begin, F)
    assert dropped == mono_dropped == [2] and np.array_equal(state, mono)
    tree = tt.built_twin(P)
    state, dropped, pos, k = tt.owner_map(tree, paths, labels, S, T, begin, F)
    assert dropped == [2] and np.array_equal(state >= 0, mono >= 0) and (state[mono >= 0] != mono[mono >= 0]).any()
    owned = np.zeros(F, dtype=bool)
    for u in range(len(T)):
        owned[begin[u]:begin[u] + T[u]] = u not in dropped
    assert np.array_equal(state >= 0, owned) and (~owned).sum() > T[2]       # -1 in front of, between and behind the utterances
    # adjacent equal units: ONE run, sliced as a whole, but the tied state follows the label POSITION of the path row
    u = 1
    sl = slice(int(begin[u]), int(begin[u] + T[u]))
    ps = tt.pos_states(tree, [labels[u]])[0]
    assert np.array_equal(state[sl], ps[pos[sl], k[sl]])
    if P > 1:
        in_run = np.asarray(labels[u])[pos[sl]] == 3
        assert len(set(pos[sl][in_run].tolist())) == 2                       # the run of the two 3s spans two positions
    from poccala_amd.AcousticModel.ContextTree import triphone_events
    ev, le = triphone_events(labels, tt.N_UNITS)
    le = le.copy()
    le[1] = -1
    rows = tt.tree_rows(le, labels, P, T, begin, F, pos, k)
    assert (rows >= 0).sum() > 50 and rows.max() < len(ev) * P and ((rows < 0) & (state >= 0)).any()
