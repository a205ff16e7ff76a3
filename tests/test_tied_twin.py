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


# ------------------------------------------------------------------ wide inventories (tests/test_gpu_tying_wide.py runs them on the device)
WIDE = [(nu, Q, P) for nu, Q in tt.DEVICE_CASES for P in (1, 3)]


def test_table_sizes_of_the_device_cases():
    """The (n_units, Q) pairs the device runs stand where they claim: 4096 words fit the LDS exactly, 4100 do not; the edge symbol is
    at bit 31 of a word or at bit 0 of the next."""
    def size(n_units, Q):
        W = (n_units + 1 + 31) // 32                               # tying_words of tying_check.h
        return W, Q * W, 4 * Q * W
    assert size(96, 1024) == (4, 4096, 16384) and size(96, 1025) == (4, 4100, 16400)
    assert 16384 <= 16 * 1024 < 16400 and tt.LDS_WORDS * 4 == 16 * 1024     # TY_QBITS_LDS: bytes <= it are staged
    assert 3 * 1025 <= 4096                                        # the validator's limit on Q
    edge = {31: (1, 0, 31), 32: (2, 1, 0), 63: (2, 1, 31), 64: (3, 2, 0), 95: (3, 2, 31), 96: (4, 3, 0)}
    for n_units, Q in tt.DEVICE_CASES:
        W, word, bit = edge[n_units]
        assert (size(n_units, Q)[0], n_units >> 5, n_units & 31) == (W, word, bit) and tt.words(n_units) == W
        assert tt.applicable_mistakes(n_units, Q) == ([1, 2, 3] if W >= 2 else []) + ([4] if (n_units, Q) == (96, 1025) else []) + \
            ([5] if (n_units, Q) == (96, 1024) else [])
    assert sorted(m for nu, Q in tt.DEVICE_CASES for m in tt.applicable_mistakes(nu, Q)) == [1] * 6 + [2] * 6 + [3] * 6 + [4, 5]


@pytest.mark.parametrize('Q', [1024, 1025])
@pytest.mark.parametrize('P', [1, 3])
def test_the_wide_chain_is_what_it_claims(P, Q):
    tree = tt.wide_chain(P, Q=Q)
    nu, W = tree.n_units, tt.words(tree.n_units)
    assert (nu, W, tree.Q) == (96, 4, Q) and tree.n_states == 73 * P and tree.n_nodes == P + 2 * 72 * P and tree.n_roots == P
    at = np.flatnonzero(tree.node_cand >= 0)
    assert (tree.node_child[at] > at[:, None]).all()               # children behind their parent, as pcl_tying_upload demands
    for k in range(P):
        f = tt.wide_follower(k, nu)
        assert tt.walk_depth(tree, f[0], f[1], f[2], k) == 72
        node, asked = k, []
        while tree.node_cand[node] >= 0:
            asked.append(int(tree.node_cand[node]))
            node = int(tree.node_child[node].max())                # (the next level is the child created last)
        assert len(set(asked)) == 72 and {3 * Q - 1} | {pos * Q + qi for pos in range(3) for qi in (0, Q - 1)} <= set(asked)
    f = [tt.wide_follower(k, nu) for k in range(3)]
    assert {u >> 5 for c in f for u in c} == set(range(W))         # between them: every word of a row
    assert f[0][0] == f[0][2] == nu                                # both neighbours the utterance edge
    assert any(u & 31 == 31 and v == u + 1 for a in f for b in f for u in (a[0], a[2]) for v in (b[0], b[2]))   # bit 31 | bit 0 of the next word
    qm = tree.q_member.astype(int)
    assert qm[Q - 1, nu] == 1                                      # the table's last word is not zero
    for u in range(nu + 1):                                        # a unit and its aliases disagree on about half of the questions
        for v in range(u % 32, nu + 1, 32):
            if v != u:
                assert 0.4 < (qm[:, u] != qm[:, v]).mean() < 0.6, (u, v)


@pytest.mark.parametrize('n_units,Q,P', WIDE)
def test_the_sample_reads_the_table_at_its_edges(n_units, Q, P):
    """What the sampled walks read of the bit table, by a plain walk over the packed table that is Tree.lookup where it makes no
    mistake: every word of some row, the first and the last word of the table, both sides of every word boundary with both answers."""
    tree, sample, want = tt.device_case(n_units, Q, P)
    W = tt.words(n_units)
    assert 3900 <= len(sample) <= 4600 and sample[:, 1].max() == n_units - 1 and sample[:, [0, 2]].max() == n_units and sample.min() == 0
    for pos in range(3):
        assert set(sample[:, pos].tolist()) >= set(range(n_units + (pos != 1)))       # every unit in every position
    edge = [u for u in tt.BOUNDARY_UNITS + (n_units,) if u <= n_units]
    assert {(l, r) for l in edge for r in edge} <= set(map(tuple, sample[:, [0, 2]].tolist()))
    assert {tuple(f) for f in tt.followers(tree)} <= set(map(tuple, sample.tolist()))
    reads = set()
    assert np.array_equal(tt.table_walk_all(tree, sample, reads=reads), want)
    by_q = {}
    for qi, u, yes in reads:
        by_q.setdefault(qi, set()).add(u >> 5)
    full = sorted(qi for qi, ws in by_q.items() if ws == set(range(W)))
    first = sorted(u for qi, u, _ in reads if qi == 0 and u < 32)
    last = sorted(u for qi, u, _ in reads if qi == Q - 1 and u >> 5 == W - 1)
    assert full and first and last
    # both sides of every word boundary in the inventory, and the edge symbol (bit 31 of a word or bit 0 of the next in every case)
    sides = sorted({u for b in range(1, W + 1) for u in (32 * b - 1, 32 * b) if u <= n_units} | {n_units})
    assert {u & 31 for u in sides} <= {0, 31} and (n_units < 32 or {31, 32} <= set(sides))
    answers = {u: {(qi, yes) for qi, v, yes in reads if v == u} for u in sides}
    for u in sides:
        assert {yes for _, yes in answers[u]} == {0, 1}, u
    print('table (%d, %d) P=%d W=%d: %d contexts, %d (question, unit) pairs read; all %d words of %d rows (first: %s); word 0 by units %s; '
          'word %d by units %s; boundary units %s: %s questions each' % (
              n_units, Q, P, W, len(sample), len({(q, u) for q, u, _ in reads}), W, len(full), full[:3], first[:6], Q * W - 1, last[:6], sides,
              [len(answers[u]) for u in sides]))


@pytest.mark.parametrize('n_units,Q,P', WIDE)
def test_every_broken_walk_differs_on_the_sample(n_units, Q, P):
    tree, sample, want = tt.device_case(n_units, Q, P)
    assert np.array_equal(tt.table_walk_all(tree, sample), want)   # without a mistake: Tree.lookup
    for m in tt.applicable_mistakes(n_units, Q):
        n = int((tt.table_walk_all(tree, sample, m) != want).any(axis=1).sum())
        print('broken walk %d at (%d, %d) P=%d: %d of %d contexts differ (%s)' % (m, n_units, Q, P, n, len(sample), tt.BROKEN[m]))
        assert n >= 1, (m, tt.BROKEN[m])


@pytest.mark.parametrize('n_units,Q,P', WIDE)
def test_the_sample_reaches_the_leaves(n_units, Q, P):
    """Every leaf of a wide chain is reached by a sampled context (its rows are made so).  A Q = 24 chain asks all 24 questions about
    every position, so a context leaves it at level l only if its unit there answers as the follower's on every question asked of that
    position above l: with random rows over at most 96 units about log2 of the number of contexts levels have such a unit.  There the
    sample reaches every leaf that ANY of the inventory's (n_units + 1)^2 n_units contexts reaches, counted here over all of them."""
    tree, sample, want = tt.device_case(n_units, Q, P)
    reachable = set()
    for k in range(P):
        reachable |= set(tree.node_state[np.unique(tt.walk_all(tree, k))].tolist())
    seen = set(want.reshape(-1).tolist())
    print('leaves (%d, %d) P=%d: %d leaves, %d reached by some context of the inventory, %d by the sample' % (n_units, Q, P, tree.n_states, len(reachable), len(seen)))
    assert seen == reachable and min(seen) >= 0
    if Q != tt.CHAIN_Q:
        assert seen == set(range(tree.n_states))
    for k in range(P):                                             # the vectorised walk that found the witnesses is Tree.lookup on the sample
        assert np.array_equal(tree.node_state[tt.walk_all(tree, k, sample)], want[:, k])


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
