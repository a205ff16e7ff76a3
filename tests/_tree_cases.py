"""Case tables of the decision-tree tests (tests/test_tree_twin.py holds every build case to the separation condition on the CPU,
tests/test_gpu_tree.py runs them on the device).

A build case is a dict: P, D, n_units, event_ctx (E, 3), q_member, R0, root_of, the statistics n / s / q, and the build's parameters.
The statistics are sums of frames on the grid k 2^-6, |x| < 8: exact in float64 in any order.  A row's frames scatter around a mean that
depends on its left and right neighbour, its centre and its position, so that questions about each of them have something to find."""
import numpy as np

GRID = 64.0


def grid_frames(rng, mean, n, D):
    x = np.round((mean[None, :] + rng.standard_normal((n, D))) * GRID) / GRID
    return np.clip(x, -7.984375, 7.984375)


def all_events(n_units):
    return np.array([(l, c, r) for l in range(n_units + 1) for c in range(n_units) for r in range(n_units + 1)], dtype=np.int32)


def member(sets, n_units):
    q = np.zeros((len(sets), n_units + 1), dtype=np.uint8)
    for i, s in enumerate(sets):
        q[i, sorted(s)] = 1
    return q


def make(seed, n_units=4, P=2, D=3, sets=None, shared_root=False, counts=(5, 40), zero_rows=(), const_dim=False, keep=None,
         centre_shift=0.0, far_left=None, **params):
    """keep: indices into all_events (lexicographic); zero_rows: statistics rows that stay unseen; far_left: the rows behind that left
    neighbour lie far from all others; const_dim: column 0 is the same value in every frame (its variance is floored)."""
    rng = np.random.default_rng(seed)
    ev = all_events(n_units)
    if keep is not None:
        ev = ev[np.asarray(keep)]
    E, R = len(ev), len(ev) * P
    shift_l, shift_r, shift_c = rng.standard_normal((n_units + 1, D)) * 1.5, rng.standard_normal((n_units + 1, D)), rng.standard_normal((n_units, D))
    if far_left is not None:                                       # the rows behind this left neighbour lie far from all others
        shift_l[far_left] = 4.0
    n, s, q = np.zeros(R, dtype=np.int64), np.zeros((R, D)), np.zeros((R, D))
    for r in range(R):
        e, k = divmod(r, P)
        if r in zero_rows:
            continue
        cnt = int(rng.integers(counts[0], counts[1] + 1))
        mean = shift_l[ev[e, 0]] + 0.5 * shift_r[ev[e, 2]] + centre_shift * shift_c[ev[e, 1]] + 0.25 * k
        x = grid_frames(rng, mean, cnt, D)
        if const_dim:
            x[:, 0] = 0.5
        n[r], s[r], q[r] = cnt, x.sum(axis=0), (x * x).sum(axis=0)
    if sets is None:
        sets = [{u} for u in range(n_units + 1)] + [{0, 1}, {1, 2, n_units}]
    if shared_root:
        root_of, R0 = np.tile(np.arange(P, dtype=np.int32), n_units), P
    else:
        root_of, R0 = np.arange(n_units * P, dtype=np.int32), n_units * P
    case = dict(P=P, D=D, n_units=n_units, event_ctx=ev, q_member=member(sets, n_units), R0=R0, root_of=root_of, n=n, s=s, q=q, min_count=1,
                min_gain=0.0, max_leaves=None, var_floor=1e-4)
    case.update(params)
    return case


def _rand_sets(seed, Q, n_units):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < Q:
        m = rng.integers(0, 2, size=n_units + 1)
        if 0 < m.sum() <= n_units:
            out.append(set(np.flatnonzero(m).tolist()))
    return out


def build_cases():
    """name -> case.  The first is the one whose same-partition ties are exact on both sides: duplicate and complementary questions."""
    c = {}
    c['dup_compl'] = make(1, sets=[{0, 1}, {0, 1}, {2, 3, 4}, {0}, {1, 2, 3, 4}, {2}, {0, 1, 3, 4}])
    c['q1'] = make(2, n_units=2, sets=[{0}])
    c['q65'] = make(3, n_units=6, P=1, D=2, sets=_rand_sets(30, 65, 6), keep=np.arange(0, 294, 5), max_leaves=14)
    c['one_unit'] = make(4, n_units=1, P=3, sets=[{1}, {0}])
    # centre 3 is seen in one context only: its roots hold one row each and cannot split
    c['one_row_root'] = make(5, keep=[i for i, e in enumerate(all_events(4)) if e[1] != 3 or (e[0] == 0 and e[2] == 0)])
    # ... and here that one context was never seen at position 1: a root with n = 0 (stays a leaf; the install is refused)
    keep = [i for i, e in enumerate(all_events(4)) if e[1] != 3 or (e[0] == 0 and e[2] == 0)]
    row0 = [i for i, k in enumerate(keep) if all_events(4)[k][1] == 3][0] * 2 + 1
    c['zero_root'] = make(6, keep=keep, zero_rows=(row0,), max_leaves=12)
    # the rows behind the utterance edge lie far from the rest: the best first split takes them off (12 rows, at most 360 frames), and
    # min_count = 400 forbids that
    c['min_count'] = make(7, n_units=3, P=1, shared_root=True, far_left=3, counts=(20, 30), min_count=400, max_leaves=4)
    c['min_count_off'] = dict(c['min_count'], min_count=1)
    c['max_leaves_mid'] = make(8, max_leaves=8 + 3)
    c['max_leaves_r0'] = make(8, max_leaves=8)
    c['min_gain'] = make(9, min_gain=60.0)
    c['var_floor'] = make(10, const_dim=True, max_leaves=14)
    c['unseen_rows'] = make(11, zero_rows=(0, 3, 17, 18, 40), max_leaves=16)
    c['shared_root'] = make(12, shared_root=True, centre_shift=4.0, sets=[{u} for u in range(5)] + [{0, 1}, {2, 3}], max_leaves=10)
    # one root of 100 rows and 33 candidates: five groups of 8 candidates, the last one ragged (the evaluation kernel walks a leaf's rows
    # one after the other whatever their number: there is no row tile whose edge 100 rows would cross)
    c['big_leaf'] = make(13, P=1, shared_root=True, sets=_rand_sets(31, 11, 4), max_leaves=9, D=5)
    return c


BIG = 2 ** 23                                                     # big_counts' factor


def _mirror(case, src=0, dst=1):
    """The rows of centre dst become bit-identical copies of centre src's (same left and right neighbour, same position): with separate
    roots the two centres' roots hold equal rows in equal order, and every question about a neighbour splits them alike."""
    ev, P = case['event_ctx'], case['P']
    at = {tuple(e): i for i, e in enumerate(ev.tolist())}
    for i, (l, c, r) in enumerate(ev.tolist()):
        if c == dst:
            j = at[(l, src, r)]
            for k in ('n', 's', 'q'):
                case[k][i * P:(i + 1) * P] = case[k][j * P:(j + 1) * P]
    return case


def edge_cases():
    """name -> case: the build's edges (tests/test_gpu_tree_edges.py runs them, tests/test_tree_twin.py holds them to the separation
    condition like the others).  The seeds were chosen on the CPU so that the condition holds; the twin alone decides that."""
    c = {}
    # the evaluation kernel gives a lane to each column of [s | q]: D = 64 fills all 128, D = 1 leaves 2 columns for 17 sums, D = 39 is the
    # front-end's width.  d14 / d40 / d49 are the first widths behind a device width (13, 39, 48): the install pads them to 26, 47 and 64.
    c['wide64'] = make(21, n_units=3, P=2, D=64, max_leaves=6 + 4)
    c['d1'] = make(22, n_units=3, P=1, D=1, max_leaves=3 + 4)
    c['d39'] = make(23, n_units=3, P=2, D=39, max_leaves=6 + 4)
    c['d14'] = make(24, n_units=3, P=1, D=14, max_leaves=3 + 4)
    c['d40'] = make(25, n_units=3, P=2, D=40, max_leaves=6 + 3)
    c['d49'] = make(26, n_units=3, P=1, D=49, max_leaves=3 + 4)
    # 24 candidates: exactly three groups of 8, no ragged last group
    c['q8_full_groups'] = make(27, shared_root=True, centre_shift=2.0, sets=[{0}, {1}, {2}, {3}, {4}, {0, 1}, {1, 2, 4}, {0, 3}], max_leaves=2 + 14)
    # set 8 = set 0 and set 7 = the complement of set 1: of one position, candidates c and c + 8 (the duplicate) lie in adjacent groups,
    # and so do c + 1 and c + 7 (the complement) for the centre and the right neighbour.  The later group's equal gain must not win.
    c['dup_across_groups'] = make(28, shared_root=True, centre_shift=4.0, sets=[{1, 2, 4}, {0, 1}, {0}, {1}, {3}, {4}, {2}, {2, 3, 4}, {1, 2, 4}],
                                  max_leaves=2 + 10)
    # the largest Q the build accepts: 4095 candidates in 512 groups, the last one ragged; 7 symbols, so most sets come many times
    c['q1365'] = make(29, n_units=6, P=1, D=2, sets=_rand_sets(32, 1365, 6), keep=np.arange(0, 294, 12), shared_root=True, max_leaves=1 + 3)
    # centres 0 and 1 hold bit-identical rows under separate roots: their bests tie exactly, the lowest node id goes first.  Built to an
    # odd and to an even number of leaves, so that one of the two stops between a leaf and its mirror image.
    c['mirror_roots_even'] = _mirror(make(30, n_units=3, P=1, max_leaves=3 + 5))
    c['mirror_roots_odd'] = _mirror(make(30, n_units=3, P=1, max_leaves=3 + 6))
    # counts beyond 32 bits: 'min_count' with n, s, q and min_count times 2^23.  A power of two scales every sum, every n and every
    # likelihood exactly (s / n and q / n keep their bits, L = -0.5 n (...) and the gains scale by 2^23 without a rounding), so the
    # twin's decisions, their sep and thr are those of 'min_count', and the case is separated because that one is.  The root holds
    # 1232 frames there: 2^20 would leave every count below 2^32; 2^23 puts the root at 1.0e10, both children beyond 2^32 and min_count
    # (3.4e9) beyond 2^31, so that a count or a threshold cut to 32 bits anywhere changes the tree.
    base = build_cases()['min_count']
    c['big_counts'] = dict(base, n=base['n'] * BIG, s=base['s'] * float(BIG), q=base['q'] * float(BIG), min_count=base['min_count'] * BIG)
    return c


# ------------------------------------------------------------------ statistics at the kernels' edges
DEVICE_DIMS = (13, 26, 39, 47, 48, 64)                            # the row strides the device holds a frame matrix at (pcl_api.hip, device_dim)
WIDTH_DIMS = (1, 12, 13, 14, 26, 27, 37, 39, 40, 45, 47, 48, 49, 63, 64)


def tail_load_dims(G):
    """The widths D at which tree_partial_kernel's element-by-element load runs for the LAST frame row: lane g loads the G columns from
    d0 = G g when d0 < D, in one piece iff (F - 1) FD + d0 + G <= F FD, that is d0 + G <= FD, FD the device width of D."""
    out = []
    for D in range(1, 65):
        FD = min(x for x in DEVICE_DIMS if x >= D)
        if any(d0 + G > FD for d0 in range(0, D, G)):
            out.append(D)
    return out


def order_case(D=13):
    """Gaussian frames whose sums tell one summation order from another: F = 2 * 2048 + 37 rows (three tiles of the counting sort), R = 9,
    two utterances that cover frame rows 0 and F - 1 with a gap between them (whose rows name a statistics row and must not count), the
    rows on either side of both tile edges in the same statistics row, row 0 with more than half of the frames, some rows -1."""
    rng = np.random.default_rng(2048)
    F, R = 2 * 2048 + 37, 9
    frames = rng.standard_normal((F, D)) * 3 + 1
    T, begin = np.array([2100, F - 2150], dtype=np.int32), np.array([0, 2150], dtype=np.int64)
    frame_row = rng.integers(-1, R, size=F).astype(np.int32)
    frame_row[rng.integers(0, F, size=F)] = 0
    frame_row[[2047, 2048]] = 3
    frame_row[[4095, 4096]] = 5
    frame_row[0], frame_row[F - 1] = 7, 8
    return frames, T, begin, frame_row, R


def width_case(D):
    """Grid frames, F = 64, one utterance over all of them; the last two frame rows are kept and go to different statistics rows"""
    rng = np.random.default_rng(300 + D)
    F, R = 64, 7
    frames = np.clip(np.round(rng.standard_normal((F, D)) * 2 * GRID) / GRID, -7.984375, 7.984375)
    frame_row = rng.integers(-1, R, size=F).astype(np.int32)
    frame_row[F - 2], frame_row[F - 1] = 2, 5
    return frames, np.array([F], dtype=np.int32), np.array([0], dtype=np.int64), frame_row, R


def long_case(T):
    """Grid frames at D = 2, one utterance of T frames from frame row 3 on, R = 5; the frames t = 16382 .. 16386 of the utterance (the
    key kernel's grid is 64 x 256 = 16384 threads an utterance: t = 16384 is the first frame of its second step) go to distinct rows."""
    rng = np.random.default_rng(400 + T % 1000)
    F, R, D, b = T + 5, 5, 2, 3
    frames = np.clip(np.round(rng.standard_normal((F, D)) * 2 * GRID) / GRID, -7.984375, 7.984375)
    frame_row = rng.integers(-1, R, size=F).astype(np.int32)
    t = np.arange(16382, min(16387, T))
    frame_row[b + t] = t % R
    return frames, np.array([T], dtype=np.int32), np.array([b], dtype=np.int64), frame_row, R


def frames_case(D, seed=0):
    """Grid frames for the exact statistics tests under PCL_TREE_CHUNK=4: R = 65 rows; rows 0..5 hold 0, 1, 3, 4, 5 and 9 frames (chunk - 1,
    chunk, chunk + 1, two chunks and one), the rest share what is left; some frames map to -1; rows in front of, between and behind the
    utterances are mapped to a row but belong to no utterance."""
    rng = np.random.default_rng(100 + seed + D)
    T = np.array([40, 0, 33, 1, 75], dtype=np.int32)
    begin = np.array([90, 60, 3, 50, 140], dtype=np.int64)         # does not ascend; gaps in front, between, behind
    F, R = 230, 65
    frames = np.clip(np.round(rng.standard_normal((F, D)) * 2 * GRID) / GRID, -7.984375, 7.984375)
    inside = np.zeros(F, dtype=bool)
    for t, b in zip(T, begin):
        inside[b:b + t] = True
    idx = np.flatnonzero(inside)
    want = [0, 1, 3, 4, 5, 9]
    frame_row = rng.integers(0, R, size=F).astype(np.int32)        # (the rows outside the utterances keep a valid row: they must not count)
    pool = rng.permutation(idx)
    at = 0
    frame_row[idx] = -2
    for r, cnt in enumerate(want):
        frame_row[pool[at:at + cnt]] = r
        at += cnt
    rest = pool[at:]
    frame_row[rest] = rng.integers(len(want), R, size=len(rest))
    frame_row[rest[:7]] = -1
    assert (frame_row[idx] >= -1).all()
    return frames, T, begin, frame_row, R
