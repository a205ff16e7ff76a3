// Everything a batch hands the kernels, planned on the host: the per-utterance offsets (BatchShape), the sparse transition structure
// (SparseTrans), the per-state segment lists with their duplicate rows (ScorePlan), the XCD-ordered tile lists (plan_tiles) and the label
// structure of a label-built batch (LabelPlan).  Plain structs and functions of plain arguments: no HIP runtime call, no device memory, no
// upload, and of the context only the sink of the error text (PCL_FAIL) -- tests/batch_plan_host_check.cpp runs all of it under the host
// sanitizers.  The kernels index with these arrays unchecked, so every planner validates first and writes its output only on success: a
// refused call leaves *out (and the descriptors) as they were.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "pcl_own.h"

// ---------------------------------------------------------------- device-side descriptors
// One scoring segment = one (utterance, emitting row): `len` consecutive frames starting at frame
// row `frame0`, written to out[out0 + t*out_stride].  Segments are sorted by GMM state; `vstart`
// is the segment's offset inside the state's virtual concatenation of frames (H4, state-major).
struct ScoreSeg {
    long long frame0;
    long long out0;
    int len;
    int out_stride;
    int vstart;
    int pad;
};
// An emission row that repeats another row of its utterance (the label names the unit twice): T values at stride N.
struct DupRow {
    long long src, dst;
    int T, N;
};
// One workgroup of the scoring kernel: frames [vstart, vstart+tile) of `state`'s concatenation.
struct ScoreTile {
    int state;
    int seg_lo, seg_hi;  // the state's segments are segs[seg_lo, seg_hi)
    int vstart;
    int seg0;            // the segment that contains vstart: a frame of the tile is almost always in seg0 or seg0 + 1
};
// One sentence HMM (time-major device matrices: element (t, n) at b_off + t*N + n).
struct UttDesc {
    long long b_off;    // into Bt / alpha / beta / lgam
    long long mat_off;  // into the ragged dense (N,N) xi output
    long long frame0;   // first frame row (or -1)
    int T, N;
    int vec_off;   // into ragged (N,) vectors
    int ptr_off;   // into row_ptr / col_ptr (N+1 entries per utterance)
    int nnz_off;   // into CSR / CSC entry arrays
    int path_off;  // into ragged (T,) vectors
};

// ---------------------------------------------------------------- the utterances' offsets
struct BatchShape {
    std::vector<UttDesc> utt;
    long long sumNT = 0, sumN = 0, sumT = 0, sumNN = 0;
    int Nmax = 0, Tmax = 0;
    long long max_frame_end = 0;   // max over utterances of frame_begin + T: re-validated against the CURRENT frame matrix
    bool has_one_frame = false;    // an utterance of ONE frame: the reference's Baum-Welch raises on it (golden G15) and it adds nothing to any accumulator
};

// U sentence HMMs of N[u] rows over T[u] frames from row frame_begin[u] of a frame matrix of F rows (frame_begin NULL: no frames, frame0 = -1)
static int plan_batch_shape(pcl_ctx *ctx, int U, const int32_t *N, const int32_t *T, const int64_t *frame_begin, long long F, BatchShape *out) {
    if (U <= 0 || !N || !T) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_create: bad arguments (U=%d)", U);
    // several kernels index the utterance with the grid's second dimension (HIP: at most 65535): say so here instead of failing a launch later
    if (U > 65535) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_create: %d utterances in one batch, at most 65535 (split the batch)", U);
    BatchShape s;
    s.utt.resize(U);
    for (int u = 0; u < U; ++u) {
        if (N[u] < 1 || T[u] < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_create: utterance %d has N=%d T=%d", u, N[u], T[u]);
        if (frame_begin && (frame_begin[u] < 0 || frame_begin[u] + T[u] > F))
            PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_create: utterance %d frames [%lld,%lld) outside the uploaded %lld frames", u,
                     (long long)frame_begin[u], (long long)frame_begin[u] + T[u], F);
        UttDesc &d = s.utt[u];
        d.b_off = s.sumNT;
        d.mat_off = s.sumNN;
        d.frame0 = frame_begin ? frame_begin[u] : -1;
        if (frame_begin) s.max_frame_end = std::max(s.max_frame_end, (long long)frame_begin[u] + T[u]);
        d.T = T[u];
        d.N = N[u];
        d.vec_off = (int)s.sumN;
        d.ptr_off = (int)(s.sumN + u);
        d.nnz_off = 0;
        d.path_off = (int)s.sumT;
        s.sumNT += (long long)N[u] * T[u];
        s.sumNN += (long long)N[u] * N[u];
        s.sumN += N[u];
        s.sumT += T[u];
        s.Nmax = std::max(s.Nmax, (int)N[u]);
        s.Tmax = std::max(s.Tmax, (int)T[u]);
        if (T[u] == 1) s.has_one_frame = true;
        // the int offsets of the next utterance, and after the last one the lengths of the ragged arrays (row_ptr / col_ptr: sum N + U)
        if (s.sumN + u + 1 > 0x7fffffffLL || s.sumT > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_create: batch too large");
    }
    *out = std::move(s);
    return PCL_OK;
}

// Does a frame matrix of F rows hold every row the batch refers to?  (A batch outlives uploads: each caller words its own refusal.)
static bool shape_fits_frames(const BatchShape &s, long long F) { return s.max_frame_end <= F; }

// A frame has one owner: the utterances' row ranges are disjoint (touching is disjoint).  The first offending pair in the order of the first
// rows, equal first rows by index: `second` starts before the end of `first`, the utterance ahead of it in that order (-1: none, frame0 < 0).
struct UttOverlap { bool found; int first, second; };
static UttOverlap shape_overlap(const BatchShape &s) {
    const std::vector<UttDesc> &utt = s.utt;
    std::vector<int> by(utt.size());
    for (size_t u = 0; u < by.size(); ++u) by[u] = (int)u;
    std::sort(by.begin(), by.end(), [&](int x, int y) { return utt[x].frame0 != utt[y].frame0 ? utt[x].frame0 < utt[y].frame0 : x < y; });
    long long end = 0;
    int prev = -1;
    for (int u : by) {
        if (utt[u].frame0 < end) return {true, prev, u};
        end = utt[u].frame0 + utt[u].T;
        prev = u;
    }
    return {false, -1, -1};
}

// ---------------------------------------------------------------- the label structure of a label-built batch
// (AcousticModel.embedded, AcousticModel.py:957-1014: a sentence HMM is its label's unit HMMs, e = S - 2 emitting rows each, between an
// entry and an exit row)
struct LabelPlan {
    std::vector<int32_t> label_len, labels;   // as the caller gave them
    std::vector<int> label_off;               // U + 1 offsets into labels
    int label_max = 0, label_len_max = 0;     // largest unit id / longest label of the batch
    std::vector<int32_t> N;                   // rows of every sentence HMM: e L + 2 (AcousticModel.py:966)
    std::vector<int32_t> row_state;           // row -> GMM state WITHOUT tying, unit e + k (embedded_prob, AcousticModel.py:990-1001), PCL_ROW_ENTRY / PCL_ROW_EXIT
    std::vector<int> occ_ptr, occ_utt, occ_row0;   // unit -> [occ_ptr[unit], occ_ptr[unit + 1]) -> (utterance, first emitting row)
};

static int plan_labels(pcl_ctx *ctx, const char *who, int U, const int32_t *label_len, const int32_t *labels, int e, int n_units, LabelPlan *out) {
    LabelPlan p;
    p.label_off.assign((size_t)U + 1, 0);
    p.N.resize(U);
    long long tot = 0, rows = 0;
    for (int u = 0; u < U; ++u) {
        if (label_len[u] < 1) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d has an empty label", who, u);
        const long long n = (long long)e * label_len[u] + 2;
        tot += label_len[u];
        rows += n;
        if (rows > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_create: batch too large");
        p.N[u] = (int32_t)n;
        p.label_off[u + 1] = (int)tot;
    }
    for (long long i = 0; i < tot; ++i)
        if (labels[i] < 0 || labels[i] >= n_units) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: unit id %d outside [0,%d)", who, labels[i], n_units);
    p.label_len.assign(label_len, label_len + U);
    p.labels.assign(labels, labels + tot);
    p.label_max = *std::max_element(labels, labels + tot);
    p.label_len_max = *std::max_element(label_len, label_len + U);
    p.row_state.resize((size_t)rows);
    p.occ_ptr.assign((size_t)n_units + 1, 0);
    for (long long i = 0; i < tot; ++i) ++p.occ_ptr[labels[i] + 1];
    for (int k = 0; k < n_units; ++k) p.occ_ptr[k + 1] += p.occ_ptr[k];
    p.occ_utt.resize((size_t)tot);
    p.occ_row0.resize((size_t)tot);
    std::vector<int> fill(p.occ_ptr.begin(), p.occ_ptr.end() - 1);
    size_t row0 = 0;
    for (int u = 0; u < U; ++u) {
        int32_t *rs = p.row_state.data() + row0;
        rs[0] = PCL_ROW_ENTRY;
        rs[p.N[u] - 1] = PCL_ROW_EXIT;
        for (int pos = 0; pos < label_len[u]; ++pos) {
            const int unit = labels[p.label_off[u] + pos];
            for (int k = 0; k < e; ++k) rs[1 + pos * e + k] = unit * e + k;
            const int q = fill[unit]++;
            p.occ_utt[q] = u;
            p.occ_row0[q] = 1 + pos * e;
        }
        row0 += p.N[u];
    }
    *out = std::move(p);
    return PCL_OK;
}

// ---------------------------------------------------------------- the sparse transition structure
// CSR successors / CSC predecessors of every utterance, both with ascending indices; entries with ln A = -inf are not stored.
// row_ptr / col_ptr: sumN + U entries (N_u + 1 per utterance at UttDesc::ptr_off, local offsets); the entries of utterance u start at
// UttDesc::nnz_off.  The arrays travel to the device and go; the batch keeps what the launchers choose their kernels by (TransShape).
struct TransShape {
    int max_outdeg = 0, max_indeg = 0;
    bool left_right = true;   // every state is reached from itself / the state before it only (what AcousticModel.embedded builds, AcousticModel.py:979-989)
    long long nnz = 0;
};
struct SparseTrans {
    std::vector<int> row_ptr, col_idx, col_ptr, row_idx;
    std::vector<double> csr_val, csc_val;
    TransShape shape;
};

// rows(u, i, emit) calls emit(column, ln A) for the finite entries of row i of utterance u, in ascending column order.  On success the
// utterances' nnz_off are set.
template <typename Rows>
static int plan_sparse_trans(pcl_ctx *ctx, const char *who, std::vector<UttDesc> &utt, Rows rows, SparseTrans *out) {
    SparseTrans s;
    size_t np = 0;
    for (const UttDesc &d : utt) np += (size_t)d.N + 1;
    s.row_ptr.resize(np);
    s.col_ptr.resize(np);
    std::vector<int> nnz_off(utt.size()), fill;
    for (size_t u = 0; u < utt.size(); ++u) {
        const UttDesc &d = utt[u];
        const int N = d.N;
        const size_t base = s.col_idx.size();
        nnz_off[u] = (int)base;
        int *rp = s.row_ptr.data() + d.ptr_off, *cp = s.col_ptr.data() + d.ptr_off;
        for (int i = 0; i < N; ++i) {
            rp[i] = (int)(s.col_idx.size() - base);
            rows((int)u, i, [&](int j, double v) {
                s.col_idx.push_back(j);
                s.csr_val.push_back(v);
                if (j != i && j != i + 1) s.shape.left_right = false;
            });
            s.shape.max_outdeg = std::max(s.shape.max_outdeg, (int)(s.col_idx.size() - base) - rp[i]);
        }
        if (s.col_idx.size() > 0x7fffffffULL) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: too many transitions", who);
        const int cnt = rp[N] = (int)(s.col_idx.size() - base);
        // CSC by a counting sort of the CSR entries: sources come out in ascending order
        std::fill(cp, cp + N + 1, 0);
        for (int k = 0; k < cnt; ++k) ++cp[s.col_idx[base + k] + 1];
        for (int j = 0; j < N; ++j) {
            s.shape.max_indeg = std::max(s.shape.max_indeg, cp[j + 1]);
            cp[j + 1] += cp[j];
        }
        fill.assign(cp, cp + N);
        s.row_idx.resize(base + cnt);
        s.csc_val.resize(base + cnt);
        for (int i = 0; i < N; ++i)
            for (int k = rp[i]; k < rp[i + 1]; ++k) {
                const int q = fill[s.col_idx[base + k]]++;
                s.row_idx[base + q] = i;
                s.csc_val[base + q] = s.csr_val[base + k];
            }
    }
    s.shape.nnz = (long long)s.col_idx.size();
    for (size_t u = 0; u < utt.size(); ++u) utt[u].nnz_off = nnz_off[u];
    *out = std::move(s);
    return PCL_OK;
}

// The two callers' rows.  The caller's dense matrices: ragged (N, N) at UttDesc::mat_off.
static auto dense_trans_rows(const std::vector<UttDesc> &utt, const double *logA) {
    return [&utt, logA](int u, int i, auto emit) {
        const int N = utt[u].N;
        const double *row = logA + utt[u].mat_off + (size_t)i * N;
        for (int j = 0; j < N; ++j)
            if (!(row[j] == -INFINITY)) emit(j, row[j]);
    };
}
// The sentence HMM of a label over the units' ln A (unit_logtrans [n_units][S][S]; embedded_transmat, AcousticModel.py:979-989): row 0 is
// the first unit's entry row at columns 0..S-1, row 1 + p e + k is row 1 + k of unit lab[p] at columns p e + c, the exit row has no successors.
static auto label_trans_rows(const std::vector<UttDesc> &utt, const LabelPlan &lab, const double *unit_logtrans, int S) {
    return [&utt, &lab, unit_logtrans, S](int u, int i, auto emit) {
        if (i == utt[u].N - 1) return;
        const int e = S - 2, p = (i == 0) ? 0 : (i - 1) / e, r = (i == 0) ? 0 : 1 + (i - 1) % e;
        const double *row = unit_logtrans + ((size_t)lab.labels[lab.label_off[u] + p] * S + r) * S;
        for (int c = 0; c < S; ++c)
            if (!(row[c] == -INFINITY)) emit(p * e + c, row[c]);
    };
}

// ---------------------------------------------------------------- the scoring work lists
// A label that names a unit twice has the same (frames, state) pair on two rows: the reference scores it once per label
// position (AcousticModel.py:897-902).  Here the FIRST row of a state in an utterance is scored (a state's segments list
// those first: scoring tiles cover [lo, hip)), the others are copies of its emission row (dup_rows_kernel); the accumulate
// pass walks all of a state's segments, each row has its own posteriors.
struct ScorePlan {
    std::vector<int32_t> row_state;               // the map the lists were built for
    std::vector<ScoreSeg> segs;                   // sorted by state (ScoreSeg::pad holds it); per state the scored rows of all utterances, then the copies
    std::vector<DupRow> dups;
    std::vector<int> seg_of_row;                  // (utterance, row) -> its segment (-1: not a GMM row)
    std::vector<int> work_states;                 // the states with work, ascending, and per such state:
    std::vector<int> state_seg_lo, state_seg_hi;  // its segment range
    std::vector<int> state_seg_hip;               // ... of which [lo, hip) are scored and [hip, hi) are copies of a scored row
    int n_segs = 0;
    int max_state = -1;                           // largest GMM state id any row refers to: re-validated against the CURRENT model
    int max_N = 0;                                // rows of the largest sentence HMM of the batch
};

// row_state: ragged (N_u,) at UttDesc::vec_off, a state of a model of J states or PCL_ROW_ENTRY / PCL_ROW_EXIT
static int plan_score(pcl_ctx *ctx, const std::vector<UttDesc> &utt, const int32_t *row_state, int J, ScorePlan *out) {
    const int U = (int)utt.size();
    ScorePlan p;
    std::vector<int> start((size_t)J + 1, 0);     // segments per state, then (exclusive scan) each state's first
    std::vector<long long> frames(J, 0);
    size_t sumN = 0;
    for (int u = 0; u < U; ++u) {
        const UttDesc &d = utt[u];
        for (int n = 0; n < d.N; ++n) {
            const int st = row_state[d.vec_off + n];
            if (st >= J || st < PCL_ROW_EXIT) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_set_states: utterance %d row %d has state %d outside [0,%d)", u, n, st, J);
            if (st < 0) continue;
            if (d.frame0 < 0) PCL_FAIL(ctx, PCL_ERR_STATE, "pcl_batch_set_states: batch was created without frame_begin");
            if ((frames[st] += d.T) > 0x7fffffffLL) PCL_FAIL(ctx, PCL_ERR_INVALID, "pcl_batch_set_states: state %d has too many frames", st);
            ++start[st + 1];
            p.max_state = std::max(p.max_state, st);
        }
        sumN += d.N;
        p.max_N = std::max(p.max_N, d.N);
    }
    for (int j = 0; j < J; ++j) start[j + 1] += start[j];
    p.n_segs = start[J];
    p.row_state.assign(row_state, row_state + sumN);
    // the first row of a state in an utterance is scored, a later one copies it
    std::vector<int> nprim(J, 0), first_row(J, -1), touched;
    std::vector<char> is_dup(sumN, 0);
    for (int u = 0; u < U; ++u) {
        const UttDesc &d = utt[u];
        touched.clear();
        for (int n = 0; n < d.N; ++n) {
            const int st = row_state[d.vec_off + n];
            if (st < 0) continue;
            if (first_row[st] < 0) {
                first_row[st] = n;
                touched.push_back(st);
                ++nprim[st];
            } else {
                is_dup[d.vec_off + n] = 1;
                p.dups.push_back(DupRow{d.b_off + first_row[st], d.b_off + n, d.T, d.N});
            }
        }
        for (int st : touched) first_row[st] = -1;
    }
    p.segs.assign(p.n_segs, ScoreSeg());
    p.seg_of_row.assign(sumN, -1);
    std::vector<int> fill(start.begin(), start.end() - 1);
    std::fill(frames.begin(), frames.end(), 0);
    for (int pass = 0; pass < 2; ++pass)                         // the scored rows of every state first, then the copies
        for (int u = 0; u < U; ++u) {
            const UttDesc &d = utt[u];
            for (int n = 0; n < d.N; ++n) {
                const int st = row_state[d.vec_off + n];
                if (st < 0 || (int)is_dup[d.vec_off + n] != pass) continue;
                p.seg_of_row[d.vec_off + n] = fill[st];
                ScoreSeg &s = p.segs[fill[st]++];
                s.frame0 = d.frame0;
                s.out0 = d.b_off + n;
                s.len = d.T;
                s.out_stride = d.N;
                s.vstart = (int)frames[st];
                s.pad = st;
                frames[st] += d.T;
            }
        }
    for (int j = 0; j < J; ++j)
        if (start[j + 1] > start[j]) {
            p.work_states.push_back(j);
            p.state_seg_lo.push_back(start[j]);
            p.state_seg_hi.push_back(start[j + 1]);
            p.state_seg_hip.push_back(start[j] + nprim[j]);
        }
    *out = std::move(p);
    return PCL_OK;
}

// XCD-aware tile order for a subset of the plan's states with work (`which` indexes work_states), tiles of tf frames: workgroups are
// dealt round-robin over the 8 XCDs (block b -> XCD b % 8, observed, speed only), so all tiles of one state are placed at block indices
// with the same residue mod 8: the state's parameter block is then fetched into ONE XCD's L2 instead of eight.
// Shorter queues are padded with empty tiles (seg_lo == seg_hi), which exit immediately.
static std::vector<ScoreTile> plan_tiles(const ScorePlan &p, const std::vector<size_t> &which, int tf) {
    constexpr int NXCD = 8;
    std::vector<ScoreTile> queue[NXCD];
    std::vector<long long> load(NXCD, 0);
    for (size_t k : which) {
        const int lo = p.state_seg_lo[k], hi = p.state_seg_hip[k];      // (the scored rows; the copies sit behind them)
        const long long tot = (long long)p.segs[hi - 1].vstart + p.segs[hi - 1].len;
        int g = 0;
        for (int x = 1; x < NXCD; ++x)
            if (load[x] < load[g]) g = x;          // least-loaded XCD queue
        int s0 = lo;
        for (long long v = 0; v < tot; v += tf) {
            while (s0 + 1 < hi && p.segs[s0 + 1].vstart <= v) ++s0;
            queue[g].push_back(ScoreTile{p.work_states[k], lo, hi, (int)v, s0});
        }
        load[g] += (tot + tf - 1) / tf;
    }
    size_t depth = 0;
    for (int x = 0; x < NXCD; ++x) depth = std::max(depth, queue[x].size());
    std::vector<ScoreTile> tiles;
    tiles.reserve(depth * NXCD);
    for (size_t q = 0; q < depth; ++q)
        for (int x = 0; x < NXCD; ++x) tiles.push_back(q < queue[x].size() ? queue[x][q] : ScoreTile{0, 0, 0, 0, 0});
    return tiles;
}
