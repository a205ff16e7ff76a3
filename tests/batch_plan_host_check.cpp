// Stand-alone check of the batch planners of poccala_amd/csrc/batch_plan.h (plan_batch_shape with shape_overlap and shape_fits_frames,
// plan_sparse_trans with both of its row enumerators, plan_score, plan_tiles, plan_labels) against a stub context.  Built with the host
// sanitizers and run as its own process by tests/test_batch_plan_host.py: exit status 0 and no sanitizer report = pass.  Expected values
// are written out by hand or computed by the naive restatements below (dense double scans, per-state searches), never by the code under test.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../poccala_amd/csrc/batch_plan.h"

struct pcl_ctx {
    std::string err;
};
int pcl_ctx_device(const pcl_ctx *) { return 0; }
void pcl_set_error(pcl_ctx *ctx, const char *msg) { ctx->err = msg; }

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

typedef std::vector<int> VI;
typedef std::vector<double> VD;
static const double NINF = -INFINITY;
static bool says(const pcl_ctx &ctx, const char *text) { return ctx.err == text; }

// the descriptors have no padding bytes: equal fields <=> equal bytes
template <typename T>
static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static bool same_shape(const BatchShape &a, const BatchShape &b) {
    return same(a.utt, b.utt) && a.sumNT == b.sumNT && a.sumN == b.sumN && a.sumT == b.sumT && a.sumNN == b.sumNN && a.Nmax == b.Nmax && a.Tmax == b.Tmax &&
           a.max_frame_end == b.max_frame_end && a.has_one_frame == b.has_one_frame;
}
static bool same_sparse(const SparseTrans &a, const SparseTrans &b) {
    return a.row_ptr == b.row_ptr && a.col_idx == b.col_idx && same(a.csr_val, b.csr_val) && a.col_ptr == b.col_ptr && a.row_idx == b.row_idx &&
           same(a.csc_val, b.csc_val) && a.shape.max_outdeg == b.shape.max_outdeg && a.shape.max_indeg == b.shape.max_indeg &&
           a.shape.left_right == b.shape.left_right && a.shape.nnz == b.shape.nnz;
}
static bool same_plan(const ScorePlan &a, const ScorePlan &b) {
    return a.row_state == b.row_state && same(a.segs, b.segs) && same(a.dups, b.dups) && a.seg_of_row == b.seg_of_row && a.work_states == b.work_states &&
           a.state_seg_lo == b.state_seg_lo && a.state_seg_hi == b.state_seg_hi && a.state_seg_hip == b.state_seg_hip && a.n_segs == b.n_segs &&
           a.max_state == b.max_state && a.max_N == b.max_N;
}
static bool same_labels(const LabelPlan &a, const LabelPlan &b) {
    return a.label_len == b.label_len && a.labels == b.labels && a.label_off == b.label_off && a.label_max == b.label_max && a.label_len_max == b.label_len_max &&
           a.N == b.N && a.row_state == b.row_state && a.occ_ptr == b.occ_ptr && a.occ_utt == b.occ_utt && a.occ_row0 == b.occ_row0;
}
static VI nnz_offs(const std::vector<UttDesc> &utt) {
    VI r;
    for (const UttDesc &d : utt) r.push_back(d.nnz_off);
    return r;
}

// ---------------------------------------------------------------- naive restatements
// offsets: every one a sum from the first utterance
static BatchShape naive_shape(int U, const int32_t *N, const int32_t *T, const int64_t *fb) {
    BatchShape s;
    s.utt.resize(U);
    for (int u = 0; u < U; ++u) {
        UttDesc d = {0, 0, fb ? (long long)fb[u] : -1, T[u], N[u], 0, u, 0, 0};
        for (int v = 0; v < u; ++v) {
            d.b_off += (long long)N[v] * T[v];
            d.mat_off += (long long)N[v] * N[v];
            d.vec_off += N[v];
            d.ptr_off += N[v];
            d.path_off += T[v];
        }
        s.utt[u] = d;
        s.sumNT += (long long)N[u] * T[u];
        s.sumNN += (long long)N[u] * N[u];
        s.sumN += N[u];
        s.sumT += T[u];
        if (N[u] > s.Nmax) s.Nmax = N[u];
        if (T[u] > s.Tmax) s.Tmax = T[u];
        if (fb && fb[u] + T[u] > s.max_frame_end) s.max_frame_end = fb[u] + T[u];
        if (T[u] == 1) s.has_one_frame = true;
    }
    return s;
}

// CSR by a scan of the rows, CSC by a scan of the columns of the dense matrices (ragged (N, N) at mat_off)
static SparseTrans naive_sparse(const std::vector<UttDesc> &utt, const VD &A, VI *nnz_off) {
    SparseTrans s;
    nnz_off->clear();
    for (const UttDesc &d : utt) {
        const int N = d.N;
        const double *a = A.data() + d.mat_off;
        nnz_off->push_back((int)s.col_idx.size());
        int cnt = 0;
        for (int i = 0; i < N; ++i) {
            s.row_ptr.push_back(cnt);
            int deg = 0;
            for (int j = 0; j < N; ++j)
                if (a[i * N + j] != NINF) {
                    s.col_idx.push_back(j);
                    s.csr_val.push_back(a[i * N + j]);
                    ++deg;
                    if (j < i || j > i + 1) s.shape.left_right = false;
                }
            cnt += deg;
            if (deg > s.shape.max_outdeg) s.shape.max_outdeg = deg;
        }
        s.row_ptr.push_back(cnt);
        cnt = 0;
        for (int j = 0; j < N; ++j) {
            s.col_ptr.push_back(cnt);
            int deg = 0;
            for (int i = 0; i < N; ++i)
                if (a[i * N + j] != NINF) {
                    s.row_idx.push_back(i);
                    s.csc_val.push_back(a[i * N + j]);
                    ++deg;
                }
            cnt += deg;
            if (deg > s.shape.max_indeg) s.shape.max_indeg = deg;
        }
        s.col_ptr.push_back(cnt);
    }
    s.shape.nnz = (long long)s.col_idx.size();
    return s;
}

// AcousticModel.embedded's embedded_transmat on ln A (lt: [n_units][S][S]): rows [0, S-1) x columns [0, S) = the first unit's rows but the
// last; then for label position i the rows [a, b) x columns [a-1, a-1+S) = the unit's rows [1, S-1), a = i (S-2) + 1, b = (i+1)(S-2) + 1
static void embed_dense(const int32_t *lab, int L, int S, const VD &lt, double *out) {
    const int N = (S - 2) * L + 2;
    for (int i = 0; i < N * N; ++i) out[i] = NINF;
    for (int r = 0; r < S - 1; ++r)
        for (int c = 0; c < S; ++c) out[r * N + c] = lt[((size_t)lab[0] * S + r) * S + c];
    for (int i = 0; i < L; ++i) {
        const int a = i * (S - 2) + 1, b = (i + 1) * (S - 2) + 1;
        for (int r = a; r < b; ++r)
            for (int c = 0; c < S; ++c) out[r * N + a - 1 + c] = lt[((size_t)lab[i] * S + 1 + r - a) * S + c];
    }
}

// per state a search of all rows: first the rows that are the first of their state in their utterance, then the others
static ScorePlan naive_plan(const std::vector<UttDesc> &utt, const std::vector<int32_t> &rs, int J) {
    ScorePlan p;
    p.row_state = rs;
    p.seg_of_row.assign(rs.size(), -1);
    for (const UttDesc &d : utt) {
        if (d.N > p.max_N) p.max_N = d.N;
        for (int n = 0; n < d.N; ++n) {
            const int st = rs[d.vec_off + n];
            if (st > p.max_state) p.max_state = st;
            if (st < 0) continue;
            for (int m = 0; m < n; ++m)
                if (rs[d.vec_off + m] == st) {
                    p.dups.push_back(DupRow{d.b_off + m, d.b_off + n, d.T, d.N});
                    break;
                }
        }
    }
    for (int j = 0; j < J; ++j) {
        const int lo = (int)p.segs.size();
        int hip = lo, v = 0;
        for (int copies = 0; copies < 2; ++copies) {
            for (const UttDesc &d : utt)
                for (int n = 0; n < d.N; ++n) {
                    if (rs[d.vec_off + n] != j) continue;
                    bool copy = false;
                    for (int m = 0; m < n; ++m) copy = copy || rs[d.vec_off + m] == j;
                    if ((int)copy != copies) continue;
                    p.seg_of_row[d.vec_off + n] = (int)p.segs.size();
                    p.segs.push_back(ScoreSeg{d.frame0, d.b_off + n, d.T, d.N, v, j});
                    v += d.T;
                }
            if (!copies) hip = (int)p.segs.size();
        }
        if ((int)p.segs.size() > lo) {
            p.work_states.push_back(j);
            p.state_seg_lo.push_back(lo);
            p.state_seg_hi.push_back((int)p.segs.size());
            p.state_seg_hip.push_back(hip);
        }
    }
    p.n_segs = (int)p.segs.size();
    return p;
}

// what plan_tiles promises, for the states `which` of plan p at tf frames a tile
static void check_tiles(const ScorePlan &p, const std::vector<size_t> &which, int tf) {
    const std::vector<ScoreTile> tiles = plan_tiles(p, which, tf);
    CHECK(tiles.size() % 8 == 0);
    if (which.empty()) CHECK(tiles.empty());
    long long want = 0;
    for (size_t k : which) {                                       // every state: its tiles in one queue, in order, no frame missed
        const int lo = p.state_seg_lo[k], hip = p.state_seg_hip[k];
        long long tot = 0;
        for (int s = lo; s < hip; ++s) tot += p.segs[s].len;
        want += (tot + tf - 1) / tf;
        int residue = -1;
        long long next = 0;
        for (size_t i = 0; i < tiles.size(); ++i) {
            const ScoreTile &t = tiles[i];
            if (t.seg_lo == t.seg_hi || t.state != p.work_states[k]) continue;
            if (residue < 0) residue = (int)(i % 8);
            CHECK((int)(i % 8) == residue);
            CHECK(t.seg_lo == lo && t.seg_hi == hip && t.vstart == next);      // only the scored segments [lo, hip) are tiled
            CHECK(t.seg0 >= lo && t.seg0 < hip && p.segs[t.seg0].vstart <= t.vstart && t.vstart < p.segs[t.seg0].vstart + p.segs[t.seg0].len);
            next += tf;
        }
        CHECK(next >= tot && next < tot + tf);
    }
    long long full = 0;
    size_t last_full = 0;
    for (size_t i = 0; i < tiles.size(); ++i) {
        const ScoreTile &t = tiles[i];
        if (t.seg_lo == t.seg_hi) CHECK(t.state == 0 && t.seg_lo == 0 && t.vstart == 0 && t.seg0 == 0);   // padding: all zero
        else ++full, last_full = i;
    }
    CHECK(full == want);
    if (full) CHECK(tiles.size() - last_full <= 8);                // no row of padding alone
}

static void check_shape(pcl_ctx *ctx) {
    BatchShape s;
    {   // U = 2, N = (3, 5), T = (2, 1)
        const int32_t N[2] = {3, 5}, T[2] = {2, 1};
        const int64_t fb[2] = {4, 0};
        CHECK(plan_batch_shape(ctx, 2, N, T, fb, 6, &s) == PCL_OK);
        const UttDesc want[2] = {{0, 0, 4, 2, 3, 0, 0, 0, 0}, {6, 9, 0, 1, 5, 3, 4, 0, 2}};
        CHECK(s.utt.size() == 2 && memcmp(s.utt.data(), want, sizeof(want)) == 0);
        CHECK(s.sumNT == 11 && s.sumNN == 34 && s.sumN == 8 && s.sumT == 3 && s.Nmax == 5 && s.Tmax == 2 && s.max_frame_end == 6 && s.has_one_frame);
        CHECK(same_shape(s, naive_shape(2, N, T, fb)));
        const int32_t T2[2] = {2, 2};
        CHECK(plan_batch_shape(ctx, 2, N, T2, fb, 6, &s) == PCL_OK && !s.has_one_frame && s.sumNT == 16);
        // no frames: frame0 = -1 and no range check (F = 0)
        CHECK(plan_batch_shape(ctx, 2, N, T, nullptr, 0, &s) == PCL_OK && s.utt[0].frame0 == -1 && s.utt[1].frame0 == -1 && s.max_frame_end == 0);
        CHECK(same_shape(s, naive_shape(2, N, T, nullptr)));
    }
    const BatchShape keep = s;
    {   // the refusals leave the output alone
        const int32_t N[2] = {3, 5}, T[2] = {2, 1}, N0[2] = {3, 0}, T0[2] = {0, 1}, T3[2] = {3, 1};
        const int64_t fb[2] = {4, 0}, neg[2] = {4, -1};
        CHECK(plan_batch_shape(ctx, 2, N0, T, fb, 6, &s) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_create: utterance 1 has N=0 T=1"));
        CHECK(plan_batch_shape(ctx, 2, N, T0, fb, 6, &s) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_create: utterance 0 has N=3 T=0"));
        CHECK(plan_batch_shape(ctx, 2, N, T3, fb, 6, &s) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_create: utterance 0 frames [4,7) outside the uploaded 6 frames"));
        CHECK(plan_batch_shape(ctx, 2, N, T, neg, 6, &s) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_create: utterance 1 frames [-1,0) outside the uploaded 6 frames"));
        CHECK(plan_batch_shape(ctx, 0, N, T, fb, 6, &s) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_create: bad arguments (U=0)"));
        CHECK(plan_batch_shape(ctx, 2, nullptr, T, fb, 6, &s) == PCL_ERR_INVALID && plan_batch_shape(ctx, 2, N, nullptr, fb, 6, &s) == PCL_ERR_INVALID);
        const std::vector<int32_t> ones(65536, 1);
        CHECK(plan_batch_shape(ctx, 65536, ones.data(), ones.data(), nullptr, 0, &s) == PCL_ERR_INVALID &&
              says(*ctx, "pcl_batch_create: 65536 utterances in one batch, at most 65535 (split the batch)"));
        CHECK(same_shape(s, keep));
        CHECK(plan_batch_shape(ctx, 65535, ones.data(), ones.data(), nullptr, 0, &s) == PCL_OK && s.sumN == 65535 && s.utt[65534].ptr_off == 2 * 65534);
        s = keep;
        const int32_t big[3] = {1 << 30, 1 << 30, 1 << 30}, one[3] = {1, 1, 1};
        CHECK(plan_batch_shape(ctx, 3, big, one, nullptr, 0, &s) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_create: batch too large"));   // rows
        CHECK(plan_batch_shape(ctx, 3, one, big, nullptr, 0, &s) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_create: batch too large"));   // frames
        CHECK(same_shape(s, keep));
    }
}

// the checks of a planned shape against the frame matrix: every utterance one row of the HMM, ranges [begin, begin + T)
static UttOverlap overlap_of(pcl_ctx *ctx, const std::vector<int64_t> &begin, const std::vector<int32_t> &T) {
    const std::vector<int32_t> N(T.size(), 1);
    BatchShape s;
    CHECK(plan_batch_shape(ctx, (int)T.size(), N.data(), T.data(), begin.data(), 1000, &s) == PCL_OK);
    return shape_overlap(s);
}
static bool is_pair(UttOverlap o, int first, int second) { return o.found && o.first == first && o.second == second; }

static void check_ranges(pcl_ctx *ctx) {
    CHECK(!shape_overlap(BatchShape()).found);                                   // empty batch
    CHECK(!overlap_of(ctx, {7}, {5}).found);                                     // one utterance
    CHECK(!overlap_of(ctx, {0, 5, 9}, {5, 4, 1}).found);                         // touching: end == next begin
    CHECK(is_pair(overlap_of(ctx, {0, 4, 9}, {5, 5, 1}), 0, 1));                 // one row shared (row 4)
    CHECK(is_pair(overlap_of(ctx, {0, 5, 9}, {5, 5, 1}), 1, 2));                 // ... further on (row 9)
    CHECK(is_pair(overlap_of(ctx, {3, 3}, {4, 4}), 0, 1));                       // identical ranges
    CHECK(is_pair(overlap_of(ctx, {20, 6, 6}, {2, 9, 1}), 1, 2));                // equal first rows: the lower index is `first`, whatever the lengths
    CHECK(is_pair(overlap_of(ctx, {20, 6, 6}, {2, 1, 9}), 1, 2));
    CHECK(!overlap_of(ctx, {30, 0, 20, 10}, {5, 10, 10, 10}).found);             // not in row order: disjoint ...
    CHECK(is_pair(overlap_of(ctx, {30, 0, 20, 10}, {5, 10, 11, 10}), 2, 0));     // ... and utterance 2 running into utterance 0, a row later
    CHECK(is_pair(overlap_of(ctx, {30, 0, 20, 10}, {5, 11, 11, 10}), 1, 3));     // two overlaps: the one at the lower rows is reported
    CHECK(is_pair(overlap_of(ctx, {0, 2, 5}, {10, 1, 1}), 0, 1));                // an utterance inside another
    {   // a batch made without frames (frame0 = -1): nothing precedes the first utterance
        const int32_t N[2] = {1, 1}, T[2] = {3, 3};
        BatchShape s;
        CHECK(plan_batch_shape(ctx, 2, N, T, nullptr, 0, &s) == PCL_OK);
        CHECK(is_pair(shape_overlap(s), -1, 0));
    }
    {   // the rows the batch refers to against a matrix of F rows
        const int32_t N[2] = {1, 1}, T[2] = {3, 4};
        const int64_t fb[2] = {6, 0};
        BatchShape s;
        CHECK(plan_batch_shape(ctx, 2, N, T, fb, 9, &s) == PCL_OK && s.max_frame_end == 9);
        CHECK(shape_fits_frames(s, 9) && shape_fits_frames(s, 10) && !shape_fits_frames(s, 8) && !shape_fits_frames(s, 0));
        CHECK(shape_fits_frames(BatchShape(), 0));
    }
}

static void check_sparse(pcl_ctx *ctx) {
    const double a = -0.1, b = -0.2, c = -0.3, d = -0.4, e = -0.5;
    BatchShape sh;
    SparseTrans t;
    {   // two 3 x 3 matrices: the first with the skip 0 -> 2, the second without
        const int32_t N[2] = {3, 3}, T[2] = {4, 4};
        CHECK(plan_batch_shape(ctx, 2, N, T, nullptr, 0, &sh) == PCL_OK);
        const VD A = {a, b, c, NINF, d, e, NINF, NINF, NINF, /**/ a, b, NINF, NINF, d, e, NINF, NINF, NINF};
        CHECK(plan_sparse_trans(ctx, "who", sh.utt, dense_trans_rows(sh.utt, A.data()), &t) == PCL_OK);
        CHECK((t.row_ptr == VI{0, 3, 5, 5, /**/ 0, 2, 4, 4}) && (t.col_idx == VI{0, 1, 2, 1, 2, /**/ 0, 1, 1, 2}));
        CHECK((t.csr_val == VD{a, b, c, d, e, /**/ a, b, d, e}));
        CHECK((t.col_ptr == VI{0, 1, 3, 5, /**/ 0, 1, 3, 4}) && (t.row_idx == VI{0, 0, 1, 0, 1, /**/ 0, 0, 1, 1}));
        CHECK((t.csc_val == VD{a, b, d, c, e, /**/ a, b, d, e}));
        CHECK(t.shape.max_outdeg == 3 && t.shape.max_indeg == 2 && !t.shape.left_right && t.shape.nnz == 9);
        CHECK(sh.utt[0].nnz_off == 0 && sh.utt[1].nnz_off == 5 && sh.utt[1].ptr_off == 4);
        // the second alone: left to right
        const int32_t N1[1] = {3};
        CHECK(plan_batch_shape(ctx, 1, N1, T, nullptr, 0, &sh) == PCL_OK);
        CHECK(plan_sparse_trans(ctx, "who", sh.utt, dense_trans_rows(sh.utt, A.data() + 9), &t) == PCL_OK);
        CHECK((t.row_ptr == VI{0, 2, 4, 4}) && (t.col_ptr == VI{0, 1, 3, 4}) && t.shape.max_outdeg == 2 && t.shape.max_indeg == 2 && t.shape.left_right);
        // nothing finite
        const VD none(9, NINF);
        CHECK(plan_sparse_trans(ctx, "who", sh.utt, dense_trans_rows(sh.utt, none.data()), &t) == PCL_OK);
        CHECK(t.shape.nnz == 0 && (t.row_ptr == VI{0, 0, 0, 0}) && (t.col_ptr == VI{0, 0, 0, 0}) && t.col_idx.empty() && t.row_idx.empty() && t.csr_val.empty() &&
              t.csc_val.empty() && t.shape.max_outdeg == 0 && t.shape.max_indeg == 0 && t.shape.left_right);
    }
    // sentence HMMs of labels: the label rows against the dense rows of the expanded matrix
    struct Case { int S, n_units; std::vector<int32_t> len, lab; };
    const Case cases[] = {{5, 2, {3, 1}, {0, 1, 0, 1}}, {3, 1, {1}, {0}}, {3, 1, {1, 1}, {0, 0}}};
    for (const Case &cs : cases) {
        const int S = cs.S, U = (int)cs.len.size();
        VD lt((size_t)cs.n_units * S * S, NINF);                   // unit k: row r goes to r and r + 1; unit 1 also skips a state; the exit row is empty
        for (int k = 0; k < cs.n_units; ++k)
            for (int r = 0; r < S - 1; ++r) {
                if (r > 0) lt[((size_t)k * S + r) * S + r] = -0.25 - k - 0.01 * r;
                lt[((size_t)k * S + r) * S + r + 1] = -0.5 - k - 0.01 * r;
                if (k == 1 && r + 2 < S) lt[((size_t)k * S + r) * S + r + 2] = -3.0 - 0.01 * r;
            }
        LabelPlan lab;
        CHECK(plan_labels(ctx, "who", U, cs.len.data(), cs.lab.data(), S - 2, cs.n_units, &lab) == PCL_OK);
        const std::vector<int32_t> T(U, 2);
        CHECK(plan_batch_shape(ctx, U, lab.N.data(), T.data(), nullptr, 0, &sh) == PCL_OK);
        VD A((size_t)sh.sumNN);
        for (int u = 0; u < U; ++u) embed_dense(cs.lab.data() + lab.label_off[u], cs.len[u], S, lt, A.data() + sh.utt[u].mat_off);
        SparseTrans from_labels, from_dense;
        CHECK(plan_sparse_trans(ctx, "who", sh.utt, label_trans_rows(sh.utt, lab, lt.data(), S), &from_labels) == PCL_OK);
        const VI off_labels = nnz_offs(sh.utt);
        CHECK(plan_sparse_trans(ctx, "who", sh.utt, dense_trans_rows(sh.utt, A.data()), &from_dense) == PCL_OK);
        VI off_naive;
        const SparseTrans naive = naive_sparse(sh.utt, A, &off_naive);
        CHECK(same_sparse(from_labels, from_dense) && same_sparse(from_labels, naive) && off_labels == nnz_offs(sh.utt) && off_labels == off_naive);
        CHECK(from_labels.shape.left_right == (cs.n_units == 1) && from_labels.shape.nnz > 0);
        for (int u = 0; u < U; ++u) {                              // the exit row has no successors
            const int *rp = from_labels.row_ptr.data() + sh.utt[u].ptr_off;
            CHECK(rp[sh.utt[u].N] == rp[sh.utt[u].N - 1]);
        }
        if (U > 1) CHECK(sh.utt[1].ptr_off == sh.utt[0].N + 1 && sh.utt[1].nnz_off == from_labels.row_ptr[sh.utt[0].N] && sh.utt[1].nnz_off > 0);
    }
}

static void check_states(pcl_ctx *ctx) {
    BatchShape sh;
    ScorePlan p;
    {   // J = 4, one emitting row per unit: utterance 0 names unit 1 twice (rows 1 and 3) around unit 3, utterance 1 names unit 1 once; units 0 and 2 have no row
        const int32_t N[2] = {5, 3}, T[2] = {4, 6};
        const int64_t fb[2] = {10, 0};
        CHECK(plan_batch_shape(ctx, 2, N, T, fb, 14, &sh) == PCL_OK);
        const std::vector<int32_t> rs = {PCL_ROW_ENTRY, 1, 3, 1, PCL_ROW_EXIT, /**/ PCL_ROW_ENTRY, 1, PCL_ROW_EXIT};
        CHECK(plan_score(ctx, sh.utt, rs.data(), 4, &p) == PCL_OK);
        // state 1: the scored rows (utterance 0 row 1, utterance 1 row 1), then the copy (utterance 0 row 3); state 3: utterance 0 row 2
        const ScoreSeg want[4] = {{10, 1, 4, 5, 0, 1}, {0, 21, 6, 3, 4, 1}, {10, 3, 4, 5, 10, 1}, {10, 2, 4, 5, 0, 3}};
        CHECK(p.n_segs == 4 && p.segs.size() == 4 && memcmp(p.segs.data(), want, sizeof(want)) == 0);
        const DupRow dup = {1, 3, 4, 5};
        CHECK(p.dups.size() == 1 && memcmp(p.dups.data(), &dup, sizeof(dup)) == 0);
        CHECK((p.seg_of_row == VI{-1, 0, 3, 2, -1, /**/ -1, 1, -1}));
        CHECK((p.work_states == VI{1, 3}) && (p.state_seg_lo == VI{0, 3}) && (p.state_seg_hi == VI{3, 4}) && (p.state_seg_hip == VI{2, 4}));
        CHECK(p.max_state == 3 && p.max_N == 5 && p.row_state == rs);
        CHECK(same_plan(p, naive_plan(sh.utt, rs, 4)));
        const ScorePlan keep = p;
        // the refusals leave the output alone
        std::vector<int32_t> bad = rs;
        bad[6] = 4;
        CHECK(plan_score(ctx, sh.utt, bad.data(), 4, &p) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_set_states: utterance 1 row 1 has state 4 outside [0,4)"));
        CHECK(same_plan(p, keep));
        bad[6] = PCL_ROW_EXIT - 1;
        CHECK(plan_score(ctx, sh.utt, bad.data(), 4, &p) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_set_states: utterance 1 row 1 has state -3 outside [0,4)"));
        CHECK(same_plan(p, keep));
        BatchShape bare;
        CHECK(plan_batch_shape(ctx, 2, N, T, nullptr, 0, &bare) == PCL_OK);
        CHECK(plan_score(ctx, bare.utt, rs.data(), 4, &p) == PCL_ERR_STATE && says(*ctx, "pcl_batch_set_states: batch was created without frame_begin"));
        CHECK(same_plan(p, keep));
        const int32_t N1[1] = {5}, Tbig[1] = {1 << 30};            // three rows of state 2 over 2^30 frames each
        const int64_t fb0[1] = {0};
        BatchShape huge;
        CHECK(plan_batch_shape(ctx, 1, N1, Tbig, fb0, 1ll << 30, &huge) == PCL_OK);
        const std::vector<int32_t> thrice = {PCL_ROW_ENTRY, 2, 2, 2, PCL_ROW_EXIT};
        CHECK(plan_score(ctx, huge.utt, thrice.data(), 4, &p) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_set_states: state 2 has too many frames"));
        CHECK(same_plan(p, keep));
        // a batch of virtual rows only needs no frames
        const std::vector<int32_t> virt = {PCL_ROW_ENTRY, PCL_ROW_ENTRY, PCL_ROW_EXIT, PCL_ROW_EXIT, PCL_ROW_EXIT, /**/ PCL_ROW_ENTRY, PCL_ROW_EXIT, PCL_ROW_EXIT};
        CHECK(plan_score(ctx, bare.utt, virt.data(), 4, &p) == PCL_OK && p.n_segs == 0 && p.work_states.empty() && p.max_state == -1 && p.dups.empty());
    }
    {   // J = 1
        const std::vector<int32_t> rs = {0, 0, PCL_ROW_EXIT, 0, PCL_ROW_EXIT, /**/ PCL_ROW_ENTRY, 0, 0};
        CHECK(plan_score(ctx, sh.utt, rs.data(), 1, &p) == PCL_OK);
        CHECK((p.work_states == VI{0}) && (p.state_seg_lo == VI{0}) && (p.state_seg_hip == VI{2}) && (p.state_seg_hi == VI{5}) && p.dups.size() == 3 && p.max_state == 0);
        CHECK((p.seg_of_row == VI{0, 2, -1, 3, -1, /**/ -1, 1, 4}) && p.segs[4].vstart == 4 + 6 + 4 + 4);
        CHECK(same_plan(p, naive_plan(sh.utt, rs, 1)));
        CHECK(plan_score(ctx, sh.utt, rs.data(), 0, &p) == PCL_ERR_INVALID);
    }
}

static void check_tiles_cases(pcl_ctx *ctx) {
    // nine states of unequal totals: state j has a row in the utterances u >= j of T = (5, 1, 9, 2, 7, 3, 8, 4, 6), and state 4 a second row
    // (a copy: not tiled) in the last
    const int U = 9, J = 9;
    const int32_t T[U] = {5, 1, 9, 2, 7, 3, 8, 4, 6};
    std::vector<int32_t> N(U), rs;
    std::vector<int64_t> fb(U);
    long long F = 0;
    for (int u = 0; u < U; ++u) {
        N[u] = u + 1 + (u == U - 1);
        for (int j = 0; j <= u; ++j) rs.push_back(j);
        if (u == U - 1) rs.push_back(4);
        fb[u] = F;
        F += T[u];
    }
    BatchShape sh;
    ScorePlan p;
    CHECK(plan_batch_shape(ctx, U, N.data(), T, fb.data(), F, &sh) == PCL_OK);
    CHECK(plan_score(ctx, sh.utt, rs.data(), J, &p) == PCL_OK && p.work_states.size() == 9 && p.state_seg_hip[4] + 1 == p.state_seg_hi[4]);
    CHECK(same_plan(p, naive_plan(sh.utt, rs, J)));
    std::vector<size_t> all, some = {7, 2, 3}, none;
    for (size_t k = 0; k < 9; ++k) all.push_back(k);
    for (int tf : {1, 4, 7, 1000}) {                               // 1000: larger than every total, one tile per state
        check_tiles(p, all, tf);
        check_tiles(p, some, tf);
        check_tiles(p, none, tf);
    }
    CHECK(plan_tiles(p, all, 1000).size() == 16 && plan_tiles(p, some, 1000).size() == 8);
    CHECK(plan_tiles(p, all, 1).size() >= 45 + 40 + 39 + 30 + 28 + 21 + 18 + 10 + 6);
    // the first eight states open the eight queues in order; the ninth goes to the least loaded one, state 7's (its 10 frames: 3 tiles of 4)
    const std::vector<ScoreTile> t4 = plan_tiles(p, all, 4);
    for (int x = 0; x < 8; ++x) CHECK(t4[x].state == x && t4[x].vstart == 0 && t4[x].seg0 == p.state_seg_lo[x]);
    CHECK(t4[3 * 8 + 7].state == 8 && t4[3 * 8 + 7].vstart == 0 && t4[4 * 8 + 7].state == 8 && t4[4 * 8 + 7].vstart == 4);
}

static void check_labels(pcl_ctx *ctx) {
    LabelPlan lab;
    const int32_t len[2] = {3, 1}, labels[4] = {2, 0, 2, 0};
    CHECK(plan_labels(ctx, "who", 2, len, labels, 2, 3, &lab) == PCL_OK);              // e = 2
    CHECK((lab.N == std::vector<int32_t>{8, 4}) && (lab.label_off == VI{0, 3, 4}) && lab.label_max == 2 && lab.label_len_max == 3);
    CHECK((lab.row_state == std::vector<int32_t>{PCL_ROW_ENTRY, 4, 5, 0, 1, 4, 5, PCL_ROW_EXIT, /**/ PCL_ROW_ENTRY, 0, 1, PCL_ROW_EXIT}));
    CHECK((lab.occ_ptr == VI{0, 2, 2, 4}) && (lab.occ_utt == VI{0, 1, 0, 0}) && (lab.occ_row0 == VI{3, 1, 1, 5}));
    CHECK(lab.label_len == std::vector<int32_t>(len, len + 2) && lab.labels == std::vector<int32_t>(labels, labels + 4));
    const LabelPlan keep = lab;
    const int32_t empty[2] = {3, 0}, high[4] = {2, 0, 3, 0}, low[4] = {2, 0, 2, -1};
    CHECK(plan_labels(ctx, "who", 2, empty, labels, 2, 3, &lab) == PCL_ERR_INVALID && says(*ctx, "who: utterance 1 has an empty label"));
    CHECK(plan_labels(ctx, "who", 2, len, high, 2, 3, &lab) == PCL_ERR_INVALID && says(*ctx, "who: unit id 3 outside [0,3)"));
    CHECK(plan_labels(ctx, "who", 2, len, low, 2, 3, &lab) == PCL_ERR_INVALID && says(*ctx, "who: unit id -1 outside [0,3)"));
    const int32_t endless[2] = {1 << 30, 1 << 30};                 // 2^31 + 4 rows: refused before a label is read
    CHECK(plan_labels(ctx, "who", 2, endless, labels, 1, 3, &lab) == PCL_ERR_INVALID && says(*ctx, "pcl_batch_create: batch too large"));
    CHECK(same_labels(lab, keep));
}

// a few hundred small random batches through every planner, against the restatements
static void sweep(pcl_ctx *ctx) {
    std::mt19937 rng(20240607);
    auto upto = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    for (int round = 0; round < 400; ++round) {
        const int U = upto(1, 4), J = upto(1, 5);
        std::vector<int32_t> N(U), T(U);
        std::vector<int64_t> fb(U);
        long long F = upto(0, 3);
        for (int u = 0; u < U; ++u) {
            N[u] = upto(1, 9);
            T[u] = upto(1, 7);
            fb[u] = F;
            F += T[u] + upto(0, 2);
        }
        BatchShape sh;
        CHECK(plan_batch_shape(ctx, U, N.data(), T.data(), fb.data(), F, &sh) == PCL_OK);
        CHECK(same_shape(sh, naive_shape(U, N.data(), T.data(), fb.data())));
        // transitions: each entry finite with probability 1/4, 1/2 or 1 (and sometimes none)
        VD A((size_t)sh.sumNN);
        const int dens = upto(0, 3);
        for (double &x : A) x = (dens && upto(1, 4) <= (dens == 3 ? 4 : dens)) ? -0.125 * upto(0, 64) : NINF;
        SparseTrans t;
        VI off;
        CHECK(plan_sparse_trans(ctx, "who", sh.utt, dense_trans_rows(sh.utt, A.data()), &t) == PCL_OK);
        CHECK(same_sparse(t, naive_sparse(sh.utt, A, &off)) && off == nnz_offs(sh.utt));
        // states: virtual rows and a few states, repeated often
        std::vector<int32_t> rs((size_t)sh.sumN);
        for (int32_t &x : rs) x = upto(PCL_ROW_EXIT, J - 1);
        ScorePlan p;
        CHECK(plan_score(ctx, sh.utt, rs.data(), J, &p) == PCL_OK);
        CHECK(same_plan(p, naive_plan(sh.utt, rs, J)));
        std::vector<size_t> which;
        for (size_t k = 0; k < p.work_states.size(); ++k)
            if (upto(0, 2)) which.push_back(k);
        check_tiles(p, which, upto(1, 9));
        // labels: the occurrence lists by a search per unit, the sentence HMMs by the expanded matrices
        const int S = upto(3, 5), e = S - 2, n_units = upto(1, 4);
        std::vector<int32_t> len(U), labels;
        for (int u = 0; u < U; ++u) {
            len[u] = upto(1, 3);
            for (int i = 0; i < len[u]; ++i) labels.push_back(upto(0, n_units - 1));
        }
        LabelPlan lab;
        CHECK(plan_labels(ctx, "who", U, len.data(), labels.data(), e, n_units, &lab) == PCL_OK);
        VI occ_ptr = {0}, occ_utt, occ_row0;
        for (int k = 0; k < n_units; ++k) {
            for (int u = 0, at = 0; u < U; at += len[u], ++u)
                for (int i = 0; i < len[u]; ++i)
                    if (labels[at + i] == k) {
                        occ_utt.push_back(u);
                        occ_row0.push_back(1 + i * e);
                    }
            occ_ptr.push_back((int)occ_utt.size());
        }
        CHECK(lab.occ_ptr == occ_ptr && lab.occ_utt == occ_utt && lab.occ_row0 == occ_row0);
        CHECK(plan_batch_shape(ctx, U, lab.N.data(), T.data(), fb.data(), F, &sh) == PCL_OK && (size_t)sh.sumN == lab.row_state.size());
        for (int u = 0, at = 0; u < U; at += len[u], ++u) {
            CHECK(lab.N[u] == e * len[u] + 2 && lab.label_off[u] == at);
            const int32_t *row = lab.row_state.data() + sh.utt[u].vec_off;
            for (int n = 0; n < lab.N[u]; ++n)
                CHECK(row[n] == (n == 0 ? PCL_ROW_ENTRY : n == lab.N[u] - 1 ? PCL_ROW_EXIT : labels[at + (n - 1) / e] * e + (n - 1) % e));
        }
        VD lt((size_t)n_units * S * S);
        for (double &x : lt) x = upto(0, 2) ? -0.125 * upto(0, 64) : NINF;
        A.assign((size_t)sh.sumNN, 0.0);
        for (int u = 0; u < U; ++u) embed_dense(labels.data() + lab.label_off[u], len[u], S, lt, A.data() + sh.utt[u].mat_off);
        CHECK(plan_sparse_trans(ctx, "who", sh.utt, label_trans_rows(sh.utt, lab, lt.data(), S), &t) == PCL_OK);
        CHECK(same_sparse(t, naive_sparse(sh.utt, A, &off)) && off == nnz_offs(sh.utt));
        CHECK(plan_score(ctx, sh.utt, lab.row_state.data(), n_units * e, &p) == PCL_OK);
        CHECK(same_plan(p, naive_plan(sh.utt, lab.row_state, n_units * e)));
    }
}

int main() {
    static_assert(sizeof(UttDesc) == 48 && sizeof(ScoreSeg) == 32 && sizeof(DupRow) == 24 && sizeof(ScoreTile) == 20, "the descriptors as the kernels read them");
    pcl_ctx ctx;
    check_shape(&ctx);
    check_ranges(&ctx);
    check_sparse(&ctx);
    check_states(&ctx);
    check_tiles_cases(&ctx);
    check_labels(&ctx);
    sweep(&ctx);
    printf("batch_plan_host_check: OK\n");
    return 0;
}
