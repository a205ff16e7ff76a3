// What every entry point that walks utterances of the resident frame matrix says once: the checks of a call's (U, T, frame_begin,
// utt_speaker), their upload, the check and upload of a label per frame row, the cut of groups of rows into chunks and its one packed
// list, and the reader of a chunk length from the environment.  Host code only (frame_keyed.h: the keyed pass that ends in a chunk plan).
// Included inside the including file's unnamed namespace, so it includes nothing itself: the including file has pcl_ctx (device,
// F, frames32), DevBuf, pcl_h2d, <algorithm> and <vector> in sight (pcl_internal.h; tests/frame_spans_host_check.cpp brings a stub of its
// own and runs these under the host sanitizers).
#pragma once

// A positive integer from the environment, else the fallback.  Read on EVERY call: tests force several chunks on a small input.
static long long env_positive_ll(const char *name, long long fallback) {
    const char *e = getenv(name);
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? v : fallback;
}

static int frames_loaded_check(pcl_ctx *ctx, const char *who) {
    if (!ctx->frames32 || ctx->F <= 0) PCL_FAIL(ctx, PCL_ERR_STATE, "%s: no frames loaded", who);
    return PCL_OK;
}

// The first of spans_check's three checks, for the caller that has a check of its own between it and the others (frame_lda.hip)
static int spans_args_check(pcl_ctx *ctx, const char *who, int U, const int32_t *T, const int64_t *frame_begin) {
    if (U < 1 || U > 65535 || !T || !frame_begin) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: U = %d utterances (1 .. 65535), or a NULL argument", who, U);
    return PCL_OK;
}

// T / frame_begin of a call: U in range and nothing NULL, every utterance inside the frame matrix, no two of them on one row (utterances
// of no frames lie nowhere).  once_clause ends the overlap message: what the caller does to a frame ONCE.  *Tmax_out = the longest.
static int spans_check(pcl_ctx *ctx, const char *who, const char *once_clause, int U, const int32_t *T, const int64_t *frame_begin, int *Tmax_out) {
    TRY(spans_args_check(ctx, who, U, T, frame_begin));
    std::vector<std::pair<long long, long long>> spans;
    int Tmax = 0;
    for (int u = 0; u < U; ++u) {
        if (T[u] < 0 || frame_begin[u] < 0 || frame_begin[u] + T[u] > ctx->F)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d covers rows [%lld, %lld) of a frame matrix of %lld rows", who, u, (long long)frame_begin[u],
                     (long long)frame_begin[u] + T[u], (long long)ctx->F);
        if (T[u] > 0) spans.emplace_back((long long)frame_begin[u], (long long)frame_begin[u] + T[u]);
        Tmax = std::max(Tmax, (int)T[u]);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); ++i)
        if (spans[i].first < spans[i - 1].second)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: the utterances overlap in the frame matrix at row %lld (%s)", who, spans[i].first, once_clause);
    *Tmax_out = Tmax;
    return PCL_OK;
}

// utt_speaker of a call: every entry -1 (no speaker) or a speaker in [0, S)
static int speakers_check(pcl_ctx *ctx, const char *who, int U, const int32_t *utt_speaker, int S) {
    if (!utt_speaker) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utt_speaker is NULL", who);
    for (int u = 0; u < U; ++u)
        if (utt_speaker[u] < -1 || utt_speaker[u] >= S) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: utterance %d has speaker %d, outside [-1, %d)", who, u, (int)utt_speaker[u], S);
    return PCL_OK;
}

// A call's T, frame_begin and (where the call has speakers) utt_speaker on the device: one pool block each, none for spk without speakers
struct DevSpans {
    DevBuf<int> T, spk;
    DevBuf<long long> begin;
    int upload(pcl_ctx *ctx, int U, const int32_t *T_host, const int64_t *frame_begin, const int32_t *utt_speaker) {
        static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "the lists travel as the caller holds them");
        TRY(T.alloc(ctx, (size_t)U));
        if (utt_speaker) TRY(spk.alloc(ctx, (size_t)U));
        TRY(begin.alloc(ctx, (size_t)U));
        HIPCHK(ctx, pcl_h2d(ctx, T, T_host, (size_t)U * sizeof(int32_t)));
        if (utt_speaker) HIPCHK(ctx, pcl_h2d(ctx, spk, utt_speaker, (size_t)U * sizeof(int32_t)));
        HIPCHK(ctx, pcl_h2d(ctx, begin, frame_begin, (size_t)U * sizeof(int64_t)));
        return PCL_OK;
    }
};

// Groups of rows that follow one another in one virtual order (group g has counts[g] rows), each cut into chunks of at most `chunk`
// rows that never straddle a group: chunk c covers the rows [chunk_v0[c], + chunk_n[c]); group g has the chunks [group_chunk0[g],
// group_chunk0[g + 1]), none when it is empty.  The rows of all groups together number < 2^31 (the callers' frame counts do).
static void plan_chunks(const std::vector<int> &counts, long long chunk, std::vector<int> *group_chunk0, std::vector<int> *chunk_v0, std::vector<int> *chunk_n) {
    group_chunk0->assign(counts.size() + 1, 0);
    chunk_v0->clear();
    chunk_n->clear();
    long long V = 0;
    for (size_t g = 0; g < counts.size(); ++g) {
        for (long long v0 = V; v0 < V + counts[g]; v0 += chunk) {
            chunk_v0->push_back((int)v0);
            chunk_n->push_back((int)std::min(chunk, V + counts[g] - v0));
        }
        V += counts[g];
        (*group_chunk0)[g + 1] = (int)chunk_v0->size();
    }
}

// A chunk plan as ONE list for one upload, behind whatever lists the caller puts in front: [prefix ... | group_chunk0 (groups + 1) |
// chunk_v0 (C) | chunk_n (C)].  group_chunk0 stays on the host as well; the three on the device after upload().
struct ChunkLists {
    std::vector<int> lists, group_chunk0;
    size_t o_chunk0 = 0, o_cv0 = 0, o_cn = 0;
    int C = 0;
    DevBuf<int> d_lists;
    const int *chunk0() const { return d_lists.p + o_chunk0; }
    const int *chunk_v0() const { return d_lists.p + o_cv0; }
    const int *chunk_n() const { return d_lists.p + o_cn; }
    void plan(std::initializer_list<const std::vector<int> *> prefix, const std::vector<int> &counts, long long chunk) {
        std::vector<int> v0, n;
        plan_chunks(counts, chunk, &group_chunk0, &v0, &n);
        C = (int)v0.size();
        lists.clear();
        for (const std::vector<int> *p : prefix) lists.insert(lists.end(), p->begin(), p->end());
        o_chunk0 = lists.size();
        o_cv0 = o_chunk0 + group_chunk0.size();
        o_cn = o_cv0 + C;
        lists.insert(lists.end(), group_chunk0.begin(), group_chunk0.end());
        lists.insert(lists.end(), v0.begin(), v0.end());
        lists.insert(lists.end(), n.begin(), n.end());
    }
    int upload(pcl_ctx *ctx) {
        TRY(d_lists.alloc(ctx, lists.size()));
        HIPCHK(ctx, pcl_h2d(ctx, d_lists, lists.data(), lists.size() * sizeof(int)));
        return PCL_OK;
    }
};

// A caller's label of every row of the frame matrix (`name`, F entries) onto the device: not NULL, frames loaded (F is theirs), every entry
// -1 (the row is not kept) or a `noun` in [0, R); the first offender is the one named.
static int upload_row_labels(pcl_ctx *ctx, const char *who, const char *name, const char *noun, const int32_t *labels, int R, DevBuf<int32_t> *d_out) {
    if (!labels) PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %s is NULL", who, name);
    TRY(frames_loaded_check(ctx, who));
    for (int64_t f = 0; f < ctx->F; ++f)
        if (labels[f] < -1 || labels[f] >= R)
            PCL_FAIL(ctx, PCL_ERR_INVALID, "%s: %s[%lld] = %d is neither -1 nor a %s in [0, %d)", who, name, (long long)f, (int)labels[f], noun, R);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TRY(d_out->alloc(ctx, (size_t)ctx->F));
    HIPCHK(ctx, pcl_h2d(ctx, *d_out, labels, (size_t)ctx->F * sizeof(int32_t)));
    return PCL_OK;
}
