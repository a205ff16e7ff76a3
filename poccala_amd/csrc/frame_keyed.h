// The keyed pass the LDA class statistics (frame_lda.hip) and the decision tree's context statistics (tree_cluster.hip) both begin with:
// a key per kept row, the rows counting-sorted by key (gmm_segment.hip's histogram / scan / stable scatter), every key's rows cut into
// chunks that never straddle a key (group = key; C = 0: no row is kept, nothing uploaded), the plan on the device as one list.  Included
// behind frame_spans.h inside the including file's unnamed namespace, with pcl_internal.h in sight.
#pragma once

// The kernel: key[g] = src[g] for the rows of the U utterances, one thread per (utterance, frame); key was set to -1 (not kept) everywhere
// before.  SPANS (LDA): span[g] = the utterance's rows [lo, hi), and src[g] is (state_class given) the row's owner state, mapped to its
// key here; without SPANS the kernel neither loads nor stores any of that.
template <bool SPANS>
__global__ __launch_bounds__(256) void row_key_kernel(const int *__restrict__ T, const long long *__restrict__ begin, const int *__restrict__ src,
                                                      const int *__restrict__ state_class, int *__restrict__ key, int2 *__restrict__ span) {
    const int u = blockIdx.y, Tu = T[u];
    const long long lo = begin[u];
    for (int t = blockIdx.x * 256 + threadIdx.x; t < Tu; t += gridDim.x * 256) {
        int c = src[lo + t];
        if (SPANS && c >= 0 && state_class) c = state_class[c];
        key[lo + t] = c;
        if (SPANS) span[lo + t] = int2{(int)lo, (int)lo + Tu};
    }
}

struct KeyedRows : ChunkLists {
    DevBuf<int> d_order;                      // the kept rows, key by key, each key's in ascending row order: chunk c = its positions [v0, v0 + n)
    DevBuf<int2> d_span;                      // (SPANS) [row] -> its utterance's rows [lo, hi)
    // d_src (F entries on the device): per row a key in [-1, R), or with d_state_class an owner state mapped through it.  The utterances
    // are validated (Tmax > 0 = their longest), the device is set.  Kernel-time group `timer` ("lda_sort", "tree_sort").
    template <bool SPANS>
    int build(pcl_ctx *ctx, const char *timer, int U, const int32_t *T, const int64_t *frame_begin, int Tmax, const int32_t *d_src, const int32_t *d_state_class, int R,
              long long chunk) {
        DevSpans d;
        DevBuf<int> d_key;
        TRY(d.upload(ctx, U, T, frame_begin, nullptr));
        TRY(d_key.alloc(ctx, (size_t)ctx->F));
        if (SPANS) TRY(d_span.alloc(ctx, (size_t)ctx->F));
        pcl_timer_begin(ctx, timer);
        HIPCHK(ctx, hipMemsetAsync(d_key, 0xff, (size_t)ctx->F * sizeof(int), ctx->stream));
        hipLaunchKernelGGL(row_key_kernel<SPANS>, dim3((unsigned)std::min(64, (Tmax + 255) / 256), (unsigned)U), dim3(256), 0, ctx->stream, d.T.p, d.begin.p, d_src,
                           d_state_class, d_key.p, d_span.p);
        std::vector<int> counts;
        const int rc = pcl_count_sort_device(ctx, ctx->F, R, d_key, &counts, &d_order);
        pcl_timer_end(ctx, timer);
        TRY(rc);
        plan({}, counts, chunk);
        return C == 0 ? PCL_OK : upload(ctx);
    }
};
