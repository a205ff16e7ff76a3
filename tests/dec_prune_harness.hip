// dec_prune_harness.hip -- the workgroup-collective helpers of poccala_amd/csrc/hmm_decode_common.h run alone, one workgroup per case,
// so that tests/test_gpu_dec_prune.py can hold them to a sort: pcl_prune_stats, pcl_prune_distinct, pcl_select_kth, pcl_prune_mark
// (the pruning path) and pcl_transfer.  Built by poccala_amd/csrc/Makefile into poccala_amd/libpoccala_dectest.so, beside the library
// and never part of it.
//
// Nothing of the decoders is included.  What the two kernels do AROUND the helpers -- how keys[] is filled, the cut
// m = int(n_old (1 - beam)), which step runs when, which LDS words each step is handed -- is RESTATED here from
// hmm_decode.hip (phase 4) and hmm_decode_lr.hip (phase E).  The harness therefore guards the helpers; the kernels' own copy of the
// glue stays guarded by the decode-level tests (tests/test_gpu_decode.py, tests/test_gpu_decode_lm.py).  The instantiations are the
// shipping ones, with the constants the kernels compile (hmm_decode_dims.inc, hmm_decode_lr_dims.inc).
//
// A case runs TWICE in the same workgroup with no LDS word cleared in between: what a call leaves behind (occupancy map, histogram,
// the candidate counter) is the next frame's input in the kernels, so a stale word shows as a second pass that differs from the first.
#include <stdio.h>

#include "hmm_decode_common.h"         // (poccala_amd/csrc, by -I: tools/dec_prune_mutants.sh puts a changed copy in front)

namespace gen {
#include "hmm_decode_dims.inc"
}
namespace lr {
#include "hmm_decode_lr_dims.inc"
}

namespace {

constexpr int HEAD = 12;            // words of a pass's record, see the kernel's end
static_assert((1 << gen::HB) == 256, "the general kernel's histogram is the occupancy map's 256 words");

struct PruneCase {
    long long off;                  // the case's first token in score / part / gone
    int n, min_distinct;
    double beam;
};

// LDS of the pruning phase as the kernel with this CAND declares it.  CAND = 0 (hmm_decode.hip): one 256-word map is the occupancy
// map and then the radix histogram, the select's words are s_sel and s_i[3].  CAND > 0 (hmm_decode_lr.hip): occ of its own, and the
// pool that holds histogram and candidates.
template <int NT, int KMAX, int HB, int CAND>
__global__ __launch_bounds__(NT) void dectest_prune(const PruneCase *cases, const double *score, const int *part, unsigned long long *head,
                                                    unsigned char *gone_out, long long total) {
    constexpr int NW = NT / 64, HBINS = 1 << HB;
    constexpr bool ONE_MAP = CAND == 0;
    __shared__ __attribute__((aligned(16))) unsigned char pool[ONE_MAP ? 16 : (size_t)HBINS * 4 + (size_t)CAND * 8];
    __shared__ unsigned int occ[256];
    __shared__ int wsum[2][NW], ws_scan[NW];
    __shared__ unsigned long long red_u[2][NW];
    __shared__ int red_i[2][NW];
    __shared__ unsigned long long s_key;
    __shared__ int s_i[4], s_int[4];
    unsigned int *hist = ONE_MAP ? occ : (unsigned int *)pool;
    unsigned long long *cand = ONE_MAP ? nullptr : (unsigned long long *)(pool + (size_t)HBINS * 4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PruneCase pc = cases[blockIdx.x];
    const int n = pc.n;
    const double *sc = score + pc.off;
    const int *pt = part + pc.off;
    // what the kernels do once, before the first frame
    if (tid < 256) occ[tid] = 0u;
    if (!ONE_MAP)
        for (int k = tid; k < HBINS; k += NT) hist[k] = 0u;
    if (tid == 0) s_int[2] = 0;
    __syncthreads();
    const int C = ((n + NT - 1) / NT) * 64, w0 = wave * C;         // this frame's ownership of the old tokens
    for (int pass = 0; pass < 2; ++pass) {
        unsigned long long keys[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int i = w0 + k * 64 + lane;
            keys[k] = (k * 64 < C && i < n && pt[i] != 0) ? pcl_okey(sc[i]) : NOKEY;
        }
        int n_old, bins, ran_distinct = 0;
        unsigned long long kmin, kmax, sel = 0ull;
        int rank = 0;
        unsigned int gone = 0u;
        pcl_prune_stats<NT, KMAX>(keys, occ, wsum[0], red_u[0], red_u[1], n_old, kmin, kmax, bins);
        const int m = (int)((double)n_old * (1.0 - pc.beam));                  // int(width * (1 - beam))
        bool prune = m > 0 && n_old >= pc.min_distinct;
        if (prune && bins < pc.min_distinct) {
            ran_distinct = 1;
            prune = pcl_prune_distinct<NT, KMAX>(keys, pc.min_distinct, red_u[0], red_i[0]);
        }
        if (prune) {
            if constexpr (ONE_MAP) pcl_select_kth<NT, KMAX, HB, 0>(keys, kmin, kmax, m, hist, nullptr, red_i[1], &s_key, &s_i[3], sel, rank);
            else pcl_select_kth<NT, KMAX, HB, CAND>(keys, kmin, kmax, m, hist, cand, ws_scan, &s_key, s_int, sel, rank);
            gone = pcl_prune_mark<NT, KMAX>(keys, sel, rank, wsum[1]);
        }
        __syncthreads();
        // ---- the record: what came out, and what the call left in LDS
        int occ_left = __syncthreads_count(tid < 256 && occ[tid] != 0u), hist_left = 0;
        for (int k0 = 0; k0 < HBINS; k0 += NT) hist_left += __syncthreads_count(k0 + tid < HBINS && hist[k0 + tid] != 0u);
        unsigned char *go = gone_out + (size_t)pass * total + pc.off;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int i = w0 + k * 64 + lane;
            if (k * 64 < C && i < n) go[i] = (unsigned char)((gone >> k) & 1u);
        }
        if (tid == 0) {
            unsigned long long *h = head + ((size_t)blockIdx.x * 2 + pass) * HEAD;
            h[0] = (unsigned long long)n_old;
            h[1] = kmin;
            h[2] = kmax;
            h[3] = (unsigned long long)bins;
            h[4] = (unsigned long long)m;
            h[5] = (unsigned long long)ran_distinct;
            h[6] = prune ? 1ull : 0ull;
            h[7] = sel;
            h[8] = (unsigned long long)(long long)rank;
            h[9] = (unsigned long long)occ_left;
            h[10] = (unsigned long long)hist_left;
            h[11] = ONE_MAP ? 0ull : (unsigned long long)(long long)s_int[2];     // (CAND = 0: the select has no candidate counter)
        }
        __syncthreads();
    }
}

struct TransferCase {
    long long off, out_off;         // into sc / nd / hs / map / taken, and into the output rows
    int n, candidate;
};

// use_map = 0: token i's state sits at i (hmm_decode.hip); 1: at map[i] & 0x7fffffff (hmm_decode_lr.hip: the index list, whose entries
// carry the "fresh" bit)
template <int NT>
__global__ __launch_bounds__(NT) void dectest_transfer(const TransferCase *cases, const double *sc, const int *nd, const int *hs, const int *map,
                                                       int use_map, int *taken, int *out_n, int *out_node, double *out_score, int *out_hist) {
    __shared__ double red_d[NT / 64];
    __shared__ int red_i[NT / 64];
    const TransferCase tc = cases[blockIdx.x];
    const int *srf = map + tc.off;
    int n_out;
    if (use_map)
        n_out = pcl_transfer<NT>(tc.n, tc.candidate, sc + tc.off, nd + tc.off, hs + tc.off, [srf](int i) { return srf[i] & 0x7fffffff; },
                                 taken + tc.off, red_d, red_i, out_node + tc.out_off, out_score + tc.out_off, out_hist + tc.out_off);
    else
        n_out = pcl_transfer<NT>(tc.n, tc.candidate, sc + tc.off, nd + tc.off, hs + tc.off, [](int i) { return i; }, taken + tc.off, red_d,
                                 red_i, out_node + tc.out_off, out_score + tc.out_off, out_hist + tc.out_off);
    if (threadIdx.x == 0) out_n[blockIdx.x] = n_out;
}

#define DT_CHK(call)                                                                                   \
    do {                                                                                               \
        const hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                        \
            fprintf(stderr, "dectest: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__);   \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

// a device copy of a host array that frees itself
template <class T>
struct HostMirror {
    T *p = nullptr;
    ~HostMirror() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t count) { return hipMalloc((void **)&p, (count ? count : 1) * sizeof(T)); }
    hipError_t upload(const T *h, size_t count) {
        const hipError_t e = alloc(count);
        return e != hipSuccess || count == 0 ? e : hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t zero(size_t count) {
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : hipMemset(p, 0, (count ? count : 1) * sizeof(T));
    }
    hipError_t download(T *h, size_t count) const { return count == 0 ? hipSuccess : hipMemcpy(h, p, count * sizeof(T), hipMemcpyDeviceToHost); }
};

template <int NT, int KMAX, int HB, int CAND>
hipError_t launch_prune(int n_cases, const PruneCase *cases, const double *score, const int *part, unsigned long long *head, unsigned char *gone,
                        long long total) {
    hipLaunchKernelGGL((dectest_prune<NT, KMAX, HB, CAND>), dim3(n_cases), dim3(NT), 0, 0, cases, score, part, head, gone, total);
    return hipGetLastError();
}

}  // namespace

#define DECTEST_API extern "C" __attribute__((visibility("default")))

// kind 0: the general kernel's instantiation (kmax 1, 2, 4, 8, 16); 1: the left-to-right kernel's (kmax 8, 16).  Host arrays in, host
// arrays out: case c owns tokens off[c] .. off[c] + n[c] of score / part / gone.  head: [n_cases][2][12] words, gone: [2][total] bytes.
// geometry, if given, receives NT, HB, CAND of the instantiation.  Returns 0, or non-zero with a line on stderr.
DECTEST_API int dectest_prune_run(int kind, int kmax, int n_cases, const int *n, const long long *off, const double *beam, const int *min_distinct,
                                  long long total, const double *score, const int *part, unsigned long long *head, unsigned char *gone,
                                  int *geometry) {
    const int NT = kind == 0 ? gen::DW : lr::LW;
    if (geometry) {
        geometry[0] = NT;
        geometry[1] = kind == 0 ? gen::HB : lr::HB;
        geometry[2] = kind == 0 ? 0 : lr::CAND;
    }
    if (n_cases <= 0 || total < 0) return 2;
    std::vector<PruneCase> pc(n_cases);
    for (int c = 0; c < n_cases; ++c) {
        if (n[c] < 0 || n[c] > kmax * NT || off[c] < 0 || off[c] + n[c] > total) {       // (a lane holds kmax keys: nothing beyond them is read)
            fprintf(stderr, "dectest: case %d: n %d off %lld outside kmax %d x %d threads / %lld tokens\n", c, n[c], off[c], kmax, NT, total);
            return 2;
        }
        pc[c] = PruneCase{off[c], n[c], min_distinct[c], beam[c]};
    }
    HostMirror<PruneCase> d_pc;
    HostMirror<double> d_score;
    HostMirror<int> d_part;
    HostMirror<unsigned long long> d_head;
    HostMirror<unsigned char> d_gone;
    DT_CHK(d_pc.upload(pc.data(), n_cases));
    DT_CHK(d_score.upload(score, total));
    DT_CHK(d_part.upload(part, total));
    DT_CHK(d_head.zero((size_t)n_cases * 2 * HEAD));
    DT_CHK(d_gone.zero((size_t)2 * total));
    hipError_t e = hipErrorInvalidValue;
#define DT_PRUNE(NS, NTC, K, CANDC) e = launch_prune<NS::NTC, K, NS::HB, CANDC>(n_cases, d_pc.p, d_score.p, d_part.p, d_head.p, d_gone.p, total)
    if (kind == 0 && kmax == 1) DT_PRUNE(gen, DW, 1, 0);
    else if (kind == 0 && kmax == 2) DT_PRUNE(gen, DW, 2, 0);
    else if (kind == 0 && kmax == 4) DT_PRUNE(gen, DW, 4, 0);
    else if (kind == 0 && kmax == 8) DT_PRUNE(gen, DW, 8, 0);
    else if (kind == 0 && kmax == 16) DT_PRUNE(gen, DW, 16, 0);
    else if (kind == 1 && kmax == 8) DT_PRUNE(lr, LW, 8, lr::CAND);
    else if (kind == 1 && kmax == 16) DT_PRUNE(lr, LW, 16, lr::CAND);
    else {
        fprintf(stderr, "dectest: no instantiation kind %d kmax %d\n", kind, kmax);
        return 2;
    }
#undef DT_PRUNE
    DT_CHK(e);
    DT_CHK(hipDeviceSynchronize());
    DT_CHK(d_head.download(head, (size_t)n_cases * 2 * HEAD));
    DT_CHK(d_gone.download(gone, (size_t)2 * total));
    return 0;
}

// kind 0: NT of the general kernel, 1: of the left-to-right kernel.  Case c owns off[c] .. off[c] + n[c] of sc / nd / hs / map and
// out_off[c] .. out_off[c] + candidate[c] of the output rows (out_total words each, untouched beyond out_n[c]).
DECTEST_API int dectest_transfer_run(int kind, int use_map, int n_cases, const int *n, const int *candidate, const long long *off,
                                     const long long *out_off, long long total, long long out_total, const double *sc, const int *nd, const int *hs,
                                     const int *map, int *out_n, int *out_node, double *out_score, int *out_hist) {
    if (n_cases <= 0 || total < 0 || out_total < 0) return 2;
    std::vector<TransferCase> tc(n_cases);
    for (int c = 0; c < n_cases; ++c) {
        if (n[c] < 0 || candidate[c] < 0 || off[c] < 0 || off[c] + n[c] > total || out_off[c] < 0 || out_off[c] + candidate[c] > out_total) {
            fprintf(stderr, "dectest: transfer case %d outside its arrays\n", c);
            return 2;
        }
        if (use_map)
            for (int i = 0; i < n[c]; ++i) {
                const int x = map[off[c] + i] & 0x7fffffff;
                if (x >= n[c]) {
                    fprintf(stderr, "dectest: transfer case %d: map entry %d points outside the case\n", c, i);
                    return 2;
                }
            }
        tc[c] = TransferCase{off[c], out_off[c], n[c], candidate[c]};
    }
    HostMirror<TransferCase> d_tc;
    HostMirror<double> d_sc, d_os;
    HostMirror<int> d_nd, d_hs, d_map, d_taken, d_on, d_onode, d_oh;
    DT_CHK(d_tc.upload(tc.data(), n_cases));
    DT_CHK(d_sc.upload(sc, total));
    DT_CHK(d_nd.upload(nd, total));
    DT_CHK(d_hs.upload(hs, total));
    DT_CHK(d_map.upload(map, total));
    DT_CHK(d_taken.zero(total));
    DT_CHK(d_on.zero(n_cases));
    DT_CHK(d_onode.upload(out_node, out_total));                  // (the caller's fill: what a case does not write stays visible)
    DT_CHK(d_os.upload(out_score, out_total));
    DT_CHK(d_oh.upload(out_hist, out_total));
    if (kind == 0)
        hipLaunchKernelGGL((dectest_transfer<gen::DW>), dim3(n_cases), dim3(gen::DW), 0, 0, d_tc.p, d_sc.p, d_nd.p, d_hs.p, d_map.p, use_map,
                           d_taken.p, d_on.p, d_onode.p, d_os.p, d_oh.p);
    else
        hipLaunchKernelGGL((dectest_transfer<lr::LW>), dim3(n_cases), dim3(lr::LW), 0, 0, d_tc.p, d_sc.p, d_nd.p, d_hs.p, d_map.p, use_map,
                           d_taken.p, d_on.p, d_onode.p, d_os.p, d_oh.p);
    DT_CHK(hipGetLastError());
    DT_CHK(hipDeviceSynchronize());
    DT_CHK(d_on.download(out_n, n_cases));
    DT_CHK(d_onode.download(out_node, out_total));
    DT_CHK(d_os.download(out_score, out_total));
    DT_CHK(d_oh.download(out_hist, out_total));
    return 0;
}
