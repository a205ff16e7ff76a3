// The descriptor stager: the uploads of a batch under construction (pcl_desc_group, pcl_internal.h) are packed into ONE page-locked staging
// buffer and copied by ONE kernel launch on the descriptor stream, with one wait at the end of the group -- pcl_batch_create_labels made 16
// separate synchronous copies from pageable memory (5.3 ms of host time per 1024-utterance batch beside a busy GPU, tools/fresh_batch_probe.py).
// The copy itself is a KERNEL that reads the staging buffer over PCIe, not hipMemcpyAsync: the copy engines serve their queue in order, and
// in a pipeline that also moves frames up and results down the descriptors sat behind the NEXT step's frame upload, which waits for its
// slot's last reader -- 15 ms per pcl_batch_create_labels (bench.py pcie_inclusive_loop).
// Only bookkeeping lives here: the launch and its wait are the caller's `flush` (pcl_desc_launch, pcl_api.hip), the page-locked memory comes
// through PinBuf's Ops -- so that tests/devbuf_host_check.cpp drives every branch below without a device.
#pragma once
#include <string.h>

#include <algorithm>

#include "pcl_own.h"

constexpr int PCL_DESC_MAX = 24;
constexpr size_t PCL_DESC_PIN_MIN = (size_t)16 << 20;   // the staging buffer's size once an array has outgrown it (or twice that array)
// What one launch of desc_copy_kernel copies, passed by value: entry k is `bytes[k]` bytes from offset `off[k]` of the staging buffer to dst[k].
struct DescCopyArgs {
    void *dst[PCL_DESC_MAX];
    unsigned long long off[PCL_DESC_MAX], bytes[PCL_DESC_MAX];
    int n = 0;
};

// flush(const DescCopyArgs &, const char *pin) -> hipError_t: copy the entries and return when they have landed.
template <typename Ops = PinOps, size_t MinCap = PCL_DESC_PIN_MIN>
struct DescStager {
    PinBuf<char, Ops> pin;
    size_t used = 0;             // bytes of `pin` taken by the pending entries
    int group = 0;               // > 0: inside a pcl_desc_group, pcl_h2d_fresh stages and does not wait
    DescCopyArgs pending;        // the staged entries of the open group

    template <typename Flush>
    hipError_t flush(Flush &&fl) {
        used = 0;
        if (pending.n == 0) return hipSuccess;
        const hipError_t e = fl(pending, static_cast<const char *>(pin));
        pending.n = 0;
        return e;
    }
    template <typename Flush>
    hipError_t stage(void *dst, const void *src, size_t bytes, Flush &&fl) {
        if (!bytes) return hipSuccess;
        const size_t need = (bytes + 255) & ~(size_t)255;            // (the copy kernel moves 16 bytes per lane: offsets stay 256-byte aligned)
        if (used + need > pin.cap() || pending.n == PCL_DESC_MAX) {
            hipError_t e = flush(fl);                                // what is staged so far has to land before the buffer is reused
            if (e != hipSuccess) return e;
            if (need > pin.cap() && (e = pin.reserve(std::max(MinCap, need * 2))) != hipSuccess) return e;
        }
        memcpy(pin + used, src, bytes);
        // ONE kernel copies all pending entries side by side: two entries with the same destination would race.  A later upload of an array
        // replaces the earlier one (pcl_batch_create_labels uploads the utterance descriptors twice: before and after the transition
        // offsets are known -- when the first version won, every utterance read utterance 0's transitions: wrong results as soon as the
        // unit matrices differ, tests/test_gpu_sweep.py::test_the_queueing_knobs_do_not_move_a_bit)
#ifndef PCL_DESC_RACE_REPRO                                            // (a build WITH this macro restores the bug: what the sweep tests must catch)
        for (int k = 0; k < pending.n; ++k)
            if (pending.dst[k] == dst) pending.bytes[k] = 0;
#endif
        pending.dst[pending.n] = dst;
        pending.off[pending.n] = used;
        pending.bytes[pending.n] = bytes;
        ++pending.n;
        used += need;
        return hipSuccess;
    }
    // groups nest: the outermost one copies
    void enter() { ++group; }
    template <typename Flush>
    hipError_t leave(Flush &&fl) {
        return --group > 0 ? hipSuccess : flush(fl);
    }
};
