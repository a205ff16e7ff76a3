// hmm_decode_lr_dims.inc -- the constants of hmm_decode_lr.hip that the instantiations of hmm_decode_common.h's helpers depend on.
// Included by the kernel inside its namespace, and by tests/dec_prune_harness.hip, which runs the helpers with the same numbers.

// 512 threads at 4 waves per SIMD: two workgroups share a CU, so the 417 utterances of a C5 shard run in ONE round of the 256 CUs
// (1024 threads: two rounds, 63 ms against 51; groups of 4 rows spill and lose 9 ms: profiles/r03_decode_c5.txt)
#ifndef PCL_DECLR_DW
#define PCL_DECLR_DW 512
#define PCL_DECLR_WAVES 4
#endif
constexpr int LW = PCL_DECLR_DW;    // threads per workgroup
constexpr int HB = 12, HBINS = 1 << HB;   // radix digit of the pruning select
constexpr int CAND = 1024;          // keys of the selected bin ranked directly
