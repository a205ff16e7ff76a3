// hmm_decode_dims.inc -- the constants of hmm_decode.hip that the instantiations of hmm_decode_common.h's helpers depend on.  Included
// by the kernel inside its namespace, and by tests/dec_prune_harness.hip, which runs the helpers with the same numbers.
#ifndef PCL_DEC_DW
#define PCL_DEC_DW 1024
#endif
constexpr int DW = PCL_DEC_DW;      // threads per workgroup
constexpr int HB = 8;               // radix digit of the pruning select: 256 bins, the same words as the occupancy map; no direct ranking
