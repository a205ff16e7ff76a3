// hmm_decode_lm.hip -- the LM = true instantiations of hmm_decode.hip's kernel (rule D6, the bigram language model at word ends:
// pcl_batch_decode_lm), in a translation unit of their own so that the LM = false kernels compile exactly as they did alone (see the
// note at the kernel).  Defines pcl_decode_general_launch_lm; everything else of hmm_decode.hip is left out here.
#define PCL_DEC_LM 1
#include "hmm_decode.hip"
