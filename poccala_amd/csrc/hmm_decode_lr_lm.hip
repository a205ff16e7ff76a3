// hmm_decode_lr_lm.hip -- the LM = true instantiations of hmm_decode_lr.hip's kernel (rule D6, the bigram language model at word
// ends: pcl_batch_decode_lm), in a translation unit of their own so that the LM = false kernels compile exactly as they did alone
// (see the note at the kernel).  Defines pcl_decode_lr_launch_lm.
#define PCL_DECLR_LM 1
#include "hmm_decode_lr.hip"
