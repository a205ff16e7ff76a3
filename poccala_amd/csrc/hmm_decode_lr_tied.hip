// hmm_decode_lr_tied.hip -- the TIED = true instantiations of hmm_decode_lr.hip's kernel (emission rows from the lexicon's tied states:
// pcl_batch_decode_tied), with and without the language model, in a translation unit of their own so that the other kernels compile
// exactly as they did alone (see the notes at the kernel).  Defines pcl_decode_lr_launch_tied.
#define PCL_DECLR_TIED 1
#include "hmm_decode_lr.hip"
