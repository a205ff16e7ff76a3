// hmm_decode_tied.hip -- the TIED = true instantiations of hmm_decode.hip's kernel (emission rows from the lexicon's tied states:
// pcl_batch_decode_tied), with and without the language model, in a translation unit of their own so that the other kernels compile
// exactly as they did alone (see the notes at the kernel).  Defines pcl_decode_general_launch_tied; everything else of hmm_decode.hip
// is left out here.
#define PCL_DEC_TIED 1
#include "hmm_decode.hip"
