// hmm_decode_lr_lat.hip -- the LAT = true instantiations of hmm_decode_lr.hip's kernel (the word lattice's records: pcl_batch_decode_lattice),
// with and without the language model and the tied states, in a translation unit of their own so that the other kernels compile exactly as
// they did alone (see the notes at the kernel).  Defines pcl_decode_lr_launch_lat.
#define PCL_DECLR_LAT 1
#include "hmm_decode_lr.hip"
