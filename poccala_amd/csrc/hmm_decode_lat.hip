// hmm_decode_lat.hip -- the LAT = true instantiations of hmm_decode.hip's kernel (the word lattice's records: pcl_batch_decode_lattice), with
// and without the language model and the tied states, in a translation unit of their own (see the notes at the kernel).  Defines
// pcl_decode_general_launch_lat.
#define PCL_DEC_LAT 1
#include "hmm_decode.hip"
