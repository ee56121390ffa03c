// ec_patterns_rot_inst.hip -- the rotated single-erasure repair kernels of
// lsec_locate_dev_rotated: the one-row patterned decode with its shard selection rotated per
// stripe (ec_kernels.h, PatternRotArgs).  One unit: a single erasure has one output row.
#define LSEC_INSTANTIATING_PATROT 1
#include "ec_kernels_impl.h"
