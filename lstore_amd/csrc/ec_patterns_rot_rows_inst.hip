// ec_patterns_rot_rows_inst.hip -- the rotated patterned decode for tables of up to LSEC_R erasures per
// pattern: the repair behind lsec_search_dev_patterns_rotated (ec_kernels.h, PatternRotArgs;
// launch_pattern_rot_rows_*).  The Makefile compiles this file once per R = 1..8 with -DLSEC_R=<R>, in
// units of their own.  One row forwards to the single-row unit (ec_patterns_rot_inst.hip), which stays
// the only one to hold those kernels.
#define LSEC_INSTANTIATING_PATROT_ROWS 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_patrot_rows_bytewise<LSEC_R>(const PatternRotArgs &, hipStream_t, int);
template hipError_t dispatch_patrot_rows_bitsliced<LSEC_R>(const PatternRotArgs &, hipStream_t, int);
}  // namespace lsec
