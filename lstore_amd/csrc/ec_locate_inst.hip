// ec_locate_inst.hip -- explicit instantiation of the locate kernels (lsec_locate_dev) for LSEC_R
// parity rows.  The Makefile compiles this file once per R (2..8: one row cannot locate) with
// -DLSEC_R=<R>, in units of their own: the objects of ec_kernels_inst.hip, ec_patterns_inst.hip
// and ec_check_inst.hip do not change.
#define LSEC_INSTANTIATING_LOC 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_loc_bytewise<LSEC_R>(const LocateArgs &, hipStream_t, int);
template hipError_t dispatch_loc_bitsliced<LSEC_R>(const LocateArgs &, hipStream_t, int, int);
}  // namespace lsec
