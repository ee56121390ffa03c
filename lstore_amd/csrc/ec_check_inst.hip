// ec_check_inst.hip -- explicit instantiation of the parity-check kernels (lsec_check_dev) for
// LSEC_R parity rows.  The Makefile compiles this file once per R (1..8) with -DLSEC_R=<R>, in
// units of their own: the objects of ec_kernels_inst.hip and ec_patterns_inst.hip do not change.
#define LSEC_INSTANTIATING_CHK 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_chk_bytewise<LSEC_R>(const CheckArgs &, hipStream_t, int);
template hipError_t dispatch_chk_bitsliced<LSEC_R>(const CheckArgs &, hipStream_t, int, int);
}  // namespace lsec
