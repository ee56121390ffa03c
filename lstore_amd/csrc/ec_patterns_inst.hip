// ec_patterns_inst.hip -- explicit instantiation of the per-stripe-pattern decode kernels for
// tables of up to LSEC_R erasures.  The Makefile compiles this file once per R (1..8) with
// -DLSEC_R=<R>, in units of their own: the objects of ec_kernels_inst.hip do not change.
#define LSEC_INSTANTIATING_PAT 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_pat_bytewise<LSEC_R>(const PatternArgs &, hipStream_t, int);
template hipError_t dispatch_pat_bitsliced<LSEC_R>(const PatternArgs &, hipStream_t, int);
}  // namespace lsec
