// ec_patterns_search_inst.hip -- explicit instantiation of the search kernels (lsec_search_dev_patterns,
// lsec_search_dev_patterns_rotated): the patterned tile bodies that try a candidate pattern on a stripe
// and sum the magic it would leave, storing nothing, for tables of up to LSEC_R erasures per pattern.
// The Makefile compiles this file once per R = 1..8 with -DLSEC_R=<R>, in units of their own, so the
// objects of the other *_inst.hip files do not change.
#define LSEC_INSTANTIATING_PATSEARCH 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_patsearch_bytewise<LSEC_R, PatternSearchArgs>(const PatternSearchArgs &, hipStream_t, int);
template hipError_t dispatch_patsearch_bitsliced<LSEC_R, PatternSearchArgs>(const PatternSearchArgs &, hipStream_t, int);
template hipError_t dispatch_patsearch_bytewise<LSEC_R, PatternSearchRotArgs>(const PatternSearchRotArgs &, hipStream_t, int);
template hipError_t dispatch_patsearch_bitsliced<LSEC_R, PatternSearchRotArgs>(const PatternSearchRotArgs &, hipStream_t, int);
}  // namespace lsec
