// ec_patterns_magic_inst.hip -- explicit instantiation of the patterned decode kernels that also sum
// the stripe magics (lsec_decode_magic_dev_patterns, lsec_decode_magic_dev_rotated) for tables of up to
// LSEC_R erasures per pattern.  The Makefile compiles this file once per R = 1..8 with -DLSEC_R=<R>, in
// units of their own, so the objects of the other *_inst.hip files do not change.
#define LSEC_INSTANTIATING_PATMAGIC 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_patmagic_bytewise<LSEC_R>(const PatternMagicArgs &, hipStream_t, int);
template hipError_t dispatch_patmagic_bitsliced<LSEC_R>(const PatternMagicArgs &, hipStream_t, int);
}  // namespace lsec
