// ec_patterns_magic_rot_inst.hip -- explicit instantiation of the patterned decode kernels that also sum
// the stripe magics over the devices of a rotated LUN with a logical pattern per stripe
// (lsec_decode_magic_dev_patterns_rotated) for tables of up to LSEC_R erasures per pattern.  The Makefile
// compiles this file once per R = 1..8 with -DLSEC_R=<R>, in units of their own, so the objects of the
// other *_inst.hip files do not change.
#define LSEC_INSTANTIATING_PATMAGICROT 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_patmagicrot_bytewise<LSEC_R>(const PatternMagicRotArgs &, hipStream_t, int);
template hipError_t dispatch_patmagicrot_bitsliced<LSEC_R>(const PatternMagicRotArgs &, hipStream_t, int);
}  // namespace lsec
