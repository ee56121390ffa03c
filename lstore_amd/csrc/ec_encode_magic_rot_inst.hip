// ec_encode_magic_rot_inst.hip -- explicit instantiation of the rotated encode kernels that also sum
// the stripe magics (lsec_encode_magic_dev_rotated) for LSEC_R parity rows.  The Makefile compiles this
// file once per R = 1..8 with -DLSEC_R=<R>, in units of their own, so the objects of the other
// *_inst.hip files do not change.
#define LSEC_INSTANTIATING_ENCMAGICROT 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_encmagicrot_bytewise<LSEC_R>(const EncodeMagicRotArgs &, hipStream_t, int);
template hipError_t dispatch_encmagicrot_bitsliced<LSEC_R>(const EncodeMagicRotArgs &, hipStream_t, int, int);
}  // namespace lsec
