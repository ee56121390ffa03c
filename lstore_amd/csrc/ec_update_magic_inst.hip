// ec_update_magic_inst.hip -- explicit instantiation of the masked parity-update kernels that also sum
// what the write does to the stripe magics (lsec_update_magic_dev_masked,
// lsec_update_magic_dev_masked_rotated) for LSEC_R parity rows.  The Makefile compiles this file once
// per R = 1..8 with -DLSEC_R=<R>, in units of their own, so the objects of the other *_inst.hip files
// do not change.
#define LSEC_INSTANTIATING_UPDMAGIC 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_updmagic_bytewise<LSEC_R>(const UpdateMaskMagicArgs &, hipStream_t, int);
template hipError_t dispatch_updmagic_bitsliced<LSEC_R>(const UpdateMaskMagicArgs &, hipStream_t, int, int);
}  // namespace lsec
