// ec_locate_rot_inst.hip -- explicit instantiation of the locate kernels over the physical devices
// of a rotated LUN (lsec_locate_dev_rotated) for LSEC_R parity rows.  The Makefile compiles this
// file once per R (2..8: one row cannot locate) with -DLSEC_R=<R>, in units of their own: the
// objects of the other *_inst.hip files do not change.
#define LSEC_INSTANTIATING_LOCROT 1
#include "ec_kernels_impl.h"

#ifndef LSEC_R
#error "compile with -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_locrot_bytewise<LSEC_R>(const LocateRotArgs &, hipStream_t, int);
template hipError_t dispatch_locrot_bitsliced<LSEC_R>(const LocateRotArgs &, hipStream_t, int, int);
}  // namespace lsec
