// ec_scrub_magic_inst.hip -- explicit instantiation of the check kernels that also sum the stripe
// magics (lsec_check_magic_dev, lsec_check_magic_dev_rotated) for one argument struct and LSEC_R parity
// rows.  The Makefile compiles this file once per (struct, R) with -DLSEC_SCRUB_ARGS=<struct>
// -DLSEC_R=<R>: CheckMagicArgs and CheckMagicRotArgs for R = 1..8, in units of their own, so the
// objects of the other *_inst.hip files do not change.
#define LSEC_INSTANTIATING_CHKMAGIC 1
#include "ec_kernels_impl.h"

#if !defined(LSEC_SCRUB_ARGS) || !defined(LSEC_R)
#error "compile with -DLSEC_SCRUB_ARGS=<argument struct> -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_chkmagic_bytewise<LSEC_R, LSEC_SCRUB_ARGS>(const LSEC_SCRUB_ARGS &, hipStream_t, int);
template hipError_t dispatch_chkmagic_bitsliced<LSEC_R, LSEC_SCRUB_ARGS>(const LSEC_SCRUB_ARGS &, hipStream_t, int, int);
}  // namespace lsec
