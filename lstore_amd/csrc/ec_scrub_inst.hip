// ec_scrub_inst.hip -- explicit instantiation of the check and locate kernels (lsec_check_dev,
// lsec_locate_dev and their _rotated forms) for one argument struct and LSEC_R parity rows.  The
// Makefile compiles this file once per (struct, R) with -DLSEC_SCRUB_ARGS=<struct> -DLSEC_R=<R>:
// CheckArgs and CheckRotArgs for R = 1..8, LocateArgs and LocateRotArgs for R = 2..8 (one row cannot
// locate), in units of their own, so the objects of the other *_inst.hip files do not change.
#define LSEC_INSTANTIATING_SCRUB 1
#include "ec_kernels_impl.h"

#if !defined(LSEC_SCRUB_ARGS) || !defined(LSEC_R)
#error "compile with -DLSEC_SCRUB_ARGS=<argument struct> -DLSEC_R=<rows>"
#endif

namespace lsec {
template hipError_t dispatch_scrub_bytewise<LSEC_R, LSEC_SCRUB_ARGS>(const LSEC_SCRUB_ARGS &, hipStream_t, int);
template hipError_t dispatch_scrub_bitsliced<LSEC_R, LSEC_SCRUB_ARGS>(const LSEC_SCRUB_ARGS &, hipStream_t, int, int);
}  // namespace lsec
