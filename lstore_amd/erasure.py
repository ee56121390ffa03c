"""Python mirror of LStore's erasure plan service (src/lio/erasure_tools.h) over liblstore_ec.so.

``Plan`` owns one ``lio_erasure_plan_t*`` created by the library and exposes

* the reference API one-to-one: ``Plan.generate`` (et_generate_plan), ``Plan.new``
  (et_new_plan), ``form_encoding_matrix`` / ``form_decoding_matrix`` / ``encode_block`` /
  ``decode_block`` called *through the struct's function pointers*, exactly as
  src/lio/segment/jerasure.c:1847 / :245 / :2242-2243 call them, plus the struct fields;
* the batched extensions (``encode_stripes`` / ``decode_stripes``) and the device-resident
  calls (``encode_dev`` / ``decode_dev``) that take torch CUDA tensors or raw shard refs.

Errors mirror the reference: calls that return a status in C raise ``ErasureError`` with
the library's message when the status is non-zero.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import subprocess
from typing import Iterable, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB_PATH = os.path.join(HERE, "liblstore_ec.so")

# method ids -- src/lio/erasure_tools.h:37-45
REED_SOL_VAN, REED_SOL_R6_OP, CAUCHY_ORIG, CAUCHY_GOOD, BLAUM_ROTH, LIBERATION, LIBER8TION, RAID4 = range(8)
JE_METHOD_NAMES = ("reed_sol_van", "reed_sol_r6_op", "cauchy_orig", "cauchy_good", "blaum_roth",
                   "liberation", "liber8tion", "raid4")


class ErasureError(RuntimeError):
    pass


# ----------------------------------------------------------------------------- ABI mirror
class PlanStruct(C.Structure):
    """src/lio/erasure_tools.h:50-65"""


_FORM = C.CFUNCTYPE(C.c_int, C.POINTER(PlanStruct))
_ENC = C.CFUNCTYPE(None, C.POINTER(PlanStruct), C.POINTER(C.c_void_p), C.c_int)
_DEC = C.CFUNCTYPE(C.c_int, C.POINTER(PlanStruct), C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int))

PlanStruct._fields_ = [
    ("strip_size", C.c_longlong),
    ("method", C.c_int),
    ("data_strips", C.c_int),
    ("parity_strips", C.c_int),
    ("w", C.c_int),
    ("packet_size", C.c_int),
    ("base_unit", C.c_int),
    ("encode_matrix", C.POINTER(C.c_int)),
    ("encode_bitmatrix", C.POINTER(C.c_int)),
    ("encode_schedule", C.POINTER(C.POINTER(C.c_int))),
    ("form_encoding_matrix", _FORM),
    ("form_decoding_matrix", _FORM),
    ("encode_block", _ENC),
    ("decode_block", _DEC),
]


class IoVec(C.Structure):
    """struct iovec (sys/uio.h), as lsec_segment_write_iov takes the tbuf's pieces."""
    _fields_ = [("iov_base", C.c_void_p), ("iov_len", C.c_size_t)]


class ShardRef(C.Structure):
    """lsec_shard_t: shard i of stripe s lives at base + s*stride (device memory)."""
    _fields_ = [("base", C.c_void_p), ("stride", C.c_longlong)]


# every function include/lstore_ec.h declares (tests check the .so exports all of them)
EXPORTS = ("nearest_prime", "et_method_type", "et_new_plan", "et_generate_plan", "et_destroy_plan",
           "et_encode", "et_decode", "et_encode_stripes", "et_decode_stripes", "lsec_encode_dev",
           "lsec_decode_dev", "et_encode_stripes_magic", "et_stripes_magic", "lsec_encode_magic_dev",
           "lsec_stripe_magic_dev", "lsec_segment_write", "lsec_segment_write_iov", "lsec_segment_encode_iov",
           "lsec_segment_straddle_bytes", "lsec_segment_read", "lsec_segment_inspect",
           "lsec_prepare_decode", "lsec_abi_version", "lsec_device_count", "lsec_last_error", "lsec_plan_kernel",
           "lsec_set_kernel_variant", "lsec_set_host_devices", "lsec_hbm_copy_dev", "lsec_hbm_mix_dev", "lsec_prepare_encode", "lsec_plan_jit", "lsec_device_numa",
           "lsec_set_tile_sharing", "lsec_tile_sharing", "lsec_host_unpin_drain", "lsec_hbm_decode_shape_dev",
           "lsec_decode_dev_patterns", "lsec_decode_dev_rotated", "lsec_check_dev", "lsec_locate_dev",
           "lsec_check_dev_rotated", "lsec_locate_dev_rotated", "lsec_update_dev",
           "lsec_encode_dev_rotated", "lsec_update_dev_rotated", "lsec_update_dev_masked",
           "lsec_update_dev_masked_rotated", "lsec_update_magic_dev_masked", "lsec_update_magic_dev_masked_rotated",
           "lsec_decode_magic_dev_patterns", "lsec_decode_magic_dev_rotated",
           "lsec_check_magic_dev", "lsec_check_magic_dev_rotated", "lsec_encode_magic_dev_rotated",
           "lsec_search_dev_patterns", "lsec_search_dev_patterns_rotated",
           "lsec_vote_dev", "lsec_vote_dev_rotated",
           "lsec_decode_dev_patterns_rotated", "lsec_decode_magic_dev_patterns_rotated")

# read / inspect flags and stripe states (include/lstore_ec.h)
READ_PARANOID, MAGIC_LEGACY, INSPECT_FIX, MAX_DEVS = 1, 2, 4, 256
# lsec_locate_dev: the two sentinels of located[] and the flag
LOCATE_CLEAN, LOCATE_MANY, LOCATE_REPAIR = 0xFF, 0xFE, 1
# lsec_search_dev_patterns: the flag (found[] takes the two sentinels of located[])
SEARCH_REPAIR = 1
# lsec_vote_dev: the classes of cls[] and the flag (ids[] takes the two sentinels of located[])
VOTE_OK, VOTE_DEGRADED, VOTE_BLANK, VOTE_LOST = range(4)
VOTE_PARANOID = 1
# lsec_check_magic_dev: the bits of bad[]
SCRUB_BAD_PARITY, SCRUB_BAD_MAGIC = 1, 2
# lsec_update_dev: the flag
UPDATE_STORE = 1
STRIPE_OK, STRIPE_EMPTY, STRIPE_BAD_MAGIC, STRIPE_REPAIRED, STRIPE_LOST_MAGIC, STRIPE_LOST_MISMATCH = range(6)


class InspectState(C.Structure):
    """lsec_inspect_state_t: counters + the carried brute-force guess of one inspection."""
    _fields_ = [("bad_stripes", C.c_longlong), ("unrecoverable", C.c_longlong), ("silent_errors", C.c_longlong),
                ("empty_stripes", C.c_longlong), ("brute_used", C.c_int),
                ("brute_badmap", C.c_ubyte * MAX_DEVS)]

_lib = None


def library_path() -> str:
    return _LIB_PATH


def build_library(force: bool = False) -> str:
    """Compile liblstore_ec.so for gfx950 in-tree (hipcc)."""
    if force or not os.path.exists(_LIB_PATH):
        jobs = str(min(8, os.cpu_count() or 1))
        subprocess.run(["make", "-s", "-j", jobs, "-C", os.path.join(HERE, "csrc")], check=True)
    return _LIB_PATH


def lib():
    """Load liblstore_ec.so.  There is no fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ErasureError(f"{_LIB_PATH} is not built; run lstore_amd.build_library() "
                           "(or `make -C lstore_amd/csrc`)")
    L = C.CDLL(_LIB_PATH)
    P = C.POINTER(PlanStruct)
    L.et_generate_plan.restype = P
    L.et_generate_plan.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.et_new_plan.restype = P
    L.et_new_plan.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.et_destroy_plan.argtypes = [P]
    L.et_destroy_plan.restype = None
    L.et_method_type.argtypes = [C.c_char_p]
    L.nearest_prime.argtypes = [C.c_int, C.c_int]
    L.et_encode.argtypes = [P, C.c_char_p, C.c_longlong, C.c_char_p, C.c_longlong, C.c_int]
    L.et_decode.argtypes = [P, C.c_longlong, C.c_char_p, C.c_longlong, C.c_char_p, C.c_longlong, C.c_int,
                            C.POINTER(C.c_int)]
    L.et_encode_stripes.argtypes = [P, C.POINTER(C.c_void_p), C.c_int, C.c_int]
    L.et_decode_stripes.argtypes = [P, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.lsec_encode_dev.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_void_p]
    L.lsec_decode_dev.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.POINTER(C.c_int), C.c_void_p]
    L.lsec_decode_dev_patterns.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.POINTER(C.c_int), C.c_int,
                                           C.c_void_p, C.c_void_p]
    L.lsec_decode_dev_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.POINTER(C.c_int), C.c_int,
                                          C.c_longlong, C.c_void_p]
    L.lsec_check_dev.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lsec_locate_dev.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_void_p]
    L.lsec_check_dev_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    L.lsec_locate_dev_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.lsec_update_dev.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.POINTER(C.c_int), C.POINTER(ShardRef),
                                  C.c_int, C.c_void_p]
    L.lsec_encode_dev_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p]
    L.lsec_update_dev_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong,
                                          C.POINTER(C.c_int), C.POINTER(ShardRef), C.c_int, C.c_void_p]
    L.lsec_update_dev_masked.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_void_p, C.POINTER(ShardRef),
                                         C.c_int, C.c_void_p]
    L.lsec_update_dev_masked_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong,
                                                 C.c_void_p, C.POINTER(ShardRef), C.c_int, C.c_void_p]
    L.lsec_update_magic_dev_masked.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_void_p, C.POINTER(ShardRef),
                                               C.c_int, C.c_void_p, C.c_void_p]
    L.lsec_update_magic_dev_masked_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong,
                                                       C.c_void_p, C.POINTER(ShardRef), C.c_int, C.c_void_p, C.c_void_p]
    L.lsec_decode_magic_dev_patterns.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.POINTER(C.c_int), C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lsec_decode_magic_dev_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.POINTER(C.c_int), C.c_int,
                                                C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lsec_decode_dev_patterns_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong,
                                                   C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p]
    L.lsec_decode_magic_dev_patterns_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong,
                                                         C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]
    L.lsec_test_predict_pattern_magic_rot_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.lsec_search_dev_patterns.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.POINTER(C.c_int), C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.lsec_search_dev_patterns_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong,
                                                   C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.lsec_test_predict_search_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.lsec_test_set_search_form.argtypes = [C.c_int, C.c_int]
    L.lsec_test_set_search_form.restype = None
    L.lsec_vote_dev.argtypes = [P, C.POINTER(ShardRef), C.POINTER(ShardRef), C.c_int, C.c_longlong, C.POINTER(C.c_int), C.c_int,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.lsec_vote_dev_rotated.argtypes = [P, C.POINTER(ShardRef), C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int,
                                        C.c_longlong, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.lsec_test_set_vote_form.argtypes = [C.c_int, C.c_int]
    L.lsec_test_set_vote_form.restype = None
    L.lsec_check_magic_dev.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
    L.lsec_check_magic_dev_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.lsec_test_predict_check_magic_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                                     C.POINTER(C.c_int)]
    L.lsec_encode_magic_dev_rotated.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_int, C.c_longlong,
                                                C.c_void_p, C.c_void_p]
    L.lsec_test_predict_encode_magic_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_int)]
    L.lsec_test_predict_pattern_magic_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.lsec_test_pattern_unused.argtypes = [P, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lsec_test_predict_masked_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_int)]
    L.lsec_test_predict_masked_magic_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_int)]
    L.lsec_test_locate_ratio.argtypes = [P, C.c_int, C.c_int]
    L.lsec_test_plan_images.argtypes = [P]
    L.lsec_test_set_pattern_split.argtypes = [C.c_int]
    L.lsec_test_set_pattern_split.restype = None
    L.lsec_test_pattern_table.argtypes = [P, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lsec_test_pattern_rot0.argtypes = [C.c_int, C.c_int, C.c_longlong]
    L.lsec_test_launch_record.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.lsec_test_predict_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_int)]
    L.lsec_test_fixed_k.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.lsec_test_apply_record.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.lsec_test_predict_apply.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                          C.c_char_p, C.POINTER(C.c_int), C.c_int]
    L.lsec_test_predict_apply_launch.argtypes = [C.c_int] * 11 + [C.POINTER(C.c_int)]
    L.lsec_test_predict_apply_plan.argtypes = [P, C.POINTER(C.c_int), C.c_longlong, C.c_int, C.POINTER(C.c_int), C.c_int]
    L.lsec_test_hold_networks.argtypes = [C.c_int]
    L.lsec_test_hold_networks.restype = None
    L.lsec_prepare_decode.argtypes = [P, C.POINTER(C.c_int)]
    L.lsec_prepare_encode.argtypes = [P]
    L.lsec_plan_jit.argtypes = [P, C.POINTER(C.c_int)]
    L.et_encode_stripes_magic.argtypes = [P, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p]
    L.et_stripes_magic.argtypes = [P, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p]
    L.lsec_encode_magic_dev.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    L.lsec_stripe_magic_dev.argtypes = [P, C.POINTER(ShardRef), C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    L.lsec_segment_write.argtypes = [P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    L.lsec_segment_write_iov.argtypes = [P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    L.lsec_segment_encode_iov.argtypes = [P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_longlong, C.c_void_p, C.c_int]
    L.lsec_segment_straddle_bytes.restype = C.c_longlong
    L.lsec_segment_straddle_bytes.argtypes = [P, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.lsec_segment_read.argtypes = [P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p,
                                    C.c_void_p]
    L.lsec_segment_inspect.argtypes = [P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(InspectState)]
    L.lsec_last_error.restype = C.c_char_p
    L.lsec_plan_kernel.argtypes = [P]
    L.lsec_set_kernel_variant.argtypes = [C.c_int, C.c_int]
    L.lsec_set_kernel_variant.restype = None
    L.lsec_set_tile_sharing.argtypes = [C.c_int]
    L.lsec_set_tile_sharing.restype = None
    L.lsec_tile_sharing.restype = C.c_int
    L.lsec_host_unpin_drain.argtypes = []
    L.lsec_host_unpin_drain.restype = C.c_int
    L.lsec_set_host_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.lsec_hbm_copy_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_void_p]
    L.lsec_hbm_mix_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p]
    L.lsec_hbm_decode_shape_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p]
    L.lsec_device_numa.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    L.lsec_test_numa_for_bus.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    L.lsec_test_server_hold.restype = C.c_longlong
    L.lsec_test_server_hold.argtypes = [C.c_int, C.c_int]
    _lib = L
    return L


def last_error() -> str:
    return (lib().lsec_last_error() or b"").decode()


def _check(rc: int, what: str) -> int:
    if rc != 0:
        raise ErasureError(f"{what} failed (rc={rc}): {last_error()}")
    return rc


def _erasure_array(erasures: Iterable[int]):
    vals = list(erasures) + [-1]
    return (C.c_int * len(vals))(*vals)


def _pattern_array(patterns):
    """erasure lists back to back, each -1 terminated (lsec_decode_dev_patterns)"""
    vals = []
    for pat in patterns:
        vals += [int(x) for x in pat] + [-1]
    return (C.c_int * max(1, len(vals)))(*vals)


def nearest_prime(w: int, which: int) -> int:
    return lib().nearest_prime(w, which)


def method_type(name: str) -> int:
    return lib().et_method_type(name.encode())


# ----------------------------------------------------------------------------- plan
class Plan:
    """One lio_erasure_plan_t owned by liblstore_ec.so."""

    def __init__(self, ptr):
        if not ptr:
            raise ErasureError(f"plan creation failed: {last_error()}")
        self._p = ptr

    # -- constructors (et_generate_plan / et_new_plan)
    @classmethod
    def generate(cls, file_size, method, k, m, w=-1, packet_low=-1, packet_high=-1) -> "Plan":
        return cls(lib().et_generate_plan(file_size, method, k, m, w, packet_low, packet_high))

    @classmethod
    def new(cls, method, strip_size, k, m, w, packet_size, base_unit=8) -> "Plan":
        return cls(lib().et_new_plan(method, strip_size, k, m, w, packet_size, base_unit))

    @classmethod
    def for_chunk(cls, method, k, m, chunk, w=-1) -> "Plan":
        """The plan segment/jerasure.c:2236-2243 builds: et_generate_plan(k*C, ...) + form_*."""
        p = cls.generate(k * chunk, method, k, m, w)
        p.form_encoding_matrix()
        p.form_decoding_matrix()
        return p

    def close(self):
        if getattr(self, "_p", None):
            lib().et_destroy_plan(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- struct fields
    @property
    def ptr(self):
        return self._p

    @property
    def s(self) -> PlanStruct:
        return self._p.contents

    k = property(lambda self: self.s.data_strips)
    m = property(lambda self: self.s.parity_strips)
    w = property(lambda self: self.s.w)
    method = property(lambda self: self.s.method)
    packet_size = property(lambda self: self.s.packet_size)
    strip_size = property(lambda self: self.s.strip_size)
    base_unit = property(lambda self: self.s.base_unit)

    @property
    def kernel(self) -> int:
        """1 = bytewise GF(2^8), 2 = bitsliced GF(2^8) (Cauchy), 3 = GF(2) bitmatrix (liberation
        family), 4 = wordwise GF(2^16/2^32) (RS), 5 = bitsliced GF(2^16/2^32) (Cauchy at
        w = 16/32), 0 = no GPU kernel"""
        return lib().lsec_plan_kernel(self._p)

    def matrix(self):
        if not self.s.encode_matrix:
            return None
        rows = 2 if self.method == REED_SOL_R6_OP else self.m
        n = rows * self.k
        return np.ctypeslib.as_array(self.s.encode_matrix, shape=(n,)).copy().reshape(rows, self.k)

    def bitmatrix(self):
        if not self.s.encode_bitmatrix:
            return None
        n = self.k * self.m * self.w * self.w
        return np.ctypeslib.as_array(self.s.encode_bitmatrix, shape=(n,)).copy().reshape(self.m * self.w, -1)

    def schedule(self):
        if not self.s.encode_schedule:
            return None
        ops, i = [], 0
        while True:
            row = self.s.encode_schedule[i]
            if row[0] == -1:
                break
            ops.append([row[x] for x in range(5)])
            i += 1
        return np.array(ops, dtype=np.int32).reshape(-1, 5)

    # -- fn-pointer calls (what the segment driver does)
    def form_encoding_matrix(self) -> int:
        return self.s.form_encoding_matrix(self._p)

    def form_decoding_matrix(self) -> int:
        return self.s.form_decoding_matrix(self._p)

    @staticmethod
    def _ptr_array(addrs: Sequence[int]):
        return (C.c_void_p * len(addrs))(*addrs)

    def encode_block(self, shards: Sequence[np.ndarray] | Sequence[int], block_size: int | None = None):
        """plan->encode_block(plan, ptr, C); shards = k+m host arrays (or raw addresses)."""
        addrs = [s if isinstance(s, int) else s.ctypes.data for s in shards]
        if block_size is None:
            block_size = shards[0].nbytes
        self.s.encode_block(self._p, self._ptr_array(addrs), block_size)

    def decode_block(self, shards, erasures: Iterable[int], block_size: int | None = None) -> int:
        """plan->decode_block(...) -> rc (0 / -1), like the reference (no exception)."""
        addrs = [s if isinstance(s, int) else s.ctypes.data for s in shards]
        if block_size is None:
            block_size = shards[0].nbytes
        return self.s.decode_block(self._p, self._ptr_array(addrs), block_size, _erasure_array(erasures))

    # -- batched host calls
    def _stripe_ptrs(self, stripes: np.ndarray):
        n, km, size = stripes.shape
        assert km == self.k + self.m and stripes.dtype == np.uint8 and stripes.flags.c_contiguous
        base = stripes.ctypes.data
        addrs = [base + (s * km + i) * size for s in range(n) for i in range(km)]
        return self._ptr_array(addrs), n, size

    def encode_stripes(self, stripes: np.ndarray) -> None:
        """stripes: uint8 [N, k+m, C] host array; parity rows are overwritten."""
        arr, n, size = self._stripe_ptrs(stripes)
        _check(lib().et_encode_stripes(self._p, arr, n, size), "et_encode_stripes")

    def decode_stripes(self, stripes: np.ndarray, erasures: Iterable[int]) -> None:
        arr, n, size = self._stripe_ptrs(stripes)
        _check(lib().et_decode_stripes(self._p, arr, n, size, _erasure_array(erasures)), "et_decode_stripes")

    def encode_stripes_ptrs(self, ptr_array, nstripes: int, block_size: int) -> None:
        _check(lib().et_encode_stripes(self._p, ptr_array, nstripes, block_size), "et_encode_stripes")

    def decode_stripes_ptrs(self, ptr_array, nstripes: int, block_size: int, erasures) -> None:
        _check(lib().et_decode_stripes(self._p, ptr_array, nstripes, block_size, _erasure_array(erasures)),
               "et_decode_stripes")

    # -- stripe magic (je_cksum_calc, segment/jerasure.c:169-182)
    def encode_stripes_magic(self, stripes: np.ndarray) -> np.ndarray:
        """Encode + per-stripe 4-byte adler32 magic over all k+m chunks; returns uint8 [N, 4]."""
        arr, n, size = self._stripe_ptrs(stripes)
        magic = np.zeros((n, 4), dtype=np.uint8)
        _check(lib().et_encode_stripes_magic(self._p, arr, n, size, magic.ctypes.data), "et_encode_stripes_magic")
        return magic

    def stripes_magic(self, stripes: np.ndarray) -> np.ndarray:
        arr, n, size = self._stripe_ptrs(stripes)
        magic = np.zeros((n, 4), dtype=np.uint8)
        _check(lib().et_stripes_magic(self._p, arr, n, size, magic.ctypes.data), "et_stripes_magic")
        return magic

    def encode_magic_dev_refs(self, refs, nstripes: int, block_size: int, magic_ptr: int, stream: int = 0) -> None:
        """lsec_encode_magic_dev over raw shard refs; magic_ptr: device address of 4*nstripes bytes."""
        _check(lib().lsec_encode_magic_dev(self._p, self.shard_refs(refs), nstripes, block_size, magic_ptr, stream),
               "lsec_encode_magic_dev")

    def stripe_magic_dev_refs(self, refs, nstripes: int, block_size: int, magic_ptr: int, stream: int = 0) -> None:
        """lsec_stripe_magic_dev over raw shard refs: the magic of the k+m chunks as they are."""
        _check(lib().lsec_stripe_magic_dev(self._p, self.shard_refs(refs), nstripes, block_size, magic_ptr, stream),
               "lsec_stripe_magic_dev")

    def encode_magic_dev(self, data, parity, magic, stream=None) -> None:
        """torch: encode + magic (uint8 [N,4] device tensor)."""
        refs, n, size = self.tensor_refs(data, parity)
        self.encode_magic_dev_refs(refs, n, size, magic.data_ptr(), _stream_handle(stream))

    def stripe_magic_dev(self, data, parity, magic, stream=None) -> None:
        refs, n, size = self.tensor_refs(data, parity)
        self.stripe_magic_dev_refs(refs, n, size, magic.data_ptr(), _stream_handle(stream))

    # -- segment adapter (segjerase_write_func + LUN placement)
    def segment_write(self, data: np.ndarray, n_shift: int = 1, first_stripe: int = 0,
                      out: "np.ndarray | None" = None) -> np.ndarray:
        """data uint8 [N, k, C] -> device images uint8 [k+m, N*(C+4)] (lsec_segment_write), written
        into `out` when given (the depots' buffers, reused across calls)."""
        n_str, k, size = data.shape
        n = self.k + self.m
        data = np.ascontiguousarray(data)
        dev = out if out is not None else np.zeros((n, n_str * (size + 4)), dtype=np.uint8)
        assert dev.shape == (n, n_str * (size + 4)) and dev.dtype == np.uint8 and dev.flags.c_contiguous
        ptrs = self._ptr_array([dev[i].ctypes.data for i in range(n)])
        _check(lib().lsec_segment_write(self._p, data.ctypes.data, n_str, size, n_shift, first_stripe, ptrs),
               "lsec_segment_write")
        return dev

    def segment_write_iov(self, pieces, nstripes: int, chunk: int, n_shift: int = 1,
                          first_stripe: int = 0) -> np.ndarray:
        """pieces: the user data as a scatter list of uint8 arrays, or ints for error pages of that
        many bytes -> device images uint8 [k+m, N*(C+4)] (lsec_segment_write_iov)."""
        n = self.k + self.m
        iov = (IoVec * max(1, len(pieces)))()
        keep = []
        for i, pc in enumerate(pieces):
            if isinstance(pc, (int, np.integer)):
                iov[i].iov_base, iov[i].iov_len = None, int(pc)
            else:
                pc = np.ascontiguousarray(pc, dtype=np.uint8)
                keep.append(pc)
                iov[i].iov_base, iov[i].iov_len = pc.ctypes.data, pc.nbytes
        dev = np.zeros((n, nstripes * (chunk + 4)), dtype=np.uint8)
        ptrs = self._ptr_array([dev[i].ctypes.data for i in range(n)])
        _check(lib().lsec_segment_write_iov(self._p, iov, len(pieces), nstripes, chunk, n_shift, first_stripe, ptrs),
               "lsec_segment_write_iov")
        return dev

    @staticmethod
    def _iov_array(pieces):
        iov = (IoVec * max(1, len(pieces)))()
        keep = []
        for i, pc in enumerate(pieces):
            if isinstance(pc, (int, np.integer)):
                iov[i].iov_base, iov[i].iov_len = None, int(pc)
            else:
                pc = np.ascontiguousarray(pc, dtype=np.uint8)
                keep.append(pc)
                iov[i].iov_base, iov[i].iov_len = pc.ctypes.data, pc.nbytes
        return iov, keep

    def segment_encode_iov(self, pieces, nstripes: int, chunk: int, parity: "np.ndarray | None" = None,
                           magic: "np.ndarray | None" = None):
        """segjerase_write_func's hand-off with no data copy (lsec_segment_encode_iov): pieces as for
        segment_write_iov.  Returns (iovs, parity uint8 [N, m, C], magic uint8 [N, 4], keep): iovs
        is a uint64 [2(k+m)N, 2] view of the iovecs [magic | chunk] in logical order (rows of address,
        length); `keep` holds what they point into (the pieces' arrays, the straddle buffer) and
        the iovec array itself."""
        n = self.k + self.m
        iov, keep = self._iov_array(pieces)
        par = parity if parity is not None else np.empty((nstripes, self.m, chunk), np.uint8)
        mag = magic if magic is not None else np.empty((nstripes, 4), np.uint8)
        assert par.nbytes >= nstripes * self.m * chunk and mag.nbytes >= nstripes * 4
        sb = lib().lsec_segment_straddle_bytes(self._p, iov, len(pieces), nstripes, chunk)
        if sb < 0:
            raise ErasureError(f"lsec_segment_straddle_bytes failed: {last_error()}")
        straddle = np.empty(max(1, sb), np.uint8)
        out = (IoVec * max(1, 2 * n * nstripes))()
        got = lib().lsec_segment_encode_iov(self._p, iov, len(pieces), nstripes, chunk, par.ctypes.data, mag.ctypes.data,
                                            straddle.ctypes.data, sb, out, 2 * n * nstripes)
        if got != 2 * n * nstripes:
            raise ErasureError(f"lsec_segment_encode_iov failed (rc={got}): {last_error()}")
        iovs = np.frombuffer(out, dtype=np.uint64).reshape(-1, 2)[:got]  # rows (address, length), no copy
        return iovs, par, mag, keep + [straddle, out]

    def segment_read(self, dev: np.ndarray, nstripes: int, chunk: int, n_shift: int = 1, first_stripe: int = 0,
                     paranoid: bool = False, missing=(), legacy_magic: bool = False):
        """device images uint8 [k+m, N*(C+4)] -> (data uint8 [N, k, C], status int32 [N], n_unrecoverable)."""
        n = self.k + self.m
        addrs = [0 if i in missing else dev[i].ctypes.data for i in range(n)]
        data = np.zeros((nstripes, self.k, chunk), dtype=np.uint8)
        status = np.zeros(nstripes, dtype=np.int32)
        flags = (READ_PARANOID if paranoid else 0) | (MAGIC_LEGACY if legacy_magic else 0)
        bad = lib().lsec_segment_read(self._p, self._ptr_array(addrs), nstripes, chunk, n_shift, first_stripe,
                                      flags, data.ctypes.data, status.ctypes.data)
        if bad < 0:
            raise ErasureError(f"lsec_segment_read failed: {last_error()}")
        return data, status, bad

    def segment_inspect(self, buf: np.ndarray, chunk: int, fix: bool = False, legacy_magic: bool = False,
                        state: "InspectState | None" = None):
        """lsec_segment_inspect over buf uint8 [N, k+m, C+4] (stripe-major [magic | chunk] records,
        repaired in place with fix=True) -> (status int32 [N], badmap uint8 [N, k+m],
        rewrite uint8 [N, k+m], state)."""
        n = self.k + self.m
        if buf.ndim != 3 or buf.shape[1] != n or buf.shape[2] != chunk + 4 or not buf.flags.c_contiguous:
            raise ValueError("buf must be a contiguous uint8 [N, k+m, C+4] array")
        nstr = buf.shape[0]
        status = np.zeros(nstr, np.int32)
        badmap = np.zeros((nstr, n), np.uint8)
        rewrite = np.zeros((nstr, n), np.uint8)
        state = InspectState() if state is None else state
        flags = (INSPECT_FIX if fix else 0) | (MAGIC_LEGACY if legacy_magic else 0)
        _check(lib().lsec_segment_inspect(self._p, buf.ctypes.data, nstr, chunk, flags, status.ctypes.data,
                                          badmap.ctypes.data, rewrite.ctypes.data, C.byref(state)),
               "lsec_segment_inspect")
        return status, badmap, rewrite, state

    # -- device-resident calls
    @staticmethod
    def shard_refs(refs: Sequence[tuple[int, int]]):
        arr = (ShardRef * len(refs))()
        for i, (base, stride) in enumerate(refs):
            arr[i].base = base
            arr[i].stride = stride
        return arr

    def tensor_refs(self, data, parity):
        """Shard refs for torch uint8 tensors data [N,k,C] and parity [N,m,C] (contiguous rows)."""
        size = data.shape[-1]
        refs = [(data.data_ptr() + j * data.stride(1), data.stride(0)) for j in range(self.k)]
        refs += [(parity.data_ptr() + i * parity.stride(1), parity.stride(0)) for i in range(parity.shape[1])]
        return refs, data.shape[0], size

    def encode_dev_refs(self, refs, nstripes: int, block_size: int, stream: int = 0) -> None:
        _check(lib().lsec_encode_dev(self._p, self.shard_refs(refs), nstripes, block_size, stream),
               "lsec_encode_dev")

    def decode_dev_refs(self, refs, nstripes: int, block_size: int, erasures, stream: int = 0) -> None:
        _check(lib().lsec_decode_dev(self._p, self.shard_refs(refs), nstripes, block_size,
                                     _erasure_array(erasures), stream), "lsec_decode_dev")

    def encode_dev(self, data, parity, stream=None) -> None:
        """torch: data uint8 [N,k,C], parity uint8 [N,m,C] on the current device."""
        refs, n, size = self.tensor_refs(data, parity)
        self.encode_dev_refs(refs, n, size, _stream_handle(stream))

    def decode_dev(self, data, parity, erasures, stream=None, out=None) -> None:
        """Rebuild erased shards of data/parity in place, or into ``out`` [N, e, C] (erased order)."""
        refs, n, size = self.tensor_refs(data, parity)
        if out is not None:
            for r, e in enumerate(sorted(set(erasures))):
                refs[e] = (out.data_ptr() + r * out.stride(1), out.stride(0))
        self.decode_dev_refs(refs, n, size, erasures, _stream_handle(stream))

    def decode_dev_patterns_refs(self, refs, nstripes: int, block_size: int, patterns, stripe_pattern_ptr: int,
                                 stream: int = 0) -> None:
        """lsec_decode_dev_patterns: stripes that do not share an erasure pattern, one launch.
        patterns: a sequence of erasure lists; stripe_pattern_ptr: device address of nstripes bytes,
        each stripe's index into patterns (0 / None with nstripes == 0: only prepare the tables)."""
        patterns = list(patterns)
        _check(lib().lsec_decode_dev_patterns(self._p, self.shard_refs(refs), nstripes, block_size,
                                              _pattern_array(patterns), len(patterns), stripe_pattern_ptr or None,
                                              stream), "lsec_decode_dev_patterns")

    def decode_dev_patterns(self, data, parity, patterns, stripe_pattern, stream=None) -> None:
        """torch: rebuild, in place, the erased shards of every stripe of data [N,k,C] / parity
        [N,m,C] under its own pattern; stripe_pattern: uint8 device tensor [N] of indices into patterns."""
        refs, n, size = self.tensor_refs(data, parity)
        if stripe_pattern.dtype.itemsize != 1 or not stripe_pattern.is_cuda or not stripe_pattern.is_contiguous() \
                or stripe_pattern.numel() != n:
            raise ValueError("stripe_pattern must be a contiguous uint8 device tensor with one entry per stripe")
        self.decode_dev_patterns_refs(refs, n, size, patterns, stripe_pattern.data_ptr(), _stream_handle(stream))

    def decode_dev_rotated_refs(self, refs, nstripes: int, block_size: int, lost, n_shift: int, first_stripe: int,
                                stream: int = 0) -> None:
        """lsec_decode_dev_rotated: degraded read of a rotated LUN.  refs[i] is PHYSICAL device i
        (stripe s holds logical chunk (i + (first_stripe + s) * n_shift) mod (k+m) there); the refs
        of the `lost` devices receive the rebuilt chunks."""
        _check(lib().lsec_decode_dev_rotated(self._p, self.shard_refs(refs), nstripes, block_size, _erasure_array(lost),
                                             n_shift, first_stripe, stream), "lsec_decode_dev_rotated")

    def decode_magic_dev_patterns_refs(self, refs, nstripes: int, block_size: int, patterns, stripe_pattern_ptr: int,
                                       magic_ptr: int, expect_ptr: int = 0, bad_ptr: int = 0, bad_count_ptr: int = 0,
                                       stream: int = 0) -> None:
        """lsec_decode_magic_dev_patterns: decode_dev_patterns_refs, and the 4 bytes at magic_ptr + 4*s (device memory,
        no alignment; 0: NULL) set to the adler32 of stripe s's k+m chunks as the decode leaves them; a stripe whose
        pattern id is >= len(patterns) is skipped.  expect_ptr (4 bytes per stripe), bad_ptr (1 byte per stripe) and
        bad_count_ptr (one aligned uint32): the comparison with the quorum magics, each optional (0)."""
        patterns = list(patterns)
        _check(lib().lsec_decode_magic_dev_patterns(self._p, None if refs is None else self.shard_refs(refs), nstripes,
                                                    block_size, _pattern_array(patterns), len(patterns),
                                                    stripe_pattern_ptr or None, magic_ptr or None, expect_ptr or None,
                                                    bad_ptr or None, bad_count_ptr or None, stream),
               "lsec_decode_magic_dev_patterns")

    def decode_magic_dev_rotated_refs(self, refs, nstripes: int, block_size: int, lost, n_shift: int, first_stripe: int,
                                      magic_ptr: int, expect_ptr: int = 0, bad_ptr: int = 0, bad_count_ptr: int = 0,
                                      stream: int = 0) -> None:
        """lsec_decode_magic_dev_rotated: decode_dev_rotated_refs with the magics of decode_magic_dev_patterns_refs;
        they are over the LOGICAL stripes, whatever the rotation."""
        _check(lib().lsec_decode_magic_dev_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes,
                                                   block_size, _erasure_array(lost), n_shift, first_stripe,
                                                   magic_ptr or None, expect_ptr or None, bad_ptr or None,
                                                   bad_count_ptr or None, stream), "lsec_decode_magic_dev_rotated")

    def decode_magic_dev_patterns(self, data, parity, patterns, stripe_pattern, magic, expect=None, bad=None,
                                  bad_count=None, stream=None) -> None:
        """torch: decode_dev_patterns, and magic (uint8 device tensor of 4 bytes per stripe, contiguous) set to the
        stripes' adler32 words as stripe_magic_dev writes them; expect (as magic), bad (uint8 [N]) and bad_count (one
        32-bit element) compare them with the quorum magics."""
        refs, n, size = self.tensor_refs(data, parity)
        if stripe_pattern.dtype.itemsize != 1 or not stripe_pattern.is_cuda or not stripe_pattern.is_contiguous() \
                or stripe_pattern.numel() != n:
            raise ValueError("stripe_pattern must be a contiguous uint8 device tensor with one entry per stripe")
        for what, t in (("magic", magic), ("expect", expect)):
            if t is not None and (t.dtype.itemsize != 1 or not t.is_cuda or not t.is_contiguous() or t.numel() != 4 * n):
                raise ValueError(f"{what} must be a contiguous uint8 device tensor of 4 bytes per stripe")
        if bad is not None and (bad.dtype.itemsize != 1 or not bad.is_cuda or not bad.is_contiguous() or bad.numel() != n):
            raise ValueError("bad must be a contiguous uint8 device tensor with one entry per stripe")
        if bad_count is not None and (bad_count.dtype.itemsize != 4 or not bad_count.is_cuda or bad_count.numel() != 1):
            raise ValueError("bad_count must be a 32-bit device tensor of one element")
        self.decode_magic_dev_patterns_refs(refs, n, size, patterns, stripe_pattern.data_ptr(), magic.data_ptr(),
                                            0 if expect is None else expect.data_ptr(), 0 if bad is None else bad.data_ptr(),
                                            0 if bad_count is None else bad_count.data_ptr(), _stream_handle(stream))

    def decode_dev_patterns_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int,
                                         patterns, stripe_pattern_ptr: int, stream: int = 0) -> None:
        """lsec_decode_dev_patterns_rotated: decode_dev_patterns_refs over the k+m PHYSICAL devices of a rotated LUN
        (refs[i]: device i, as check_dev_rotated_refs).  The patterns and stripe_pattern are those of the logical view:
        logical chunk c of stripe s is read from, and if erased rebuilt on, the device that holds it in that stripe.
        refs None / pointers 0 with nstripes == 0: only prepare the tables."""
        patterns = list(patterns)
        _check(lib().lsec_decode_dev_patterns_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes,
                                                      block_size, n_shift, first_stripe, _pattern_array(patterns),
                                                      len(patterns), stripe_pattern_ptr or None, stream),
               "lsec_decode_dev_patterns_rotated")

    def decode_magic_dev_patterns_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int,
                                               patterns, stripe_pattern_ptr: int, magic_ptr: int, expect_ptr: int = 0,
                                               bad_ptr: int = 0, bad_count_ptr: int = 0, stream: int = 0) -> None:
        """lsec_decode_magic_dev_patterns_rotated: decode_dev_patterns_rotated_refs with the magics, expect, bad and
        bad_count of decode_magic_dev_patterns_refs; the magics are over the LOGICAL stripes, whatever the rotation."""
        patterns = list(patterns)
        _check(lib().lsec_decode_magic_dev_patterns_rotated(self._p, None if refs is None else self.shard_refs(refs),
                                                            nstripes, block_size, n_shift, first_stripe,
                                                            _pattern_array(patterns), len(patterns),
                                                            stripe_pattern_ptr or None, magic_ptr or None, expect_ptr or None,
                                                            bad_ptr or None, bad_count_ptr or None, stream),
               "lsec_decode_magic_dev_patterns_rotated")

    def search_dev_patterns_refs(self, refs, nstripes: int, block_size: int, patterns, expect_ptr: int, found_ptr: int,
                                 select_ptr: int = 0, trial_ptr: int = 0, counts_ptr: int = 0, flags: int = 0,
                                 stream: int = 0) -> None:
        """lsec_search_dev_patterns: every candidate of `patterns` (a sequence of erasure lists of logical chunk ids) tried
        on every selected stripe, no chunk written.  found_ptr (1 byte per stripe): the first candidate whose rebuilt
        stripe sums to the 4 bytes at expect_ptr + 4*s, LOCATE_MANY if none does, LOCATE_CLEAN where the byte at
        select_ptr + s (0: every stripe is selected) is 0.  trial_ptr (4 bytes per stripe and candidate) and counts_ptr
        (two aligned uint32: found, LOCATE_MANY) are optional (0).  flags: SEARCH_REPAIR rebuilds every found stripe in
        place behind the search.  refs None / pointers 0 with nstripes == 0: only prepare the tables."""
        patterns = list(patterns)
        _check(lib().lsec_search_dev_patterns(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                              _pattern_array(patterns), len(patterns), select_ptr or None, expect_ptr or None,
                                              found_ptr or None, trial_ptr or None, counts_ptr or None, flags, stream),
               "lsec_search_dev_patterns")

    def search_dev_patterns_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int, patterns,
                                         expect_ptr: int, found_ptr: int, select_ptr: int = 0, trial_ptr: int = 0,
                                         counts_ptr: int = 0, flags: int = 0, stream: int = 0) -> None:
        """lsec_search_dev_patterns_rotated: search_dev_patterns_refs over the k+m PHYSICAL devices of a rotated LUN
        (refs[i]: device i, as check_dev_rotated_refs).  Patterns, found and trial are those of the logical view."""
        patterns = list(patterns)
        _check(lib().lsec_search_dev_patterns_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes,
                                                      block_size, n_shift, first_stripe, _pattern_array(patterns),
                                                      len(patterns), select_ptr or None, expect_ptr or None, found_ptr or None,
                                                      trial_ptr or None, counts_ptr or None, flags, stream),
               "lsec_search_dev_patterns_rotated")

    def search_dev_patterns(self, data, parity, patterns, expect, found, select=None, trial=None, counts=None,
                            repair: bool = False, stream=None) -> None:
        """torch: search data [N,k,C] / parity [N,m,C] for the candidate pattern that fits each stripe's quorum magic.
        expect: uint8 device tensor of 4 bytes per stripe; found, select: uint8 [N]; trial: uint8 of 4 bytes per stripe
        and candidate; counts: a 32-bit tensor of two elements; repair: rebuild the found stripes in place."""
        refs, n, size = self.tensor_refs(data, parity)
        npat = len(list(patterns))
        for what, t, want in (("expect", expect, 4 * n), ("found", found, n), ("select", select, n),
                              ("trial", trial, 4 * n * npat)):
            if t is None and what in ("select", "trial"):
                continue
            if t is None or t.dtype.itemsize != 1 or not t.is_cuda or not t.is_contiguous() or t.numel() != want:
                raise ValueError(f"{what} must be a contiguous uint8 device tensor of {want} bytes")
        if counts is not None and (counts.dtype.itemsize != 4 or not counts.is_cuda or not counts.is_contiguous()
                                   or counts.numel() != 2):
            raise ValueError("counts must be a contiguous 32-bit device tensor of two elements")
        self.search_dev_patterns_refs(refs, n, size, patterns, expect.data_ptr(), found.data_ptr(),
                                      0 if select is None else select.data_ptr(), 0 if trial is None else trial.data_ptr(),
                                      0 if counts is None else counts.data_ptr(), SEARCH_REPAIR if repair else 0,
                                      _stream_handle(stream))

    def vote_dev_refs(self, stored, refs, nstripes: int, block_size: int, patterns, quorum_ptr: int, cls_ptr: int,
                      ids_ptr: int = 0, outside_ptr: int = 0, counts_ptr: int = 0, flags: int = 0, stream: int = 0) -> None:
        """lsec_vote_dev: the quorum vote over the k+m stored magics of every stripe.  stored: k+m (base, stride), the 4
        bytes at base + s*stride are chunk i's stored magic (no alignment; base 0: unreadable; None: NULL).  refs: the
        chunks, read by the blank scan alone (None: no scan, no VOTE_BLANK).  patterns: a sequence of erasure lists of
        logical chunk ids to look each stripe's outside set up in, or None.  quorum_ptr (4 bytes per stripe), cls_ptr (1
        byte per stripe: VOTE_OK / _DEGRADED / _BLANK / _LOST); ids_ptr (1 byte per stripe, usable as stripe_pattern),
        outside_ptr (aligned uint64 per stripe) and counts_ptr (five aligned uint32) are optional (0).  flags:
        VOTE_PARANOID gives OK stripes a pattern id too."""
        pats = None if patterns is None else list(patterns)
        _check(lib().lsec_vote_dev(self._p, None if stored is None else self.shard_refs(stored),
                                   None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                   None if pats is None else _pattern_array(pats), 0 if pats is None else len(pats),
                                   quorum_ptr or None, cls_ptr or None, ids_ptr or None, outside_ptr or None,
                                   counts_ptr or None, flags, stream), "lsec_vote_dev")

    def vote_dev_rotated_refs(self, stored, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int, patterns,
                              quorum_ptr: int, cls_ptr: int, ids_ptr: int = 0, outside_ptr: int = 0, counts_ptr: int = 0,
                              flags: int = 0, stream: int = 0) -> None:
        """lsec_vote_dev_rotated: vote_dev_refs over the k+m PHYSICAL devices of a rotated LUN (stored[i], refs[i]: device
        i, as check_dev_rotated_refs).  Patterns, ids and outside are those of the logical view."""
        pats = None if patterns is None else list(patterns)
        _check(lib().lsec_vote_dev_rotated(self._p, None if stored is None else self.shard_refs(stored),
                                           None if refs is None else self.shard_refs(refs), nstripes, block_size, n_shift,
                                           first_stripe, None if pats is None else _pattern_array(pats),
                                           0 if pats is None else len(pats), quorum_ptr or None, cls_ptr or None,
                                           ids_ptr or None, outside_ptr or None, counts_ptr or None, flags, stream),
               "lsec_vote_dev_rotated")

    def check_dev_refs(self, refs, nstripes: int, block_size: int, syndrome_ptr: int, bad_count_ptr: int = 0,
                       stream: int = 0) -> None:
        """lsec_check_dev: one-pass parity check.  syndrome_ptr: device address of nstripes uint32 words,
        bit r of word s set when parity row r of stripe s differs from the stored chunk; bad_count_ptr:
        device address of one uint32 that receives the number of nonzero words (0: not wanted).  The
        call sets both itself; the shards (refs None: NULL) are only read."""
        _check(lib().lsec_check_dev(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                    syndrome_ptr or None, bad_count_ptr or None, stream), "lsec_check_dev")

    def check_dev(self, data, parity, syndrome, bad_count=None, stream=None) -> None:
        """torch: check data [N,k,C] against parity [N,m,C]; syndrome: int32 / uint32 device tensor [N],
        bad_count: such a tensor of one element, or None."""
        refs, n, size = self.tensor_refs(data, parity)
        if syndrome.dtype.itemsize != 4 or not syndrome.is_cuda or not syndrome.is_contiguous() or syndrome.numel() != n:
            raise ValueError("syndrome must be a contiguous 32-bit device tensor with one entry per stripe")
        self.check_dev_refs(refs, n, size, syndrome.data_ptr(), 0 if bad_count is None else bad_count.data_ptr(),
                            _stream_handle(stream))

    def locate_dev_refs(self, refs, nstripes: int, block_size: int, syndrome_ptr: int, hyp_ptr: int, located_ptr: int,
                        counts_ptr: int = 0, repair: bool = False, stream: int = 0) -> None:
        """lsec_locate_dev: find (repair: and rebuild in place) the one corrupt chunk of each stripe.  Device
        addresses: syndrome_ptr, nstripes uint32 (the words of lsec_check_dev); hyp_ptr, nstripes uint64 (bit
        j: data chunk j alone explains the stripe); located_ptr, nstripes bytes (LOCATE_CLEAN, a chunk id or
        LOCATE_MANY); counts_ptr, two uint32 (located, LOCATE_MANY; 0: not wanted).  The call sets all of them."""
        _check(lib().lsec_locate_dev(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                     syndrome_ptr or None, hyp_ptr or None, located_ptr or None, counts_ptr or None,
                                     LOCATE_REPAIR if repair else 0, stream), "lsec_locate_dev")

    def locate_dev(self, data, parity, syndrome, hyp, located, counts=None, repair=False, stream=None) -> None:
        """torch: locate in data [N,k,C] / parity [N,m,C]; syndrome: 32-bit device tensor [N], hyp: 64-bit [N],
        located: uint8 [N], counts: 32-bit [2] or None."""
        refs, n, size = self.tensor_refs(data, parity)
        for name, t, item, count in (("syndrome", syndrome, 4, n), ("hyp", hyp, 8, n), ("located", located, 1, n),
                                     ("counts", counts, 4, 2)):
            if t is not None and (t.dtype.itemsize != item or not t.is_cuda or not t.is_contiguous() or t.numel() != count):
                raise ValueError(f"{name} must be a contiguous device tensor of {count} elements of {item} bytes")
        self.locate_dev_refs(refs, n, size, syndrome.data_ptr(), hyp.data_ptr(), located.data_ptr(),
                             0 if counts is None else counts.data_ptr(), repair, _stream_handle(stream))

    def check_dev_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int,
                               syndrome_ptr: int, bad_count_ptr: int = 0, stream: int = 0) -> None:
        """lsec_check_dev_rotated: check_dev_refs over the PHYSICAL devices of a rotated LUN (refs[i]: device i,
        as decode_dev_rotated_refs takes them).  The outputs are those of each stripe's logical view."""
        _check(lib().lsec_check_dev_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                            n_shift, first_stripe, syndrome_ptr or None, bad_count_ptr or None, stream),
               "lsec_check_dev_rotated")

    def check_magic_dev_refs(self, refs, nstripes: int, block_size: int, syndrome_ptr: int, magic_ptr: int,
                             expect_ptr: int = 0, bad_ptr: int = 0, counts_ptr: int = 0, stream: int = 0) -> None:
        """lsec_check_magic_dev: check_dev_refs, and in the same pass the 4 bytes at magic_ptr + 4*s (device memory,
        no alignment; 0: NULL) set to the adler32 of stripe s's k+m chunks as stored.  expect_ptr (4 bytes per
        stripe: the quorum magics), bad_ptr (1 byte per stripe: SCRUB_BAD_PARITY | SCRUB_BAD_MAGIC) and counts_ptr
        (two aligned uint32: parity-bad, magic-bad) are each optional (0)."""
        _check(lib().lsec_check_magic_dev(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                          syndrome_ptr or None, magic_ptr or None, expect_ptr or None, bad_ptr or None,
                                          counts_ptr or None, stream), "lsec_check_magic_dev")

    def check_magic_dev_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int,
                                     syndrome_ptr: int, magic_ptr: int, expect_ptr: int = 0, bad_ptr: int = 0,
                                     counts_ptr: int = 0, stream: int = 0) -> None:
        """lsec_check_magic_dev_rotated: check_magic_dev_refs over the PHYSICAL devices of a rotated LUN (refs[i]:
        device i).  Syndromes and magics are those of each stripe's LOGICAL view, whatever the rotation."""
        _check(lib().lsec_check_magic_dev_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes,
                                                  block_size, n_shift, first_stripe, syndrome_ptr or None,
                                                  magic_ptr or None, expect_ptr or None, bad_ptr or None,
                                                  counts_ptr or None, stream), "lsec_check_magic_dev_rotated")

    @staticmethod
    def _check_magic_tensors(n, syndrome, magic, expect, bad, counts):
        for what, t, item, count in (("syndrome", syndrome, 4, n), ("magic", magic, 1, 4 * n), ("expect", expect, 1, 4 * n),
                                     ("bad", bad, 1, n), ("counts", counts, 4, 2)):
            if t is not None and (t.dtype.itemsize != item or not t.is_cuda or not t.is_contiguous() or t.numel() != count):
                raise ValueError(f"{what} must be a contiguous device tensor of {count} elements of {item} bytes")

    def check_magic_dev(self, data, parity, syndrome, magic, expect=None, bad=None, counts=None, stream=None) -> None:
        """torch: check_dev, and magic (uint8 device tensor of 4 bytes per stripe, contiguous) set to the stripes'
        adler32 words as stripe_magic_dev writes them; expect (as magic), bad (uint8 [N]) and counts (32-bit [2])
        compare them with the quorum magics."""
        refs, n, size = self.tensor_refs(data, parity)
        self._check_magic_tensors(n, syndrome, magic, expect, bad, counts)
        self.check_magic_dev_refs(refs, n, size, syndrome.data_ptr(), magic.data_ptr(),
                                  0 if expect is None else expect.data_ptr(), 0 if bad is None else bad.data_ptr(),
                                  0 if counts is None else counts.data_ptr(), _stream_handle(stream))

    def check_magic_dev_rotated(self, devs, n_shift: int, first_stripe: int, syndrome, magic, expect=None, bad=None,
                                counts=None, stream=None) -> None:
        """torch: check_magic_dev over devs [k+m, N, C], the physical devices of a rotated LUN (devs[i, s]: the chunk
        of stripe s on device i)."""
        if devs.dim() != 3 or devs.dtype.itemsize != 1 or not devs.is_cuda or devs.stride(2) != 1:
            raise ValueError("devs must be a uint8 device tensor [k+m, N, C] with contiguous chunks")
        n, size = devs.shape[1], devs.shape[2]
        refs = [(devs[i].data_ptr(), devs.stride(1)) for i in range(devs.shape[0])]
        self._check_magic_tensors(n, syndrome, magic, expect, bad, counts)
        self.check_magic_dev_rotated_refs(refs, n, size, n_shift, first_stripe, syndrome.data_ptr(), magic.data_ptr(),
                                          0 if expect is None else expect.data_ptr(), 0 if bad is None else bad.data_ptr(),
                                          0 if counts is None else counts.data_ptr(), _stream_handle(stream))

    def locate_dev_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int,
                                syndrome_ptr: int, hyp_ptr: int, located_ptr: int, located_dev_ptr: int = 0,
                                counts_ptr: int = 0, dev_faults_ptr: int = 0, repair: bool = False, stream: int = 0) -> None:
        """lsec_locate_dev_rotated: locate_dev_refs over the PHYSICAL devices of a rotated LUN.  syndrome, hyp,
        located and counts are those of each stripe's logical view; located_dev_ptr (nstripes bytes, 0: not
        wanted) receives the device holding each located chunk, dev_faults_ptr (k+m uint32, 0: not wanted) the
        located stripes per device.  repair rebuilds each located chunk in place on its device."""
        _check(lib().lsec_locate_dev_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                             n_shift, first_stripe, syndrome_ptr or None, hyp_ptr or None,
                                             located_ptr or None, located_dev_ptr or None, counts_ptr or None,
                                             dev_faults_ptr or None, LOCATE_REPAIR if repair else 0, stream),
               "lsec_locate_dev_rotated")

    def update_dev_refs(self, refs, nstripes: int, block_size: int, cols, fresh_refs, store: bool = False,
                        stream: int = 0) -> None:
        """lsec_update_dev: parity update for a partial-stripe write.  cols: the changed data chunk ids;
        fresh_refs[i]: the new content of chunk cols[i]; refs: the k+m logical chunks, of which only
        refs[cols[i]] (the old contents) and the parity are used -- every other data entry may be (0, 0).
        store: also write the fresh bytes over the old chunks.  refs / cols / fresh_refs None: NULL."""
        _check(lib().lsec_update_dev(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                     None if cols is None else _erasure_array(cols),
                                     None if fresh_refs is None else self.shard_refs(fresh_refs),
                                     UPDATE_STORE if store else 0, stream), "lsec_update_dev")

    def update_dev(self, data, parity, cols, fresh, store=False, stream=None) -> None:
        """torch: bring parity [N,m,C] up to date for data [N,k,C] whose chunks `cols` change to fresh
        [N,len(cols),C] (in the order of cols); data still holds the old bytes of those chunks, and with
        store=True receives the fresh ones.  The other chunks of data are not read."""
        refs, n, size = self.tensor_refs(data, parity)
        cols = list(cols)
        if fresh.dtype.itemsize != 1 or not fresh.is_cuda or fresh.dim() != 3 or fresh.shape[0] != n \
                or fresh.shape[1] != len(cols) or fresh.shape[2] != size or fresh.stride(2) != 1:
            raise ValueError("fresh must be a uint8 device tensor [N, len(cols), C] with contiguous rows")
        fresh_refs = [(fresh.data_ptr() + i * fresh.stride(1), fresh.stride(0)) for i in range(len(cols))]
        self.update_dev_refs(refs, n, size, cols, fresh_refs, store, _stream_handle(stream))

    def encode_dev_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int,
                                stream: int = 0) -> None:
        """lsec_encode_dev_rotated: encode_dev_refs over the PHYSICAL devices of a rotated LUN (refs[i]: device i,
        as check_dev_rotated_refs takes them): each stripe's parity goes to the devices its rotation names.
        refs None: NULL."""
        _check(lib().lsec_encode_dev_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                             n_shift, first_stripe, stream), "lsec_encode_dev_rotated")

    def encode_magic_dev_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int,
                                      magic_ptr: int, stream: int = 0) -> None:
        """lsec_encode_magic_dev_rotated: encode_dev_rotated_refs, and in the same pass the 4 bytes at magic_ptr + 4*s
        (device memory, no alignment, pure output; 0: NULL) set to the adler32 of stripe s's k+m chunks in LOGICAL
        order, the parity rows as just formed: what check_magic_dev_rotated_refs would write behind the encode.
        refs None: NULL."""
        _check(lib().lsec_encode_magic_dev_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes,
                                                   block_size, n_shift, first_stripe, magic_ptr or None, stream),
               "lsec_encode_magic_dev_rotated")

    def encode_magic_dev_rotated(self, devs, n_shift: int, first_stripe: int, magic, stream=None) -> None:
        """torch: encode_magic_dev_rotated_refs over devs [k+m, N, C], the physical devices of a rotated LUN (devs[i, s]:
        the chunk of stripe s on device i); magic: uint8 device tensor of 4 bytes per stripe, contiguous."""
        if devs.dim() != 3 or devs.dtype.itemsize != 1 or not devs.is_cuda or devs.stride(2) != 1:
            raise ValueError("devs must be a uint8 device tensor [k+m, N, C] with contiguous chunks")
        n, size = devs.shape[1], devs.shape[2]
        if magic.dtype.itemsize != 1 or not magic.is_cuda or not magic.is_contiguous() or magic.numel() != 4 * n:
            raise ValueError(f"magic must be a contiguous device tensor of {4 * n} elements of 1 byte")
        refs = [(devs[i].data_ptr(), devs.stride(1)) for i in range(devs.shape[0])]
        self.encode_magic_dev_rotated_refs(refs, n, size, n_shift, first_stripe, magic.data_ptr(), _stream_handle(stream))

    def update_dev_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int, cols,
                                fresh_refs, store: bool = False, stream: int = 0) -> None:
        """lsec_update_dev_rotated: update_dev_refs over the PHYSICAL devices of a rotated LUN.  cols are logical
        data chunk ids and fresh_refs[i] is a logical buffer (not rotated); the old chunks and the parity are
        taken from, and written to, the devices each stripe's rotation names.  refs / cols / fresh_refs None: NULL."""
        _check(lib().lsec_update_dev_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                             n_shift, first_stripe, None if cols is None else _erasure_array(cols),
                                             None if fresh_refs is None else self.shard_refs(fresh_refs),
                                             UPDATE_STORE if store else 0, stream), "lsec_update_dev_rotated")

    def update_dev_masked_refs(self, refs, nstripes: int, block_size: int, stripe_cols_ptr: int, fresh_refs,
                               store: bool = False, stream: int = 0) -> None:
        """lsec_update_dev_masked: update_dev_refs with a changed set per stripe.  stripe_cols_ptr: device address
        of nstripes uint64 words, bit j of word s: data chunk j of stripe s changes (0: NULL).  fresh_refs has k
        entries BY LOGICAL CHUNK ID; (0, 0) leaves column j out of the call, and refs[j] is then ignored.
        refs / fresh_refs None: NULL."""
        _check(lib().lsec_update_dev_masked(self._p, None if refs is None else self.shard_refs(refs), nstripes, block_size,
                                            stripe_cols_ptr or None,
                                            None if fresh_refs is None else self.shard_refs(fresh_refs),
                                            UPDATE_STORE if store else 0, stream), "lsec_update_dev_masked")

    def update_dev_masked_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int,
                                       stripe_cols_ptr: int, fresh_refs, store: bool = False, stream: int = 0) -> None:
        """lsec_update_dev_masked_rotated: update_dev_masked_refs over the PHYSICAL devices of a rotated LUN (refs[i]:
        device i).  The masks and fresh_refs are logical; the old chunks and the parity are taken from, and written
        to, the devices each stripe's rotation names."""
        _check(lib().lsec_update_dev_masked_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes,
                                                    block_size, n_shift, first_stripe, stripe_cols_ptr or None,
                                                    None if fresh_refs is None else self.shard_refs(fresh_refs),
                                                    UPDATE_STORE if store else 0, stream), "lsec_update_dev_masked_rotated")

    def update_dev_masked(self, data, parity, stripe_cols, fresh, store=False, stream=None) -> None:
        """torch: bring parity [N,m,C] up to date for data [N,k,C] where chunk j of stripe s changes to fresh[s, j]
        whenever bit j of stripe_cols[s] is set; stripe_cols: 64-bit device tensor [N], fresh: uint8 [N,k,C].  data
        still holds the old bytes, and with store=True receives the fresh ones of the changed chunks."""
        refs, n, size = self.tensor_refs(data, parity)
        if stripe_cols.dtype.itemsize != 8 or not stripe_cols.is_cuda or not stripe_cols.is_contiguous() \
                or stripe_cols.numel() != n:
            raise ValueError("stripe_cols must be a contiguous 64-bit device tensor with one entry per stripe")
        if fresh.dtype.itemsize != 1 or not fresh.is_cuda or fresh.dim() != 3 or fresh.shape[0] != n \
                or fresh.shape[1] != self.k or fresh.shape[2] != size or fresh.stride(2) != 1:
            raise ValueError("fresh must be a uint8 device tensor [N, k, C] with contiguous rows")
        fresh_refs = [(fresh.data_ptr() + j * fresh.stride(1), fresh.stride(0)) for j in range(self.k)]
        self.update_dev_masked_refs(refs, n, size, stripe_cols.data_ptr(), fresh_refs, store, _stream_handle(stream))

    def update_magic_dev_masked_refs(self, refs, nstripes: int, block_size: int, stripe_cols_ptr: int, fresh_refs,
                                     magic_ptr: int, store: bool = False, stream: int = 0) -> None:
        """lsec_update_magic_dev_masked: update_dev_masked_refs, and the 4 bytes at magic_ptr + 4*s (device memory, no
        alignment; 0: NULL) moved from the adler32 of stripe s as it was to that of stripe s with the chunks replaced."""
        _check(lib().lsec_update_magic_dev_masked(self._p, None if refs is None else self.shard_refs(refs), nstripes,
                                                  block_size, stripe_cols_ptr or None,
                                                  None if fresh_refs is None else self.shard_refs(fresh_refs),
                                                  UPDATE_STORE if store else 0, magic_ptr or None, stream),
               "lsec_update_magic_dev_masked")

    def update_magic_dev_masked_rotated_refs(self, refs, nstripes: int, block_size: int, n_shift: int, first_stripe: int,
                                             stripe_cols_ptr: int, fresh_refs, magic_ptr: int, store: bool = False,
                                             stream: int = 0) -> None:
        """lsec_update_magic_dev_masked_rotated: update_dev_masked_rotated_refs with the magics of
        update_magic_dev_masked_refs; they are over the LOGICAL stripes, whatever the rotation."""
        _check(lib().lsec_update_magic_dev_masked_rotated(self._p, None if refs is None else self.shard_refs(refs), nstripes,
                                                          block_size, n_shift, first_stripe, stripe_cols_ptr or None,
                                                          None if fresh_refs is None else self.shard_refs(fresh_refs),
                                                          UPDATE_STORE if store else 0, magic_ptr or None, stream),
               "lsec_update_magic_dev_masked_rotated")

    def update_magic_dev_masked(self, data, parity, stripe_cols, fresh, magic, store=False, stream=None) -> None:
        """torch: update_dev_masked, and magic (uint8 device tensor [N, 4], contiguous: the stripes' adler32 words as
        stripe_magic_dev writes them) brought from the old stripes' to the new stripes'."""
        refs, n, size = self.tensor_refs(data, parity)
        if stripe_cols.dtype.itemsize != 8 or not stripe_cols.is_cuda or not stripe_cols.is_contiguous() \
                or stripe_cols.numel() != n:
            raise ValueError("stripe_cols must be a contiguous 64-bit device tensor with one entry per stripe")
        if fresh.dtype.itemsize != 1 or not fresh.is_cuda or fresh.dim() != 3 or fresh.shape[0] != n \
                or fresh.shape[1] != self.k or fresh.shape[2] != size or fresh.stride(2) != 1:
            raise ValueError("fresh must be a uint8 device tensor [N, k, C] with contiguous rows")
        if magic.dtype.itemsize != 1 or not magic.is_cuda or not magic.is_contiguous() or magic.numel() != 4 * n:
            raise ValueError("magic must be a contiguous uint8 device tensor of 4 bytes per stripe")
        fresh_refs = [(fresh.data_ptr() + j * fresh.stride(1), fresh.stride(0)) for j in range(self.k)]
        self.update_magic_dev_masked_refs(refs, n, size, stripe_cols.data_ptr(), fresh_refs, magic.data_ptr(), store,
                                          _stream_handle(stream))

    def prepare_decode(self, erasures) -> None:
        _check(lib().lsec_prepare_decode(self._p, _erasure_array(erasures)), "lsec_prepare_decode")

    def prepare_encode(self) -> None:
        """Build the encode image on the current device and wait for a wide code's XOR network."""
        _check(lib().lsec_prepare_encode(self._p), "lsec_prepare_encode")

    def jit(self, erasures=None) -> bool:
        """True when the encode (or the decode of `erasures`) runs on a compiled XOR network."""
        return bool(lib().lsec_plan_jit(self._p, None if erasures is None else _erasure_array(erasures)))


def _stream_handle(stream) -> int:
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


def device_count() -> int:
    return lib().lsec_device_count()


def set_host_devices(devices: Sequence[int] = ()) -> None:
    """lsec_set_host_devices: devices serving host-memory calls (empty = the current device)."""
    arr = (C.c_int * max(1, len(devices)))(*devices)
    _check(lib().lsec_set_host_devices(arr, len(devices)), "lsec_set_host_devices")


def device_numa(dev: int) -> tuple[int, list[int]]:
    """lsec_device_numa: (NUMA node or -1, the node's CPUs this process may use) of device dev."""
    node = C.c_int(-1)
    cpus = (C.c_int * 4096)()
    n = lib().lsec_device_numa(dev, C.byref(node), cpus, 4096)
    if n < 0:
        raise ErasureError(f"lsec_device_numa failed: {last_error()}")
    return node.value, list(cpus[:n])


def numa_for_bus(root: str, bus: str) -> tuple[int, list[int]]:
    """Test hook: the placement of PCI function `bus` under the sysfs tree `root`."""
    node = C.c_int(-1)
    cpus = (C.c_int * 4096)()
    n = lib().lsec_test_numa_for_bus(root.encode(), bus.encode(), C.byref(node), cpus, 4096)
    if n < 0:
        raise ErasureError(f"lsec_test_numa_for_bus failed: {last_error()}")
    return node.value, list(cpus[:n])


TILES_STATIC, TILES_SHARED, TILES_TAIL = 0, 1, 2


def set_tile_sharing(mode) -> None:
    """lsec_set_tile_sharing: TILES_STATIC (each XCD its eighth), TILES_SHARED (all tiles through
    per-XCD counters with stealing) or TILES_TAIL (the default: a static 7/8, the rest shared);
    True / False select TILES_SHARED / TILES_STATIC"""
    lib().lsec_set_tile_sharing(int(mode))


def tile_sharing() -> int:
    return int(lib().lsec_tile_sharing())


def set_kernel_variant(bytewise: int = 0, bitsliced: int = 0) -> None:
    lib().lsec_set_kernel_variant(bytewise, bitsliced)


PATH_NETWORK, PATH_PACKET_NETWORK, PATH_GENERIC = 1, 2, 4


def apply_path() -> int:
    """Test hook: what this thread's last encode_dev / decode_dev launched, as PATH_* bits (a
    w = 16 / 32 network that leaves a ragged tail to the generic kernel: PATH_NETWORK | PATH_GENERIC)."""
    return int(lib().lsec_test_apply_path())


FORM_FAMILIES = ("chk", "loc", "chkrot", "locrot", "pat", "patrot", "upd", "encrot", "updrot")
Form = collections.namedtuple("Form", "family sliced R KC IT VW BF DW")
Form.__doc__ = """One separately compiled kernel of the check / locate / patterned / rotated / update calls: family (one of
FORM_FAMILIES), sliced (plan kernel 2), R rows; bytewise: KC (0 = K at run time), IT steps of VW dwords
per lane, BF branch-free; bit-sliced: DW dwords per lane (the others 0)."""


# the families added behind the nine (FORM_FAMILIES stays as it is): family number 10 onwards
MASKED_FAMILIES = ("updmask",)
# and behind those (MASKED_FAMILIES stays as it is too): family number 11, the masked update that keeps the magics
MAGIC_FAMILIES = ("updmaskmagic",)


# and behind those (MAGIC_FAMILIES stays as it is too): family number 12, the patterned decode that leaves the magics
PATMAGIC_FAMILIES = ("patmagic",)


# and behind those (PATMAGIC_FAMILIES stays as it is too): family numbers 13 and 14, the check that leaves the magics
# and its rotated form
CHKMAGIC_FAMILIES = ("chkmagic", "chkmagicrot")


# and behind those (CHKMAGIC_FAMILIES stays as it is too): family number 15, the rotated encode that leaves the magics
ENCMAGIC_FAMILIES = ("encmagicrot",)


# and behind those (ENCMAGIC_FAMILIES stays as it is too): family numbers 16 and 17, the search over candidate patterns
# and its rotated form
SEARCH_FAMILIES = ("patsearch", "patsearchrot")


# and behind those (SEARCH_FAMILIES stays as it is too): family number 18, the patterned decode that leaves the magics
# over the devices of a rotated LUN with a logical pattern per stripe
PATMAGICROT_FAMILIES = ("patmagicrot",)


def _form(v) -> Form:
    return Form((FORM_FAMILIES + MASKED_FAMILIES + MAGIC_FAMILIES + PATMAGIC_FAMILIES + CHKMAGIC_FAMILIES +
                 ENCMAGIC_FAMILIES + SEARCH_FAMILIES + PATMAGICROT_FAMILIES)[v[0] - 1], bool(v[1]), *(int(x) for x in v[2:8]))


def launch_record() -> list:
    """Test hook: the Forms this thread's last check_dev / locate_dev / decode_dev_patterns / decode_dev_rotated
    / check_dev_rotated / locate_dev_rotated / update_dev / encode_dev_rotated / update_dev_rotated / update_dev_masked(_rotated) / update_magic_dev_masked(_rotated) / decode_magic_dev_patterns / decode_magic_dev_rotated / check_magic_dev(_rotated) / encode_magic_dev_rotated call launched, in order (a locate with repair: its patterned
    decode too; a split call: every launch)."""
    buf = (C.c_int * (8 * 16))()
    n = lib().lsec_test_launch_record(buf, 16)
    if n > 16:
        raise ErasureError(f"lsec_test_launch_record: {n} launches, 16 are kept")
    return [_form(buf[8 * i:8 * i + 8]) for i in range(n)]


def predict_form(family: str, plan_kernel: int, k: int, rows: int, packet: int = 0, block_size: int = 0) -> Form:
    """Test hook (no GPU): the Form a launch of `family` takes for a plan of kernel 1 (bytewise) or 2
    (bit-sliced) with k inputs and `rows` rows (pat: the table's largest erasure count), asked of the
    functions the dispatch itself calls."""
    out = (C.c_int * 8)()
    _check(lib().lsec_test_predict_form(FORM_FAMILIES.index(family) + 1, plan_kernel, k, rows, packet, block_size, out),
           "lsec_test_predict_form")
    return _form(out)


def predict_masked_form(plan_kernel: int, k: int, rows: int, packet: int = 0, block_size: int = 0) -> Form:
    """Test hook (no GPU): the Form ("updmask") update_dev_masked_refs and update_dev_masked_rotated_refs launch for
    a plan of kernel 1 or 2 with k columns and `rows` rows, asked of the functions the dispatch itself calls."""
    out = (C.c_int * 8)()
    _check(lib().lsec_test_predict_masked_form(plan_kernel, k, rows, packet, block_size, out),
           "lsec_test_predict_masked_form")
    return _form(out)


def predict_masked_magic_form(plan_kernel: int, k: int, rows: int, packet: int = 0, block_size: int = 0) -> Form:
    """Test hook (no GPU): the Form ("updmaskmagic") update_magic_dev_masked_refs and
    update_magic_dev_masked_rotated_refs launch for a plan of kernel 1 or 2 with k columns and `rows` rows, asked of
    the functions the dispatch itself calls."""
    out = (C.c_int * 8)()
    _check(lib().lsec_test_predict_masked_magic_form(plan_kernel, k, rows, packet, block_size, out),
           "lsec_test_predict_masked_magic_form")
    return _form(out)


def predict_pattern_magic_form(plan_kernel: int, k: int, rows: int, packet: int = 0) -> Form:
    """Test hook (no GPU): the Form ("patmagic") decode_magic_dev_patterns_refs and decode_magic_dev_rotated_refs launch
    for a plan of kernel 1 or 2 with k inputs and a table of at most `rows` erasures per pattern (a table of empty
    patterns: 1), asked of the function the dispatch itself calls."""
    out = (C.c_int * 8)()
    _check(lib().lsec_test_predict_pattern_magic_form(plan_kernel, k, rows, packet, out),
           "lsec_test_predict_pattern_magic_form")
    return _form(out)


def predict_pattern_magic_rot_form(plan_kernel: int, k: int, rows: int, packet: int = 0) -> Form:
    """Test hook (no GPU): the Form ("patmagicrot") decode_magic_dev_patterns_rotated_refs launches for a plan of
    kernel 1 or 2 with k inputs and a table of at most `rows` erasures per pattern (a table of empty patterns: 1),
    asked of the function the dispatch itself calls."""
    out = (C.c_int * 8)()
    _check(lib().lsec_test_predict_pattern_magic_rot_form(plan_kernel, k, rows, packet, out),
           "lsec_test_predict_pattern_magic_rot_form")
    return _form(out)


def predict_search_form(rotated: bool, plan_kernel: int, k: int, rows: int, packet: int = 0) -> Form:
    """Test hook (no GPU): the Form ("patsearch", or "patsearchrot" with `rotated`) search_dev_patterns_refs and
    search_dev_patterns_rotated_refs launch for a plan of that kernel with k inputs and a candidate list of at most
    `rows` erasures per pattern (at least 1: a list of empty patterns launches the one-row form)."""
    out = (C.c_int * 8)()
    _check(lib().lsec_test_predict_search_form(1 if rotated else 0, plan_kernel, k, rows, packet, out),
           "lsec_test_predict_search_form")
    return _form(out)


def set_search_form(cand_outer: bool = False, plain_loads: bool = True) -> None:
    """Test hook: the search's tile order (cand_outer: the piece of the chunk innermost, not the candidate) and load
    kind (plain_loads: plain, not non-temporal) for A/B runs; the defaults are what ships, and the results do not depend
    on either."""
    lib().lsec_test_set_search_form(1 if cand_outer else 0, 1 if plain_loads else 0)


def set_vote_form(plain_loads: bool = False, steps: int = 2) -> None:
    """Test hook: the load kind of the vote's blank scan (plain_loads: plain, not non-temporal) and its tile (steps: 2 or
    4 16-byte steps per lane) for A/B runs; the defaults are what ships, and the results do not depend on either."""
    lib().lsec_test_set_vote_form(1 if plain_loads else 0, steps)


def predict_check_magic_form(rotated: bool, plan_kernel: int, k: int, rows: int, packet: int = 0, block_size: int = 0) -> Form:
    """Test hook (no GPU): the Form ("chkmagic", or "chkmagicrot" with `rotated`) check_magic_dev_refs and
    check_magic_dev_rotated_refs launch for a plan of kernel 1 or 2 with k inputs and `rows` rows, asked of the
    functions the dispatch itself calls."""
    out = (C.c_int * 8)()
    _check(lib().lsec_test_predict_check_magic_form(1 if rotated else 0, plan_kernel, k, rows, packet, block_size, out),
           "lsec_test_predict_check_magic_form")
    return _form(out)


def predict_encode_magic_form(plan_kernel: int, k: int, rows: int, packet: int = 0, block_size: int = 0) -> Form:
    """Test hook (no GPU): the Form ("encmagicrot") encode_magic_dev_rotated_refs launches for a plan of kernel 1 or 2
    with k inputs and `rows` rows, asked of the functions the dispatch itself calls."""
    out = (C.c_int * 8)()
    _check(lib().lsec_test_predict_encode_magic_form(plan_kernel, k, rows, packet, block_size, out),
           "lsec_test_predict_encode_magic_form")
    return _form(out)


def predict_forms(call: str, plan_kernel: int, k: int, rows: int, packet: int = 0, block_size: int = 0,
                  repair: bool = False) -> list:
    """Test hook (no GPU): what launch_record() holds after one unsplit call of `call` (a family name): its
    form, and behind a repairing locate the one-row patterned decode's (pat, or patrot for locrot)."""
    forms = [predict_form(call, plan_kernel, k, rows, packet, block_size)]
    if repair:
        forms.append(predict_form({"loc": "pat", "locrot": "patrot"}[call], plan_kernel, k, 1, packet, block_size))
    return forms


# The apply family -- what encode_dev, decode_dev and encode_magic_dev launch -- has a record of its own layout
# behind the fifteen families above (those tuples and Form stay as they are).
ApplyForm = collections.namedtuple("ApplyForm", "kind R KC IT VW BF DW w acc magic sub loop")
ApplyForm.__doc__ = """One separately compiled kernel behind encode_dev / decode_dev / encode_magic_dev: kind (1 bytewise, 2
bit-sliced, 3 bitmatrix, 4 GF(2^w) wordwise or transposed, 5 GF(2^w) bit-sliced), R rows; bytewise: KC (0 = K at run
time), IT steps of VW dwords per lane, BF branch-free; bit-sliced: DW dwords per lane; kinds 3-5: w; acc: the
accumulate instantiation of a later input group; magic: the fused stripe-magic instantiation; sub: kind 3, 1 the
kernel of its word size and 0 the any-w kernel; kind 4, 1 the transposed kernel and 0 the mask-per-bit one; loop:
bytewise kernels that hold two whole tile loops, 1 the plain-XOR first row's and 0 the other's, -1 where the kernel
has one loop."""
APPLY_RECORD_MAX = 64


def _apply_forms(buf, n: int) -> list:
    return [ApplyForm(*(int(x) for x in buf[12 * i:12 * i + 12])) for i in range(n)]


def apply_record() -> list:
    """Test hook: the ApplyForms this thread's last encode_dev / decode_dev / encode_magic_dev call launched from the
    table dispatch, in order: input groups x row launches x stripe ranges (a compiled network's launch is not among
    them, nor the magic pass of a two-pass encode_magic_dev)."""
    buf = (C.c_int * (12 * APPLY_RECORD_MAX))()
    n = lib().lsec_test_apply_record(buf, APPLY_RECORD_MAX)
    if n > APPLY_RECORD_MAX:
        raise ErasureError(f"lsec_test_apply_record: {n} launches, {APPLY_RECORD_MAX} are kept")
    return _apply_forms(buf, n)


def predict_apply(kind: int, k: int, rows: int, w: int = 8, packet: int = 0, block_size: int = 0, magic: bool = False,
                  variants=(0, 0), row_ones=None) -> list:
    """Test hook (no GPU): what apply_record() holds after one unsplit call of a k x rows matrix of kernel `kind` while
    no network is ready, under the two kernel-variant values; magic: encode_magic_dev; row_ones: per row, whether it
    is all ones.  Asked of the functions the calls themselves go through."""
    buf = (C.c_int * (12 * 256))()
    ones = bytes(1 if x else 0 for x in row_ones) if row_ones is not None else None
    if ones is not None and len(ones) != rows:
        raise ValueError("row_ones needs one entry per row")
    n = _check_nonneg(lib().lsec_test_predict_apply(kind, k, rows, w, packet, block_size, 1 if magic else 0, variants[0],
                                                    variants[1], ones, buf, 256), "lsec_test_predict_apply")
    return _apply_forms(buf, n)


def predict_apply_launch(kind: int, k: int, rows: int, w: int = 8, packet: int = 0, acc: bool = False, magic: bool = False,
                         dw_pref: int = 0, variants=(0, 0), first_row_ones: bool = False) -> ApplyForm:
    """Test hook (no GPU): the ApplyForm of one launch of k inputs and `rows` rows, unsplit: predict_apply cuts a call
    into the launches the engine makes, so a kernel compiled for more rows than a launch ever gets is named here alone."""
    out = (C.c_int * 12)()
    _check(lib().lsec_test_predict_apply_launch(kind, k, rows, w, packet, 1 if acc else 0, 1 if magic else 0, dw_pref,
                                                variants[0], variants[1], 1 if first_row_ones else 0, out),
           "lsec_test_predict_apply_launch")
    return ApplyForm(*(int(x) for x in out))


def predict_apply_plan(plan: "Plan", erasures=None, block_size: int = 0, magic: bool = False) -> list:
    """Test hook (no GPU): predict_apply for the plan's own matrices under the kernel variants in force: its encode
    (erasures None; magic: encode_magic_dev) or the decode of `erasures`."""
    buf = (C.c_int * (12 * 256))()
    era = _erasure_array(erasures) if erasures is not None else None
    n = _check_nonneg(lib().lsec_test_predict_apply_plan(plan._p, era, block_size, 1 if magic else 0, buf, 256),
                      "lsec_test_predict_apply_plan")
    return _apply_forms(buf, n)


def hold_networks(on: bool = True) -> None:
    """Test hook: while on, no compiled network counts as ready, so encode_dev / decode_dev run the table kernels
    under the automatic policy, as on a plan's first calls."""
    lib().lsec_test_hold_networks(1 if on else 0)


def fixed_k() -> tuple:
    """Test hook (no GPU): the K for which the bytewise kernels have fixed-K forms (LSEC_FIXED_K)."""
    buf = (C.c_int * 64)()
    return tuple(buf[:lib().lsec_test_fixed_k(buf, 64)])


def set_pattern_split(stripes: int = 0) -> None:
    """Test hook: a patterned decode (and update_dev, encode_dev_rotated, encode_magic_dev_rotated, update_dev_rotated) launches at most `stripes` stripes at a time (0: no extra split)."""
    lib().lsec_test_set_pattern_split(int(stripes))


def pattern_rot0(n: int, n_shift: int, first_stripe: int) -> int:
    """Test hook: (first_stripe * n_shift) mod n as lsec_decode_dev_rotated computes it."""
    return _check_nonneg(lib().lsec_test_pattern_rot0(n, n_shift, first_stripe), "lsec_test_pattern_rot0")


def _check_nonneg(rc: int, what: str) -> int:
    if rc < 0:
        raise ErasureError(f"{what} failed (rc={rc}): {last_error()}")
    return rc


def pattern_table_entry(plan: "Plan", pattern_id: int, patterns=None, lost=None, n_shift: int = 0):
    """Test hook (no GPU): entry pattern_id of the host table of lsec_decode_dev_patterns (patterns
    given) or lsec_decode_dev_rotated (lost, n_shift; pattern_id is the rotation) ->
    (nout, in_sel [k], out_sel [nout], rows [nout, k]); nout = -1 for a rotation that cannot occur."""
    k, n = plan.k, plan.k + plan.m
    nout = C.c_int(0)
    in_sel, out_sel, coef = (C.c_int * k)(), (C.c_int * n)(), (C.c_int * (n * k))()
    pats = None if patterns is None else list(patterns)
    _check(lib().lsec_test_pattern_table(plan.ptr, None if pats is None else _pattern_array(pats),
                                         0 if pats is None else len(pats),
                                         None if lost is None else _erasure_array(lost), n_shift, pattern_id,
                                         C.byref(nout), in_sel, out_sel, coef), "lsec_test_pattern_table")
    e = max(0, nout.value)
    return nout.value, list(in_sel[:k]), list(out_sel[:e]), np.array(coef[:e * k], dtype=np.int32).reshape(e, k)


def pattern_unused_entry(plan: "Plan", pattern_id: int, patterns=None, lost=None, n_shift: int = 0):
    """Test hook (no GPU): what the magic form sums for entry pattern_id of pattern_table_entry's table ->
    (nout, in_sel [k], out_sel [nout], unused): the shard indices it loads as inputs (nout 0, the checksum-only
    path: the data chunks), those it rebuilds, and the survivors it loads for the checksum alone."""
    k, n = plan.k, plan.k + plan.m
    nout = C.c_int(0)
    in_sel, out_sel, unused = (C.c_int * k)(), (C.c_int * n)(), (C.c_int * n)()
    pats = None if patterns is None else list(patterns)
    nu = _check_nonneg(lib().lsec_test_pattern_unused(plan.ptr, None if pats is None else _pattern_array(pats),
                                                      0 if pats is None else len(pats),
                                                      None if lost is None else _erasure_array(lost), n_shift, pattern_id,
                                                      C.byref(nout), in_sel, out_sel, unused), "lsec_test_pattern_unused")
    return nout.value, list(in_sel[:k]), list(out_sel[:max(0, nout.value)]), list(unused[:nu])


def host_unpin_drain() -> None:
    """lsec_host_unpin_drain: wait until registrations left to the background unpinner are dropped"""
    lib().lsec_host_unpin_drain()


def locate_ratio(plan: "Plan", r: int, j: int) -> int:
    """Test hook (no GPU): Q[r][j] = g[r+1][j] / g[0][j] of the host ratio image lsec_locate_dev uploads."""
    return _check_nonneg(lib().lsec_test_locate_ratio(plan.ptr, r, j), "lsec_test_locate_ratio")


def plan_images(plan: "Plan") -> int:
    """Test hook: the device allocations the plan owns now, over every per-device image (one per device it is on)."""
    return _check_nonneg(lib().lsec_test_plan_images(plan.ptr), "lsec_test_plan_images")
