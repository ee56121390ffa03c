"""Host side of lsec_check_dev_rotated / lsec_locate_dev_rotated (check, locate and repair over the
physical devices of a rotated LUN): the symbols, the Python mirror and the argument validation,
checked without a GPU.  nstripes == 0 validates the arguments and touches no GPU, so every refusal
here is reached before anything could be enqueued; the pointers handed in are never dereferenced.
"""
import ctypes as C
import os
import re

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

FAKE = 0x7F00_0000_1000  # an address that is a multiple of 8: only its alignment is looked at
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lstore_ec.h")
NAMES = ("lsec_check_dev_rotated", "lsec_locate_dev_rotated")


def shards_of(n, base=FAKE, stride=8192):
    sh = (E.ShardRef * n)()
    for i in range(n):
        sh[i].base, sh[i].stride = base + i * 4096, stride
    return sh


def check(p, sh, nstripes, size, n_shift=1, first=5, syndrome=None, bad_count=None):
    return L.lib().lsec_check_dev_rotated(p.ptr, sh, nstripes, size, n_shift, first, syndrome, bad_count, None)


def locate(p, sh, nstripes, size, n_shift=1, first=5, syndrome=None, hyp=None, located=None, located_dev=None, counts=None,
           dev_faults=None, flags=0):
    return L.lib().lsec_locate_dev_rotated(p.ptr, sh, nstripes, size, n_shift, first, syndrome, hyp, located, located_dev,
                                           counts, dev_faults, flags, None)


def refused(call, words, *args, **kw):
    assert call(*args, **kw) == -1, (call.__name__, words)
    msg = E.last_error()
    assert msg and words in msg, (call.__name__, words, msg)


def both_refused(words, p, sh, nstripes, size, **kw):
    refused(check, words, p, sh, nstripes, size, **kw)
    refused(locate, words, p, sh, nstripes, size, **kw)


@pytest.fixture(scope="module")
def rs63(built):
    with L.Plan.for_chunk(L.REED_SOL_VAN, 6, 3, 4096) as p:
        yield p


def test_symbols_mirror_and_abi_version(built):
    lib = L.lib()
    with open(HEADER) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), f"{name} is not declared in the header"
        assert name in E.EXPORTS and hasattr(lib, name)
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the calls by their symbols
    for name in ("check_dev_rotated_refs", "locate_dev_rotated_refs"):
        assert callable(getattr(L.Plan, name))


def test_zero_stripes_validate_only(rs63):
    # NULL outputs
    assert check(rs63, shards_of(9), 0, 4096) == 0, E.last_error()
    assert locate(rs63, shards_of(9), 0, 4096) == 0, E.last_error()
    # NULL bases stay valid with no stripes (the prepare-ahead convention of the *_dev calls)
    assert check(rs63, shards_of(9, base=0, stride=0), 0, 4096) == 0, E.last_error()
    assert locate(rs63, shards_of(9, base=0, stride=0), 0, 4096) == 0, E.last_error()
    # every output given; located and located_dev at odd addresses
    assert check(rs63, shards_of(9), 0, 4096, syndrome=FAKE, bad_count=FAKE + 4) == 0, E.last_error()
    assert locate(rs63, shards_of(9), 0, 4096, syndrome=FAKE, hyp=FAKE + 64, located=FAKE + 129, located_dev=FAKE + 257,
                  counts=FAKE + 4, dev_faults=FAKE + 512) == 0, E.last_error()
    # with the repair flag: the single-erasure tables are prepared
    assert locate(rs63, shards_of(9), 0, 4096, flags=E.LOCATE_REPAIR) == 0, E.last_error()
    # n_shift beyond k+m is taken mod k+m, first_stripe may be anything up to 2^63 - 1
    assert locate(rs63, shards_of(9), 0, 4096, n_shift=11, first=(1 << 63) - 1) == 0, E.last_error()
    assert check(rs63, shards_of(9), 0, 4096, n_shift=0, first=0) == 0, E.last_error()
    # the mirror, NULL outputs
    refs = [(FAKE + i * 4096, 8192) for i in range(9)]
    rs63.check_dev_rotated_refs(refs, 0, 4096, 1, 5, 0)
    rs63.locate_dev_rotated_refs(refs, 0, 4096, 1, 5, 0, 0, 0)
    rs63.locate_dev_rotated_refs(refs, 0, 4096, 3, 3_000_000_007, 0, 0, 0, repair=True)


def test_repair_adds_no_limit(built):
    """RS(16+4) at n_shift = 1: 20 devices x 20 rotations would be 400 (rotation, chunk) records"""
    with L.Plan.for_chunk(L.REED_SOL_VAN, 16, 4, 4096) as p:
        assert locate(p, shards_of(20), 0, 4096, n_shift=1, flags=E.LOCATE_REPAIR) == 0, E.last_error()


def test_refuses_negative_rotation(rs63):
    both_refused("n_shift", rs63, shards_of(9), 0, 4096, n_shift=-1)
    assert "negative" in E.last_error()
    both_refused("first_stripe", rs63, shards_of(9), 0, 4096, first=-1)
    assert "negative" in E.last_error()


def test_refuses_other_plan_kernels(built):
    with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 3
        both_refused("plan kernel 3", p, shards_of(7), 0, 7 * 32 * 4)
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
        assert p.kernel == 4
        both_refused("plan kernel 4", p, shards_of(9), 0, 4096)


def test_refuses_wide_stripes_and_one_parity_row(built):
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
        refused(check, "m=9", p, shards_of(15), 0, 4096)
        assert "1..8" in E.last_error()
        refused(locate, "m=9", p, shards_of(15), 0, 4096)
        assert "2..8" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
        both_refused("k=65", p, shards_of(68), 0, 4096)
        assert "1..64" in E.last_error()
    with L.Plan.new(L.RAID4, 4096, 6, 1, 8, 0, 1) as p:
        assert check(p, shards_of(7), 0, 4096) == 0, E.last_error()  # one row checks ...
        refused(locate, "m=1", p, shards_of(7), 0, 4096)             # ... and cannot locate
        assert "2..8" in E.last_error() and "one parity row cannot locate" in E.last_error()


def test_refuses_null_and_misaligned_pointers(rs63):
    both_refused("devs is NULL", rs63, None, 0, 4096)
    both_refused("multiple of 8 bytes", rs63, shards_of(9, base=FAKE + 4), 0, 4096)   # a base, lsec_shard_t's rule
    refused(check, "multiple of 8 bytes", rs63, shards_of(9, stride=8196), 4, 4096, syndrome=FAKE)  # a stride
    refused(locate, "multiple of 8 bytes", rs63, shards_of(9, stride=8196), 4, 4096, syndrome=FAKE, hyp=FAKE, located=FAKE)
    refused(check, "syndrome is NULL", rs63, shards_of(9), 4, 4096)
    refused(locate, "syndrome is NULL", rs63, shards_of(9), 4, 4096, hyp=FAKE, located=FAKE)
    refused(locate, "hyp is NULL", rs63, shards_of(9), 4, 4096, syndrome=FAKE, located=FAKE)
    refused(locate, "located is NULL", rs63, shards_of(9), 4, 4096, syndrome=FAKE, hyp=FAKE)
    both_refused("syndrome", rs63, shards_of(9), 0, 4096, syndrome=FAKE + 2)
    assert "multiple of 4" in E.last_error()
    refused(check, "bad_count", rs63, shards_of(9), 0, 4096, syndrome=FAKE, bad_count=FAKE + 2)
    assert "multiple of 4" in E.last_error()
    refused(locate, "hyp", rs63, shards_of(9), 0, 4096, syndrome=FAKE, hyp=FAKE + 4)
    assert "multiple of 8" in E.last_error()
    refused(locate, "counts", rs63, shards_of(9), 0, 4096, syndrome=FAKE, hyp=FAKE, located=FAKE + 1, counts=FAKE + 6)
    assert "multiple of 4" in E.last_error()
    refused(locate, "dev_faults", rs63, shards_of(9), 0, 4096, syndrome=FAKE, hyp=FAKE, located=FAKE + 1, located_dev=FAKE + 3,
            dev_faults=FAKE + 2)
    assert "multiple of 4" in E.last_error()
    refused(locate, "LSEC_LOCATE_REPAIR", rs63, shards_of(9), 0, 4096, flags=2)  # an unknown flag bit


def test_refuses_block_sizes(rs63):
    both_refused("multiple of 8", rs63, shards_of(9), 0, 4100)
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 2
        assert check(p, shards_of(9), 0, 8 * 64 * 2) == 0, E.last_error()
        assert locate(p, shards_of(9), 0, 8 * 64 * 2, flags=E.LOCATE_REPAIR) == 0, E.last_error()
        both_refused("w*packet_size = 512", p, shards_of(9), 0, 8 * 64 * 2 + 64)


def test_not_a_plan(built):
    fake = (C.c_char * 512)()
    plan = C.cast(fake, C.POINTER(E.PlanStruct))
    assert L.lib().lsec_check_dev_rotated(plan, shards_of(9), 0, 4096, 1, 0, None, None, None) == -1
    assert "not an lstore_ec plan" in E.last_error()
    assert L.lib().lsec_locate_dev_rotated(plan, shards_of(9), 0, 4096, 1, 0, None, None, None, None, None, None, 0, None) == -1
    assert "not an lstore_ec plan" in E.last_error()
