"""Host side of lsec_check_dev (the one-pass parity check of device-resident stripes): the symbol, the
Python mirror and the argument validation, checked without a GPU.  nstripes == 0 validates the
arguments and touches no GPU, so every refusal here is reached before anything could be enqueued;
the pointers handed in are never dereferenced.
"""
import ctypes as C

import pytest

import lstore_amd as L
from lstore_amd import erasure as E

FAKE = 0x7F00_0000_1000  # an address that is a multiple of 8: only its alignment is looked at


def shards_of(n, base=FAKE, stride=8192):
    sh = (E.ShardRef * n)()
    for i in range(n):
        sh[i].base, sh[i].stride = base + i * 4096, stride
    return sh


def check(p, sh, nstripes, size, syndrome=None, bad_count=None):
    return L.lib().lsec_check_dev(p.ptr, sh, nstripes, size, syndrome, bad_count, None)


def refused(p, sh, nstripes, size, words, syndrome=None, bad_count=None):
    assert check(p, sh, nstripes, size, syndrome, bad_count) == -1, words
    msg = E.last_error()
    assert msg and words in msg, (words, msg)


@pytest.fixture(scope="module")
def rs63(built):
    with L.Plan.for_chunk(L.REED_SOL_VAN, 6, 3, 4096) as p:
        yield p


def test_symbol_mirror_and_abi_version(built):
    lib = L.lib()
    assert "lsec_check_dev" in E.EXPORTS and hasattr(lib, "lsec_check_dev")
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the call by its symbol
    for name in ("check_dev_refs", "check_dev"):
        assert callable(getattr(L.Plan, name))


def test_zero_stripes_validate_only(rs63):
    assert check(rs63, shards_of(9), 0, 4096) == 0, E.last_error()
    assert check(rs63, shards_of(9), 0, 4096, FAKE, FAKE + 4) == 0, E.last_error()
    rs63.check_dev_refs([(FAKE + i * 4096, 8192) for i in range(9)], 0, 4096, 0)  # the mirror, NULL syndrome
    # NULL bases stay valid with no stripes (the prepare-ahead convention of the *_dev calls)
    assert check(rs63, shards_of(9, base=0, stride=0), 0, 4096) == 0, E.last_error()


def test_refuses_other_plan_kernels(built):
    with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 3
        refused(p, shards_of(7), 0, 7 * 32 * 4, "plan kernel 3")
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
        assert p.kernel == 4
        refused(p, shards_of(9), 0, 4096, "plan kernel 4")


def test_refuses_wide_stripes(built):
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
        refused(p, shards_of(15), 0, 4096, "m=9")
        assert "1..8" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
        refused(p, shards_of(68), 0, 4096, "k=65")
        assert "1..64" in E.last_error()


def test_refuses_null_and_misaligned_pointers(rs63):
    refused(rs63, None, 0, 4096, "shards is NULL")
    refused(rs63, shards_of(9), 4, 4096, "syndrome is NULL")
    refused(rs63, shards_of(9, base=FAKE + 4), 0, 4096, "multiple of 8 bytes")   # a base, lsec_shard_t's rule
    refused(rs63, shards_of(9, stride=8196), 4, 4096, "multiple of 8 bytes", syndrome=FAKE)  # a stride
    refused(rs63, shards_of(9), 0, 4096, "syndrome", syndrome=FAKE + 2)
    assert "multiple of 4" in E.last_error()
    refused(rs63, shards_of(9), 0, 4096, "bad_count", syndrome=FAKE, bad_count=FAKE + 6)
    assert "multiple of 4" in E.last_error()


def test_refuses_block_sizes(rs63):
    refused(rs63, shards_of(9), 0, 4100, "multiple of 8")
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 2
        assert check(p, shards_of(9), 0, 8 * 64 * 2) == 0, E.last_error()
        refused(p, shards_of(9), 0, 8 * 64 * 2 + 64, "w*packet_size = 512")


def test_not_a_plan(built):
    fake = (C.c_char * 512)()
    assert L.lib().lsec_check_dev(C.cast(fake, C.POINTER(E.PlanStruct)), shards_of(9), 0, 4096, None, None, None) == -1
    assert "not an lstore_ec plan" in E.last_error()
