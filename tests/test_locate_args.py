"""Host side of lsec_locate_dev (find and repair the corrupt chunk of device-resident stripes): the
symbol, the Python mirror, the argument validation and the ratio image, checked without a GPU.
nstripes == 0 validates the arguments and touches no GPU, so every refusal here is reached before
anything could be enqueued; the pointers handed in are never dereferenced.
"""
import ctypes as C

import numpy as np
import pytest

import lstore_amd as L
import oracle as O
from lstore_amd import erasure as E

FAKE = 0x7F00_0000_1000  # an address that is a multiple of 8: only its alignment is looked at


def shards_of(n, base=FAKE, stride=8192):
    sh = (E.ShardRef * n)()
    for i in range(n):
        sh[i].base, sh[i].stride = base + i * 4096, stride
    return sh


def locate(p, sh, nstripes, size, syndrome=None, hyp=None, located=None, counts=None, flags=0):
    return L.lib().lsec_locate_dev(p.ptr, sh, nstripes, size, syndrome, hyp, located, counts, flags, None)


def refused(p, sh, nstripes, size, words, **out):
    assert locate(p, sh, nstripes, size, **out) == -1, words
    msg = E.last_error()
    assert msg and words in msg, (words, msg)


@pytest.fixture(scope="module")
def rs63(built):
    with L.Plan.for_chunk(L.REED_SOL_VAN, 6, 3, 4096) as p:
        yield p


def test_symbol_mirror_and_abi_version(built):
    lib = L.lib()
    assert "lsec_locate_dev" in E.EXPORTS and hasattr(lib, "lsec_locate_dev")
    assert lib.lsec_abi_version() == 3  # purely additive: a caller detects the call by its symbol
    for name in ("locate_dev_refs", "locate_dev"):
        assert callable(getattr(L.Plan, name))
    assert (E.LOCATE_CLEAN, E.LOCATE_MANY, E.LOCATE_REPAIR) == (0xFF, 0xFE, 1)


def test_zero_stripes_validate_only(rs63):
    assert locate(rs63, shards_of(9), 0, 4096) == 0, E.last_error()
    assert locate(rs63, shards_of(9), 0, 4096, FAKE, FAKE + 64, FAKE + 129, FAKE + 4) == 0, E.last_error()  # located odd
    rs63.locate_dev_refs([(FAKE + i * 4096, 8192) for i in range(9)], 0, 4096, 0, 0, 0)  # the mirror, NULL outputs
    # NULL bases stay valid with no stripes (the prepare-ahead convention of the *_dev calls)
    assert locate(rs63, shards_of(9, base=0, stride=0), 0, 4096) == 0, E.last_error()
    # with the repair flag the single-erasure table is prepared: the matrix work where there is no device
    assert locate(rs63, shards_of(9), 0, 4096, flags=E.LOCATE_REPAIR) == 0, E.last_error()


def test_refuses_other_plan_kernels(built):
    with L.Plan.new(L.LIBERATION, 7 * 32 * 4, 5, 2, 7, 32, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 3
        refused(p, shards_of(7), 0, 7 * 32 * 4, "plan kernel 3")
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 3, 16, 0, 8) as p:
        assert p.kernel == 4
        refused(p, shards_of(9), 0, 4096, "plan kernel 4")


def test_refuses_one_parity_row_and_wide_stripes(built):
    with L.Plan.new(L.RAID4, 4096, 6, 1, 8, 0, 1) as p:
        refused(p, shards_of(7), 0, 4096, "m=1")
        assert "2..8" in E.last_error() and "one parity row cannot locate" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 6, 9, 8, 0, 8) as p:
        refused(p, shards_of(15), 0, 4096, "m=9")
        assert "2..8" in E.last_error()
    with L.Plan.new(L.REED_SOL_VAN, 4096, 65, 3, 8, 0, 8) as p:
        refused(p, shards_of(68), 0, 4096, "k=65")
        assert "1..64" in E.last_error()


def test_refuses_null_and_misaligned_pointers(rs63):
    refused(rs63, None, 0, 4096, "shards is NULL")
    refused(rs63, shards_of(9), 4, 4096, "syndrome is NULL", hyp=FAKE, located=FAKE)
    refused(rs63, shards_of(9), 4, 4096, "hyp is NULL", syndrome=FAKE, located=FAKE)
    refused(rs63, shards_of(9), 4, 4096, "located is NULL", syndrome=FAKE, hyp=FAKE)
    refused(rs63, shards_of(9, base=FAKE + 4), 0, 4096, "multiple of 8 bytes")   # a base, lsec_shard_t's rule
    refused(rs63, shards_of(9, stride=8196), 4, 4096, "multiple of 8 bytes", syndrome=FAKE, hyp=FAKE, located=FAKE)  # a stride
    refused(rs63, shards_of(9), 0, 4096, "syndrome", syndrome=FAKE + 2)
    assert "multiple of 4" in E.last_error()
    refused(rs63, shards_of(9), 0, 4096, "hyp", syndrome=FAKE, hyp=FAKE + 4)
    assert "multiple of 8" in E.last_error()
    refused(rs63, shards_of(9), 0, 4096, "counts", syndrome=FAKE, hyp=FAKE, located=FAKE + 1, counts=FAKE + 6)
    assert "multiple of 4" in E.last_error()
    refused(rs63, shards_of(9), 0, 4096, "LSEC_LOCATE_REPAIR", flags=6)  # an unknown flag bit


def test_refuses_block_sizes(rs63):
    refused(rs63, shards_of(9), 0, 4100, "multiple of 8")
    with L.Plan.new(L.CAUCHY_GOOD, 8 * 64 * 2, 6, 3, 8, 64, 8) as p:
        p.form_encoding_matrix()
        assert p.kernel == 2
        assert locate(p, shards_of(9), 0, 8 * 64 * 2) == 0, E.last_error()
        refused(p, shards_of(9), 0, 8 * 64 * 2 + 64, "w*packet_size = 512")


def test_not_a_plan(built):
    fake = (C.c_char * 512)()
    assert L.lib().lsec_locate_dev(C.cast(fake, C.POINTER(E.PlanStruct)), shards_of(9), 0, 4096, None, None, None, None,
                                   0, None) == -1
    assert "not an lstore_ec plan" in E.last_error()


# ---------------------------------------------------------------- the ratio image
def gf_tables():
    """GF(2^8) over 0x11D, built here: exp / log"""
    exp, log, x = [0] * 510, [0] * 256, 1
    for i in range(255):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    for i in range(255, 510):
        exp[i] = exp[i - 255]
    return exp, log


@pytest.mark.parametrize("name,method,k,m,packet", [("rs63", L.REED_SOL_VAN, 6, 3, 0), ("r6_62", L.REED_SOL_R6_OP, 6, 2, 0),
                                                     ("rs128", L.REED_SOL_VAN, 12, 8, 0), ("cg63", L.CAUCHY_GOOD, 6, 3, 8)])
def test_ratio_image(built, name, method, k, m, packet):
    """Q[r][j] of the host image = g[r+1][j] / g[0][j], g the yardstick's coding matrix"""
    exp, log = gf_tables()
    g = O.coding_matrix(method, k, m, 8)
    assert g is not None and g.shape == (m, k) and (g != 0).all()
    size = 4096 if not packet else 8 * packet * 4
    with L.Plan.new(method, size, k, m, 8, packet, 8) as p:
        assert p.form_encoding_matrix() == 0
        got = np.array([[E.locate_ratio(p, r, j) for j in range(k)] for r in range(m - 1)])
        want = np.array([[exp[log[int(g[r + 1, j])] + 255 - log[int(g[0, j])]] for j in range(k)] for r in range(m - 1)])
        assert np.array_equal(got, want), (name, got, want)
        with pytest.raises(E.ErasureError, match="outside"):
            E.locate_ratio(p, m - 1, 0)
